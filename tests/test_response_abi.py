"""libcatint_response without a GPU (the method of tests/test_equil_abi.py).  The NumPy restatement of include/catint_response.h
(tests/response_ref.py, which tests/test_gpu_response.py compares the device with) is checked against known answers: the Debye-Hueckel
capacitance to second order in the grid, Kornyshev's bell-shaped capacitance of the steric double layer, the derivative of the oracle's
own stationary solutions (also with the general reaction and wall tables of case G), and its omega -> 0 limit; and the cases of the
device tests are shown to see every entry of their tables.  The library builds for gfx950 and exports what the header declares, the ctypes
mirrors have the compiler's layouts, every validation error is returned before any device call, the kernels compiled into it are exactly
the thirty-two instances listed here and none of the other five libraries gained one.  The calculator's opt-in path is driven with fake
solvers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import kernel_census as K
from tests import response_cases as RC
from tests import response_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {'catresp_params': 'CatrespParams', 'catresp_outputs': 'CatrespOutputs'}

# response_kernel<block size N + 1, complex, records>
INSTANCES = {'catresp::response_kernel<%d, %s, %s>' % (nb, cx, rec) for nb in range(2, 10) for cx in ('false', 'true') for rec in ('false', 'true')}


# ---- the reference against known answers -------------------------------------------------------------------------------------------
def capacitance(case, p=None, c=None, phi=None):
    p = case.make() if p is None else p
    if c is None:
        c, phi = case.bulk_state()
    r = RR.response(p, c, phi)
    assert r['dsigma'].imag == 0.0
    return float(r['dsigma'].real)


def test_debye_hueckel_capacitance_dirichlet_wall_is_second_order():
    errs = []
    for nx in (41, 81, 161):
        case = RC.debye_hueckel(nx, stern=False)
        errs.append(capacitance(case) / (RC.EPS / case.lam) - 1.0)
    print('C_d against eps / lambda_D at nx = 41 / 81 / 161: %+.3e %+.3e %+.3e' % tuple(errs))
    assert 3.6 <= errs[0] / errs[1] <= 4.4 and 3.6 <= errs[1] / errs[2] <= 4.4
    assert abs(errs[2]) < 1e-3


def test_debye_hueckel_capacitance_stern_wall_is_first_order():
    errs = []
    for nx in (41, 81, 161):
        case = RC.debye_hueckel(nx, stern=True)
        errs.append(capacitance(case) / (1.0 / (1.0 / 0.2 + case.lam / RC.EPS)) - 1.0)
    print('C_d against 1 / (1 / C_S + lambda_D / eps) at nx = 41 / 81 / 161: %+.3e %+.3e %+.3e' % tuple(errs))
    assert 1.8 <= errs[0] / errs[1] <= 2.2 and 1.8 <= errs[1] / errs[2] <= 2.2


def test_kornyshev_bell_of_the_steric_double_layer():
    case = RC.kornyshev()
    state, values, errs = None, [], []
    for i in range(9):
        phiM = -0.1 * i
        if i == 0:
            p = case.make(0.0)
            c, phi = case.bulk_state()
        else:
            p, c, phi = case.solve(phiM, start=state)
        state = (c, phi)
        cd = capacitance(case, p, c, phi)
        values.append(cd)
        errs.append(cd / RC.kornyshev_formula(case, phiM) - 1.0)
    print('C_d against Kornyshev at 0 .. -0.8 V: ' + ' '.join('%+.2e' % e for e in errs))
    assert np.abs(errs).max() <= 5e-3
    assert int(np.argmax(values)) == 2          # the bell: the largest value is the one at -0.2 V


@pytest.fixture(scope='module')
def state_F():
    case = RC.case_F()
    return (case,) + case.solve()


def stacked(r):
    return np.concatenate([r['dc'], r['dphi'][None]])


@pytest.fixture(scope='module')
def state_G():
    """case G (tests/response_cases.py): general reaction and wall tables"""
    case = RC.case_G(21)
    return (case,) + case.solve()


def tangent_against_differences(state):
    case, p, c, phi = state
    prof = stacked(RR.response(p, c, phi))
    errs = []
    for h in (1e-3, 1e-4):
        _, ca, pa = case.solve(case.phiM + h, start=(c, phi))
        _, cb, pb = case.solve(case.phiM - h, start=(c, phi))
        errs.append(RR.rel_rows(np.concatenate([ca - cb, (pa - pb)[None]]) / (2.0 * h), prof))
    print('%s: central differences against the tangent at h = 1e-3, 1e-4: %.2e %.2e' % ((case.name,) + tuple(errs)))
    assert 50.0 <= errs[0] / errs[1] <= 200.0      # the h^2 law
    assert errs[1] <= 5e-7


def test_the_tangent_is_the_derivative_of_the_oracle_s_solutions(state_F):
    tangent_against_differences(state_F)


def test_the_tangent_of_case_G_is_the_derivative_of_the_oracle_s_solutions(state_G):
    """... through a repeated reactant, an empty side, a catalyst, four entries per side and three wall reactions"""
    tangent_against_differences(state_G)


def test_the_flux_tangent_is_the_derivative_of_the_oracle_s_solutions():
    """('flux', 1) about a prescribed flux of 1e-6 mol m^-2 s^-1.  A relative step of 1e-4 moves the state by 6e-11 of its size, which
    is the size of the rounding error of the oracle's solves (cond(J) eps): central differences then measure that noise -- 5.7e-5 at a
    relative step of 1e-4, 5.0e-6 at 1e-3, growing as 1 / h where a truncation error would fall as h^2 -- not the tangent.  The state is
    close to linear in the flux, so the bound of the phiM check, 5e-7, is asserted at the relative step 0.1, where the rounding share is
    5e-8; the figures of the smaller steps are printed."""
    case = RC.case_F(flux=[0.0, 1e-6, 0.0])
    flux_tangent_against_differences(case)


def flux_tangent_against_differences(case):
    base = case.flux.copy()
    p, c, phi = case.solve()
    prof = stacked(RR.response(p, c, phi, perturbation=('flux', 1)))
    errs = []
    for rel in (1e-1, 1e-3, 1e-4):
        e = np.zeros(case.N)
        e[1] = rel * 1e-6
        _, ca, pa = case.solve(start=(c, phi), flux=base + e)
        _, cb, pb = case.solve(start=(c, phi), flux=base - e)
        errs.append(RR.rel_rows(np.concatenate([ca - cb, (pa - pb)[None]]) / (2.0 * e[1]), prof))
    print('%s, flux: central differences against the tangent at relative steps 1e-1, 1e-3, 1e-4: %.2e %.2e %.2e' % ((case.name,) + tuple(errs)))
    assert errs[0] <= 5e-7


def test_the_flux_tangent_of_case_G_is_the_derivative_of_the_oracle_s_solutions():
    """The same check and bound about the prescribed flux [0, 1e-6, 0, 0] of case G"""
    case = RC.case_G(21)
    case.flux = np.array([0.0, 1e-6, 0.0, 0.0])
    flux_tangent_against_differences(case)


def test_the_complex_solve_tends_to_the_real_one(state_F):
    """At omega = 1e-6 / tau_D the real part is the static response to 1e-9 (its correction is second order in omega tau), and the
    imaginary part is first order: below omega tau_D, as no relaxation time of the diffusion problem exceeds L^2 / D_min"""
    complex_against_real(state_F)


def test_the_complex_solve_of_case_G_tends_to_the_real_one(state_G):
    complex_against_real(state_G)


def complex_against_real(state):
    case, p, c, phi = state
    real = RR.response(p, c, phi)
    for method in RR.METHODS:
        cx = RR.response(p, c, phi, 1e-6 / case.tau_D, method=method)
        pairs = [(stacked(cx), stacked(real))] + [(np.atleast_1d(cx[k]).reshape(-1, 1), np.atleast_1d(real[k]).reshape(-1, 1))
                                                 for k in ('dphi_surface', 'dc_surface', 'dsigma', 'dwall_flux')]
        worst_re = max(RR.rel_rows(a.real, b) for a, b in pairs)
        worst_im = max(RR.rel_rows(b + 1j * a.imag, b) for a, b in pairs)
        print('%s: real part off by %.1e, imaginary part %.1e of the static response' % (method, worst_re, worst_im))
        assert worst_re <= 1e-9 and worst_im <= 1e-6, (method, worst_re, worst_im)


def test_the_two_solution_methods_agree(state_F):
    """... to the rounding of the case: what tests/test_gpu_response.py builds its tolerance from must itself stay below 1e-8"""
    methods_agree(state_F)


def test_the_two_solution_methods_agree_on_case_G(state_G):
    methods_agree(state_G)


def methods_agree(state):
    case, p, c, phi = state
    for w in case.omegas():
        for pert in ('phiM', ('flux', 1)):
            d = RR.disagreement(RR.response(p, c, phi, w, pert, 'banded'), RR.response(p, c, phi, w, pert, 'elimination'))
            assert d < 1e-8, (w, pert, d)


# ---- the power of the general-table cases ------------------------------------------------------------------------------------------
G_CASES = {'G nx=5': lambda: RC.case_G(5), 'G nx=21': lambda: RC.case_G(21), 'G8 nx=7': lambda: RC.case_G8(7), 'G8 nx=34': lambda: RC.case_G8(34)}
POWER = 1000.0


def only_live_side_is_empty(reaction):
    """a reaction none of whose sides with a rate holds a species: a constant source, whose part of the Jacobian is zero by construction"""
    lhs, rhs, kf, kr = reaction
    return not ((kf != 0.0 and len(lhs)) or (kr != 0.0 and len(rhs)))


@pytest.mark.parametrize('name', sorted(G_CASES))
def test_the_device_cases_can_see_every_entry_of_their_tables(name):
    """What tests/test_gpu_response.py (and its siblings, which eliminate the same rows) can notice: at the case's largest potential and
    omega = 0, with the state held fixed, the phiM response without one reaction, or without one wall reaction, differs from the full one
    by at least POWER = 1000 times the tolerance the device test uses there (10 x the disagreement of the two methods, not below 1e-11).
    A reaction whose only live side is empty (reaction 3 of G8) is exempt, its Jacobian part being zero; its 'kr' column of
    tests/sens_ref.py must not vanish instead.  Measured (tolerances 1.0e-11 .. 1.8e-10): the weakest entries are those of G8 at nx = 34, wall
    reaction 0 (1.5e5 tolerances) and, among the reactions, 3.1e5; at nx = 7 every entry of G8 moves the result by at least 2.3e6
    tolerances, and every entry of G by at least 7.9e6."""
    import copy
    from tests import sens_ref as SR
    case = G_CASES[name]()
    p, c, phi = case.solve()
    full = RR.response(p, c, phi, 0.0, 'phiM', 'banded')
    tol = max(10.0 * RR.disagreement(full, RR.response(p, c, phi, 0.0, 'phiM', 'elimination')), 1e-11)
    moved = {}
    for table in ('reactions', 'wall_kinetics'):
        entries = getattr(p, table)
        for r in range(len(entries)):
            if table == 'reactions' and only_live_side_is_empty(case.reactions[r]):
                col = SR.sensitivities(p, c, phi, [('kr', r)])
                assert np.abs(col['dc_surface']).max() > 0.0 and np.abs(col['dcurrent']).max() > 0.0, (name, r)
                continue
            less = copy.copy(p)
            setattr(less, table, entries[:r] + entries[r + 1:])
            moved[(table, r)] = RR.disagreement(RR.response(less, c, phi, 0.0, 'phiM', 'banded'), full) / tol
    exempt = [r for r in range(len(case.reactions)) if only_live_side_is_empty(case.reactions[r])]
    assert exempt == ([3] if name.startswith('G8') else [])
    assert len(moved) == len(p.reactions) - len(exempt) + len(p.wall_kinetics)
    weakest = min(moved, key=moved.get)
    print('%s: tolerance %.1e; the weakest entry, %s %d, moves the response by %.1e tolerances; reactions at least %.1e, wall reactions %.1e'
          % (name, tol, weakest[0], weakest[1], moved[weakest], min(v for k, v in moved.items() if k[0] == 'reactions'),
             min(v for k, v in moved.items() if k[0] == 'wall_kinetics')))
    assert moved[weakest] >= POWER, (weakest, moved[weakest])


# ---- the library -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_response_library
    return build_response_library()


@pytest.fixture(scope='module')
def responder(libpath):
    from catint_amd import _response
    with _response.Responder(0) as o:
        yield o


def header_source(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    from catint_amd import _response
    declared = sorted(set(re.findall(r'\b(catresp_[a-z0-9_]+)\s*\(', header_source('catint_response.h'))))
    assert declared == sorted(_response.SYMBOLS) and len(declared) == 6
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(catresp_[a-z0-9_]+)\b', exported))) == declared
    assert not re.findall(r'\bpnp_[a-z0-9_]+\b', exported)          # and no pnp_* symbol


def test_the_sources_are_not_part_of_the_other_libraries():
    from catint_amd import build
    others = build.SOURCES + build.OBSERVE_SOURCES + build.BALANCE_SOURCES + build.REGRID_SOURCES + build.EQUIL_SOURCES
    assert not any('catresp' in s or 'response' in s for s in others)
    assert os.path.dirname(build.RESPONSE_LIB) == os.path.dirname(build.LIB)
    assert build.RESPONSE_SOURCES == ['catresp.hip'] and os.path.isdir(build.RESPONSE_DIR)
    assert callable(build.response_needs_build)
    listed = {os.path.realpath(p) for p in build.RESPONSE_HEADERS}
    for h in ('catint_response.h', 'catint_pnp.h'):
        assert os.path.realpath(os.path.join(ROOT, 'include', h)) in listed
    assert os.path.realpath(os.path.join(build.CSRC, 'pnp_post.h')) in listed
    from tests.test_build_deps import reached
    sources = [os.path.join(build.RESPONSE_DIR, f) for f in build.RESPONSE_SOURCES]
    assert not reached(sources) - listed - {os.path.realpath(f) for f in sources}
    # build() of the driver entry point builds it
    assert 'build_response_library(' in open(os.path.join(ROOT, '__graft_entry__.py')).read()


def header_structs():
    out = {}
    for body, struct in re.findall(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', header_source('catint_response.h'), flags=re.S):
        fields = []
        for decl in body.split(';'):
            decl = decl.strip()
            if not decl:
                continue
            names = decl.split(None, 1)[1] if not decl.startswith('const') else decl.split(None, 2)[2]
            fields += [n.strip().lstrip('*').strip() for n in names.split(',')]
        out[struct] = fields
    return out


@pytest.fixture(scope='module')
def compiler_layout(tmp_path_factory):
    structs = header_structs()
    assert set(PAIRS) <= set(structs)
    d = tmp_path_factory.mktemp('response_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_response.h"', 'int main(void) {']
    for s in PAIRS:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (s, s))
        for f in structs[s]:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    for name, macro in (('maxnx', 'CATRESP_MAX_NX'), ('maxspecies', 'CATRESP_MAX_SPECIES'), ('maxfreq', 'CATRESP_MAX_FREQ'),
                        ('dirichlet', 'CATRESP_WALL_DIRICHLET'), ('stern', 'CATRESP_WALL_STERN'), ('phim', 'CATRESP_PHIM'),
                        ('wallflux', 'CATRESP_WALL_FLUX'), ('einval', 'CATRESP_EINVAL'), ('enomem', 'CATRESP_ENOMEM'),
                        ('edevice', 'CATRESP_EDEVICE')):
        lines.append('  printf("%s n %%d\\n", %s);' % (name, macro))
    lines += ['  return 0;', '}']
    (d / 'abi.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(d / 'abi.c'), '-o', str(d / 'abi')])
    layout = {}
    for line in subprocess.check_output([str(d / 'abi')]).decode().splitlines():
        s, f, v = line.split()
        layout.setdefault(s, {})[f] = int(v)
    return layout


@pytest.mark.parametrize('cname', sorted(PAIRS))
def test_ctypes_mirror_matches_the_compiler(cname, compiler_layout):
    from catint_amd import _response
    cls = getattr(_response, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_of_the_binding_are_the_header_s(compiler_layout):
    from catint_amd import _response
    assert _response.MAX_NX == compiler_layout['maxnx']['n'] == 4098 and _response.MAX_SPECIES == compiler_layout['maxspecies']['n'] == 8
    assert _response.MAX_FREQ == compiler_layout['maxfreq']['n'] == 256
    assert _response.WALL == {'dirichlet': compiler_layout['dirichlet']['n'], 'stern': compiler_layout['stern']['n']}
    assert (_response.PHIM, _response.WALL_FLUX) == (compiler_layout['phim']['n'], compiler_layout['wallflux']['n'])
    assert (_response.EINVAL, _response.ENOMEM, _response.EDEVICE) == tuple(compiler_layout[k]['n'] for k in ('einval', 'enomem', 'edevice'))


def fake_view(nx=16, N=2, B=2, phi=0x1000, size=None):
    """A view no device stands behind: validation must reject it without reading it."""
    from catint_amd import _response
    return _response.PnpDeviceView(C.sizeof(_response.PnpDeviceView) if size is None else size, 2, N, nx, (nx + 15) // 16 * 16, 0, B, 0x1000, phi,
                                   0x1000, None)


def good_args(view):
    nx, N, B = max(view.nx, 1), max(view.nspecies, 1), max(view.batch, 1)
    return dict(D=np.full(N, 1e-9), charges=np.where(np.arange(N) % 2, -RC.F, RC.F), x=np.arange(nx) * 1e-9, beta=0.4, eps=RC.EPS, dx=1e-9,
                phiM=np.linspace(0.1, -0.1, B))


WALL1 = {'species': [0], 'nu': [[1.0, -1.0]], 'k': [[1e-6], [1e-6]]}


def call(responder, view, **kw):
    from catint_amd import _response
    args = good_args(view)
    args.update(kw)
    with pytest.raises(_response.ResponseError) as e:
        responder.solve(view, **args)
    return e.value


@pytest.mark.parametrize('what, make, word', [
    ('compat handle: no potential row', lambda: (fake_view(phi=None), {}), 'potential'),
    ('nx below 3', lambda: (fake_view(nx=2), {}), 'nx'),
    ('nx above 4098', lambda: (fake_view(nx=4099, B=1), {}), 'nx'),
    ('more than 8 species', lambda: (fake_view(N=9), {}), 'species'),
    ('x not increasing', lambda: (fake_view(), {'x': np.array([0.0, 1.0, 2.0, 2.0] + list(range(3, 15)), float)}), 'increasing'),
    ('struct_size of the parameters', lambda: (fake_view(), {'struct_size': 8}), 'catresp_params.struct_size'),
    ('struct_size of the view', lambda: (fake_view(size=12), {}), 'struct_size'),
    ('a zero D', lambda: (fake_view(), {'D': np.array([1e-9, 0.0])}), 'species 1'),
    ('an infinite charge', lambda: (fake_view(), {'charges': np.array([np.inf, 1.0])}), 'finite charge'),
    ('a negative radius', lambda: (fake_view(), {'mpb_radius': np.array([3e-10, -3e-10])}), 'radius'),
    ('a NaN radius', lambda: (fake_view(), {'mpb_radius': np.array([3e-10, np.nan])}), 'radius'),
    ('beta zero', lambda: (fake_view(), {'beta': 0.0}), 'beta'),
    ('eps zero', lambda: (fake_view(), {'eps': 0.0}), 'eps'),
    ('eps infinite', lambda: (fake_view(), {'eps': np.inf}), 'eps'),
    ('dx negative', lambda: (fake_view(), {'dx': -1e-9}), 'dx'),
    ('dx NaN', lambda: (fake_view(), {'dx': np.nan}), 'dx'),
    ('velocity NaN', lambda: (fake_view(), {'velocity': np.nan}), 'velocity'),
    ('negative max_waves', lambda: (fake_view(), {'max_waves': -1}), 'max_waves'),
    ('an unknown wall', lambda: (fake_view(), {'wall_bc': 2}), 'wall_bc'),
    ('a Stern wall without a capacitance', lambda: (fake_view(), {'wall_bc': 'stern', 'stern_capacitance': 0.0}), 'Stern'),
    ('a Stern wall with a negative capacitance', lambda: (fake_view(), {'wall_bc': 'stern', 'stern_capacitance': -0.2}), 'Stern'),
    ('a Stern wall with an infinite capacitance', lambda: (fake_view(), {'wall_bc': 'stern', 'stern_capacitance': np.inf}), 'Stern'),
    ('an unknown perturbation', lambda: (fake_view(), {'perturbation': 2}), 'perturbation'),
    ('a perturbed species outside the system', lambda: (fake_view(), {'perturbation': ('flux', 2)}), 'perturbed species 2'),
    ('a negative perturbed species', lambda: (fake_view(), {'perturbation': ('flux', -1)}), 'perturbed species -1'),
    ('a negative omega', lambda: (fake_view(), {'omega': [0.0, -1.0]}), 'omega[1]'),
    ('a NaN omega', lambda: (fake_view(), {'omega': [np.nan]}), 'omega[0]'),
    ('an infinite omega', lambda: (fake_view(), {'omega': [1.0, 2.0, np.inf]}), 'omega[2]'),
    ('no frequency', lambda: (fake_view(), {'omega': []}), 'nfreq'),
    ('too many frequencies', lambda: (fake_view(), {'omega': np.arange(257.0)}), 'nfreq'),
    ('a lane outside the batch', lambda: (fake_view(), {'lanes': [0, 2]}), 'lane index 2'),
    ('a negative lane', lambda: (fake_view(), {'lanes': [-1]}), 'lane index -1'),
    ('a reaction that names species 2 of 2', lambda: (fake_view(), {'reactions': [([0], [2], 1.0, 1.0)]}), 'species index 2'),
    ('a reaction with five reactants', lambda: (fake_view(), {'reactions': [([0] * 5, [1], 1.0, 1.0)]}), 'n_lhs'),
    ('seventeen reactions', lambda: (fake_view(), {'reactions': [([0], [1], 1.0, 1.0)] * 17}), 'nreactions'),
    ('a wall reaction that names species 2 of 2', lambda: (fake_view(), {'wall': dict(WALL1, species=[2])}), 'wall reaction 0'),
    ('a wall table without rate constants', lambda: (fake_view(), {'wall': {'species': [0], 'nu': [[1.0, -1.0]]}}), 'rate constants'),
    ('nine wall reactions', lambda: (fake_view(), {'wall': {'species': [0] * 9, 'nu': np.ones((9, 2)), 'k': np.ones((2, 9))}}), 'n_wall'),
])
def test_validation_errors_come_before_any_device_call(responder, what, make, word):
    from catint_amd import _response
    view, kw = make()
    err = call(responder, view, **kw)
    assert err.code == _response.EINVAL, (what, str(err))
    assert word in str(err), (what, str(err))
    assert responder.last_kernel == '' and responder.last_kernel_ms == -1.0


def test_null_arguments_and_null_context(responder, libpath):
    from catint_amd import _response
    lib = _response.load_library()
    p = _response.CatrespParams(struct_size=C.sizeof(_response.CatrespParams))
    o = _response.CatrespOutputs()
    v = fake_view()
    assert lib.catresp_solve(responder._h, None, C.byref(p), C.byref(o)) == _response.EINVAL
    assert b'null' in lib.catresp_last_error(responder._h)
    assert lib.catresp_solve(responder._h, C.byref(v), None, C.byref(o)) == _response.EINVAL
    assert lib.catresp_solve(responder._h, C.byref(v), C.byref(p), None) == _response.EINVAL
    assert lib.catresp_solve(None, None, C.byref(p), C.byref(o)) == _response.EINVAL
    assert lib.catresp_create(0, None) == _response.EINVAL
    assert lib.catresp_last_kernel(responder._h) == b''
    # D, charges and x NULL
    assert lib.catresp_solve(responder._h, C.byref(v), C.byref(p), C.byref(o)) == _response.EINVAL
    assert b'D, charges and x' in lib.catresp_last_error(responder._h)
    # potentials and frequencies NULL; negative nlanes; nlanes above the batch without a lane list
    a = good_args(v)
    p.D, p.charges, p.x = _response._dptr(a['D']), _response._dptr(a['charges']), _response._dptr(a['x'])
    p.beta, p.eps, p.dx, p.nfreq, p.nlanes = 0.4, RC.EPS, 1e-9, 1, 2
    assert lib.catresp_solve(responder._h, C.byref(v), C.byref(p), C.byref(o)) == _response.EINVAL
    assert b'phiM and omega' in lib.catresp_last_error(responder._h)
    om = np.zeros(1)
    p.phiM, p.omega = _response._dptr(a['phiM']), _response._dptr(om)
    p.nlanes = -1
    assert lib.catresp_solve(responder._h, C.byref(v), C.byref(p), C.byref(o)) == _response.EINVAL
    assert b'nlanes' in lib.catresp_last_error(responder._h)
    p.nlanes = 3
    assert lib.catresp_solve(responder._h, C.byref(v), C.byref(p), C.byref(o)) == _response.EINVAL
    assert b'nlanes above the batch' in lib.catresp_last_error(responder._h)
    # every output NULL: nothing to do, and no device call
    p.nlanes = 2
    assert lib.catresp_solve(responder._h, C.byref(v), C.byref(p), C.byref(o)) == 0
    assert lib.catresp_last_kernel(responder._h) == b''


def test_an_empty_lane_list_makes_no_device_call(responder):
    """nlanes == 0: valid, and done before the first device call (this machine may have no device at all)."""
    v = fake_view()
    out = responder.solve(v, lanes=[], omega=[0.0, 1.0], profiles=True, **good_args(v))
    assert out['dsigma'].shape == (0, 2) and out['dc_surface'].shape == (0, 2, 2) and out['dc'].shape == (0, 2, 2, 16)
    assert out['dphi'].shape == (0, 2, 16) and out['status'].shape == (0, 2) and out['dsigma'].dtype == np.complex128
    assert responder.last_kernel == ''


def test_compiled_kernels_are_the_thirty_two_instances(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert len(INSTANCES) == 32
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)


def test_the_other_libraries_gained_no_kernel():
    from catint_amd.build import (BALANCE_LIB, EQUIL_LIB, OBSERVE_LIB, REGRID_LIB, build_balance_library, build_equil_library, build_library,
                                  build_observe_library, build_regrid_library)
    build_library()
    build_observe_library()
    build_balance_library()
    build_regrid_library()
    build_equil_library()
    try:
        compiled = set(K.compiled_kernels())
        for lib in (OBSERVE_LIB, BALANCE_LIB, REGRID_LIB, EQUIL_LIB):
            compiled |= K.compiled_kernels(lib=lib)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert not [n for n in compiled if 'catresp' in n or 'response' in n]
    from catint_amd import _capi
    assert not [s for s in _capi.SYMBOLS if 'catresp' in s or 'response' in s]        # no pnp_* symbol was added for it
    assert hasattr(_capi.PnpSolver, 'get_response')


# ---- the calculator's opt-in path, with fake solvers -------------------------------------------------------------------------------
def ladder_parts():
    from tests.test_host_physical import LadderSolver, make_tp

    class ResponseLadderSolver(LadderSolver):
        """LadderSolver with get_response: records the call and returns recognisable numbers"""

        def get_state(self, potential=True, derived=True):
            return self.c.copy(), self.phi.copy(), np.zeros_like(self.phi), np.zeros_like(self.phi)

        def get_response(self, omega=(0.0,), perturbation='phiM', lanes=None, profiles=False, max_waves=0):
            om = np.asarray(omega, float)
            self.calls.append(('get_response', om.copy(), perturbation))
            y = (1.0 + np.arange(self.B))[:, None] * (2.0 + 1j * om[None, :])
            out = {'omega': om, 'admittance': y, 'impedance': 1.0 / y, 'dsigma': y * 0.25, 'status': np.zeros((self.B, len(om)), np.int32)}
            if (om == 0).any():
                out['differential_capacitance'] = 0.5 * (1.0 + np.arange(self.B))
            return out
    return ResponseLadderSolver, make_tp


def run_with(monkeypatch, newton):
    from catint_amd.calculator import Calculator
    Solver, make_tp = ladder_parts()
    phis = np.array([0.1, 0.2, 0.3])
    tp = make_tp(phis)
    tp.newton = newton
    calc = Calculator(transport=tp, calc='comsol')
    made = []

    def fake(B, **kw):
        made.append(Solver(B, tp.nx, 3))
        return made[-1]
    monkeypatch.setattr(calc, '_physical_solver', fake)
    calc.run()
    assert len(made) == 1
    return calc, tp, made[0]


def test_without_the_option_the_call_sequence_is_unchanged(monkeypatch):
    runs = []
    for newton in ({}, {'response': False}):
        calc, tp, s = run_with(monkeypatch, newton)
        runs.append([c[0] for c in s.calls])
        assert calc.response is None and 'differential_capacitance' not in tp.alldata[0]['system']
    assert runs[0] == runs[1] == ['set_batch', 'solve']


def test_with_the_option_one_response_call_after_the_solve(monkeypatch):
    calc, tp, s = run_with(monkeypatch, {'response': {'omega': [0.0, 1e3]}})
    assert [c[0] for c in s.calls] == ['set_batch', 'solve', 'get_response']
    assert np.array_equal(s.calls[-1][1], [0.0, 1e3]) and s.calls[-1][2] == 'phiM'
    for b in range(3):
        d = tp.alldata[b]['system']
        assert d['differential_capacitance'] == 0.5 * (b + 1)
        assert np.array_equal(d['response_omega'], [0.0, 1e3])
        assert np.array_equal(d['admittance'], (b + 1) * np.array([2.0, 2.0 + 1e3j])) and np.allclose(d['impedance'] * d['admittance'], 1.0)
    # True: the static response alone
    calc, tp, s = run_with(monkeypatch, {'response': True})
    assert np.array_equal(s.calls[-1][1], [0.0]) and tp.alldata[2]['system']['differential_capacitance'] == 1.5
    # a list without omega = 0 has no differential capacitance
    calc, tp, s = run_with(monkeypatch, {'response': {'omega': [10.0]}})
    assert tp.alldata[0]['system']['differential_capacitance'] is None and tp.alldata[0]['system']['admittance'].shape == (1,)


def test_the_option_belongs_to_the_physical_mode():
    from catint_amd.calculator import Calculator, CalculatorError
    _, make_tp = ladder_parts()
    tp = make_tp(np.array([0.1]))
    tp.newton = {'response': True}
    with pytest.raises(CalculatorError, match='physical mode'):
        Calculator(transport=tp, calc='Crank-Nicolson', dt=1e-9, tmax=1e-8)
    Calculator(transport=tp, calc='comsol')
    # ... also when the option arrives after the constructor
    tp2 = make_tp(np.array([0.1]))
    calc = Calculator(transport=tp2, calc='Crank-Nicolson', dt=1e-9, tmax=1e-8)
    tp2.newton = {'response': True}
    with pytest.raises(CalculatorError, match='physical mode'):
        calc.run()


def test_a_rate_function_without_alpha_is_warned_about(monkeypatch):
    """The response holds rate constants fixed: K(phiM) without alpha loses dK/dphiM, and run() says so; with alpha it is silent"""
    import warnings
    from catint_amd.calculator import Calculator
    Solver, make_tp = ladder_parts()
    for alpha, expect in ((0.0, True), (-19.0, False)):
        tp = make_tp(np.array([0.1, 0.2, 0.3]))
        tp.newton = {'response': True}
        calc = Calculator(transport=tp, calc='comsol')
        calc.set_surface_kinetics([{'species': 'CO2', 'rate': lambda phiM: 1e-9 * np.exp(-phiM), 'alpha': alpha, 'stoichiometry': {'CO2': -1.0}}])
        monkeypatch.setattr(calc, '_physical_solver', lambda B, **kw: Solver(B, tp.nx, 3))
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            calc.run()
        assert any('dK/dphiM' in str(w.message) for w in seen) == expect
