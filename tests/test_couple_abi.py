"""libcatint_couple without a GPU (the method of tests/test_response_abi.py).  The NumPy restatement of include/catint_couple.h
(tests/couple_ref.py, which tests/test_gpu_couple.py compares the device with) is checked against known answers: central differences
of the oracle's stationary solves, the flux response of tests/response_ref.py column by column, the damping rule and the singularity
check on hand-made numbers.  The library builds for gfx950 and exports what the header declares, the ctypes mirrors have the
compiler's layouts, every validation error is returned before any device call, and the kernels compiled into it are exactly the eight
instances listed here.  The Newton loop of Calculator.set_microkinetics(..., scf='newton') is driven on the CPU with the oracle as the
transport and tests/kinetics_ref.py as the kinetics (convergence in the stated number of steps, superlinear, to the fixed point of the
mixing loop), and with fakes (freezing, the retry ladder, failed lanes, result keys, the excluded combinations).

Measured (CPU): the tangent against central differences at the relative flux step 0.1: 5.5e-8 (bound 5e-7); against
response_ref's flux response: 8e-13 (case G with its general reaction table, nx = 21: 1.2e-7 and 9e-13); the Newton loop: 2 steps at the eight potentials of the end-to-end case (residuals 1, 5e-6 ..
7e-4, <= 1.1e-9), 3 / 6 / 6 steps at -0.5 / -0.7 / -0.9 V; its fluxes against the mixing loop's (23 iterations): 8e-9."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import couple_ref as CR
from tests import kernel_census as K
from tests import kinetics_ref as KR
from tests import response_cases as RC
from tests import response_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {'catcpl_params': 'CatcplParams', 'catcpl_outputs': 'CatcplOutputs'}
INSTANCES = {'catcpl::couple_kernel<%d>' % nb for nb in range(2, 10)}


# ---- the reference against known answers -------------------------------------------------------------------------------------------
def plain_F(flux=None):
    """case F without its wall table: the coupling is defined for prescribed fluxes only"""
    case = RC.case_F(flux=flux)
    case.wall = None
    return case


@pytest.fixture(scope='module')
def state_F():
    case = plain_F(flux=[0.0, -1e-6, 1e-6])
    return (case,) + case.solve()


@pytest.fixture(scope='module')
def state_G():
    """case G (tests/response_cases.py: general reaction tables) without its wall table, about the prescribed fluxes of the sensitivity
    tests"""
    case = RC.case_G(21)
    case.wall, case.flux = None, np.array([0.0, -1e-6, 1e-6, 0.0])
    return (case,) + case.solve()


def test_the_tangent_is_the_derivative_of_the_oracle_s_solutions(state_F):
    """Central differences of stationary solves at the relative flux step 0.1 tests/test_response_abi.py found usable (smaller steps
    measure the rounding of the solves), with the bound measured there: 5e-7."""
    tangent_against_differences(state_F)


def test_the_tangent_of_case_G_is_the_derivative_of_the_oracle_s_solutions(state_G):
    tangent_against_differences(state_G)


def tangent_against_differences(state):
    case, p, c, phi = state
    T = CR.tangent_banded(p, c, phi)
    fd = np.zeros_like(T)
    h = 0.1 * 1e-6
    for j in range(case.N):
        e = np.zeros(case.N)
        e[j] = h
        _, ca, pa = case.solve(start=(c, phi), flux=case.flux + e)
        _, cb, pb = case.solve(start=(c, phi), flux=case.flux - e)
        fd[:case.N, j] = (ca[:, 0] - cb[:, 0]) / (2.0 * h)
        fd[case.N, j] = (pa[0] - pb[0]) / (2.0 * h)
    err = max(CR.rel(fd[:, j], T[:, j]) for j in range(case.N))
    print('%s: central differences against the tangent, relative flux step 0.1: %.2e' % (case.name, err))
    assert err <= 5e-7


def test_every_column_is_the_flux_response_of_the_response_reference(state_F):
    columns_against_the_response_reference(state_F)


def test_every_column_of_case_G_is_the_flux_response_of_the_response_reference(state_G):
    columns_against_the_response_reference(state_G)


def columns_against_the_response_reference(state):
    case, p, c, phi = state
    for method in CR.METHODS:
        T = CR.METHODS[method](p, c, phi)
        worst = 0.0
        for j in range(case.N):
            r = RR.response(p, c, phi, 0.0, ('flux', j), 'elimination' if method == 'schur' else 'banded')
            worst = max(worst, CR.rel(T[:case.N, j], r['dc_surface'].real), CR.rel(T[case.N, j], r['dphi_surface'].real))
        print('%s against response_ref: %.1e' % (method, worst))
        assert worst <= 1e-9, (method, worst)
    assert CR.rel_T(CR.tangent_schur(p, c, phi), CR.tangent_banded(p, c, phi)) < 1e-8


def test_the_damping_rule_on_hand_made_numbers():
    cs = np.array([10.0, 2.0, 0.0, 5.0])
    assert CR.damping(cs, np.array([-1.0, 1.0, -3.0, 0.0]), 0.01, 0.05) == 1.0          # nothing binds; c_s = 0 does not enter
    assert CR.damping(cs, np.array([-18.0, 1.0, -3.0, 0.0]), 0.01, 0.05) == 0.5         # 0.9 * 10 / 18
    assert CR.damping(cs, np.array([-18.0, -9.0, 0.0, 0.0]), 0.01, 0.05) == 0.9 * 2.0 / 9.0
    assert CR.damping(cs, np.array([-1.0, 1.0, 0.0, 0.0]), -0.2, 0.05) == 0.25          # lambda |dphi| <= dphi_max
    assert CR.damping(cs, np.array([-1.0, 1.0, 0.0, 0.0]), -0.2, 0.0) == 1.0            # switched off
    assert CR.damping(cs, np.array([-18.0, 1.0, 0.0, 0.0]), 0.5, 0.05) == 0.1           # the smaller of the two
    # through the step: T = [[2, 0], [0, 1], [0.1, 0]], no kinetic feedback, so dflux = -(g - K)
    T = np.array([[2.0, 0.0], [0.0, 1.0], [0.1, 0.0]])
    out = CR.step_from_tangent(T, np.array([1.0, 1.0]), g=[0.0, 0.0], K=[-1.0, 0.25], Kc=np.zeros((2, 2)), Kphi=np.zeros(2), dphi_max=0.0)
    assert out['status'] == 0 and np.array_equal(out['dflux'], [-1.0, 0.25]) and np.array_equal(out['dc_surface'], [-2.0, 0.25])
    assert out['lambda'] == 0.45 and np.array_equal(out['flux_new'], [-0.45, 0.45 * 0.25])
    assert (np.array([1.0, 1.0]) + out['lambda'] * out['dc_surface'])[0] == pytest.approx(0.1, abs=1e-15)
    out = CR.step_from_tangent(T, np.array([1.0, 1.0]), g=[0.0, 0.0], K=[-1.0, 0.25], Kc=np.zeros((2, 2)), Kphi=np.zeros(2), rf=2.0, dphi_max=0.05)
    assert np.array_equal(out['dflux'], [-2.0, 0.5]) and out['lambda'] == 0.225 and out['dphi_surface'] == -0.2


def test_status_3_on_a_singular_newton_matrix():
    T = np.array([[2.0, 0.5], [0.25, 1.0], [0.1, -0.2]])
    cs, g, K = np.array([1.0, 1.0]), [1.0, 2.0], [0.5, 0.5]
    Kc = np.linalg.inv(T[:2])                       # A = I - Kc T_c = 0 up to rounding: every entry is noise
    out = CR.step_from_tangent(T, cs, g, K, Kc, np.zeros(2))
    assert out['status'] == 3 and np.abs(out['A']).max() < 1e-15
    Kc = np.array([[0.5, 0.0], [0.0, 0.0]]) @ np.linalg.inv(T[:2]) * 2.0          # A = diag(0, 1) up to rounding
    out = CR.step_from_tangent(T, cs, g, K, Kc, np.zeros(2))
    assert out['status'] == 3
    out = CR.step_from_tangent(T, cs, g, K, 0.5 * Kc, np.zeros(2))             # A = diag(1/2, 1)
    assert out['status'] == 0 and np.allclose(out['A'], np.diag([0.5, 1.0]), atol=1e-15)
    # the pivoting: a zero on the diagonal of a regular matrix is no singularity
    x, sing = CR.solve_pivoted(np.array([[0.0, 1.0], [2.0, 0.0]]), np.array([3.0, 4.0]), 2.0)
    assert not sing and np.array_equal(x, [2.0, 3.0])


# ---- the library -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_couple_library
    return build_couple_library()


@pytest.fixture(scope='module')
def coupler(libpath):
    from catint_amd import _couple
    with _couple.Coupler(0) as o:
        yield o


def header_source(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    from catint_amd import _couple
    declared = sorted(set(re.findall(r'\b(catcpl_[a-z0-9_]+)\s*\(', header_source('catint_couple.h'))))
    assert declared == sorted(_couple.SYMBOLS) and len(declared) == 6
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(catcpl_[a-z0-9_]+)\b', exported))) == declared
    assert not re.findall(r'\b(?:pnp|catresp|catkin)_[a-z0-9_]+\b', exported)          # and no symbol of another library


def test_the_sources_are_a_library_of_their_own():
    from catint_amd import build
    others = (build.SOURCES + build.OBSERVE_SOURCES + build.BALANCE_SOURCES + build.REGRID_SOURCES + build.EQUIL_SOURCES + build.RESPONSE_SOURCES
              + build.KINETICS_SOURCES)
    assert not any('catcpl' in s or 'couple' in s for s in others)
    assert os.path.dirname(build.COUPLE_LIB) == os.path.dirname(build.LIB)
    assert build.COUPLE_SOURCES == ['catcpl.hip'] and os.path.isdir(build.COUPLE_DIR) and callable(build.couple_needs_build)
    listed = {os.path.realpath(p) for p in build.COUPLE_HEADERS}
    for h in ('catint_couple.h', 'catint_pnp.h'):
        assert os.path.realpath(os.path.join(ROOT, 'include', h)) in listed
    from tests.test_build_deps import reached
    sources = [os.path.join(build.COUPLE_DIR, f) for f in build.COUPLE_SOURCES]
    assert not reached(sources) - listed - {os.path.realpath(f) for f in sources}
    assert 'build_couple_library(' in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    from catint_amd import _capi
    assert not [s for s in _capi.SYMBOLS if 'catcpl' in s or 'coupl' in s] and hasattr(_capi.PnpSolver, 'get_coupling')


def header_structs():
    out = {}
    for body, struct in re.findall(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', header_source('catint_couple.h'), flags=re.S):
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
    d = tmp_path_factory.mktemp('couple_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_couple.h"', '#include "catint_response.h"', 'int main(void) {']
    for s in PAIRS:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (s, s))
        for f in structs[s]:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    for name, macro in (('maxnx', 'CATCPL_MAX_NX'), ('maxspecies', 'CATCPL_MAX_SPECIES'), ('dirichlet', 'CATCPL_WALL_DIRICHLET'),
                        ('stern', 'CATCPL_WALL_STERN'), ('einval', 'CATCPL_EINVAL'), ('enomem', 'CATCPL_ENOMEM'), ('edevice', 'CATCPL_EDEVICE'),
                        ('samelimits', 'CATCPL_MAX_NX == CATRESP_MAX_NX && CATCPL_MAX_SPECIES == CATRESP_MAX_SPECIES && '
                                       'CATCPL_PIVOT_GROWTH_LIMIT == CATRESP_PIVOT_GROWTH_LIMIT && CATCPL_PIVOT_GROWTH_LIMIT == 1e8 && '
                                       'CATCPL_SINGULAR == 1e-12')):
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
    from catint_amd import _couple
    cls = getattr(_couple, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_of_the_binding_are_the_header_s(compiler_layout):
    from catint_amd import _couple
    assert _couple.MAX_NX == compiler_layout['maxnx']['n'] == 4098 and _couple.MAX_SPECIES == compiler_layout['maxspecies']['n'] == 8
    assert _couple.WALL == {'dirichlet': compiler_layout['dirichlet']['n'], 'stern': compiler_layout['stern']['n']}
    assert (_couple.EINVAL, _couple.ENOMEM, _couple.EDEVICE) == tuple(compiler_layout[k]['n'] for k in ('einval', 'enomem', 'edevice'))
    assert compiler_layout['samelimits']['n'] == 1 and (_couple.PIVOT_GROWTH_LIMIT, _couple.SINGULAR, CR.GROWTH, CR.SINGULAR) == (1e8, 1e-12, 1e8, 1e-12)


def fake_view(nx=16, N=2, B=2, phi=0x1000, size=None, status=0x1000):
    """A view no device stands behind: validation must reject it without reading it."""
    from catint_amd import _couple
    return _couple.PnpDeviceView(C.sizeof(_couple.PnpDeviceView) if size is None else size, 2, N, nx, (nx + 15) // 16 * 16, 0, B, 0x1000, phi,
                                 status, None)


def good_args(view, n=None):
    nx, N, B = max(view.nx, 1), max(view.nspecies, 1), max(view.batch, 1)
    n = B if n is None else n
    return dict(D=np.full(N, 1e-9), charges=np.where(np.arange(N) % 2, -RC.F, RC.F), x=np.arange(nx) * 1e-9, beta=0.4, eps=RC.EPS, dx=1e-9,
                flux=np.zeros((n, N)), K=np.ones((n, N)), Kc=np.zeros((n, N, N)), Kphi=np.zeros((n, N)))


def call(coupler, view, **kw):
    from catint_amd import _couple
    args = good_args(view)
    args.update(kw)
    with pytest.raises(_couple.CoupleError) as e:
        coupler.solve(view, **args)
    return e.value


@pytest.mark.parametrize('what, make, word', [
    ('compat handle: no potential row', lambda: (fake_view(phi=None), {}), 'potential'),
    ('a view without a status row', lambda: (fake_view(status=None), {}), 'status row'),
    ('nx below 3', lambda: (fake_view(nx=2), {}), 'nx'),
    ('nx above 4098', lambda: (fake_view(nx=4099, B=1), {}), 'nx'),
    ('more than 8 species', lambda: (fake_view(N=9), {}), 'species'),
    ('x not increasing', lambda: (fake_view(), {'x': np.array([0.0, 1.0, 2.0, 2.0] + list(range(3, 15)), float)}), 'increasing'),
    ('struct_size of the parameters', lambda: (fake_view(), {'struct_size': 8}), 'catcpl_params.struct_size'),
    ('struct_size of the outputs', lambda: (fake_view(), {'out_struct_size': 8}), 'catcpl_outputs.struct_size'),
    ('struct_size of the view', lambda: (fake_view(size=12), {}), 'struct_size'),
    ('a zero D', lambda: (fake_view(), {'D': np.array([1e-9, 0.0])}), 'species 1'),
    ('an infinite charge', lambda: (fake_view(), {'charges': np.array([np.inf, 1.0])}), 'finite charge'),
    ('a negative radius', lambda: (fake_view(), {'mpb_radius': np.array([3e-10, -3e-10])}), 'radius'),
    ('a NaN radius', lambda: (fake_view(), {'mpb_radius': np.array([3e-10, np.nan])}), 'radius'),
    ('beta zero', lambda: (fake_view(), {'beta': 0.0}), 'beta'),
    ('eps infinite', lambda: (fake_view(), {'eps': np.inf}), 'eps'),
    ('dx NaN', lambda: (fake_view(), {'dx': np.nan}), 'dx'),
    ('velocity NaN', lambda: (fake_view(), {'velocity': np.nan}), 'velocity'),
    ('negative max_waves', lambda: (fake_view(), {'max_waves': -1}), 'max_waves'),
    ('an unknown wall', lambda: (fake_view(), {'wall_bc': 2}), 'wall_bc'),
    ('a Stern wall without a capacitance', lambda: (fake_view(), {'wall_bc': 'stern', 'stern_capacitance': 0.0}), 'Stern'),
    ('a Stern wall with an infinite capacitance', lambda: (fake_view(), {'wall_bc': 'stern', 'stern_capacitance': np.inf}), 'Stern'),
    ('a roughness factor of zero', lambda: (fake_view(), {'rf': 0.0}), 'rf'),
    ('a NaN roughness factor', lambda: (fake_view(), {'rf': np.nan}), 'rf'),
    ('an infinite dphi_max', lambda: (fake_view(), {'dphi_max': np.inf}), 'dphi_max'),
    ('a lane outside the batch', lambda: (fake_view(), {'lanes': [0, 2]}), 'lane index 2'),
    ('a negative lane', lambda: (fake_view(), {'lanes': [-1, 0]}), 'lane index -1'),
    ('a reaction that names species 2 of 2', lambda: (fake_view(), {'reactions': [([0], [2], 1.0, 1.0)]}), 'species index 2'),
    ('a reaction with five reactants', lambda: (fake_view(), {'reactions': [([0] * 5, [1], 1.0, 1.0)]}), 'n_lhs'),
    ('seventeen reactions', lambda: (fake_view(), {'reactions': [([0], [1], 1.0, 1.0)] * 17}), 'nreactions'),
    ('no kinetic flux', lambda: (fake_view(), {'K': None}), 'flux, K, Kc and Kphi'),
    ('no dflux_dc', lambda: (fake_view(), {'Kc': None}), 'flux, K, Kc and Kphi'),
])
def test_validation_errors_come_before_any_device_call(coupler, what, make, word):
    from catint_amd import _couple
    view, kw = make()
    err = call(coupler, view, **kw)
    assert err.code == _couple.EINVAL, (what, str(err))
    assert word in str(err), (what, str(err))
    assert coupler.last_kernel == '' and coupler.last_kernel_ms == -1.0


def test_null_arguments_and_null_context(coupler, libpath):
    from catint_amd import _couple
    lib = _couple.load_library()
    p = _couple.CatcplParams(struct_size=C.sizeof(_couple.CatcplParams))
    o = _couple.CatcplOutputs(struct_size=C.sizeof(_couple.CatcplOutputs))
    v = fake_view()
    assert lib.catcpl_solve(coupler._h, None, C.byref(p), C.byref(o)) == _couple.EINVAL
    assert b'null' in lib.catcpl_last_error(coupler._h)
    assert lib.catcpl_solve(coupler._h, C.byref(v), None, C.byref(o)) == _couple.EINVAL
    assert lib.catcpl_solve(coupler._h, C.byref(v), C.byref(p), None) == _couple.EINVAL
    assert lib.catcpl_solve(None, None, C.byref(p), C.byref(o)) == _couple.EINVAL
    assert lib.catcpl_create(0, None) == _couple.EINVAL
    assert lib.catcpl_last_kernel(coupler._h) == b''
    assert lib.catcpl_solve(coupler._h, C.byref(v), C.byref(p), C.byref(o)) == _couple.EINVAL
    assert b'D, charges and x' in lib.catcpl_last_error(coupler._h)
    a = good_args(v)
    p.D, p.charges, p.x = _couple._dptr(a['D']), _couple._dptr(a['charges']), _couple._dptr(a['x'])
    p.beta, p.eps, p.dx, p.rf, p.dphi_max = 0.4, RC.EPS, 1e-9, 1.0, 0.05
    p.nlanes = -1
    assert lib.catcpl_solve(coupler._h, C.byref(v), C.byref(p), C.byref(o)) == _couple.EINVAL
    assert b'nlanes' in lib.catcpl_last_error(coupler._h)
    p.nlanes = 3
    assert lib.catcpl_solve(coupler._h, C.byref(v), C.byref(p), C.byref(o)) == _couple.EINVAL
    assert b'nlanes above the batch' in lib.catcpl_last_error(coupler._h)
    # every output NULL: nothing to do, and no device call
    p.nlanes = 2
    p.flux, p.K, p.Kc, p.Kphi = (_couple._dptr(a[k]) for k in ('flux', 'K', 'Kc', 'Kphi'))
    assert lib.catcpl_solve(coupler._h, C.byref(v), C.byref(p), C.byref(o)) == 0
    assert lib.catcpl_last_kernel(coupler._h) == b''


def test_an_empty_lane_list_makes_no_device_call(coupler):
    """nlanes == 0: valid, and done before the first device call (this machine may have no device at all)."""
    v = fake_view()
    out = coupler.solve(v, lanes=[], **good_args(v, 0))
    assert out['T_c'].shape == (0, 2, 2) and out['T_phi'].shape == (0, 2) and out['lambda'].shape == (0,) and out['status'].shape == (0,)
    assert sorted(out) == sorted(list(CR.FIELDS) + ['status'])
    assert coupler.last_kernel == ''


def test_compiled_kernels_are_the_eight_instances(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert len(INSTANCES) == 8
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)


# ---- the Newton loop on the CPU: the oracle as the transport, kinetics_ref as the kinetics -----------------------------------------
class OracleSolver(object):
    """What the Newton loop uses of a PnpSolver, on oracle/pnp_physical.py (Stern wall, uniform grid) and tests/couple_ref.py"""

    def __init__(self, tp, B, tol=1e-10, fail=None):
        self.tp, self.B, self.N, self.nx, self.tol = tp, B, tp.nspecies, tp.nx, tol
        self.cb = [tp.species[sp]['bulk_concentration'] for sp in tp.species]
        self.CS, self.pzc = float(tp.system['Stern capacitance']) * 1e-2, float(tp.system.get('phiPZC', 0.0))
        self.mask, self.calls, self.closed = None, [], False
        self.fail = fail or (lambda solver, lane, flux: False)          # a transport solve that is made to fail (the retry ladder)
        self.status = np.zeros(B, np.int32)

    def problem(self, b, phiM=None, flux=None):
        from oracle import pnp_physical as PH
        tp = self.tp
        return PH.PhysicalProblem(D=tp.D, charges=tp.charges, beta=tp.beta, eps=tp.eps, dx=tp.dx, nx=tp.nx, c_bulk=self.cb,
                                  phiM=self.phiM[b] if phiM is None else phiM, flux=self.flux[b] if flux is None else flux,
                                  stern_capacitance=self.CS, phi_pzc=self.pzc)

    def set_batch(self, c0, pb, vz, flux):
        self.c = np.array(c0, float).reshape(self.B, self.N, self.nx)
        self.phi = np.zeros((self.B, self.nx))
        self.phiM, self.flux = np.array(pb, float)[:, 0], np.array(flux, float).reshape(self.B, self.N)

    def lanes(self):
        return range(self.B) if self.mask is None else np.flatnonzero(self.mask)

    def _solve(self, b, p):
        from oracle import pnp_physical as PH
        c, phi, it, _ = PH.newton_step(p, self.c[b], self.phi[b], self.c[b], np.inf, tol=self.tol, maxit=50)
        self.c[b], self.phi[b] = c, phi
        self.status[b] = 0 if it <= 50 and np.isfinite(c).all() else 1
        return self.status[b]

    def solve_stationary(self, tol=0.0, maxit=0):
        """(the cold start: from the bulk state to phiM in stages of 0.1 V about phiPZC)"""
        self.calls.append(('solve_stationary',))
        for b in self.lanes():
            n = max(1, int(np.ceil(abs(self.phiM[b] - self.pzc) / 0.1)))
            for s in range(1, n + 1):
                if self._solve(b, self.problem(b, phiM=self.pzc + (self.phiM[b] - self.pzc) * s / n)):
                    break
        return self.status.copy()

    def solve_surface(self, flux=None, nsteps=0):
        self.calls.append(('solve_surface', None if self.mask is None else list(np.flatnonzero(self.mask)), np.array(flux, float)))
        self.flux = np.array(flux, float).reshape(self.B, self.N)
        for b in self.lanes():
            if self.fail(self, b, self.flux[b]):
                self.c[b], self.status[b] = np.nan, 2
            else:
                self._solve(b, self.problem(b))
        cs, vs, _ = self.get_surface()
        return cs, vs, np.zeros(self.B), self.status.copy()

    def get_surface(self):
        return self.c[:, :, 0].copy(), self.phi[:, 0].copy(), np.zeros(self.B)

    def get_state(self, potential=True, derived=True):
        return self.c.copy(), self.phi.copy()

    def set_lanes(self, lanes, c, phi=None):
        self.calls.append(('set_lanes', list(lanes)))
        self.c[np.asarray(lanes)], self.phi[np.asarray(lanes)] = c, phi

    def set_lane_mask(self, mask=None):
        self.mask = None if mask is None else np.asarray(mask).copy()

    def device_view(self):
        return self

    def get_coupling(self, flux, kin, rf=1.0, lanes=None, dphi_max=0.05, fields=None, max_waves=0):
        self.calls.append(('get_coupling', list(lanes)))
        outs = []
        for i, b in enumerate(lanes):
            assert np.array_equal(np.asarray(flux)[b], self.flux[b])          # the fluxes the state was solved with
            outs.append(CR.step(self.problem(b), self.c[b], self.phi[b], np.asarray(flux)[b], kin['flux'][i], kin['dflux_dc'][i],
                                kin['dflux_dphi'][i][:, 1], rf, dphi_max))
        res = {k: np.array([o[k] for o in outs]) for k in fields}
        res['status'] = np.array([o['status'] for o in outs], np.int32)
        return res

    def close(self):
        self.closed = True


class OracleKinetics(object):
    """KineticsSolver's solve on the view path, on kinetics_ref.solve_fp64 with sensitivities"""

    def __init__(self, poison=None):
        self.calls, self.closed, self.poison = [], False, poison

    def solve(self, view, tab, phiM, lanes=None, potential_drop='stern', stern_capacitance=0.0, phi_pzc=0.0, gamma=None, theta_guess=None,
              fields=None, **kw):
        assert isinstance(view, OracleSolver) and len(lanes) == len(phiM)
        lanes = np.asarray(lanes)
        r = KR.solve_fp64(tab, phiM, view.c[lanes][:, :, 0], view.phi[lanes][:, 0], w=1 if potential_drop == 'stern' else 0, CS=stern_capacitance,
                          phi_pzc=phi_pzc, gamma=gamma, theta_guess=theta_guess, sens=True)
        self.calls.append({'lanes': list(lanes), 'guess': None if theta_guess is None else np.array(theta_guess), 'iterations': r['iterations'].copy(),
                           'fields': tuple(fields)})
        if self.poison is not None:
            self.poison(self, lanes, r)
        return {k: r[k] for k in tuple(fields) + ('status', 'iterations')}

    def close(self):
        self.closed = True


def newton_on_the_cpu(phis, tau=2e-9, rf=None, fail=None, poison=None, max_iter=1000, dphi_max=None):
    from catint_amd.calculator import Calculator
    from tests.test_gpu_kinetics import e2e_model, e2e_transport
    import tests.test_gpu_kinetics as TK
    old = TK.E2E_PHIS
    TK.E2E_PHIS = list(phis)
    try:
        tp = e2e_transport()
    finally:
        TK.E2E_PHIS = old
    tp.newton = {'direct_span': 10.0}          # the fake walks its own path to the potential
    if dphi_max is not None:
        tp.newton['dphi_max'] = dphi_max
    if rf is not None:
        tp.system['RF'] = rf
    calc = Calculator(transport=tp, calc='comsol', tau_scf=tau)
    calc.set_microkinetics(e2e_model(tp), site_density=2e-6, scf='newton')
    kin, made = OracleKinetics(poison), []
    calc._kinetics_solver = lambda: kin

    def fake(B, **kw):
        made.append(OracleSolver(tp, B, fail=fail))
        return made[-1]
    calc._physical_solver = fake
    out = calc.run_scf_cycle(max_iter=max_iter)
    assert len(made) == 1 and made[0].closed and kin.closed
    return out, calc, tp, made[0], kin


def residual_sequences(out):
    """per lane: the residuals of its steps, then the one it ended at"""
    h = out['newton_residual_history']
    return [[r for r in h[:, b] if np.isfinite(r)] + [out['accuracy'][b]] for b in range(h.shape[1])]


def check_superlinear(out):
    h, lam = out['newton_residual_history'], out['damping']
    for b in range(h.shape[1]):
        seq = residual_sequences(out)[b]
        steps = [i for i in range(h.shape[0]) if np.isfinite(h[i, b])]
        for n, i in enumerate(steps):
            if seq[n] < 1e-2 and lam[i, b] == 1.0:
                assert seq[n + 1] < max(seq[n] ** 1.5, 2e-9), (b, seq)


@pytest.fixture(scope='module')
def e2e_newton():
    from tests.test_gpu_kinetics import E2E_PHIS
    return newton_on_the_cpu(E2E_PHIS)


def test_newton_converges_in_three_steps_at_the_eight_potentials(e2e_newton):
    out, calc, tp, solver, kin = e2e_newton
    print('Newton steps %d; residuals per lane: %s' % (out['iterations'], ['%s' % ['%.1e' % r for r in s] for s in residual_sequences(out)]))
    assert out['converged'].all() and not out['failed'].any()
    assert out['iterations'] <= 3 and (out['accuracy'] <= 2e-9).all()
    check_superlinear(out)
    # one cold solve and one solve per step: far fewer than the 23 of the mixing loop
    assert out['transport_solves'] == 1 + out['iterations']
    # the result's keys: today's without 'mix', plus the loop's own
    assert 'mix' not in out
    for k in ('surface_concentration', 'flux', 'current_density', 'surface_pH', 'accuracy', 'converged', 'failed', 'iterations', 'history', 'coverage',
              'flux_scale', 'kinetic_status', 'coupling_status', 'newton_residual_history', 'damping'):
        assert k in out, k
    assert out['newton_residual_history'].shape == out['damping'].shape == (out['iterations'], 8)
    assert (out['kinetic_status'] == 0).all() and (out['coupling_status'] == 0).all()
    assert np.allclose(out['coverage'].sum(axis=1), 1.0, atol=1e-12)
    for i in range(8):
        assert np.array_equal(tp.alldata[i]['system']['coverage'], out['coverage'][i])
        assert tp.alldata[i]['species']['CO']['flux'] == out['flux'][i, 3]
    # kinetics: the first call cold, the later ones warm-started, with the fields the loop needs
    assert kin.calls[0]['guess'] is None and kin.calls[1]['guess'] is not None and kin.calls[-1]['iterations'].max() <= 3
    assert set(kin.calls[0]['fields']) >= {'flux', 'flux_scale', 'dflux_dc', 'dflux_dphi'}


def test_the_fixed_point_is_the_mixing_loop_s(e2e_newton):
    from tests.test_gpu_kinetics import scf_on_the_cpu
    out = e2e_newton[0]
    mixed, _ = scf_on_the_cpu()
    assert mixed['converged'].all()
    err = np.abs(out['flux'] - mixed['flux']).max(axis=1) / np.abs(mixed['flux']).max(axis=1)
    print('Newton against the mixing loop (%d iterations): fluxes differ by %.1e' % (mixed['iterations'], err.max()))
    assert (err <= 1e-6).all(), err


def test_newton_at_strong_depletion_converges_within_eight_steps():
    """-0.5, -0.7 and -0.9 V: CO2 at the wall falls to 1e-3 mol/m^3; the first steps are damped by the positivity rule"""
    out, calc, tp, solver, kin = newton_on_the_cpu([-0.5, -0.7, -0.9])
    seqs = residual_sequences(out)
    print('steps per lane %s; damping %s; CO2 at the wall %s' % ([len(s) - 1 for s in seqs], out['damping'].T.tolist(),
                                                                  out['surface_concentration'][:, 2]))
    assert out['converged'].all() and not out['failed'].any()
    assert max(len(s) - 1 for s in seqs) <= 8 and (out['accuracy'] <= 2e-9).all()
    assert np.nanmin(out['damping']) < 1.0 and (out['surface_concentration'] > 0).all()
    check_superlinear(out)
    # lanes leave the later calls as they converge
    sizes = [len(c['lanes']) for c in kin.calls]
    assert sizes == sorted(sizes, reverse=True)


# ---- the Calculator path with fakes ------------------------------------------------------------------------------------------------
def test_converged_lanes_are_frozen_and_leave_the_later_calls():
    from tests.test_gpu_kinetics import E2E_PHIS
    # a loose tolerance that the weakly coupled lanes meet a step before the others
    out, calc, tp, solver, kin = newton_on_the_cpu(E2E_PHIS, tau=1e-5)
    assert out['converged'].all()
    masks = [c[1] for c in solver.calls if c[0] == 'solve_surface']
    coupled = [c[1] for c in solver.calls if c[0] == 'get_coupling']
    assert masks == coupled and all(m is not None for m in masks)
    kin_lanes = [c['lanes'] for c in kin.calls]
    assert kin_lanes[0] == list(range(8))
    for earlier, later in zip(kin_lanes, kin_lanes[1:]):
        assert set(later) <= set(earlier)
    assert len(kin_lanes[-1]) < 8 or len(kin_lanes) == 2
    # a frozen lane's flux is not touched by the later solves
    fluxes = [c[2] for c in solver.calls if c[0] == 'solve_surface']
    for m, f in zip(masks, fluxes):
        frozen = [b for b in range(8) if b not in m]
        assert np.array_equal(f[frozen], solver.flux[frozen])
    assert solver.mask is None          # the mask is lifted when the loop is done


def test_a_failed_transport_solve_is_retried_with_the_step_halved():
    from tests.test_gpu_kinetics import E2E_PHIS
    seen = {}

    def fail(solver, lane, flux):
        """lane 3 fails its first two tries of the first step; lane 5 fails always"""
        n = seen[lane] = seen.get(lane, 0) + 1
        return (lane == 3 and n <= 2) or lane == 5
    out, calc, tp, solver, kin = newton_on_the_cpu(E2E_PHIS, fail=fail)
    assert list(np.flatnonzero(out['failed'])) == [5] and list(np.flatnonzero(~out['converged'])) == [5]
    assert out['damping'][0, 3] == 0.25 and np.isnan(out['damping'][0, 5]) and (np.delete(out['damping'][0], [3, 5]) == 1.0).all()
    assert seen[5] == 4                                                        # the step and three halvings
    # each retry starts from the state before the step, restricted to the lanes that failed
    sets = [c[1] for c in solver.calls if c[0] == 'set_lanes']
    assert sets[:3] == [[3, 5], [3, 5], [5]] and sets[3] == [5]
    retries = [c[1] for c in solver.calls if c[0] == 'solve_surface'][:4]
    assert retries == [list(range(8)), [3, 5], [3, 5], [5]]
    # lane 3 still converges, to the same fixed point
    ref = newton_on_the_cpu(E2E_PHIS)[0]
    assert np.allclose(out['flux'][3], ref['flux'][3], rtol=1e-8) and out['accuracy'][3] <= 2e-9
    assert out['transport_solves'] > ref['transport_solves']


def test_kinetic_and_coupling_failures_leave_as_failed():
    from tests.test_gpu_kinetics import E2E_PHIS

    def poison(kin, lanes, r):
        if len(kin.calls) == 2 and 2 in lanes:          # lane 2's coverages are not found in the second call
            r['status'][list(lanes).index(2)] = 1
        if len(kin.calls) == 1:                          # lane 6: a kinetic feedback that makes the Newton matrix singular
            i = list(lanes).index(6)
            r['dflux_dc'][i] = np.nan
    out, calc, tp, solver, kin = newton_on_the_cpu(E2E_PHIS, poison=poison)
    assert list(np.flatnonzero(out['failed'])) == [2, 6]
    assert out['kinetic_status'][2] == 1 and out['coupling_status'][6] == 3 and out['coupling_status'][2] == 0
    assert out['converged'][[0, 1, 3, 4, 5, 7]].all() and tp.alldata[6]['system']['coupling_status'] == 3


def test_the_roughness_factor_scales_what_the_transport_sees():
    from tests.test_gpu_kinetics import E2E_PHIS
    out, calc, tp, solver, kin = newton_on_the_cpu(E2E_PHIS[:3], rf=2.0)
    assert calc.RF == 2.0 and out['converged'].all()
    assert np.allclose(solver.flux, 2.0 * out['flux'], rtol=1e-14)          # the transport carries rf times the kinetic flux
    end = KR.solve_fp64(calc.microkinetics['tables'], np.array(E2E_PHIS[:3]), out['surface_concentration'], solver.phi[:, 0], w=1, CS=0.2,
                        phi_pzc=0.1, sens=False)
    assert np.allclose(end['flux'], out['flux'], rtol=1e-8, atol=1e-30)


def test_max_iter_stops_the_loop_without_failing_the_lanes():
    from tests.test_gpu_kinetics import E2E_PHIS
    out = newton_on_the_cpu(E2E_PHIS[:2], max_iter=1)[0]
    assert out['iterations'] == 1 and not out['converged'].any() and not out['failed'].any() and np.isfinite(out['accuracy']).all()


def test_the_excluded_combinations_raise():
    from catint_amd.calculator import Calculator, CalculatorError
    from tests.test_gpu_kinetics import e2e_model, e2e_transport
    from tests.test_host_physical import make_tp
    tp = e2e_transport()
    calc = Calculator(transport=tp, calc='comsol')
    with pytest.raises(CalculatorError, match="'mixing' or 'newton'"):
        calc.set_microkinetics(e2e_model(tp), scf='anderson')
    calc.set_microkinetics(e2e_model(tp), scf='newton')
    with pytest.raises(CalculatorError, match='flux_callback'):
        calc.run_scf_cycle(flux_callback=lambda state: np.zeros((8, 4)))
    with pytest.raises(CalculatorError, match='transport_fn'):
        calc.run_scf_cycle(transport_fn=lambda flux: (flux, flux[:, 0], flux[:, 0]))
    with pytest.raises(CalculatorError, match='exclude each other'):
        calc.set_surface_kinetics([{'species': 'CO2', 'rate': lambda phiM: 1e-9 + 0 * phiM, 'stoichiometry': {'CO2': -1.0}}])
    # the compat mode has no microkinetics at all
    tp2 = make_tp(np.array([0.1]))
    calc2 = Calculator(transport=tp2, calc='Crank-Nicolson', dt=1e-9, tmax=1e-8)
    with pytest.raises(CalculatorError, match='physical mode'):
        calc2.set_microkinetics(e2e_model(tp), scf='newton')
    # the default stays the mixing loop: no 'scf' entry, so run_scf_cycle takes the path it took
    calc.set_microkinetics(e2e_model(tp))
    assert 'scf' not in calc.microkinetics
