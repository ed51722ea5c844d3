"""libcatint_sens without a device: the NumPy restatement of include/catint_sens.h (tests/sens_ref.py) against the oracle, the library's
ABI, its validation, its kernel set, and the calculator's opt-in path with a fake solver.

(a) The analytic right-hand sides -dF/dp equal central differences of oracle.pnp_physical.residual in the parameter at fixed state.
(b) The reference's du_0 equals central differences of the oracle's RE-SOLVED stationary states.
(c) Its PHIM and WALL_FLUX columns are those of tests/response_ref.py at omega = 0 and of tests/couple_ref.py.
(d) A direction in bulk composition is the weighted sum of the single-species columns."""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from catint_amd import _sens          # fails without the feature
from oracle import pnp_physical as PH
from tests import couple_ref as CR
from tests import kernel_census as K
from tests import response_cases as RC
from tests import response_ref as RR
from tests import sens_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {'catsens_params': 'CatsensParams', 'catsens_outputs': 'CatsensOutputs'}
INSTANCES = {'catsens::sens_kernel<%d, 8>' % nb for nb in range(2, 10)}
FLUX_F = np.array([0.0, -1e-6, 1e-6])
FLUX_G = np.array([0.0, -1e-6, 1e-6, 0.0])
# the size of a step where the parameter itself is 0 (case E has no convection, and most of its prescribed fluxes are 0): the values
# case F carries (reaction 2 of case G has no backward rate)
ZERO_SCALE = {'velocity': 1e-3, 'flux': 1e-6, 'kr': 1.2e5}


def every_kind(p):
    """... with the rate constants of every reaction and of every wall reaction"""
    return (['phiM', 'stern_capacitance', 'velocity'] + [('wall_k', r) for r in range(len(p.wall_kinetics))]
            + [(kind, r) for r in range(len(p.reactions)) for kind in ('kf', 'kr')]
            + [(kind, j) for kind in ('flux', 'c_bulk', 'D') for j in range(p.N)])


def moved(case, flux, kind, index, delta):
    """The case's problem with one parameter moved by delta"""
    p = case.make(flux=flux)
    if kind == 'phiM':
        p.phiM += delta
    elif kind == 'flux':
        p.flux = p.flux.copy()
        p.flux[index] += delta
    elif kind == 'c_bulk':
        p.c_bulk = p.c_bulk.copy()
        p.c_bulk[index] += delta
    elif kind == 'D':
        p.D = p.D.copy()
        p.D[index] += delta
    elif kind in ('kf', 'kr'):
        p.reactions = copy.deepcopy(p.reactions)
        p.reactions[index][kind] += delta
    elif kind == 'wall_k':
        p.wall_kinetics = copy.deepcopy(p.wall_kinetics)
        p.wall_kinetics[index]['k'] += delta
    elif kind == 'stern_capacitance':
        p.CS += delta
    elif kind == 'velocity':
        p.velocity += delta
    return p


def value(p, kind, index):
    if kind in ('kf', 'kr'):
        return p.reactions[index][kind]
    if kind == 'wall_k':
        return p.wall_kinetics[index]['k']
    v = {'phiM': p.phiM, 'flux': p.flux, 'c_bulk': p.c_bulk, 'D': p.D, 'stern_capacitance': p.CS, 'velocity': p.velocity}[kind]
    return float(np.atleast_1d(v)[index] if np.ndim(v) else v)


@pytest.fixture(scope='module')
def state_F():
    case = RC.case_F()
    p, c, phi = case.solve(flux=FLUX_F)
    return case, p, c, phi


@pytest.fixture(scope='module')
def state_E():
    case = RC.case_E(34)
    p, c, phi = case.solve()
    return case, p, c, phi


@pytest.fixture(scope='module')
def state_G():
    """case G (tests/response_cases.py): general reaction and wall tables"""
    case = RC.case_G(21)
    p, c, phi = case.solve(flux=FLUX_G)
    return case, p, c, phi


@pytest.mark.parametrize('name', ['F', 'E', 'G'])
def test_the_right_hand_sides_are_the_derivatives_of_the_oracle_s_residual(name, state_F, state_E, state_G):
    """(a) Central differences at relative step 1e-6 (of ZERO_SCALE where the parameter is 0), max-norm relative to the largest entry of
    the column.  Measured: at most 1.4e-10 for every kind whose derivative does not go through the edge fluxes' convection term
    (the prescribed fluxes, whose step is 1e-12: 4.8e-9); the three 'D' columns of case F (velocity -1e-3 m/s) 1.4e-6, 3.8e-6, 1.4e-6
    (case E, without convection: 1.1e-10) and the 'velocity' column 2.2e-6 in both cases.
    Those are the difference quotient's own rounding, not the formula's: the quotient divides differences of edge fluxes whose
    two terms are 1e2 .. 1e3 and cancel, by a step of 1e-6 D = 2e-15 (eps 1e3 / 2e-15 = 1e2 against entries of 4e7).  (b) below
    confirms the same columns to 1e-8 through re-solved states.  Bound: 5 x the worst value measured, 3.8e-6.
    Case G (every rate constant of its four reactions and three wall reactions): the residual's rows hold reaction terms of 0.2 that
    cancel, and a relative step of 1e-6 in a prescribed flux, a 'kr' or a 'wall_k' moves them by 1e-13 .. 1e-12, so at that step the
    quotient measures its own rounding: flux 6.5e-5, kr 8.1e-6, wall_k 6.3e-6, kf 4.2e-7, falling as 1 / step to 2.5e-12, 1.8e-11,
    1.2e-12, 3.2e-13 at the relative step 1.  The residual is linear in these four kinds, so the quotient has no truncation error at
    any step: case G takes them at the relative step 1e-2 and then meets the bounds of F and E unchanged (measured: flux 5.1e-9,
    kr 3.0e-9, wall_k 3.8e-10, kf 3.0e-11; D 3.0e-6, velocity 1.1e-6, every other kind at most 1.8e-10)."""
    case, p, c, phi = {'F': state_F, 'E': state_E, 'G': state_G}[name]
    worst = {}
    for spec in every_kind(p):
        kind, index = SR.split(spec)
        r = SR.rhs(p, c, phi, p.flux, kind, index)
        v = value(p, kind, index)
        rel = 1e-2 if name == 'G' and kind in ('flux', 'kf', 'kr', 'wall_k') else 1e-6
        d = rel * (abs(v) if v != 0 else ZERO_SCALE[kind])
        fd = -(PH.residual(moved(case, p.flux, kind, index, d), c, phi, c, np.inf)
               - PH.residual(moved(case, p.flux, kind, index, -d), c, phi, c, np.inf)) / (2 * d)
        scale = np.abs(r).max()
        err = np.abs(fd - r).max() / scale if scale > 0 else np.abs(fd).max()
        worst[kind] = max(worst.get(kind, 0.0), err)
    print('case %s: worst error of -dF/dp against central differences, by kind: %s' % (name, {k: '%.1e' % v for k, v in worst.items()}))
    assert max(worst.values()) <= 2e-5, worst
    assert max(v for k, v in worst.items() if k not in ('D', 'velocity')) <= 1e-8, worst
    if name == 'E':
        # species without flux, reaction or convection: D does not enter their rows at all
        assert all(not SR.rhs(p, c, phi, p.flux, 'D', j).any() for j in (0, 1, 2, 6, 7))


def test_the_reference_is_the_derivative_of_the_oracle_s_solutions(state_F):
    """(b) Case F with flux = [0, -1e-6, 1e-6]: du_0 against central differences of re-solved stationary states, per parameter the
    smallest error over relative steps 1e-2, 1e-3, 1e-4.  Measured: flux columns 4.3e-7, 3.9e-7, 5.2e-7; D 1e-8; every other
    parameter at most 2.3e-9.  Bound 2e-6."""
    reference_against_resolved_states(state_F)


def test_the_reference_of_case_G_is_the_derivative_of_the_oracle_s_solutions(state_G):
    """(b) Case G with flux = [0, -1e-6, 1e-6, 0], every rate constant of its tables among the parameters: the same steps and bound.
    Measured: flux columns up to 9.7e-7, ('kr', 3) 1.0e-7, the wall rate constants up to 5.6e-8, every other rate constant at most 5.2e-9"""
    reference_against_resolved_states(state_G)


def reference_against_resolved_states(state):
    case, p, c, phi = state
    specs = every_kind(p)
    ref = SR.sensitivities(p, c, phi, specs, p.flux)
    worst = {}
    for m, spec in enumerate(specs):
        kind, index = SR.split(spec)
        v = value(p, kind, index)
        mine = np.concatenate([ref['dc_surface'][m], [ref['dphi_surface'][m]]])
        best = np.inf
        for rel in (1e-2, 1e-3, 1e-4):
            d = rel * (abs(v) if v != 0 else ZERO_SCALE[kind])
            ends = []
            for sgn in (1.0, -1.0):
                c2, phi2, it, _ = PH.newton_step(moved(case, p.flux, kind, index, sgn * d), c, phi, c, np.inf, tol=1e-12, maxit=80)
                assert it <= 80
                ends.append(np.concatenate([c2[:, 0], [phi2[0]]]))
            best = min(best, np.abs((ends[0] - ends[1]) / (2 * d) - mine).max() / np.abs(mine).max())
        worst[spec] = best
    print('case %s: du_0 against differences of re-solved states: %s' % (case.name, {str(k): '%.1e' % v for k, v in worst.items()}))
    assert max(worst.values()) <= 2e-6, worst


@pytest.mark.parametrize('name', ['F', 'E', 'G'])
def test_the_control_columns_are_those_of_the_response_and_coupling_references(name, state_F, state_E, state_G):
    """(c)"""
    case, p, c, phi = {'F': state_F, 'E': state_E, 'G': state_G}[name]
    specs = ['phiM'] + [('flux', j) for j in range(p.N)]
    for method in SR.METHODS:
        ref = SR.sensitivities(p, c, phi, specs, p.flux, method)
        for m, spec in enumerate(specs):
            rr = RR.response(p, c, phi, 0.0, spec, 'banded')
            for k in SR.FIELDS:
                want = np.real(rr['admittance' if k == 'dcurrent' else k])
                assert SR.rel_columns(np.atleast_1d(ref[k][m])[None], np.atleast_1d(want)[None])[0] <= 1e-9, (name, method, spec, k)
    # the coupling's tangent is defined without a wall table
    bare = copy.copy(p)
    bare.wall_kinetics = []
    ref = SR.sensitivities(bare, c, phi, specs[1:], p.flux)
    for T in (CR.tangent_banded(bare, c, phi), CR.tangent_schur(bare, c, phi)):
        assert CR.rel_T(ref['dc_surface'].T, T[:p.N]) <= 1e-9 and CR.rel(ref['dphi_surface'], T[p.N]) <= 1e-9


def test_a_direction_in_bulk_composition_is_the_weighted_sum_of_its_columns(state_F):
    """(d) an electroneutral salt: species 0 (+1) and 2 (-2) in the ratio 2 : 1"""
    case, p, c, phi = state_F
    w = np.array([2.0, 0.0, 1.0])
    assert (w * p.q).sum() == 0.0
    ref = SR.sensitivities(p, c, phi, [('c_bulk', w), ('c_bulk', 0), ('c_bulk', 2), ('c_bulk', np.array([0.0, 1.0, 0.0])), ('c_bulk', 1)], p.flux)
    for k in SR.FIELDS:
        assert np.array_equal(ref[k][0], 0.0 + 2.0 * ref[k][1] + 1.0 * ref[k][2]), k
        assert np.array_equal(ref[k][3], ref[k][4]), k
    # ... and it is the derivative along the direction: residual differences with all three bulk values moved
    r = sum(w[j] * SR.rhs(p, c, phi, p.flux, 'c_bulk', j) for j in range(3))
    d = 1e-4
    pp, pm = case.make(flux=FLUX_F), case.make(flux=FLUX_F)
    pp.c_bulk, pm.c_bulk = p.c_bulk + d * w, p.c_bulk - d * w
    fd = -(PH.residual(pp, c, phi, c, np.inf) - PH.residual(pm, c, phi, c, np.inf)) / (2 * d)
    assert np.abs(fd - r).max() <= 1e-9


def test_the_two_methods_agree_far_inside_the_condition_of_the_device_tests(state_F, state_E, state_G):
    for case, p, c, phi in (state_F, state_E, state_G):
        specs = every_kind(p)
        dis = SR.disagreement(SR.sensitivities(p, c, phi, specs, p.flux, 'banded'), SR.sensitivities(p, c, phi, specs, p.flux, 'schur'))
        assert max(v.max() for v in dis.values()) < 1e-9, dis


# ---- the library -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_sens_library
    return build_sens_library()


@pytest.fixture(scope='module')
def sensitizer(libpath):
    with _sens.Sensitizer(0) as o:
        yield o


def header_source(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    declared = sorted(set(re.findall(r'\b(catsens_[a-z0-9_]+)\s*\(', header_source('catint_sens.h'))))
    assert declared == sorted(_sens.SYMBOLS) and len(declared) == 6
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(catsens_[a-z0-9_]+)\b', exported))) == declared
    assert not re.findall(r'\b(?:pnp|catresp|catkin|catcpl|catobs|catbal|catgrid|cateq)_[a-z0-9_]+\b', exported)     # none of another library


def test_the_sources_are_a_library_of_their_own():
    from catint_amd import build
    others = (build.SOURCES + build.OBSERVE_SOURCES + build.BALANCE_SOURCES + build.REGRID_SOURCES + build.EQUIL_SOURCES + build.RESPONSE_SOURCES
              + build.KINETICS_SOURCES + build.COUPLE_SOURCES)
    assert not any('catsens' in s or 'sens' in s for s in others)
    assert os.path.dirname(build.SENS_LIB) == os.path.dirname(build.LIB)
    assert build.SENS_SOURCES == ['catsens.hip'] and os.path.isdir(build.SENS_DIR) and callable(build.sens_needs_build)
    listed = {os.path.realpath(p) for p in build.SENS_HEADERS}
    assert {os.path.realpath(p) for p in build._TEAM_HEADERS} <= listed
    for h in ('catint_sens.h', 'catint_pnp.h'):
        assert os.path.realpath(os.path.join(ROOT, 'include', h)) in listed
    from tests.test_build_deps import reached
    sources = [os.path.join(build.SENS_DIR, f) for f in build.SENS_SOURCES]
    assert not reached(sources) - listed - {os.path.realpath(f) for f in sources}
    assert 'build_sens_library(' in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    from catint_amd import _capi
    assert not [s for s in _capi.SYMBOLS if 'catsens' in s or 'sens' in s] and hasattr(_capi.PnpSolver, 'get_sensitivities')


def header_structs():
    out = {}
    for body, struct in re.findall(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', header_source('catint_sens.h'), flags=re.S):
        fields = []
        for decl in body.split(';'):
            decl = decl.strip()
            if not decl:
                continue
            names = decl.split(None, 1)[1] if not decl.startswith('const') else decl.split(None, 2)[2]
            fields += [n.strip().lstrip('*').strip() for n in names.split(',')]
        out[struct] = fields
    return out


MACROS = (('maxnx', 'CATSENS_MAX_NX'), ('maxspecies', 'CATSENS_MAX_SPECIES'), ('maxparams', 'CATSENS_MAX_PARAMS'), ('chunk', 'CATSENS_CHUNK'),
          ('dirichlet', 'CATSENS_WALL_DIRICHLET'), ('stern', 'CATSENS_WALL_STERN'), ('einval', 'CATSENS_EINVAL'), ('enomem', 'CATSENS_ENOMEM'),
          ('edevice', 'CATSENS_EDEVICE'), ('nkinds', 'CATSENS_NKINDS'), ('phiM', 'CATSENS_PHIM'), ('flux', 'CATSENS_WALL_FLUX'),
          ('c_bulk', 'CATSENS_BULK_CONCENTRATION'), ('D', 'CATSENS_DIFFUSION'), ('kf', 'CATSENS_RATE_FORWARD'), ('kr', 'CATSENS_RATE_BACKWARD'),
          ('wall_k', 'CATSENS_WALL_RATE'), ('stern_capacitance', 'CATSENS_STERN_CAPACITANCE'), ('velocity', 'CATSENS_VELOCITY'),
          ('samelimits', 'CATSENS_MAX_NX == CATCPL_MAX_NX && CATSENS_MAX_SPECIES == CATCPL_MAX_SPECIES && '
                         'CATSENS_PIVOT_GROWTH_LIMIT == CATCPL_PIVOT_GROWTH_LIMIT && CATSENS_PIVOT_GROWTH_LIMIT == 1e8 && '
                         'CATSENS_PHIM == CATRESP_PHIM && CATSENS_WALL_FLUX == CATRESP_WALL_FLUX'))


@pytest.fixture(scope='module')
def compiler_layout(tmp_path_factory):
    structs = header_structs()
    assert set(PAIRS) <= set(structs)
    d = tmp_path_factory.mktemp('sens_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_sens.h"', '#include "catint_couple.h"', '#include "catint_response.h"',
             'int main(void) {']
    for s in PAIRS:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (s, s))
        for f in structs[s]:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    for name, macro in MACROS:
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
    cls = getattr(_sens, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_of_the_binding_are_the_header_s(compiler_layout):
    n = {k: v['n'] for k, v in compiler_layout.items() if 'n' in v}
    assert _sens.MAX_NX == n['maxnx'] == 4098 and _sens.MAX_SPECIES == n['maxspecies'] == 8 and _sens.MAX_PARAMS == n['maxparams'] == 64
    assert _sens.CHUNK == n['chunk'] == 8
    assert _sens.WALL == {'dirichlet': n['dirichlet'], 'stern': n['stern']}
    assert (_sens.EINVAL, _sens.ENOMEM, _sens.EDEVICE) == (n['einval'], n['enomem'], n['edevice'])
    assert _sens.KINDS == {k: n[k] for k in SR.KINDS} and len(_sens.KINDS) == n['nkinds'] and sorted(_sens.KINDS.values()) == list(range(9))
    assert n['samelimits'] == 1 and _sens.PIVOT_GROWTH_LIMIT == 1e8
    assert tuple(_sens.FIELDS) == SR.FIELDS


def fake_view(nx=16, N=2, B=2, phi=0x1000, size=None, status=0x1000):
    """A view no device stands behind: validation must reject it without reading it."""
    return _sens.PnpDeviceView(C.sizeof(_sens.PnpDeviceView) if size is None else size, 2, N, nx, (nx + 15) // 16 * 16, 0, B, 0x1000, phi,
                               status, None)


WALL2 = {'species': [0], 'nu': [[-1.0, 1.0]], 'k': [[1e-6], [1e-6]], 'alpha': None, 'saturation': None}


def good_args(view, n=None):
    nx, N, B = max(view.nx, 1), max(view.nspecies, 1), max(view.batch, 1)
    n = B if n is None else n
    return dict(D=np.full(N, 1e-9), charges=np.where(np.arange(N) % 2, -RC.F, RC.F), x=np.arange(nx) * 1e-9, beta=0.4, eps=RC.EPS, dx=1e-9,
                phiM=np.zeros(B), flux=np.zeros((n, N)), parameters=['phiM', ('c_bulk', 0)])


def call(sensitizer, view, **kw):
    args = good_args(view)
    args.update(kw)
    with pytest.raises(_sens.SensError) as e:
        sensitizer.solve(view, **args)
    return e.value


@pytest.mark.parametrize('what, make, word', [
    ('compat handle: no potential row', lambda: (fake_view(phi=None), {}), 'potential'),
    ('a view without a status row', lambda: (fake_view(status=None), {}), 'status row'),
    ('nx below 3', lambda: (fake_view(nx=2), {}), 'nx'),
    ('nx above 4098', lambda: (fake_view(nx=4099, B=1), {}), 'nx'),
    ('more than 8 species', lambda: (fake_view(N=9), {}), 'species'),
    ('x not increasing', lambda: (fake_view(), {'x': np.array([0.0, 1.0, 2.0, 2.0] + list(range(3, 15)), float)}), 'increasing'),
    ('struct_size of the parameters', lambda: (fake_view(), {'struct_size': 8}), 'catsens_params.struct_size'),
    ('struct_size of the outputs', lambda: (fake_view(), {'out_struct_size': 8}), 'catsens_outputs.struct_size'),
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
    ('a lane outside the batch', lambda: (fake_view(), {'lanes': [0, 2]}), 'lane index 2'),
    ('a negative lane', lambda: (fake_view(), {'lanes': [-1, 0]}), 'lane index -1'),
    ('a reaction that names species 2 of 2', lambda: (fake_view(), {'reactions': [([0], [2], 1.0, 1.0)]}), 'species index 2'),
    ('a reaction with five reactants', lambda: (fake_view(), {'reactions': [([0] * 5, [1], 1.0, 1.0)]}), 'n_lhs'),
    ('seventeen reactions', lambda: (fake_view(), {'reactions': [([0], [1], 1.0, 1.0)] * 17}), 'nreactions'),
    ('a wall reaction that names species 2 of 2', lambda: (fake_view(), {'wall': dict(WALL2, species=[2])}), 'wall reaction 0'),
    ('nine wall reactions', lambda: (fake_view(), {'wall': {'species': [0] * 9, 'nu': np.zeros((9, 2)), 'k': np.zeros((2, 9))}}), 'n_wall'),
    ('no parameters', lambda: (fake_view(), {'parameters': []}), 'nparams'),
    ('sixty-five parameters', lambda: (fake_view(), {'parameters': ['phiM'] * 65}), 'nparams'),
    ('an unknown kind', lambda: (fake_view(), {'parameters': ['phiM', (9, 0)]}), 'unknown kind 9'),
    ('a negative kind', lambda: (fake_view(), {'parameters': [(-1, 0)]}), 'unknown kind'),
    ('a flux of species 2 of 2', lambda: (fake_view(), {'parameters': [('flux', 2)]}), 'species index 2'),
    ('a bulk concentration of species -1', lambda: (fake_view(), {'parameters': [('c_bulk', -1)]}), 'species index -1'),
    ('a diffusion coefficient of species 2 of 2', lambda: (fake_view(), {'parameters': [('D', 2)]}), 'species index 2'),
    ('kf of reaction 0 of none', lambda: (fake_view(), {'parameters': [('kf', 0)]}), 'reaction index 0'),
    ('kr of reaction 1 of 1', lambda: (fake_view(), {'parameters': [('kr', 1)], 'reactions': [([0], [1], 1.0, 1.0)]}), 'reaction index 1'),
    ('a wall rate of reaction 0 of none', lambda: (fake_view(), {'parameters': [('wall_k', 0)]}), 'wall reaction index 0'),
    ('a wall rate of reaction 1 of 1', lambda: (fake_view(), {'parameters': [('wall_k', 1)], 'wall': WALL2}), 'wall reaction index 1'),
    ('the Stern capacitance of a Dirichlet wall', lambda: (fake_view(), {'parameters': ['stern_capacitance']}), 'Dirichlet wall'),
    ('no flux', lambda: (fake_view(), {'flux': None, 'lanes': [0, 1]}), 'flux is required'),
    ('a NaN phi_pzc', lambda: (fake_view(), {'phi_pzc': np.nan}), 'phi_pzc'),
    ('an infinite phi_pzc', lambda: (fake_view(), {'phi_pzc': np.inf}), 'phi_pzc'),
])
def test_validation_errors_come_before_any_device_call(sensitizer, what, make, word):
    view, kw = make()
    err = call(sensitizer, view, **kw)
    assert err.code == _sens.EINVAL, (what, str(err))
    assert word in str(err), (what, str(err))
    assert sensitizer.last_kernel == '' and sensitizer.last_kernel_ms == -1.0


def test_null_arguments_and_null_context(sensitizer, libpath):
    lib = _sens.load_library()
    p = _sens.CatsensParams(struct_size=C.sizeof(_sens.CatsensParams))
    o = _sens.CatsensOutputs(struct_size=C.sizeof(_sens.CatsensOutputs))
    v = fake_view()
    assert lib.catsens_solve(sensitizer._h, None, C.byref(p), C.byref(o)) == _sens.EINVAL
    assert b'null' in lib.catsens_last_error(sensitizer._h)
    assert lib.catsens_solve(sensitizer._h, C.byref(v), None, C.byref(o)) == _sens.EINVAL
    assert lib.catsens_solve(sensitizer._h, C.byref(v), C.byref(p), None) == _sens.EINVAL
    assert lib.catsens_solve(None, None, C.byref(p), C.byref(o)) == _sens.EINVAL
    assert lib.catsens_create(0, None) == _sens.EINVAL
    assert lib.catsens_last_kernel(sensitizer._h) == b''
    assert lib.catsens_solve(sensitizer._h, C.byref(v), C.byref(p), C.byref(o)) == _sens.EINVAL
    assert b'D, charges and x' in lib.catsens_last_error(sensitizer._h)
    a = good_args(v)
    p.D, p.charges, p.x = _sens._dptr(a['D']), _sens._dptr(a['charges']), _sens._dptr(a['x'])
    p.beta, p.eps, p.dx = 0.4, RC.EPS, 1e-9
    assert lib.catsens_solve(sensitizer._h, C.byref(v), C.byref(p), C.byref(o)) == _sens.EINVAL
    assert b'phiM is required' in lib.catsens_last_error(sensitizer._h)
    p.phiM = _sens._dptr(a['phiM'])
    p.nparams = 1
    assert lib.catsens_solve(sensitizer._h, C.byref(v), C.byref(p), C.byref(o)) == _sens.EINVAL
    assert b'kind and index' in lib.catsens_last_error(sensitizer._h)
    kind, index = _sens.encode(['phiM'])
    p.kind, p.index = _sens._iptr(kind), _sens._iptr(index)
    p.nlanes = -1
    assert lib.catsens_solve(sensitizer._h, C.byref(v), C.byref(p), C.byref(o)) == _sens.EINVAL
    assert b'nlanes' in lib.catsens_last_error(sensitizer._h)
    p.nlanes = 3
    assert lib.catsens_solve(sensitizer._h, C.byref(v), C.byref(p), C.byref(o)) == _sens.EINVAL
    assert b'nlanes above the batch' in lib.catsens_last_error(sensitizer._h)
    p.nlanes = 2
    assert lib.catsens_solve(sensitizer._h, C.byref(v), C.byref(p), C.byref(o)) == _sens.EINVAL
    assert b'flux is required' in lib.catsens_last_error(sensitizer._h)
    # every output NULL: nothing to do, and no device call
    p.flux = _sens._dptr(a['flux'])
    assert lib.catsens_solve(sensitizer._h, C.byref(v), C.byref(p), C.byref(o)) == 0
    assert lib.catsens_last_kernel(sensitizer._h) == b''


def test_an_empty_lane_list_makes_no_device_call(sensitizer):
    """nlanes == 0: valid, and done before the first device call (this machine may have no device at all)."""
    v = fake_view()
    out = sensitizer.solve(v, lanes=[], **good_args(v, 0))
    assert out['dc_surface'].shape == (0, 2, 2) and out['dphi_surface'].shape == (0, 2) and out['dcurrent'].shape == (0, 2)
    assert out['dwall_flux'].shape == (0, 2, 2) and out['status'].shape == (0,)
    assert sorted(out) == sorted(list(SR.FIELDS) + ['status'])
    assert sensitizer.last_kernel == ''


def test_compiled_kernels_are_the_eight_instances(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert len(INSTANCES) == 8
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)


def test_parameter_lists_are_encoded_as_the_header_numbers_them():
    kind, index = _sens.encode(['phiM', ('flux', 1), ('c_bulk', 2), ('D', 0), ('kf', 3), ('kr', 4), ('wall_k', 1), 'stern_capacitance', 'velocity'])
    assert kind.tolist() == list(range(9)) and index.tolist() == [0, 1, 2, 0, 3, 4, 1, 0, 0] and kind.dtype == index.dtype == np.int32
    for bad in ('D', 'phi', ('phiM', 0), ('rate', 1)):
        with pytest.raises(ValueError):
            _sens.encode([bad])


# ---- the calculator's opt-in path, with a fake solver ------------------------------------------------------------------------------
def ladder_parts():
    from tests.test_host_physical import LadderSolver, make_tp

    class SensLadderSolver(LadderSolver):
        """LadderSolver with get_sensitivities: records the call and returns recognisable numbers"""

        def get_state(self, potential=True, derived=True):
            return self.c.copy(), self.phi.copy(), np.zeros_like(self.phi), np.zeros_like(self.phi)

        def get_sensitivities(self, parameters, lanes=None, fields=None, flux=None, max_waves=0):
            self.calls.append(('get_sensitivities', list(parameters)))
            P, lane = len(parameters), (1.0 + np.arange(self.B))
            col = 1.0 + np.arange(P)
            base = lane[:, None] * col[None, :]
            return {'parameters': list(parameters), 'status': np.zeros(self.B, np.int32), 'dcurrent': 8.0 * base, 'dphi_surface': 0.5 * base,
                    'dsigma': 0.25 * base, 'dc_surface': base[:, :, None] * np.ones(3), 'dwall_flux': base[:, :, None] * np.ones(3),
                    'elasticity': {'dcurrent': 3.0 * base, 'dwall_flux': base[:, :, None] * np.ones(3)}}
    return SensLadderSolver, make_tp


def run_with(monkeypatch, newton, RF=None):
    from catint_amd.calculator import Calculator
    Solver, make_tp = ladder_parts()
    tp = make_tp(np.array([0.1, 0.2, 0.3]))
    tp.newton = newton
    if RF is not None:
        tp.system['RF'] = RF
    calc = Calculator(transport=tp, calc='comsol')
    made = []

    def fake(B, **kw):
        made.append(Solver(B, tp.nx, 3))
        return made[-1]
    monkeypatch.setattr(calc, '_physical_solver', fake)
    calc.run()
    assert len(made) == 1
    return calc, tp, made[0]


def test_without_the_option_nothing_changes(monkeypatch):
    runs, keys = [], []
    for newton in ({}, {'sensitivities': None}, {'sensitivities': []}):
        calc, tp, s = run_with(monkeypatch, newton)
        runs.append([c[0] for c in s.calls])
        keys.append(sorted(tp.alldata[0]['system']))
        assert calc.sensitivities is None and 'sensitivities' not in tp.alldata[0]['system']
    assert runs[0] == runs[1] == runs[2] == ['set_batch', 'solve'] and keys[0] == keys[1] == keys[2]


def test_with_the_option_one_call_after_the_solve_fills_the_keys(monkeypatch):
    calc0, tp0, _ = run_with(monkeypatch, {})
    names = list(tp0.species.keys())
    user = [('D', names[1]), ('flux', names[0]), 'phiM', ('wall_k', 0), ('c_bulk', 2)]
    calc, tp, s = run_with(monkeypatch, {'sensitivities': user})
    assert [c[0] for c in s.calls] == ['set_batch', 'solve', 'get_sensitivities']
    assert s.calls[-1][1] == [('D', 1), ('flux', 0), 'phiM', ('wall_k', 0), ('c_bulk', 2)]          # species by name -> index
    assert sorted(set(tp.alldata[0]['system']) - set(tp0.alldata[0]['system'])) == ['sensitivities']
    col = 1.0 + np.arange(5)
    for b in range(3):
        d = tp.alldata[b]['system']['sensitivities']
        assert sorted(d) == ['dcurrent_density', 'dsurface_charge', 'dsurface_concentration', 'dsurface_potential', 'elasticity', 'parameters']
        assert d['parameters'] == user
        assert np.array_equal(d['dcurrent_density'], 8.0 * (b + 1) * col) and np.array_equal(d['dsurface_potential'], 0.5 * (b + 1) * col)
        assert np.array_equal(d['dsurface_charge'], 0.25 * (b + 1) * col) and d['dsurface_concentration'].shape == (5, 3)
        assert np.array_equal(d['elasticity']['dcurrent'], 3.0 * (b + 1) * col)
    # RF = 2: the solver was handed RF * flux and RF * k.  Per geometric area the current is divided by RF; a derivative with respect
    # to the user's flux or wall rate constant is chained with RF; elasticities are unchanged
    calc, tp, s = run_with(monkeypatch, {'sensitivities': user}, RF=2.0)
    chain = np.array([1.0, 2.0, 1.0, 2.0, 1.0])
    for b in range(3):
        d = tp.alldata[b]['system']['sensitivities']
        assert np.array_equal(d['dcurrent_density'], 8.0 * (b + 1) * col * chain / 2.0)
        assert np.array_equal(d['dsurface_potential'], 0.5 * (b + 1) * col * chain)
        assert np.array_equal(d['dsurface_concentration'], ((b + 1) * col * chain)[:, None] * np.ones(3))
        assert np.array_equal(d['dsurface_charge'], 0.25 * (b + 1) * col * chain)
        assert np.array_equal(d['elasticity']['dcurrent'], 3.0 * (b + 1) * col)


def test_the_option_belongs_to_the_physical_mode():
    from catint_amd.calculator import Calculator, CalculatorError
    _, make_tp = ladder_parts()
    tp = make_tp(np.array([0.1]))
    tp.newton = {'sensitivities': ['phiM']}
    with pytest.raises(CalculatorError, match='physical mode'):
        Calculator(transport=tp, calc='Crank-Nicolson', dt=1e-9, tmax=1e-8)
    Calculator(transport=tp, calc='comsol')
    tp2 = make_tp(np.array([0.1]))
    calc = Calculator(transport=tp2, calc='Crank-Nicolson', dt=1e-9, tmax=1e-8)
    tp2.newton = {'sensitivities': ['phiM']}
    with pytest.raises(CalculatorError, match='physical mode'):
        calc.run()
    tp3 = make_tp(np.array([0.1]))
    tp3.newton = {'sensitivities': [('D', 'no such species')]}
    with pytest.raises(CalculatorError, match='names no species'):
        Calculator(transport=tp3, calc='comsol')
