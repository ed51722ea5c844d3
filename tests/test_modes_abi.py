"""libcatint_modes without a device: the NumPy restatement of include/catint_modes.h (tests/modes_ref.py) against a dense eigensolver and
against the oracle's own backward-Euler step, the library's ABI, its validation, its kernel set, and the calculator's opt-in path with a
fake solver.

(a) The Ritz values of the reference that have converged are eigenvalues of the dense A = solve(J, diag(S)), and the largest ones.
(b) One backward-Euler step of the oracle with dt = 1 / lambda halves a perturbation along a mode, up to a term linear in its amplitude."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from catint_amd import _modes          # fails without the feature
from oracle import pnp_physical as PH
from tests import kernel_census as K
from tests import modes_ref as MR
from tests import response_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {'catmodes_params': 'CatmodesParams', 'catmodes_outputs': 'CatmodesOutputs'}
INSTANCES = {'catmodes::modes_kernel<%d, 8>' % nb for nb in range(2, 10)}
FLUX_F = np.array([0.0, -1e-6, 1e-6])
FLUX_G = np.array([0.0, -1e-6, 1e-6, 0.0])          # case G: general reaction and wall tables
SUBSPACE, ITERATIONS = 8, 12          # the defaults of PnpSolver.get_relaxation


def cpu_cases():
    return {'N=2 nx=33 stern': (RC.small(2, 33, stern=True), None), 'N=3 nx=48 stern steric': (RC.small(3, 48, stern=True, steric=True), None),
            'F': (RC.case_F(), FLUX_F), 'E': (RC.case_E(34), None), 'G': (RC.case_G(21), FLUX_G)}


_states = {}


def state(name):
    if name not in _states:
        case, flux = cpu_cases()[name]
        _states[name] = case.solve(flux=flux)
    return _states[name]


@pytest.mark.parametrize('name', sorted(cpu_cases()))
def test_converged_ritz_values_are_the_largest_dense_eigenvalues(name):
    """(a) Subspace 8, 12 passes, the start vectors of the binding.  Every Ritz value with residual <= 1e-8 lies within
    10 kappa_j residual_j |theta_j| of a dense eigenvalue (kappa_j: the condition number of that eigenvalue from the dense left and right
    eigenvectors), no two of them claim the same one, and the ones they claim are the largest in modulus; at least the three slowest
    rates have converged; with both solution methods.
    The slowest pairs converge to residuals of 1e-15, below the rounding error eps cond(J) of a plain solve (the two plain methods differ
    by 5.6e-14 |theta| on case F, 7 times the bound), so both sides of this comparison solve with two steps of iterative refinement
    (tests/modes_ref.py: solve).  Measured then: |theta - dense| / bound at most 0.28; the plain solves give the same converged values
    to 1.6e-11 |theta| (asserted below 1e-10)."""
    p, c, phi = state(name)
    dth, kap = MR.dense(p, c, phi)
    start = _modes.default_start(SUBSPACE, p.N, p.nx, 0)
    plain = {}
    for method in MR.METHODS:
        ref = MR.iterate(p, c, phi, start, ITERATIONS, method, refine=2)
        assert not ref['breakdown']
        theta, s, res = MR.ritz_pairs(ref['ritz'], ref['gram'])
        ok = np.flatnonzero(res <= 1e-8)
        assert len(ok) >= 3 and np.array_equal(ok, np.arange(len(ok))), res
        hit = MR.match(theta[ok], dth)
        err = np.abs(theta[ok] - dth[hit])
        bound = 10.0 * kap[hit] * res[ok] * np.abs(theta[ok])
        print('%s, %s: %d converged; |theta - dense| / bound: %s; residuals %s' % (name, method, len(ok), err / bound, res[ok]))
        assert len(set(hit)) == len(hit)
        assert (np.abs(dth[hit]) >= np.abs(dth[len(ok) - 1]) * (1.0 - 1e-12)).all(), hit
        assert (err <= bound).all(), (method, err / bound)
        # the plain solves, which the device is compared with, give the same values to the rounding error of a solve
        t0 = MR.ritz_pairs(*MR.iterate(p, c, phi, start, ITERATIONS, method)['history'][-1])[0]
        plain[method] = np.abs(t0[ok] - theta[ok]).max() / np.abs(theta[ok]).min()
    print('%s: plain against refined solves, relative difference of the converged Ritz values: %s' % (name, plain))
    assert max(plain.values()) < 1e-10


def slowest_real_mode(p, c, phi):
    """(lambda, dc [N][nx], dphi [nx]) of the slowest converged real mode, scaled so that the largest relative change of a concentration is 1"""
    ref = MR.iterate(p, c, phi, _modes.default_start(SUBSPACE, p.N, p.nx, 0), ITERATIONS)
    theta, s, res = MR.ritz_pairs(ref['ritz'], ref['gram'])
    j = [j for j in range(len(theta)) if res[j] <= 1e-8 and theta[j].imag == 0.0][0]
    v = np.einsum('jke,j->ke', ref['basis'], s[:, j].real)
    v = v / np.abs(v[:p.N] / c).max()
    return 1.0 / theta[j].real, v[:p.N], v[p.N]


def halving_deviation(step, c, phi, dc, dphi, eps):
    """max-norm of (state after one step from u* + eps mode) - u* - eps mode / 2 over the concentrations, relative to eps mode / 2"""
    c1, _ = step(c + eps * dc, phi + eps * dphi)
    return np.abs((c1 - c) - 0.5 * eps * dc).max() / np.abs(0.5 * eps * dc).max()


def test_one_backward_euler_step_of_the_oracle_halves_a_mode():
    """(b) S (u1 - u0) / dt + F(u1) = 0 from u0 = u* + eps v with J v = lambda S v and dt = 1 / lambda leaves u1 = u* + eps v / 2 to first
    order, in every unknown (the potential of u0 does not enter).  The deviation is the second-order term, linear in eps: between eps =
    1e-3 and 1e-4 it falls by a factor within [8, 12].  Measured: 3.611e-5 and 3.611e-6, ratio 10.00 (N = 3, nx = 48, Stern wall,
    steric ions, lambda_1 = 6.27e6 1/s)."""
    name = 'N=3 nx=48 stern steric'
    p, c, phi = state(name)
    lam, dc, dphi = slowest_real_mode(p, c, phi)
    assert lam > 0

    def step(c0, phi0):
        c1, phi1, it, _ = PH.newton_step(p, c0, phi0, c0, 1.0 / lam, tol=1e-13, maxit=80)
        assert it <= 80
        return c1, phi1
    d3, d4 = halving_deviation(step, c, phi, dc, dphi, 1e-3), halving_deviation(step, c, phi, dc, dphi, 1e-4)
    print('%s: lambda = %.6e 1/s; deviation from one half %.3e at eps = 1e-3, %.3e at 1e-4, ratio %.2f' % (name, lam, d3, d4, d3 / d4))
    assert 1.0 / 12.0 <= d4 / d3 <= 1.0 / 8.0, (d3, d4)
    assert d3 < 1e-2


def test_the_reference_reports_a_breakdown_for_equal_start_columns():
    p, c, phi = state('N=2 nx=33 stern')
    start = _modes.default_start(4, p.N, p.nx, 0)
    start[2] = start[0]
    assert MR.iterate(p, c, phi, start, 2)['breakdown'] and not MR.iterate(p, c, phi, _modes.default_start(4, p.N, p.nx, 0), 2)['breakdown']


def test_the_binding_s_eigenproblem_is_the_reference_s():
    p, c, phi = state('F')
    ref = MR.iterate(p, c, phi, _modes.default_start(SUBSPACE, p.N, p.nx, 0), ITERATIONS)
    a, b = _modes.ritz_pairs(ref['ritz'], ref['gram']), MR.ritz_pairs(ref['ritz'], ref['gram'])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    bad = ref['ritz'].copy()
    bad[0, 0] = np.nan
    assert all(np.isnan(x).all() for x in _modes.ritz_pairs(bad, ref['gram']))


# ---- the library -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_modes_library
    return build_modes_library()


@pytest.fixture(scope='module')
def solver(libpath):
    with _modes.ModeSolver(0) as o:
        yield o


def header_source(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    declared = sorted(set(re.findall(r'\b(catmodes_[a-z0-9_]+)\s*\(', header_source('catint_modes.h'))))
    assert declared == sorted(_modes.SYMBOLS) and len(declared) == 6
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(catmodes_[a-z0-9_]+)\b', exported))) == declared
    assert not re.findall(r'\b(?:pnp|catresp|catkin|catcpl|catobs|catbal|catgrid|cateq|catsens|catdrc)_[a-z0-9_]+\b', exported)     # none of another library


def test_the_sources_are_a_library_of_their_own():
    from catint_amd import build
    others = (build.SOURCES + build.OBSERVE_SOURCES + build.BALANCE_SOURCES + build.REGRID_SOURCES + build.EQUIL_SOURCES + build.RESPONSE_SOURCES
              + build.KINETICS_SOURCES + build.COUPLE_SOURCES + build.SENS_SOURCES + build.DRC_SOURCES)
    assert not any('modes' in s for s in others)
    assert os.path.dirname(build.MODES_LIB) == os.path.dirname(build.LIB)
    assert build.MODES_SOURCES == ['catmodes.hip'] and os.path.isdir(build.MODES_DIR) and callable(build.modes_needs_build)
    listed = {os.path.realpath(p) for p in build.MODES_HEADERS}
    assert {os.path.realpath(p) for p in build._TEAM_HEADERS} <= listed
    for h in ('catint_modes.h', 'catint_pnp.h'):
        assert os.path.realpath(os.path.join(ROOT, 'include', h)) in listed
    from tests.test_build_deps import reached
    sources = [os.path.join(build.MODES_DIR, f) for f in build.MODES_SOURCES]
    assert not reached(sources) - listed - {os.path.realpath(f) for f in sources}
    assert 'build_modes_library(' in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    from catint_amd import _capi
    assert not [s for s in _capi.SYMBOLS if 'catmodes' in s or 'modes' in s] and hasattr(_capi.PnpSolver, 'get_relaxation')


def header_structs():
    out = {}
    for body, struct in re.findall(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', header_source('catint_modes.h'), flags=re.S):
        fields = []
        for decl in body.split(';'):
            decl = decl.strip()
            if not decl:
                continue
            names = decl.split(None, 1)[1] if not decl.startswith('const') else decl.split(None, 2)[2]
            fields += [n.strip().lstrip('*').strip() for n in names.split(',')]
        out[struct] = fields
    return out


MACROS = (('maxnx', 'CATMODES_MAX_NX'), ('maxspecies', 'CATMODES_MAX_SPECIES'), ('maxsubspace', 'CATMODES_MAX_SUBSPACE'),
          ('maxiterations', 'CATMODES_MAX_ITERATIONS'), ('dirichlet', 'CATMODES_WALL_DIRICHLET'), ('stern', 'CATMODES_WALL_STERN'),
          ('einval', 'CATMODES_EINVAL'), ('enomem', 'CATMODES_ENOMEM'), ('edevice', 'CATMODES_EDEVICE'),
          ('samelimits', 'CATMODES_MAX_NX == CATSENS_MAX_NX && CATMODES_MAX_SPECIES == CATSENS_MAX_SPECIES && '
                         'CATMODES_PIVOT_GROWTH_LIMIT == CATRESP_PIVOT_GROWTH_LIMIT && CATMODES_PIVOT_GROWTH_LIMIT == 1e8 && '
                         'CATMODES_MAX_SUBSPACE == CATSENS_CHUNK && CATMODES_BREAKDOWN == 1e-10 && '
                         'CATMODES_WALL_STERN == CATRESP_WALL_STERN && CATMODES_WALL_DIRICHLET == CATRESP_WALL_DIRICHLET'))


@pytest.fixture(scope='module')
def compiler_layout(tmp_path_factory):
    structs = header_structs()
    assert set(PAIRS) <= set(structs)
    d = tmp_path_factory.mktemp('modes_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_modes.h"', '#include "catint_sens.h"', '#include "catint_response.h"',
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
    cls = getattr(_modes, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_of_the_binding_are_the_header_s(compiler_layout):
    n = {k: v['n'] for k, v in compiler_layout.items() if 'n' in v}
    assert _modes.MAX_NX == n['maxnx'] == 4098 and _modes.MAX_SPECIES == n['maxspecies'] == 8
    assert _modes.MAX_SUBSPACE == n['maxsubspace'] == 8 and _modes.MAX_ITERATIONS == n['maxiterations'] == 64
    assert _modes.WALL == {'dirichlet': n['dirichlet'], 'stern': n['stern']}
    assert (_modes.EINVAL, _modes.ENOMEM, _modes.EDEVICE) == (n['einval'], n['enomem'], n['edevice'])
    assert n['samelimits'] == 1 and _modes.PIVOT_GROWTH_LIMIT == 1e8 and _modes.BREAKDOWN == MR.BREAKDOWN == 1e-10
    assert tuple(_modes.FIELDS) == ('ritz', 'gram', 'basis')
    assert (_modes.OK, _modes.PIVOT, _modes.UNSOLVED, _modes.BREAKDOWN_STATUS) == (0, 1, 2, 3)


def fake_view(nx=16, N=2, B=2, phi=0x1000, size=None, status=0x1000):
    """A view no device stands behind: validation must reject it without reading it."""
    return _modes.PnpDeviceView(C.sizeof(_modes.PnpDeviceView) if size is None else size, 2, N, nx, (nx + 15) // 16 * 16, 0, B, 0x1000, phi,
                                status, None)


WALL2 = {'species': [0], 'nu': [[-1.0, 1.0]], 'k': [[1e-6], [1e-6]], 'alpha': None, 'saturation': None}


def good_args(view, m=2):
    nx, N, B = max(view.nx, 1), max(view.nspecies, 1), max(view.batch, 1)
    return dict(D=np.full(N, 1e-9), charges=np.where(np.arange(N) % 2, -RC.F, RC.F), x=np.arange(nx) * 1e-9, beta=0.4, eps=RC.EPS, dx=1e-9,
                phiM=np.zeros(B), start=np.ones((m, N + 1, nx)), iterations=2)


def call(solver, view, **kw):
    args = good_args(view, kw.pop('m', 2))
    args.update(kw)
    with pytest.raises(_modes.ModesError) as e:
        solver.solve(view, **args)
    return e.value


@pytest.mark.parametrize('what, make, word', [
    ('compat handle: no potential row', lambda: (fake_view(phi=None), {}), 'potential'),
    ('a view without a status row', lambda: (fake_view(status=None), {}), 'status row'),
    ('nx below 3', lambda: (fake_view(nx=2), {}), 'nx'),
    ('nx above 4098', lambda: (fake_view(nx=4099, B=1), {}), 'nx'),
    ('more than 8 species', lambda: (fake_view(N=9), {}), 'species'),
    ('x not increasing', lambda: (fake_view(), {'x': np.array([0.0, 1.0, 2.0, 2.0] + list(range(3, 15)), float)}), 'increasing'),
    ('struct_size of the parameters', lambda: (fake_view(), {'struct_size': 8}), 'catmodes_params.struct_size'),
    ('struct_size of the outputs', lambda: (fake_view(), {'out_struct_size': 8}), 'catmodes_outputs.struct_size'),
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
    ('a subspace of 0', lambda: (fake_view(), {'subspace': 0}), 'subspace = 0'),
    ('a subspace of 9', lambda: (fake_view(), {'subspace': 9}), 'subspace = 9'),
    ('a negative subspace', lambda: (fake_view(), {'subspace': -1}), 'subspace = -1'),
    ('a subspace above the rank of S', lambda: (fake_view(nx=3, N=2), {'m': 5}), 'rank of S'),
    ('no passes', lambda: (fake_view(), {'iterations': 0}), 'iterations = 0'),
    ('sixty-five passes', lambda: (fake_view(), {'iterations': 65}), 'iterations = 65'),
    ('no start vectors', lambda: (fake_view(), {'start': None, 'subspace': 2}), 'start is required'),
])
def test_validation_errors_come_before_any_device_call(solver, what, make, word):
    view, kw = make()
    err = call(solver, view, **kw)
    assert err.code == _modes.EINVAL, (what, str(err))
    assert word in str(err), (what, str(err))
    assert solver.last_kernel == '' and solver.last_kernel_ms == -1.0


def test_the_largest_admitted_subspace_passes_validation(solver):
    """m = N (nx - 1) = 4 at nx = 3 is not rejected: with no lane selected the call returns before any device call"""
    v = fake_view(nx=3, N=2)
    out = solver.solve(v, lanes=[], **good_args(v, 4))
    assert out['ritz'].shape == (0, 4, 4) and solver.last_kernel == ''


def test_null_arguments_and_null_context(solver, libpath):
    lib = _modes.load_library()
    p = _modes.CatmodesParams(struct_size=C.sizeof(_modes.CatmodesParams))
    o = _modes.CatmodesOutputs(struct_size=C.sizeof(_modes.CatmodesOutputs))
    v = fake_view()
    assert lib.catmodes_solve(solver._h, None, C.byref(p), C.byref(o)) == _modes.EINVAL
    assert b'null' in lib.catmodes_last_error(solver._h)
    assert lib.catmodes_solve(solver._h, C.byref(v), None, C.byref(o)) == _modes.EINVAL
    assert lib.catmodes_solve(solver._h, C.byref(v), C.byref(p), None) == _modes.EINVAL
    assert lib.catmodes_solve(None, None, C.byref(p), C.byref(o)) == _modes.EINVAL
    assert lib.catmodes_create(0, None) == _modes.EINVAL
    assert lib.catmodes_last_kernel(solver._h) == b''
    assert lib.catmodes_solve(solver._h, C.byref(v), C.byref(p), C.byref(o)) == _modes.EINVAL
    assert b'D, charges and x' in lib.catmodes_last_error(solver._h)
    a = good_args(v)
    p.D, p.charges, p.x = _modes._dptr(a['D']), _modes._dptr(a['charges']), _modes._dptr(a['x'])
    p.beta, p.eps, p.dx = 0.4, RC.EPS, 1e-9
    assert lib.catmodes_solve(solver._h, C.byref(v), C.byref(p), C.byref(o)) == _modes.EINVAL
    assert b'phiM is required' in lib.catmodes_last_error(solver._h)
    p.phiM = _modes._dptr(a['phiM'])
    assert lib.catmodes_solve(solver._h, C.byref(v), C.byref(p), C.byref(o)) == _modes.EINVAL
    assert b'subspace' in lib.catmodes_last_error(solver._h)
    p.subspace = 2
    assert lib.catmodes_solve(solver._h, C.byref(v), C.byref(p), C.byref(o)) == _modes.EINVAL
    assert b'iterations' in lib.catmodes_last_error(solver._h)
    p.iterations = 3
    p.nlanes = -1
    assert lib.catmodes_solve(solver._h, C.byref(v), C.byref(p), C.byref(o)) == _modes.EINVAL
    assert b'nlanes' in lib.catmodes_last_error(solver._h)
    p.nlanes = 3
    assert lib.catmodes_solve(solver._h, C.byref(v), C.byref(p), C.byref(o)) == _modes.EINVAL
    assert b'nlanes above the batch' in lib.catmodes_last_error(solver._h)
    p.nlanes = 2
    assert lib.catmodes_solve(solver._h, C.byref(v), C.byref(p), C.byref(o)) == _modes.EINVAL
    assert b'start is required' in lib.catmodes_last_error(solver._h)
    # every output NULL: nothing to do, and no device call
    p.start = _modes._dptr(a['start'])
    assert lib.catmodes_solve(solver._h, C.byref(v), C.byref(p), C.byref(o)) == 0
    assert lib.catmodes_last_kernel(solver._h) == b''


def test_an_empty_lane_list_makes_no_device_call(solver):
    """nlanes == 0: valid, and done before the first device call (this machine may have no device at all)."""
    v = fake_view()
    out = solver.solve(v, lanes=[], fields=['ritz', 'gram', 'basis'], **good_args(v))
    assert out['ritz'].shape == (0, 2, 2) and out['gram'].shape == (0, 2, 2) and out['basis'].shape == (0, 2, 3, 16) and out['status'].shape == (0,)
    assert sorted(out) == ['basis', 'gram', 'ritz', 'status']
    assert solver.last_kernel == ''


def test_compiled_kernels_are_the_eight_instances(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert len(INSTANCES) == 8
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)


def test_the_default_start_is_seeded_and_shared():
    a, b = _modes.default_start(8, 3, 48, 0), _modes.default_start(8, 3, 48, 0)
    assert a.shape == (8, 4, 48) and np.array_equal(a, b) and not np.array_equal(a, _modes.default_start(8, 3, 48, 1))
    assert not MR.orth(a)[1]


# ---- the calculator's opt-in path, with a fake solver ------------------------------------------------------------------------------
def ladder_parts():
    from tests.test_host_physical import LadderSolver, make_tp

    class ModesLadderSolver(LadderSolver):
        """LadderSolver with get_relaxation: records the call and returns recognisable numbers"""

        def get_state(self, potential=True, derived=True):
            return self.c.copy(), self.phi.copy(), np.zeros_like(self.phi), np.zeros_like(self.phi)

        def get_relaxation(self, nmodes=3, **kw):
            self.calls.append(('get_relaxation', dict(kw, nmodes=nmodes)))
            lane = 1.0 + np.arange(self.B)
            rates = lane[:, None] * (1.0 + np.arange(nmodes))[None, :] * (1e6 + 0j)
            stable = np.array([True, False, None][:self.B] + [None] * max(0, self.B - 3), dtype=object)
            return {'rates': rates, 'time_constants': 1.0 / rates.real, 'residual': np.full((self.B, nmodes), 1e-12),
                    'converged': np.ones((self.B, nmodes), bool), 'stable': stable, 'status': np.zeros(self.B, np.int32),
                    'ritz': np.zeros((self.B, 8, 8)), 'gram': np.zeros((self.B, 8, 8))}
    return ModesLadderSolver, make_tp


def run_with(monkeypatch, newton):
    from catint_amd.calculator import Calculator
    Solver, make_tp = ladder_parts()
    tp = make_tp(np.array([0.1, 0.2, 0.3]))
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


def test_without_the_option_nothing_changes(monkeypatch):
    runs, keys = [], []
    for newton in ({}, {'relaxation': None}, {'relaxation': False}):
        calc, tp, s = run_with(monkeypatch, newton)
        runs.append([c[0] for c in s.calls])
        keys.append(sorted(tp.alldata[0]['system']))
        assert calc.relaxation is None and 'relaxation' not in tp.alldata[0]['system']
    assert runs[0] == runs[1] == runs[2] == ['set_batch', 'solve'] and keys[0] == keys[1] == keys[2]


def test_with_the_option_one_call_after_the_solve_fills_the_key(monkeypatch):
    calc0, tp0, _ = run_with(monkeypatch, {})
    calc, tp, s = run_with(monkeypatch, {'relaxation': True})
    assert [c[0] for c in s.calls] == ['set_batch', 'solve', 'get_relaxation'] and s.calls[-1][1] == {'nmodes': 3}
    assert sorted(set(tp.alldata[0]['system']) - set(tp0.alldata[0]['system'])) == ['relaxation']
    for b in range(3):
        d = tp.alldata[b]['system']['relaxation']
        assert sorted(d) == ['converged', 'rates', 'residual', 'stable', 'status', 'time_constants']
        assert np.array_equal(d['rates'], (b + 1) * np.array([1e6, 2e6, 3e6]) + 0j) and d['status'] == 0
        assert d['stable'] is [True, False, None][b]
    calc, tp, s = run_with(monkeypatch, {'relaxation': {'nmodes': 2, 'iterations': 20, 'rtol': 1e-6}})
    assert s.calls[-1][1] == {'nmodes': 2, 'iterations': 20, 'rtol': 1e-6}
    assert tp.alldata[1]['system']['relaxation']['rates'].shape == (2,)


def test_the_option_belongs_to_the_physical_mode():
    from catint_amd.calculator import Calculator, CalculatorError
    _, make_tp = ladder_parts()
    tp = make_tp(np.array([0.1]))
    tp.newton = {'relaxation': True}
    with pytest.raises(CalculatorError, match='physical mode'):
        Calculator(transport=tp, calc='Crank-Nicolson', dt=1e-9, tmax=1e-8)
    Calculator(transport=tp, calc='comsol')
    tp2 = make_tp(np.array([0.1]))
    calc = Calculator(transport=tp2, calc='Crank-Nicolson', dt=1e-9, tmax=1e-8)
    tp2.newton = {'relaxation': {'nmodes': 2}}
    with pytest.raises(CalculatorError, match='physical mode'):
        calc.run()
    tp3 = make_tp(np.array([0.1]))
    tp3.newton = {'relaxation': {'modes': 2}}
    with pytest.raises(CalculatorError, match='unknown argument'):
        Calculator(transport=tp3, calc='comsol')
