"""libcatint_regrid on the device (PnpSolver.resample / resample_to / set_lanes_device, Calculator's tp.newton['coarse_nx']) against the
NumPy restatement of include/catint_regrid.h in tests/test_regrid_abi.py.

Tolerances.  Parity: the result is a convex combination H c_e + G c_{e+1} of two positive values with G, H from four exponentials and
two quotients each; device and NumPy differ in the exponential (<= 2 ulp against libm) and the reciprocal (1.1e-16), and an error d of
the argument u ~ 20 (itself a sum with rounding errors ~ 20 * 1.1e-16) moves exp by d: a few 1e-15 relative in all.  The project's fp64
parity tolerance 1e-9 is asserted, per element, relative to the value itself (no cancellation: the value is its own scale); the
potential to 1e-9 (|phi_e| + |phi_{e+1}|).  The worst ratio is printed.  Everything else that can be exact is asserted bit for bit."""
import importlib.util
import os

import numpy as np
import pytest

from catint_amd import PnpSolver, _regrid          # fails without the feature
from catint_amd.host import graded_mesh
from catint_amd.units import unit_F, unit_R, unit_eps0
from tests.test_regrid_abi import bernoulli, cell_table, resample_ref

pytestmark = pytest.mark.gpu

BETA = 1.0 / (unit_R * 298.15)
EPS = 78.36 * unit_eps0
TOL = 1e-9
B, N = 5, 3
Z = np.array([1.0, -1.0, 2.0])
Q = Z * unit_F
D = 1e-9 * (1.0 + 0.3 * np.arange(N))
RADII = 3e-10 * (1.0 + 0.1 * np.arange(N))


def source_grid(nx):
    return np.concatenate([[0.0], np.cumsum(1e-10 * 1.04 ** np.minimum(np.arange(nx - 1), 150))])


def target_grid(x, nxt):
    """Another grading of the same interval: no target point but the two ends is a source node"""
    xt = x[0] + (x[-1] - x[0]) * np.linspace(0.0, 1.0, nxt) ** 1.7
    xt[-1] = x[-1]
    return xt


def nested(x):
    """Midpoint refinement: 2 nx - 1 points, every other one a source node"""
    xt = np.empty(2 * len(x) - 1)
    xt[0::2] = x
    xt[1::2] = 0.5 * (x[:-1] + x[1:])
    return xt


def state(nx, seed=0):
    """Smooth positive concentrations; a random-walk potential whose steps reach 0.25 V: |u| up to 19.5 for the divalent ion"""
    rng = np.random.RandomState(100 * nx + seed)
    s = np.linspace(0.0, 1.0, nx)
    f = rng.uniform(0.5, 3.0, (B, N, 1))
    p = rng.uniform(0.0, 2 * np.pi, (B, N, 1))
    cb = 10.0 * (1.0 + np.arange(N))[None, :, None] * rng.uniform(0.5, 1.5, (B, N, 1))
    c = cb * np.exp(0.5 * np.sin(2 * np.pi * f * s[None, None, :] + p))
    steps = rng.uniform(0.0, 0.25, (B, nx)) * rng.choice([-1.0, 1.0], (B, nx))
    steps[:, 1] = 0.25
    return np.ascontiguousarray(c), np.ascontiguousarray(np.cumsum(steps, axis=1))


_handles = {}


@pytest.fixture(scope='module')
def handle():
    """handle(nx) -> (solver holding state(nx), c, phi): one handle per source grid, shared by the tests (the physics go to the library
    with every call: the handle is only the owner of the state)"""
    def get(nx):
        if nx not in _handles:
            x = source_grid(nx)
            s = PnpSolver(N, nx, float(x[1] - x[0]), 1.0, BETA, EPS, D, Q, method='Newton', batch_capacity=B)
            s.set_newton(wall_bc='stern', stern_capacitance=0.2)
            s.set_grid(x)
            c, phi = state(nx)
            s.set_batch(c, np.zeros((B, 4)), np.zeros(B), np.zeros((B, N)))
            s.set_potential(phi)
            _handles[nx] = (s, c, phi)
        return _handles[nx]
    yield get
    for s, _, _ in _handles.values():
        s.close()
    _handles.clear()


@pytest.fixture(scope='module')
def regridder():
    with _regrid.Regridder(0) as r:
        yield r


def waves_of(nx, nxt):
    big = max(nx, nxt)
    return 1 if big <= 1026 else 2 if big <= 2050 else 4


def reference(x, c, phi, xt, steric, velocity, lanes=None):
    lanes = range(len(c)) if lanes is None else lanes
    out = [resample_ref(x, c[b], phi[b], xt, Q, BETA, D, velocity, RADII if steric else None) for b in lanes]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# every instance at its smallest grid pair
PAIRS = [(10, 19), (66, 130), (130, 66), (1030, 70), (70, 1030), (66, 2052), (4098, 3)]


@pytest.mark.parametrize('steric, velocity', [(False, 0.0), (True, 0.0), (False, 0.3), (True, -0.2)])
@pytest.mark.parametrize('nx, nxt', PAIRS)
def test_parity_with_the_restatement(handle, regridder, nx, nxt, steric, velocity):
    s, c, phi = handle(nx)
    x = source_grid(nx)
    xt = target_grid(x, nxt)
    wy = waves_of(nx, nxt)
    got = regridder.resample(s.device_view(), D, Q, x, BETA, xt, mpb_radius=RADII if steric else None, velocity=velocity, max_waves=wy)
    assert regridder.last_kernel == 'catgrid::regrid_kernel<%d, %s>' % (wy, 'true' if steric else 'false')
    assert regridder.last_kernel_ms > 0.0
    want_c, want_phi = reference(x, c, phi, xt, steric, velocity)
    e, _ = cell_table(x, xt)
    f = np.minimum(e + 1, nx - 1)
    umax = np.abs(Q[None, :, None] * BETA * (phi[:, None, f] - phi[:, None, e])).max()
    err_c = np.abs(got['c'] - want_c) / np.abs(want_c)
    scale_phi = np.abs(phi[:, e]) + np.abs(phi[:, f])
    err_phi = np.abs(got['phi'] - want_phi) / np.where(scale_phi > 0, scale_phi, 1.0)
    print('%d -> %d steric=%s velocity=%g: largest |u| %.1f; c %.2e, phi %.2e of their scales' % (nx, nxt, steric, velocity, umax, err_c.max(),
                                                                                               err_phi.max()))
    assert (got['c'] > 0).all() and np.isfinite(got['c']).all()
    assert err_c.max() <= TOL and err_phi.max() <= TOL
    assert umax >= (15.0 if nxt > 3 else 0.0)


def test_the_cases_reach_every_instance():
    from tests.test_regrid_abi import INSTANCES
    assert {'catgrid::regrid_kernel<%d, %s>' % (waves_of(a, b), s) for a, b in PAIRS for s in ('false', 'true')} == INSTANCES


@pytest.mark.parametrize('nx', [10, 66, 1030])
@pytest.mark.parametrize('steric', [False, True])
def test_own_grid_and_nested_nodes_bit_for_bit(handle, regridder, nx, steric):
    s, c, phi = handle(nx)
    x = source_grid(nx)
    kw = dict(mpb_radius=RADII if steric else None, velocity=0.1)
    own = regridder.resample(s.device_view(), D, Q, x, BETA, x, **kw)
    assert np.array_equal(own['c'], c) and np.array_equal(own['phi'], phi)
    fine = regridder.resample(s.device_view(), D, Q, x, BETA, nested(x), **kw)
    assert np.array_equal(fine['c'][:, :, 0::2], c) and np.array_equal(fine['phi'][:, 0::2], phi)
    lo, hi = np.minimum(c[:, :, :-1], c[:, :, 1:]), np.maximum(c[:, :, :-1], c[:, :, 1:])
    mid = fine['c'][:, :, 1::2]
    assert (mid >= lo * (1 - 1e-15)).all() and (mid <= hi * (1 + 1e-15)).all()        # a convex combination of the cell's ends


def test_lane_lists_grid_sizes_and_output_forms_bit_for_bit(handle, regridder):
    nx, nxt = 130, 67
    s, c, phi = handle(nx)
    x = source_grid(nx)
    xt = target_grid(x, nxt)
    kw = dict(mpb_radius=RADII, velocity=-0.2)
    full = regridder.resample(s.device_view(), D, Q, x, BETA, xt, **kw)
    for lanes in ([3], [4, 0, 2], [1, 1, 3, 0, 4, 2, 1], list(range(B))[::-1]):
        part = regridder.resample(s.device_view(), D, Q, x, BETA, xt, lanes=lanes, **kw)
        assert np.array_equal(part['c'], full['c'][lanes]) and np.array_equal(part['phi'], full['phi'][lanes]), lanes
    for waves in (1, 2, 3):          # one, two, three workgroups walk the five operating points
        small = regridder.resample(s.device_view(), D, Q, x, BETA, xt, max_waves=waves, **kw)
        assert np.array_equal(small['c'], full['c']) and np.array_equal(small['phi'], full['phi']), waves
    # host only, device only, both: the device result is read back through a handle of the target grid
    with PnpSolver(N, nxt, float(xt[1] - xt[0]), 1.0, BETA, EPS, D, Q, method='Newton', batch_capacity=B) as t:
        t.set_newton(wall_bc='stern', stern_capacitance=0.2)
        t.set_grid(xt)
        assert t.row_pitch == _regrid.row_pitch(nxt)
        for to_host in (False, True):
            t.set_batch(np.ones((B, N, nxt)), np.zeros((B, 4)), np.zeros(B), np.zeros((B, N)))
            out = regridder.resample(s.device_view(), D, Q, x, BETA, xt, to_host=to_host, device=True, **kw)
            assert set(out) == ({'c', 'phi', 'c_dev', 'phi_dev'} if to_host else {'c_dev', 'phi_dev'})
            if to_host:
                assert np.array_equal(out['c'], full['c']) and np.array_equal(out['phi'], full['phi'])
            t.set_lanes_device(out['c_dev'], out['phi_dev'])
            ct, pt = t.get_state(derived=False)
            assert np.array_equal(ct, full['c']) and np.array_equal(pt, full['phi'])


# ---- hand-over and warm start: a binary electrolyte at a Stern wall ----------------------------------------------------------------
CB = np.array([100.0, 100.0])
Q2, D2 = np.array([unit_F, -unit_F]), np.array([1.957e-9, 1.185e-9])
DEBYE = np.sqrt(EPS / BETA / (Q2 ** 2 * CB).sum())
LENGTH = 60e-9
PHIM = np.array([0.3, -0.3, 0.35, -0.4, 0.45, -0.45, 0.5, -0.5])


def binary(x, nlanes=len(PHIM), start=True):
    s = PnpSolver(2, len(x), float(x[1] - x[0]), 1.0, BETA, EPS, D2, Q2, method='Newton', batch_capacity=nlanes)
    s.set_newton(wall_bc='stern', stern_capacitance=0.2)
    s.set_grid(x)
    if start:
        bulk(s, x, nlanes)
    return s


def bulk(s, x, nlanes=len(PHIM)):
    pb = np.zeros((nlanes, 4))
    pb[:, 0] = PHIM[:nlanes]
    s.set_batch(np.repeat(np.repeat(CB[None, :, None], len(x), axis=2), nlanes, axis=0), pb, np.zeros(nlanes), np.zeros((nlanes, 2)))


@pytest.fixture(scope='module')
def coarse():
    """The coarse solution: 66 graded points, phiM - phiPZC of 0.3 .. 0.5 V of both signs"""
    x = graded_mesh(LENGTH, DEBYE / 10.0, 66)
    s = binary(x)
    st = s.solve_stationary()
    assert (st == 0).all(), st
    yield s, x
    s.close()


def test_hand_over_on_the_device_is_the_host_path_to_the_bit(coarse):
    """resample + set_lanes (over the host) on one handle, resample_to (on the device) on its twin: the same bits, so the same solve.
    The lanes that were not named keep their state; and on a nested refinement the fine handle's own balance library sees the parent
    edges' fluxes on the sub-edges."""
    src, x = coarse
    xf = nested(x)
    lanes, dst = [6, 1, 3], [0, 5, 2]
    with binary(xf) as a, binary(xf) as b:
        before_c, before_phi = b.get_state(derived=False)
        c, phi = src.resample(xf, lanes=lanes)
        a.set_lanes(dst, c, phi)
        src.resample_to(b, lanes=lanes, dst_lanes=dst)
        ca, pa = a.get_state(derived=False)
        cb_, pb_ = b.get_state(derived=False)
        assert np.array_equal(ca, cb_) and np.array_equal(pa, pb_)
        assert np.array_equal(cb_[dst], c) and np.array_equal(pb_[dst], phi)
        rest = [i for i in range(len(PHIM)) if i not in dst]
        assert np.array_equal(cb_[rest], before_c[rest]) and np.array_equal(pb_[rest], before_phi[rest])
        # the fluxes of the sub-edges, derived by the balance library from the fine handle's state, are the parent edges'
        Jc = src.get_balance(fields=['flux'], scalars=False)['flux'][lanes]
        Jf = b.get_balance(fields=['flux'], scalars=False)['flux'][dst]
        h = np.diff(xf)
        u = Q2[None, :, None] * BETA * np.diff(phi, axis=1)[:, None, :]
        scale = (D2[None, :, None] / h) * (np.abs(bernoulli(-u) * c[:, :, 1:]) + np.abs(bernoulli(u) * c[:, :, :-1]))
        err = np.abs(Jf - np.repeat(Jc, 2, axis=2)) / scale
        print('sub-edge fluxes against the parent edges: %.2e of scale' % err.max())
        assert err.max() <= TOL
        # the solves of the two handles agree to the bit (a solve reads whole rows: the pads were left alone on both)
        pbd = np.zeros((len(PHIM), 4))
        pbd[dst, 0] = PHIM[lanes]           # the destination lanes take the operating points of the lanes they came from
        pbd[rest, 0] = PHIM[rest]
        out = []
        for s in (a, b):
            s.set_pb(pbd, np.zeros(len(PHIM)))
            st = s.solve_stationary()
            out.append((st, s.newton_iterations()) + s.get_state(derived=False))
        assert np.array_equal(out[0][0], out[1][0]) and (out[0][0] == 0).all()
        assert np.array_equal(out[0][1], out[1][1])
        assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])
        # all lanes, default lane lists
        src.resample_to(b)
        call, pall = src.resample(xf)
        cb_, pb_ = b.get_state(derived=False)
        assert np.array_equal(cb_, call) and np.array_equal(pb_, pall)


def warm_start_counts(coarse_handle, x):
    """Newton iterations of the 130-point solve from the bulk state and from the resampled 66-point solution, and both end states"""
    xf = graded_mesh(LENGTH, DEBYE / 10.0, 130)
    with binary(xf) as cold, binary(xf) as warm:
        st_cold = cold.solve_stationary()
        it_cold = cold.newton_iterations()
        coarse_handle.resample_to(warm)
        st_warm = warm.solve_stationary()
        it_warm = warm.newton_iterations()
        return (st_cold, it_cold) + cold.get_state(derived=False), (st_warm, it_warm) + warm.get_state(derived=False)


def test_warm_start_from_the_coarse_solution(coarse):
    src, x = coarse
    (st_cold, it_cold, c_cold, p_cold), (st_warm, it_warm, c_warm, p_warm) = warm_start_counts(src, x)
    print('Newton iterations at 130 points over %d lanes: %d from the bulk state, %d from the resampled 66-point solution (per lane %s / %s)'
          % (len(PHIM), it_cold.sum(), it_warm.sum(), it_cold.tolist(), it_warm.tolist()))
    assert (st_warm == 0).all() and (st_cold == 0).all()
    assert it_warm.sum() < it_cold.sum()
    err_c = (np.abs(c_warm - c_cold) / np.abs(c_cold)).max()
    err_p = np.abs(p_warm - p_cold).max() / np.abs(p_cold).max()
    print('end states: c %.2e, phi %.2e relative' % (err_c, err_p))
    assert err_c <= 1e-8 and err_p <= 1e-8


def test_calculator_mesh_continuation_on_the_co2r_sweep():
    """tp.newton['coarse_nx'] on the 7-species CO2R sweep (examples/co2r_physical_sweep.py), 8 lanes at 130 points, against the default
    path: the same status, surface concentrations and current densities."""
    from catint_amd.calculator import Calculator
    spec = importlib.util.spec_from_file_location('co2r_physical_sweep', os.path.join(os.path.dirname(__file__), '..', 'examples',
                                                                                       'co2r_physical_sweep.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    runs = {}
    for name, extra in (('default', {}), ('coarse', {'coarse_nx': 66})):
        tp, phis = ex.build(8, 130)
        calc = Calculator(transport=tp, calc='comsol')
        tp.newton = dict({'tol': 1e-10, 'maxit': 80}, **extra)
        calc.set_surface_kinetics([{'species': 'CO2', 'rate': ex.tafel_rate(tp), 'stoichiometry': {'CO2': -1.0, 'CO': 1.0, 'OH-': 2.0}}])
        calc.run()
        names = list(tp.species.keys())
        cs = np.array([[tp.alldata[i]['species'][sp]['surface_concentration'] for sp in names] for i in range(8)])
        runs[name] = (np.array(calc.status), cs, np.array(calc.kinetic_flux), calc.newton_iterations_total, getattr(calc, 'mesh_continuation', None))
    assert runs['default'][4] is None and runs['coarse'][4]['coarse_nx'] == 66
    print('Newton iterations of all lanes: default path %d, mesh continuation %d (%s)' % (runs['default'][3], runs['coarse'][3], runs['coarse'][4]))
    assert np.array_equal(runs['default'][0], runs['coarse'][0]) and (runs['coarse'][0] == 0).all()
    err_c = np.abs(runs['coarse'][1] / runs['default'][1] - 1.0).max()
    j0, j1 = runs['default'][2], runs['coarse'][2]
    assert np.array_equal(j0 == 0.0, j1 == 0.0)
    err_j = (np.abs(j1 - j0) / np.where(j0 != 0.0, np.abs(j0), 1.0)).max()
    print('surface concentrations %.2e, current densities %.2e relative' % (err_c, err_j))
    assert err_c <= 1e-8 and err_j <= 1e-8
