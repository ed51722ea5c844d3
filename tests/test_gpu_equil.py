"""libcatint_equil on the device (PnpSolver.equilibrium / set_equilibrium) against the NumPy restatement of include/catint_equil.h in
tests/pb_ref.py, which tests/test_equil_abi.py pins to the oracle of the physical mode.

Tolerances.  Device and restatement run the same damped Newton iteration to the same stopping rule (update below 1e-10 thermal
voltages), so both end within a rounding-level distance of the root of the same discrete system: the residual is evaluated to a few
1e-16 of its terms and the Jacobian's inverse is bounded by the screening term ((Debye length / h)^2 <= 1e4 here), which leaves the
potentials some 1e-12 |phiM - phi_bulk| apart.  A concentration is a0 exp(-q beta (phi - phi_bulk)) / (1 + S): an error d of the
potential moves it by |q| beta d relative (78 / V for the divalent ion).  Asserted: phi to 1e-9 |phiM - phi_bulk|, c to 1e-9 relative,
per element; the worst ratios are printed.  Iteration counts may differ by one (an update that lands on either side of tol).
Everything else that can be exact is asserted bit for bit."""
import ctypes as C

import numpy as np
import pytest

from catint_amd import PnpSolver, _equil          # fails without the feature
from catint_amd.units import unit_F, unit_R, unit_eps0
from oracle import pnp_physical as PH
from tests import pb_ref
from tests.test_equil_abi import INSTANCES

pytestmark = pytest.mark.gpu

BETA = 1.0 / (unit_R * 298.15)
EPS = 78.36 * unit_eps0
TOL = 1e-9
B, N = 5, 3
Q = np.array([1.0, -1.0, -2.0]) * unit_F
D = np.array([1.957e-9, 1.185e-9, 0.923e-9])
RADII = np.array([4e-10, 3e-10, 3.5e-10])
# bulk concentrations of the five operating points (electroneutral: c0 = c1 + 2 c2) and their bulk potentials
CB = np.array([[120.0, 100.0, 10.0], [60.0, 50.0, 5.0], [240.0, 200.0, 20.0], [130.0, 100.0, 15.0], [12.0, 10.0, 1.0]])
PHIB = np.array([0.0, 0.01, -0.02, 0.0, 0.03])
WALLS = {'dirichlet': (np.array([-0.25, -0.1, 0.05, 0.15, 0.25]), 0.0), 'stern': (np.array([-1.0, -0.5, 0.2, 0.6, 1.0]), 0.2)}
PZC = 0.05

# every instance at its smallest grid
SIZES = [10, 66, 130, 258, 514, 1026, 1030, 2052, 4098]


def shape_of(nx):
    """(P, WY) of pnp::post::choose_shape"""
    m = nx - 2
    if m > 2048:
        return 16, 4
    if m > 1024:
        return 16, 2
    return [p for p in (1, 2, 4, 8, 16) if m <= 64 * p][0], 1


def grid(nx):
    """20 nm, mildly graded towards the wall up to 1026 points; uniform beyond (40 nm)"""
    if nx > 1026:
        return np.linspace(0.0, 40e-9, nx)
    s = np.linspace(0.0, 1.0, nx)
    return 20e-9 * (0.3 * s + 0.7 * s * s)


_handles = {}
_refs = {}


@pytest.fixture(scope='module')
def handle():
    """handle(nx, wall, steric) -> PnpSolver of a zero-flux batch of the B operating points in the bulk state"""
    def get(nx, wall='stern', steric=True):
        key = (nx, wall, steric)
        if key not in _handles:
            x = grid(nx)
            s = PnpSolver(N, nx, float(x[1] - x[0]), 1.0, BETA, EPS, D, Q, method='Newton', batch_capacity=B)
            s.set_newton(wall_bc=wall, stern_capacitance=WALLS[wall][1], phi_pzc=PZC if wall == 'stern' else 0.0,
                         mpb_radius=RADII if steric else None)
            s.set_grid(x)
            bulk(s, wall)
            _handles[key] = s
        return _handles[key]
    yield get
    for s in _handles.values():
        s.close()
    _handles.clear()


def bulk(s, wall):
    pb = np.zeros((B, 4))
    pb[:, 0], pb[:, 1] = WALLS[wall][0], PHIB
    s.set_batch(np.repeat(CB[:, :, None], s.nx, axis=2), pb, np.zeros(B), np.zeros((B, N)))


def reference(nx, wall, steric, maxit=100):
    """tests/pb_ref.py of the B operating points, computed once"""
    key = (nx, wall, steric, maxit)
    if key not in _refs:
        x = grid(nx)
        out = [pb_ref.solve(x, float(x[1] - x[0]), Q, BETA, EPS, CB[b], WALLS[wall][0][b], PHIB[b], RADII if steric else None,
                            WALLS[wall][1] if wall == 'stern' else None, PZC if wall == 'stern' else 0.0, maxit=maxit) for b in range(B)]
        _refs[key] = tuple(np.array([o[j] for o in out]) for j in range(4))
        for a in _refs[key]:
            a.setflags(write=False)
    return _refs[key]


def same(a, b, keys=('c', 'phi', 'status', 'iterations')):
    return all(np.array_equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize('steric', [False, True])
@pytest.mark.parametrize('wall', ['dirichlet', 'stern'])
@pytest.mark.parametrize('nx', SIZES)
def test_parity_with_the_restatement(handle, nx, wall, steric):
    s = handle(nx, wall, steric)
    P, WY = shape_of(nx)
    got = s.equilibrium(max_waves=WY)                 # one workgroup walks all lanes
    assert s._equilibrator.last_kernel == 'cateq::pb_kernel<%d, %d, %s>' % (P, WY, 'true' if steric else 'false')
    assert s._equilibrator.last_kernel_ms > 0.0
    c, phi, status, its = reference(nx, wall, steric)
    span = np.abs(WALLS[wall][0] - PHIB)[:, None]
    err_c = np.abs(got['c'] - c) / np.abs(c)
    err_phi = np.abs(got['phi'] - phi) / span
    print('nx=%d %s steric=%s: iterations %s (restatement %s); c %.2e relative, phi %.2e of |phiM - phi_bulk|; largest exponent %.1f'
          % (nx, wall, steric, got['iterations'].tolist(), its.tolist(), err_c.max(), err_phi.max(),
             np.abs(Q[None, :, None] * BETA * (phi - PHIB[:, None])[:, None, :]).max()))
    assert (status == 0).all() and (got['status'] == 0).all()
    assert np.isfinite(got['c']).all() and (got['c'] > 0).all()
    assert err_c.max() <= TOL and err_phi.max() <= TOL
    assert np.abs(got['iterations'] - its).max() <= 1
    # the boundary rows, as the definition states them
    assert np.array_equal(got['phi'][:, -1], PHIB)
    if wall == 'dirichlet':
        assert np.array_equal(got['phi'][:, 0], WALLS[wall][0])


def test_the_cases_reach_every_instance():
    assert {'cateq::pb_kernel<%d, %d, %s>' % (shape_of(nx) + (s,)) for nx in SIZES for s in ('false', 'true')} == INSTANCES


@pytest.mark.parametrize('nx', [10, 130, 1030, 2052])
def test_any_number_of_workgroups_gives_the_same_bits(handle, nx):
    s = handle(nx)
    _, WY = shape_of(nx)
    want = s.equilibrium()
    assert (want['status'] == 0).all()
    for groups in (1, 2, 3):
        assert same(s.equilibrium(max_waves=groups * WY), want), groups


@pytest.mark.parametrize('nx', [66, 1030])
def test_lane_subsets_and_permutations_with_repeats(handle, nx):
    s = handle(nx)
    want = s.equilibrium()
    for lanes in ([3], [4, 0, 2], [1, 1, 4, 3, 1, 0, 2, 2], list(range(B))[::-1]):
        got = s.equilibrium(lanes=lanes)
        assert all(np.array_equal(got[k], want[k][lanes]) for k in ('c', 'phi', 'status', 'iterations')), lanes
    # another potential for the same lanes: lane b at the wall potential of lane 4 - b is not lane b's result ...
    other = s.equilibrium(phiM=WALLS['stern'][0][::-1])
    assert not np.array_equal(other['phi'][0], want['phi'][0])
    # ... and with equal bulk values it is the other lane's: the result depends on the parameters, not on the slot
    pb = np.zeros((B, 4))
    pb[:, 0] = WALLS['stern'][0]
    s.set_batch(np.repeat(np.repeat(CB[:1, :, None], s.nx, axis=2), B, axis=0), pb, np.zeros(B), np.zeros((B, N)))
    try:
        a, b = s.equilibrium(), s.equilibrium(phiM=WALLS['stern'][0][::-1])
        assert same(b, {k: v[::-1] for k, v in a.items()})
    finally:
        bulk(s, 'stern')


def read_device(address, count):
    """count doubles from a device address of this process"""
    hip = C.CDLL('libamdhip64.so')
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(count)
    assert hip.hipMemcpy(out.ctypes.data, C.c_void_p(address), out.nbytes, 2) == 0       # hipMemcpyDeviceToHost
    return out


@pytest.mark.parametrize('nx', [10, 66, 1030, 4098])
def test_host_and_device_outputs_carry_the_same_bits_and_pads_are_zero(handle, nx):
    s = handle(nx)
    eq = _equil.Equilibrator(0)
    try:
        args = (s.device_view(), Q, grid(nx), BETA, EPS, float(grid(nx)[1] - grid(nx)[0]), WALLS['stern'][0], PHIB, CB)
        kw = dict(mpb_radius=RADII, wall_bc='stern', stern_capacitance=0.2, phi_pzc=PZC)
        host = eq.solve(*args, to_host=True, device=False, **kw)
        both = eq.solve(*args, to_host=True, device=True, **kw)
        assert same(both, host) and same(host, s.equilibrium())
        dev = eq.solve(*args, to_host=False, device=True, **kw)
        assert 'c' not in dev and np.array_equal(dev['status'], host['status']) and np.array_equal(dev['iterations'], host['iterations'])
        pitch = s.row_pitch
        assert pitch >= nx and pitch % 16 == 0
        c = read_device(dev['c_dev'], B * N * pitch).reshape(B, N, pitch)
        phi = read_device(dev['phi_dev'], B * pitch).reshape(B, pitch)
        assert np.array_equal(c[:, :, :nx], host['c']) and np.array_equal(phi[:, :nx], host['phi'])
        assert not c[:, :, nx:].any() and not phi[:, nx:].any() and not np.signbit(c[:, :, nx:]).any()
    finally:
        eq.close()


def oracle_counts(s, wall, state_c, state_phi):
    """Iterations the oracle's Newton step takes from the given state, per lane, and how far it moves it"""
    x = s.grid
    counts, moved = [], 0.0
    for b in range(B):
        p = PH.PhysicalProblem(D=D, charges=Q, beta=BETA, eps=EPS, dx=float(x[1] - x[0]), nx=len(x), c_bulk=CB[b], phiM=WALLS[wall][0][b],
                               phi_bulk=PHIB[b], stern_capacitance=WALLS[wall][1] if wall == 'stern' else None,
                               phi_pzc=PZC if wall == 'stern' else 0.0, mpb_radius=RADII, x=x)
        c2, phi2, it, _ = PH.newton_step(p, state_c[b], state_phi[b], state_c[b], np.inf, tol=1e-10)
        counts.append(it)
        moved = max(moved, np.abs(c2 - state_c[b]).max() / np.abs(state_c[b]).max(), np.abs(phi2 - state_phi[b]).max() / np.abs(state_phi[b]).max())
    return np.array(counts), moved


@pytest.mark.parametrize('wall', ['dirichlet', 'stern'])
def test_hand_over_to_a_zero_flux_handle(handle, wall):
    """set_equilibrium, then solve_stationary: the solver finds itself at a root of its own residual"""
    s = handle(130, wall)
    try:
        st_bulk = s.solve_stationary()
        it_bulk = s.newton_iterations()
        bulk(s, wall)
        before_c, before_phi = s.get_state(derived=False)
        lanes = [4, 1, 2, 0]                          # lane 3 is not named
        eq = s.set_equilibrium(lanes=lanes)
        assert (eq['status'] == 0).all() and eq['status'].shape == (4,) and (eq['iterations'] >= 2).all()
        c0, phi0 = s.get_state(derived=False)
        assert np.array_equal(c0[3], before_c[3]) and np.array_equal(phi0[3], before_phi[3])
        host = s.equilibrium()
        assert np.array_equal(c0[lanes], host['c'][lanes]) and np.array_equal(phi0[lanes], host['phi'][lanes])
        # all lanes, default lane list
        eq = s.set_equilibrium()
        assert (eq['status'] == 0).all() and np.array_equal(eq['iterations'], host['iterations'])
        c0, phi0 = s.get_state(derived=False)
        assert np.array_equal(c0, host['c']) and np.array_equal(phi0, host['phi'])
        st = s.solve_stationary()
        it = s.newton_iterations()
        c1, phi1 = s.get_state(derived=False)
        want, moved_oracle = oracle_counts(s, wall, c0, phi0)
        moved = max(np.abs(c1 - c0).max() / np.abs(c0).max(), np.abs(phi1 - phi0).max() / np.abs(phi0).max())
        print('%s: Newton iterations from the equilibrium state %s (oracle %s), from the bulk state %s (status %s); the solve moved the state '
              'by %.1e relative (oracle %.1e)' % (wall, it.tolist(), want.tolist(), it_bulk.tolist(), st_bulk.tolist(), moved, moved_oracle))
        assert (st == 0).all()
        assert ((it == want) | (it == want + 1)).all()
        assert moved < TOL
        assert (it_bulk > it).all()
    finally:
        bulk(s, wall)


def test_the_iteration_limit_ends_the_loop(handle):
    s = handle(130)
    before = s.get_state(derived=False)
    lanes = [0, 4]                                    # -1.0 V and +1.0 V
    got = s.equilibrium(lanes=lanes, maxit=2)
    assert (got['status'] == 1).all() and (got['iterations'] == 2).all()
    assert np.isfinite(got['c']).all() and np.isfinite(got['phi']).all()
    c, phi, status, its = reference(130, 'stern', True, maxit=2)
    assert (status[lanes] == 1).all() and (its[lanes] == 2).all()
    assert np.abs(got['phi'] - phi[lanes]).max() <= TOL * 1.0 and (np.abs(got['c'] - c[lanes]) <= TOL * np.abs(c[lanes])).all()
    after = s.get_state(derived=False)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # the limit is per call: the next one converges
    assert (s.equilibrium(lanes=lanes)['status'] == 0).all()


def test_calculator_equilibrium_start_on_the_co2r_sweep():
    """tp.newton['equilibrium_start'] on the 7-species CO2R sweep (examples/co2r_physical_sweep.py: buffer reactions, Tafel kinetics at
    the wall, steric K+, Stern layer), 8 lanes at 130 points, against the default path: where the default walks its continuation stages,
    one solve from the device's equilibrium state reaches the same status and the same currents (1e-9 relative: both paths end Newton
    at the same tolerance of the same system)."""
    import importlib.util
    import os
    from catint_amd.calculator import Calculator
    spec = importlib.util.spec_from_file_location('co2r_physical_sweep', os.path.join(os.path.dirname(__file__), '..', 'examples',
                                                                                       'co2r_physical_sweep.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    runs = {}
    for name, extra in (('default', {}), ('equilibrium', {'equilibrium_start': True})):
        tp, phis = ex.build(8, 130)
        calc = Calculator(transport=tp, calc='comsol')
        tp.newton = dict({'tol': 1e-10, 'maxit': 80}, **extra)
        calc.set_surface_kinetics([{'species': 'CO2', 'rate': ex.tafel_rate(tp), 'stoichiometry': {'CO2': -1.0, 'CO': 1.0, 'OH-': 2.0}}])
        calc.run()
        names = list(tp.species.keys())
        runs[name] = (np.array(calc.status), np.array(calc.kinetic_flux)[:, names.index('CO')], calc.newton_iterations_total,
                      calc.continuation_stages, getattr(calc, 'equilibrium_start', None))
    assert runs['default'][4] is None and runs['default'][3] > 1
    assert runs['equilibrium'][3] == 1 and runs['equilibrium'][4]['pb_failed'] == 0
    print('Newton iterations of all lanes: %d stages %d, equilibrium start %d (%s)' % (runs['default'][3], runs['default'][2], runs['equilibrium'][2],
                                                                                       runs['equilibrium'][4]))
    assert np.array_equal(runs['default'][0], runs['equilibrium'][0]) and (runs['equilibrium'][0] == 0).all()
    j0, j1 = runs['default'][1], runs['equilibrium'][1]
    err_j = (np.abs(j1 - j0) / np.abs(j0)).max()
    print('current densities %.2e relative' % err_j)
    assert (j0 != 0.0).all() and err_j <= TOL
