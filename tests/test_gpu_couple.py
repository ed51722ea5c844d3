"""libcatint_couple on the device (PnpSolver.get_coupling) against the NumPy restatement of include/catint_couple.h in
tests/couple_ref.py, which tests/test_couple_abi.py pins to known answers (the method of tests/test_gpu_response.py).

For every case the oracle's converged states of B = 5 operating points (the case's phiM times 1, 0.75, 0.5, 0.25, 0.1; no wall table:
the coupling is defined for prescribed fluxes) are uploaded, one solve_stationary runs, the device's own state is downloaded and the
reference is linearised AT THAT STATE.  The kinetic inputs K, Kc, Kphi are seeded random numbers scaled by the reference's tangent so
that rf (Kc T_c + Kphi (x) T_phi) has a row-sum norm of at most 0.9 -- cond(A) <= 1e3 is asserted on the CPU side -- and the residual
g - rf K moves the surface concentrations by a few per cent.

Tolerance: per output and system, 10 x the disagreement of the reference's two methods (banded LU with the N right-hand sides; the
Schur recursion) on that system, not below 1e-11 -- the project's rule from tests/test_gpu_response.py.  That disagreement must itself
stay below 1e-8 (asserted).  The worst ratios device error / tolerance are printed by every test.  Measured on the MI355X (also in
DESIGN.md section 7i): 0.90 at N = 2, nx = 19 (dc_surface: 1.0e-11 against 1.15e-11), every other small case at most 0.36, case F 0.28,
case E 0.17, with reference disagreements up to 1.6e-11; the general reaction tables of cases G and G8 (without their wall tables):
G 0.05 / 0.11 at nx = 5 / 21, G8 0.09 / 0.10 at nx = 7 / 34, reference disagreements up to 4.1e-12 (its two tangents agree to 1.6e-12); the tangent equals the flux response of libcatint_response bit for bit (asserted); the
end-to-end case takes 2 Newton steps and 3 transport solves where the mixing loop takes 23 iterations, the fluxes equal to 8.1e-9.
Everything that can be exact is asserted bit for bit."""
import numpy as np
import pytest

from catint_amd import PnpSolver, _couple          # fails without the feature
from tests import couple_ref as CR
from tests import kinetics_ref as KR
from tests import response_cases as RC
from tests.test_couple_abi import INSTANCES

pytestmark = pytest.mark.gpu

B = len(RC.SCALES)
ALL = list(_couple.FIELDS)
LAUNCHED = set()
_cache = {}


def open_solver(case, n, maxit=50, tol=1e-10):
    s = PnpSolver(case.N, case.nx, case.dx, 1.0, RC.BETA, RC.EPS, case.D, case.q, method='Newton', batch_capacity=n)
    s.set_newton(wall_bc='dirichlet' if case.CS is None else 'stern', stern_capacitance=case.CS or 0.0, mpb_radius=case.radii, tol=tol,
                 maxit=maxit)
    s.set_grid(case.x)
    if case.velocity:
        s.set_convection(case.velocity)
    if case.reactions:
        s.set_reactions(case.reactions)
    return s


def load(s, case, phis, states):
    n = len(phis)
    pb = np.zeros((n, 4))
    pb[:, 0] = phis
    s.set_batch(np.stack([c for c, _ in states]), pb, np.zeros(n), np.zeros((n, case.N)))
    s.set_lanes(list(range(n)), np.stack([c for c, _ in states]), np.stack([phi for _, phi in states]))


def without_wall(case):
    case.wall = None
    return case


def prepared(case):
    """(solver, phis, [(problem, c, phi)] at the device's own state) of a case without a wall table, solved once per session"""
    if case.name not in _cache:
        phis = case.phiM * np.array(RC.SCALES)
        states, st = [None] * B, None
        for b in np.argsort(np.abs(phis)):                    # continuation from the smallest potential up
            _, c, phi = case.solve(phis[b], start=st, tol=1e-11) if st is not None else case.solve(phis[b], tol=1e-11)
            states[b] = st = (c, phi)
        s = open_solver(case, B)
        load(s, case, phis, states)
        status = s.solve_stationary()
        assert (status == 0).all(), (case.name, status)
        c, phi = s.get_state(derived=False)
        _cache[case.name] = (s, phis, [(case.make(phis[b]), c[b], phi[b]) for b in range(B)])
    return _cache[case.name]


def from_the_bulk(case, phis):
    """a handle whose lanes the device itself solved from the bulk state (small potentials)"""
    key = (case.name, len(phis))
    if key not in _cache:
        s = open_solver(case, len(phis))
        load(s, case, phis, [case.bulk_state()] * len(phis))
        assert (s.solve_stationary() == 0).all()
        _cache[key] = (s, np.asarray(phis, float), None)
    return _cache[key][0]


@pytest.fixture(scope='module', autouse=True)
def close_all():
    yield
    for s, _, _ in _cache.values():
        s.close()
    _cache.clear()


def call(s, flux, kin, **kw):
    out = s.get_coupling(flux, kin, **kw)
    LAUNCHED.add(s._coupler.last_kernel)
    assert s._coupler.last_kernel_ms > 0.0
    return out


def kinetic_inputs(T, cs, g, seed, rf=1.0):
    """Seeded random K, Kc, Kphi of one point, scaled by the tangent T [(N+1), N]: ||rf (Kc T_c + Kphi (x) T_phi)||_inf <= 0.9 and a
    residual that moves the surface concentrations by at most 5 %"""
    N = T.shape[1]
    rng = np.random.RandomState(seed)
    rowmax = np.abs(T[:N]).max(axis=1)
    Kc = 0.7 * rng.uniform(-1, 1, (N, N)) / (N * N * np.where(rowmax > 0, rowmax, 1.0)[None, :] * rf)
    pmax = np.abs(T[N]).max()
    Kphi = 0.2 * rng.uniform(-1, 1, N) / (N * (pmax if pmax > 0 else 1.0) * rf)
    with np.errstate(divide='ignore'):
        room = np.where(np.abs(T[:N]) > 0, cs[:, None] / np.abs(T[:N]), np.inf).min(axis=0)       # per flux: what moves a c_s by itself
    G = 0.05 * rng.uniform(-1, 1, N) * np.where(np.isfinite(room), room, 0.0) / N
    return (np.asarray(g, float) - G) / rf, Kc, Kphi


def kin_of(lin, flux, rf=1.0, seed=0):
    """{'flux', 'dflux_dc', 'dflux_dphi'} [B]... for the states of `lin`, with the reference's tangent as the scale"""
    K, Kc, Kp = [], [], []
    for b, (p, c, phi) in enumerate(lin):
        k, kc, kp = kinetic_inputs(CR.tangent_banded(p, c, phi), c[:, 0], flux[b], 1000 * seed + b, rf)
        K.append(k), Kc.append(kc), Kp.append(np.stack([np.zeros(p.N), kp], axis=1))
    return {'flux': np.array(K), 'dflux_dc': np.array(Kc), 'dflux_dphi': np.array(Kp)}


def check(case, rf=1.0, dphi_max=0.05):
    """The device against the reference linearised at the device's state: the worst error / tolerance over points and outputs"""
    s, phis, lin = prepared(case)
    flux = np.zeros((B, case.N))
    kin = kin_of(lin, flux, rf)
    got = call(s, flux, kin, rf=rf, dphi_max=dphi_max)
    assert (got['status'] == 0).all(), got['status']
    worst, worst_dis, where = 0.0, 0.0, ''
    for b, (p, c, phi) in enumerate(lin):
        args = (p, c, phi, flux[b], kin['flux'][b], kin['dflux_dc'][b], kin['dflux_dphi'][b][:, 1], rf, dphi_max)
        ra, rb = CR.step(*args, method='banded'), CR.step(*args, method='schur')
        assert ra['status'] == 0 and ra['cond'] <= 1e3, (case.name, b, ra['cond'])
        dis = CR.disagreement(ra, rb)
        err = CR.disagreement({k: got[k][b] for k in CR.FIELDS}, ra)
        for k in CR.FIELDS:
            assert dis[k] < 1e-8, (case.name, b, k, dis[k])
            tol = max(10.0 * dis[k], 1e-11)
            if err[k] / tol > worst:
                where = 'point %d, %s: error %.2e, reference disagreement %.2e' % (b, k, err[k], dis[k])
            worst, worst_dis = max(worst, err[k] / tol), max(worst_dis, dis[k])
    print('%s: worst device error / tolerance %.3f (reference disagreement up to %.1e; %s)' % (case.name, worst, worst_dis, where))
    assert worst <= 1.0, (case.name, worst, where)
    return got, kin, flux


def same(a, b, keys=None):
    for k in (keys or a):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- against the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', range(1, 9))
@pytest.mark.parametrize('nx', [3, 19])
def test_every_block_size_at_the_smallest_grid_and_a_short_one(N, nx):
    check(RC.small(N, nx))


@pytest.mark.parametrize('N', [2, 4, 8])
def test_stern_and_steric_variants(N):
    check(RC.small(N, 19, stern=True, steric=True), rf=1.0 + 0.5 * N)
    check(RC.small(N, 19, stern=True, steric=False))
    check(RC.small(N, 19, stern=False, steric=True), dphi_max=0.0)


def test_case_F_every_term_of_the_physics():
    check(without_wall(RC.case_F()), rf=2.5)


def test_case_E_block_size_nine():
    check(without_wall(RC.case_E(34)))


G_CASES = {'G nx=5': lambda: RC.case_G(5), 'G nx=21': lambda: RC.case_G(21), 'G8 nx=7': lambda: RC.case_G8(7), 'G8 nx=34': lambda: RC.case_G8(34)}


@pytest.mark.parametrize('name', sorted(G_CASES))
def test_general_reaction_tables(name):
    """Cases G and G8 (tests/response_cases.py) without their wall tables: every shape of an entry of the reaction table in the rows of
    the Jacobian the tangent is eliminated from"""
    check(without_wall(G_CASES[name]()), rf=1.5)


def test_table_entries_without_effect_change_no_bit_and_a_dropped_reaction_does():
    """tests/response_cases.py: table_properties (the library takes no wall table)"""
    case = without_wall(RC.case_G(21))
    s, phis, lin = prepared(case)
    flux = np.zeros((B, case.N))
    kin = kin_of(lin, flux)
    RC.table_properties(s, case, lambda: call(s, flux, kin), ['T_c', 'T_phi', 'dflux', 'flux_new', 'dc_surface', 'dphi_surface'], wall=False)


def test_the_cases_reach_every_instance():
    """(after the cases above in file order: LAUNCHED collects last_kernel of every call)"""
    assert LAUNCHED == INSTANCES, sorted(LAUNCHED ^ INSTANCES)


@pytest.mark.parametrize('name', ['F', 'E', 'N=4'])
def test_the_tangent_is_the_flux_response_of_libcatint_response(name):
    """Column j of T equals catresp_solve(CATRESP_WALL_FLUX, species j, omega = 0): within the tolerance of the parity checks, and bit
    for bit -- the two kernels form the rows of the Jacobian with the same functions (catint_amd/csrc/pnp_team.h) and eliminate them
    with the same Gauss-Jordan step, written out in each, so a column goes through the same operations in the same order"""
    case = {'F': lambda: without_wall(RC.case_F()), 'E': lambda: without_wall(RC.case_E(34)), 'N=4': lambda: RC.small(4, 19, True, True)}[name]()
    s, phis, lin = prepared(case)
    flux = np.zeros((B, case.N))
    got = call(s, flux, kin_of(lin, flux), fields=['T_c', 'T_phi'])
    worst, exact = 0.0, True
    for j in range(case.N):
        r = s.get_response(omega=[0.0], perturbation=('flux', j))
        assert (r['status'] == 0).all() and (r['dc_surface'].imag == 0).all()
        for b, (p, c, phi) in enumerate(lin):
            tol = max(10.0 * CR.rel_T(CR.tangent_schur(p, c, phi), CR.tangent_banded(p, c, phi)), 1e-11)
            worst = max(worst, CR.rel(got['T_c'][b][:, j], r['dc_surface'][b, 0].real) / tol, CR.rel(got['T_phi'][b][j], r['dphi_surface'][b, 0].real) / tol)
        exact = exact and np.array_equal(got['T_c'][:, :, j], r['dc_surface'][:, 0].real) and np.array_equal(got['T_phi'][:, j], r['dphi_surface'][:, 0].real)
    print('%s: T against the flux response of libcatint_response: worst difference / tolerance %.3f, bit-identical: %s' % (case.name, worst, exact))
    assert worst <= 1.0
    assert exact


# ---- bit for bit -------------------------------------------------------------------------------------------------------------------
def random_kin(n, N, T_c, T_phi, seed):
    """kinetic inputs for n points scaled by the device's own tangent of a first call"""
    rng = np.random.RandomState(seed)
    rowmax = np.abs(T_c).max(axis=2)
    Kc = 0.7 * rng.uniform(-1, 1, (n, N, N)) / (N * N * np.where(rowmax > 0, rowmax, 1.0)[:, None, :])
    pmax = np.abs(T_phi).max(axis=1)
    Kp = 0.2 * rng.uniform(-1, 1, (n, N)) / (N * np.where(pmax > 0, pmax, 1.0)[:, None])
    return {'flux': 1e-7 * rng.uniform(-1, 1, (n, N)), 'dflux_dc': Kc, 'dflux_dphi': np.stack([np.zeros((n, N)), Kp], axis=2)}


def bitwise_handle(N, n):
    case = RC.small(N, 19, stern=(N == 4), steric=(N == 8))
    s = from_the_bulk(case, -0.1 * np.linspace(0.1, 1.0, n))
    flux = np.zeros((n, N))
    zero = {'flux': np.zeros((n, N)), 'dflux_dc': np.zeros((n, N, N)), 'dflux_dphi': np.zeros((n, N, 2))}
    first = call(s, flux, zero, fields=['T_c', 'T_phi'])
    return s, flux, random_kin(n, N, first['T_c'], first['T_phi'], 7 + N)


@pytest.mark.parametrize('N, n', [(2, 23), (4, 13), (8, 8)])
def test_waves_lanes_and_requested_outputs_do_not_change_the_bits(N, n):
    """Batches beyond one wave's teams (21, 12, 7) that are no multiples of them"""
    s, flux, kin = bitwise_handle(N, n)
    before = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    want = call(s, flux, kin)
    assert (want['status'] == 0).all() and all(np.isfinite(want[k]).all() for k in ALL)
    same(call(s, flux, kin, max_waves=1), want)
    same(call(s, flux, kin, max_waves=2), want)
    rng = np.random.RandomState(N)
    for lanes in (rng.permutation(n), np.array([n - 1, 0, 0, n // 2, n - 1]), np.array([n // 2]), np.arange(n - 1)):
        sub = {k: v[lanes] for k, v in kin.items()}
        got = call(s, flux, sub, lanes=lanes, max_waves=int(rng.randint(0, 3)))
        for k in ALL + ['status']:
            assert np.array_equal(got[k], want[k][lanes]), (k, lanes)
    for fields in (['flux_new'], ['lambda', 'dphi_surface'], ['T_c'], ['dc_surface', 'dflux', 'T_phi']):
        got = call(s, flux, kin, fields=fields)
        assert sorted(got) == sorted(fields + ['status'])
        same(got, want, fields + ['status'])
    # outputs not asked for stay untouched: room for n + 1 points, and rows the call does not name
    o = s._obs
    out = {k: np.full((n + 1,) + _couple.FIELDS[k](N), 7.0) for k in ALL}
    out['status'] = np.full(n + 1, 77, np.int32)
    named = ['T_c', 'lambda', 'flux_new']
    part = {k: out[k][:n] for k in named + ['status']}
    s._coupler.solve(s.device_view(), o['D'], o['charges'], o['x'], o['beta'], o['eps'], o['dx'], flux, kin['flux'], kin['dflux_dc'],
                     np.ascontiguousarray(kin['dflux_dphi'][:, :, 1]), lanes=np.arange(n), mpb_radius=o['mpb_radius'], wall_bc=o['wall_bc'],
                     stern_capacitance=o['stern_capacitance'], fields=named, out=part)
    for k in ALL + ['status']:
        fill = 77 if k == 'status' else 7.0
        assert (out[k][n] == fill).all(), k
        if k in named + ['status']:
            assert np.array_equal(out[k][:n], want[k]), k
        else:
            assert (out[k] == fill).all(), k
    after = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


# ---- status ------------------------------------------------------------------------------------------------------------------------
def test_an_unsolved_lane_and_a_nan_input_report_2_in_their_lane_only():
    case = RC.Case('unconverged', RC.D2, RC.Q2, [100.0, 100.0], RC.kornyshev().x, -0.8, radii=[4e-10, 4e-10])
    flux = np.zeros((B, 2))
    kin = {'flux': np.full((B, 2), 1e-9), 'dflux_dc': np.zeros((B, 2, 2)), 'dflux_dphi': np.zeros((B, 2, 2))}
    results = []
    for phis in (np.zeros(B), np.array([0.0, 0.0, -0.8, 0.0, 0.0])):
        with open_solver(case, B, maxit=1) as s:
            load(s, case, phis, [case.bulk_state()] * B)
            status = s.solve_stationary()
            results.append((status, call(s, flux, kin)))
            if not phis.any():
                bad = {k: v.copy() for k, v in kin.items()}
                bad['dflux_dc'][3, 1, 0] = np.nan
                nan_in = call(s, flux, bad)
                bad = {k: v.copy() for k, v in kin.items()}
                bad['flux'][0, 1] = np.inf
                inf_in = call(s, flux, bad)
    (st0, clean), (st1, got) = results
    assert (st0 == 0).all() and st1[2] != 0 and (np.delete(st1, 2) == 0).all()
    assert (clean['status'] == 0).all()
    for res, lane in ((got, 2), (nan_in, 3), (inf_in, 0)):
        assert res['status'][lane] == 2 and (np.delete(res['status'], lane) == 0).all()
        for k in ALL:
            assert np.isnan(res[k][lane]).all(), k
            assert np.array_equal(np.delete(res[k], lane, axis=0), np.delete(clean[k], lane, axis=0)), k


def test_a_small_pivot_is_reported_for_its_lane_only():
    """The pivot monitor on data (tests/response_cases.py: small_pivot): status 1 in lane 2, whose neighbours equal those of a batch
    in which lane 2 holds another uniform state"""
    case, cbs = RC.small_pivot()
    plain = RC.Case('small pivot: the state', case.D, case.q, case.cb, case.x, 0.0)
    flux = np.zeros((B, 2))
    kin = {'flux': np.full((B, 2), 1e-9), 'dflux_dc': np.zeros((B, 2, 2)), 'dflux_dphi': np.zeros((B, 2, 2))}
    results = []
    # (the other state of lane 2 is lane 0's: with the reaction the species-0 operator is oscillatory, and an arbitrary level can
    #  itself meet a vanishing pivot on the way to the wall -- 5 mol/m^3 does)
    for lane2 in (cbs[RC.SMALL_PIVOT_LANE], cbs[0]):
        levels = list(cbs)
        levels[RC.SMALL_PIVOT_LANE] = lane2
        with open_solver(plain, B) as s:
            states = [(np.full((2, case.nx), cb), np.zeros(case.nx)) for cb in levels]
            load(s, plain, np.zeros(B), states)
            assert (s.solve_stationary() == 0).all()
            s.set_lanes(list(range(B)), np.stack([c for c, _ in states]), np.stack([phi for _, phi in states]))
            s.set_reactions(case.reactions)
            results.append(call(s, flux, kin))
    got, clean = results
    want = np.zeros(B, np.int32)
    want[RC.SMALL_PIVOT_LANE] = 1
    assert np.array_equal(got['status'], want) and (clean['status'] == 0).all()
    for k in ALL:
        assert np.array_equal(np.delete(got[k], RC.SMALL_PIVOT_LANE, axis=0), np.delete(clean[k], RC.SMALL_PIVOT_LANE, axis=0)), k


def test_a_singular_newton_matrix_is_reported_for_its_lane_only():
    """Kc = T_c^-1 / rf from the device's own tangent and Kphi = 0: A = I - I"""
    s, flux, kin = bitwise_handle(4, 13)
    rf = 1.5
    first = call(s, flux, kin, rf=rf)
    assert (first['status'] == 0).all()
    lane = 6
    assert np.linalg.cond(first['T_c'][lane]) < 1e8
    bad = {k: v.copy() for k, v in kin.items()}
    bad['dflux_dc'][lane] = np.linalg.inv(first['T_c'][lane]) / rf
    bad['dflux_dphi'][lane] = 0.0
    got = call(s, flux, bad, rf=rf)
    assert got['status'][lane] == 3 and (np.delete(got['status'], lane) == 0).all()
    for k in ALL:
        assert np.array_equal(np.delete(got[k], lane, axis=0), np.delete(first[k], lane, axis=0)), k
    same({k: got[k][lane] for k in ('T_c', 'T_phi')}, {k: first[k][lane] for k in ('T_c', 'T_phi')})


# ---- damping -----------------------------------------------------------------------------------------------------------------------
def test_a_step_that_would_empty_the_surface_is_damped_as_the_reference_damps_it():
    case = RC.small(3, 19, stern=True)
    s, phis, lin = prepared(case)
    flux = np.zeros((B, 3))
    kin = {'flux': np.zeros((B, 3)), 'dflux_dc': np.zeros((B, 3, 3)), 'dflux_dphi': np.zeros((B, 3, 2))}
    refs = []
    for b, (p, c, phi) in enumerate(lin):
        T = CR.tangent_banded(p, c, phi)
        k = j = b % 3
        kin['flux'][b, j] = -5.0 * c[k, 0] / T[k, j]          # dflux = K - g: dc_surface_k = -5 c_k(0) through its own flux alone
        refs.append(CR.step(p, c, phi, flux[b], kin['flux'][b], kin['dflux_dc'][b], np.zeros(3), 1.0, 0.0))
    got = call(s, flux, kin, dphi_max=0.0)
    assert (got['status'] == 0).all()
    for b, (p, c, phi) in enumerate(lin):
        cs = c[:, 0]
        assert got['lambda'][b] < 1.0 and refs[b]['lambda'] < 1.0
        assert abs(got['lambda'][b] - refs[b]['lambda']) <= 1e-9 * refs[b]['lambda']
        assert (cs + got['lambda'][b] * got['dc_surface'][b] >= 0.1 * cs * (1.0 - 1e-12)).all()
        assert np.isclose((cs + got['lambda'][b] * got['dc_surface'][b]) / cs, 0.1, rtol=1e-9).any()          # the bound is attained
        assert np.array_equal(got['flux_new'][b], flux[b] + got['lambda'][b] * got['dflux'][b])
    # the limit on the surface potential: dphi_max a tenth of the undamped step of lane 0
    full = call(s, flux, {k: 1e-3 * v if k == 'flux' else v for k, v in kin.items()}, dphi_max=0.0)
    assert (full['lambda'] == 1.0).all()
    lim = 0.1 * abs(full['dphi_surface'][0])
    got = call(s, flux, {k: 1e-3 * v if k == 'flux' else v for k, v in kin.items()}, dphi_max=lim)
    assert abs(got['lambda'][0] - 0.1) <= 1e-15 and (got['lambda'] * np.abs(got['dphi_surface']) <= lim * (1 + 1e-15)).all()
    same(got, full, ['dflux', 'dc_surface', 'dphi_surface', 'T_c', 'T_phi'])


def test_a_species_absent_from_the_surface_does_not_enter_the_rule():
    q = np.array([1.0, 1.0, -1.0]) * RC.F
    case = RC.Case('absent species', RC.E_D[:3], q, [50.0, 0.0, 50.0], RC.small(3, 19).x, -0.05, CS=0.2)
    s = from_the_bulk(case, np.array([-0.05, -0.02]))
    c, phi = s.get_state(derived=False)
    assert (c[:, 1] == 0.0).all() and (c[:, 0, 0] > 0).all()
    flux = np.zeros((2, 3))
    zero = {'flux': np.zeros((2, 3)), 'dflux_dc': np.zeros((2, 3, 3)), 'dflux_dphi': np.zeros((2, 3, 2))}
    T = call(s, flux, zero, fields=['T_c'])['T_c']
    assert (T[:, 1, 1] > 0).all()
    kin = dict(zero, flux=np.zeros((2, 3)))
    kin['flux'][:, 1] = -1e-3 / T[:, 1, 1]          # would take c_1(0) = 0 to -1e-3 mol/m^3
    got = call(s, flux, kin, dphi_max=0.0)
    assert (got['status'] == 0).all() and (got['dc_surface'][:, 1] < 0).all()
    assert (got['lambda'] == 1.0).all(), got['lambda']


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_newton_scf_cycle_on_the_small_stern_wall_case():
    from catint_amd.calculator import Calculator
    from tests.test_gpu_kinetics import E2E_PHIS, e2e_model, e2e_transport
    tp = e2e_transport()
    calc = Calculator(transport=tp, calc='comsol', tau_scf=2e-9)
    model = e2e_model(tp)
    calc.set_microkinetics(model, site_density=2e-6, scf='newton')
    out = calc.run_scf_cycle()
    print('Newton steps %d, transport solves %d, residuals %s, damping %s' % (out['iterations'], out['transport_solves'], out['accuracy'],
                                                                              out['damping'].tolist()))
    assert out['converged'].all() and not out['failed'].any() and out['iterations'] <= 3
    assert (out['kinetic_status'] == 0).all() and (out['coupling_status'] == 0).all() and 'mix' not in out
    tp2 = e2e_transport()
    mixing = Calculator(transport=tp2, calc='comsol', tau_scf=1e-8)
    mixing.set_microkinetics(e2e_model(tp2), site_density=2e-6)
    ref = mixing.run_scf_cycle(max_iter=200)
    assert ref['converged'].all()
    err = np.abs(out['flux'] - ref['flux']).max(axis=1) / np.abs(ref['flux']).max(axis=1)
    print('against the mixing loop (%d iterations, one transport solve each): fluxes differ by %.1e' % (ref['iterations'], err.max()))
    assert (err <= 1e-5).all(), err
    assert out['transport_solves'] < ref['iterations']
    # the fixed point: the fluxes are the model's at the final surface state
    tab = dict(model.tables(), site_density=2e-6)
    end = KR.solve_fp64(tab, np.array(E2E_PHIS), out['surface_concentration'], np.array([tp.alldata[i]['system']['surface_potential'] for i in range(8)]),
                        w=1, CS=0.2, phi_pzc=0.1, sens=False)
    assert np.allclose(end['flux'], out['flux'], rtol=1e-8, atol=1e-30)
    assert (out['flux'][:, 2] < 0).all() and np.all(np.diff(out['flux'][:, 3]) > 0)
