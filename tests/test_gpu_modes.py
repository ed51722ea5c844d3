"""libcatint_modes on the device (PnpSolver.get_relaxation) against the NumPy restatement of include/catint_modes.h in tests/modes_ref.py,
which tests/test_modes_abi.py pins to a dense eigensolver and to the oracle's backward-Euler step (the method of tests/test_gpu_sens.py).

For every case the oracle's converged states of B = 5 operating points (the case's phiM times 1, 0.75, 0.5, 0.25, 0.1) are uploaded, one
solve_stationary runs, the device's own state is downloaded and the reference iterates AT THAT STATE from the same start vectors:
subspace min(8, N (nx - 1)), 12 passes.

Tolerance of a Ritz value, relative to |theta_j|: MARGIN = 10 times the disagreement of the reference's two solution methods (banded LU;
the Schur recursion with substitution) on the converged Ritz values of that operating point -- the largest over them, not below 1e-11:
the project's rule from tests/test_gpu_sens.py -- plus 10 kappa_j residual_j, what the iteration itself has not resolved (kappa_j from the
dense eigenvectors, residual_j the larger of the device's and the reference's).  Tolerance of the projector Q Q^T, in the max-norm:
MARGIN times the disagreement of the two methods' projectors, not below 1e-11.
Measured on the MI355X, worst device error / tolerance: Ritz values 0.19 (N = 1, nx = 3; disagreement of the methods 2.8e-9), 0.12
(N = 1, nx = 19 and N = 5, nx = 3), every other case <= 0.10; projector 0.81 (N = 2, nx = 3; disagreement 8.9e-10), 0.79 (N = 5, nx = 3),
0.71 (N = 6, nx = 3), every nx = 19 case <= 0.07, case F 0.015, case E 0.008.  The disagreement of the methods is up to 8.8e-9 on the
three- and four-point grids, where the rates are decades apart (cond(W) up to 5e7), and at most 5e-12 from nx = 19 on.
The general reaction and wall tables of cases G and G8: Ritz values 0.021 / 0.040 (G, nx = 5 / 21: 7 and 3 converged pairs per point)
and 0.005 / 0.002 (G8, nx = 7 / 34: 6 pairs), projector 0.099 / 0.100 and 0.021 / 0.002, no breakdown, disagreements up to 3.2e-12.
Everything that can be exact is asserted bit for bit."""
import numpy as np
import pytest

from catint_amd import PnpSolver, _modes          # fails without the feature
from tests import modes_ref as MR
from tests import response_cases as RC
from tests.test_gpu_sens import load, open_solver, small_flux
from tests.test_modes_abi import INSTANCES

pytestmark = pytest.mark.gpu

B = len(RC.SCALES)
MARGIN, FLOOR, RTOL = 10.0, 1e-11, 1e-8
ITERATIONS = 12
ALL = list(_modes.FIELDS)
LAUNCHED = set()
_cache = {}


def subspace(case):
    return min(_modes.MAX_SUBSPACE, case.N * (case.nx - 1))


def prepared(case, flux):
    """(solver, phis, [(problem, c, phi)] at the device's own state), solved once per session"""
    if case.name not in _cache:
        phis = case.phiM * np.array(RC.SCALES)
        states, st = [None] * B, None
        for b in np.argsort(np.abs(phis)):                    # continuation from the smallest potential up
            _, c, phi = case.solve(phis[b], flux=flux, start=st, tol=1e-11) if st is not None else case.solve(phis[b], flux=flux, tol=1e-11)
            states[b] = st = (c, phi)
        s = open_solver(case, B)
        fl = np.tile(np.zeros(case.N) if flux is None else flux, (B, 1))
        load(s, case, phis, states, fl)
        status = s.solve_stationary()
        assert (status == 0).all(), (case.name, status)
        c, phi = s.get_state(derived=False)
        _cache[case.name] = (s, phis, [(case.make(phis[b], fl[b]), c[b], phi[b]) for b in range(B)])
    return _cache[case.name]


def from_the_bulk(case, phis, flux):
    """a handle whose lanes the device itself solved from the bulk state (small potentials)"""
    key = (case.name, len(phis))
    if key not in _cache:
        n = len(phis)
        s = open_solver(case, n)
        load(s, case, phis, [case.bulk_state()] * n, np.tile(flux, (n, 1)))
        assert (s.solve_stationary() == 0).all()
        _cache[key] = (s, np.asarray(phis, float), None)
    return _cache[key][0]


@pytest.fixture(scope='module', autouse=True)
def close_all():
    yield
    for entry in _cache.values():
        entry[0].close()
    _cache.clear()


def raw(s, start, iterations=ITERATIONS, lanes=None, fields=ALL, phiM=None, **kw):
    """catmodes_solve about the handle's state"""
    o = s._obs
    if getattr(s, '_mode_solver', None) is None:
        s._mode_solver = _modes.ModeSolver(o['device'])
    out = s._mode_solver.solve(s.device_view(), o['D'], o['charges'], o['x'], o['beta'], o['eps'], o['dx'], o['phiM'] if phiM is None else phiM,
                               start, iterations=iterations, lanes=np.arange(s.B) if lanes is None else np.asarray(lanes),
                               mpb_radius=o['mpb_radius'], wall_bc=o['wall_bc'], stern_capacitance=o['stern_capacitance'], velocity=o['velocity'],
                               reactions=o['reactions'], wall=o['wall'], fields=fields, **kw)
    LAUNCHED.add(s._mode_solver.last_kernel)
    assert s._mode_solver.last_kernel_ms > 0.0
    return out


def check(case, flux):
    """The device against the reference iterated at the device's state: the worst error / tolerance of the converged Ritz values and of
    the projector over the operating points"""
    s, phis, lin = prepared(case, flux)
    m = subspace(case)
    start = _modes.default_start(m, case.N, case.nx, 0)
    got = raw(s, start)
    assert (got['status'] == 0).all(), got['status']
    user = s.get_relaxation(nmodes=3, subspace=m, iterations=ITERATIONS, profiles=True)
    LAUNCHED.add(s._mode_solver.last_kernel)
    assert np.array_equal(user['ritz'], got['ritz']) and np.array_equal(user['gram'], got['gram']) and (user['status'] == 0).all()
    worst_v, worst_p, worst_dis, nconv = 0.0, 0.0, 0.0, []
    for b, (p, c, phi) in enumerate(lin):
        ra, rb = MR.iterate(p, c, phi, start, ITERATIONS, 'banded'), MR.iterate(p, c, phi, start, ITERATIONS, 'schur')
        assert not ra['breakdown'] and not rb['breakdown']
        ta, _, resa = MR.ritz_pairs(ra['ritz'], ra['gram'])
        tb, _, resb = MR.ritz_pairs(rb['ritz'], rb['gram'])
        td, sd, resd = MR.ritz_pairs(got['ritz'][b], got['gram'][b])
        dth, kap = MR.dense(p, c, phi, refine=0)
        conv = [j for j in range(m) if max(resa[j], resb[j]) <= RTOL]
        assert conv, (case.name, b, resa)
        dis = max(np.abs(ta[j] - tb[MR.match(ta[j:j + 1], tb)[0]]) / np.abs(ta[j]) for j in conv)
        assert dis < 1e-8, (case.name, b, dis)
        for j in conv:
            jd = MR.match(ta[j:j + 1], td)[0]
            if resd[jd] > RTOL:          # a pair at the edge of convergence: the reference calls it converged, the device not yet
                assert resd[jd] <= 10.0 * max(resa[j], resb[j]), (case.name, b, j, resd[jd], resa[j])
            tol = max(MARGIN * dis, FLOOR) + 10.0 * kap[MR.match(ta[j:j + 1], dth)[0]] * max(resa[j], resd[jd])
            worst_v = max(worst_v, np.abs(td[jd] - ta[j]) / np.abs(ta[j]) / tol)
        nconv.append(len(conv))
        # the user's view of the same numbers
        k = min(3, m)
        assert np.array_equal(user['rates'][b], 1.0 / td[:k]) and np.array_equal(user['converged'][b], resd[:k] <= RTOL)
        if user['converged'][b].any():
            assert user['stable'][b] == bool((user['rates'][b][user['converged'][b]].real > 0).all())
        # the projector
        pa, pb = MR.projector(ra['basis']), MR.projector(rb['basis'])
        dp = np.abs(pa - pb).max()
        assert dp < 1e-8, (case.name, b, dp)
        basis = got['basis'][b]
        q = basis.reshape(m, -1)
        # one sweep of modified Gram-Schmidt leaves an overlap of the order eps cond(W) between its columns (Bjorck 1967); cond(W) of
        # the last sweep is 5e2 at nx = 19 and up to 5e7 on the three- and four-point grids, where the rates are decades apart
        assert np.abs(q @ q.T - np.eye(m)).max() <= max(MARGIN * np.finfo(float).eps * ra['cond'], 1e-13), ra['cond']
        worst_p = max(worst_p, np.abs(MR.projector(basis) - pa).max() / max(MARGIN * dp, FLOOR))
        worst_dis = max(worst_dis, dis, dp)
        # the profiles are Q s_j, unit norm
        v = np.concatenate([user['dc'][b], user['dphi'][b][:, None, :]], axis=1)
        assert np.allclose((np.abs(v) ** 2).sum(axis=(1, 2)), 1.0, rtol=1e-12)
        assert np.allclose(v[0], np.einsum('jke,j->ke', basis, sd[:, 0]) / np.linalg.norm(np.einsum('jke,j->ke', basis, sd[:, 0])), rtol=1e-10, atol=1e-13)
    print('%s: converged pairs per point %s; worst Ritz value error / tolerance %.3f, projector %.3f (reference disagreement up to %.1e)'
          % (case.name, nconv, worst_v, worst_p, worst_dis))
    assert worst_v <= 1.0 and worst_p <= 1.0, (case.name, worst_v, worst_p)
    return got


def same(a, b, keys=None):
    for k in (keys or a):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- against the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', range(1, 9))
@pytest.mark.parametrize('nx', [3, 4, 19])
def test_every_block_size_at_the_smallest_grids_and_a_short_one(N, nx):
    """nx = 3: one interior row, subspace 2 N at most (N = 1 .. 3: the whole range of S, every pair converges at once); nx = 4: the first
    grid on which first_row enters a point; nx = 19: no multiple of anything.  Ritz values and projectors (module docstring)."""
    case = RC.small(N, nx)
    check(case, small_flux(case))


@pytest.mark.parametrize('N', [2, 4, 8])
def test_stern_and_steric_variants(N):
    for stern, steric in ((True, True), (True, False), (False, True)):
        case = RC.small(N, 19, stern=stern, steric=steric)
        check(case, small_flux(case))


def test_case_F_every_term_of_the_physics_with_its_wall_table():
    check(RC.case_F(), np.array([0.0, -1e-6, 1e-6]))


def test_case_E_block_size_nine():
    check(RC.case_E(34), None)


FLUX_G = np.array([0.0, -1e-6, 1e-6, 0.0])
G_CASES = {'G nx=5': lambda: (RC.case_G(5), FLUX_G), 'G nx=21': lambda: (RC.case_G(21), FLUX_G),
           'G8 nx=7': lambda: (RC.case_G8(7), None), 'G8 nx=34': lambda: (RC.case_G8(34), None)}


@pytest.mark.parametrize('name', sorted(G_CASES))
def test_general_reaction_and_wall_tables(name):
    """Cases G and G8 (tests/response_cases.py): every shape of an entry of the reaction and wall tables in the rows of the Jacobian the
    iteration solves with"""
    check(*G_CASES[name]())


def test_table_entries_without_effect_change_no_bit_and_a_dropped_reaction_does():
    """tests/response_cases.py: table_properties, on the Ritz matrices and the basis of five passes"""
    case = RC.case_G(21)
    s, phis, lin = prepared(case, FLUX_G)
    start = _modes.default_start(subspace(case), case.N, case.nx, 0)
    RC.table_properties(s, case, lambda: raw(s, start, iterations=5), ALL)


def test_the_cases_reach_every_instance():
    """(after the cases above in file order: LAUNCHED collects last_kernel of every call)"""
    assert LAUNCHED == INSTANCES, sorted(LAUNCHED ^ INSTANCES)


# ---- bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N, n', [(2, 23), (4, 13), (8, 8)])
def test_waves_lanes_lists_outputs_and_the_workspace_cap_do_not_change_the_bits(N, n, monkeypatch):
    """Batches beyond one wave's teams (21, 12, 7) that are no multiples of them: a partial last group, several waves, and, with the
    workspace capped to one wave's slots, several turns"""
    case = RC.small(N, 19, stern=(N == 4), steric=(N == 8))
    s = from_the_bulk(case, -0.1 * np.linspace(0.1, 1.0, n), small_flux(case))
    start = _modes.default_start(8, N, 19, 3)
    before = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    want = raw(s, start, iterations=5)
    assert (want['status'] == 0).all() and all(np.isfinite(want[k]).all() for k in ALL)
    assert all(np.abs(want['ritz'][b]).min() > 0 for b in range(n))
    assert not np.array_equal(want['ritz'][0], want['ritz'][1])
    same(raw(s, start, iterations=5, max_waves=1), want)
    same(raw(s, start, iterations=5, max_waves=2), want)
    monkeypatch.setenv('CATMODES_WORKSPACE_BYTES', '1')          # at least one wave's systems stay resident: one wave walks all groups
    same(raw(s, start, iterations=5), want)
    monkeypatch.delenv('CATMODES_WORKSPACE_BYTES')
    rng = np.random.RandomState(N)
    for lanes in (rng.permutation(n), np.array([n - 1, 0, 0, n // 2, n - 1]), np.array([n // 2]), np.arange(n - 1)):
        got = raw(s, start, iterations=5, lanes=lanes, max_waves=int(rng.randint(0, 3)))
        for k in ALL + ['status']:
            assert np.array_equal(got[k], want[k][lanes]), (k, lanes)
    for fields in (['ritz'], ['gram'], ['basis'], ['gram', 'basis'], []):
        got = raw(s, start, iterations=5, fields=fields)
        assert sorted(got) == sorted(fields + ['status'])
        same(got, want, fields + ['status'])
    # outputs not asked for stay untouched: room for n + 1 points, and rows the call does not name
    out = {k: np.full((n + 1,) + _modes.FIELDS[k](8, N, 19), 7.0) for k in ALL}
    out['status'] = np.full(n + 1, 77, np.int32)
    named = ['gram']
    part = {k: out[k][:n] for k in named + ['status']}
    raw(s, start, iterations=5, fields=named, out=part)
    for k in ALL + ['status']:
        fill = 77 if k == 'status' else 7.0
        assert (out[k][n] == fill).all(), k
        if k in named + ['status']:
            assert np.array_equal(out[k][:n], want[k]), k
        else:
            assert (out[k] == fill).all(), k
    # fewer columns and fewer passes are other numbers, not a reordering: they only have to be well-formed
    small = raw(s, start[:3], iterations=1)
    assert small['ritz'].shape == (n, 3, 3) and small['basis'].shape == (n, 3, N + 1, 19) and (small['status'] == 0).all()
    after = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


# ---- status ------------------------------------------------------------------------------------------------------------------------
def test_an_unsolved_lane_and_a_nan_input_report_2_in_their_lane_only():
    case = RC.Case('unconverged', RC.D2, RC.Q2, [100.0, 100.0], RC.kornyshev().x, -0.8, radii=[4e-10, 4e-10])
    start = _modes.default_start(8, 2, case.nx, 0)
    results = []
    for phis in (np.zeros(B), np.array([0.0, 0.0, -0.8, 0.0, 0.0])):
        with open_solver(case, B, maxit=1) as s:
            load(s, case, phis, [case.bulk_state()] * B, np.zeros((B, 2)))
            status = s.solve_stationary()
            results.append((status, raw(s, start, iterations=3)))
            if not phis.any():
                bad = phis.copy()
                bad[3] = np.nan
                nan_in = raw(s, start, iterations=3, phiM=bad)
    (st0, clean), (st1, got) = results
    assert (st0 == 0).all() and st1[2] != 0 and (np.delete(st1, 2) == 0).all()
    assert (clean['status'] == 0).all()
    for res, lane in ((got, 2), (nan_in, 3)):
        assert res['status'][lane] == 2 and (np.delete(res['status'], lane) == 0).all()
        for k in ALL:
            assert np.isnan(res[k][lane]).all(), k
            assert np.array_equal(np.delete(res[k], lane, axis=0), np.delete(clean[k], lane, axis=0)), k


def test_two_equal_start_columns_report_a_breakdown_in_every_lane():
    """finite numbers throughout: the dependent column is dropped, not divided by its norm"""
    case = RC.small(3, 19, stern=True)
    s = from_the_bulk(case, -0.1 * np.linspace(0.2, 1.0, 4), small_flux(case))
    start = _modes.default_start(6, 3, 19, 0)
    assert (raw(s, start, iterations=3)['status'] == 0).all()
    start[4] = start[1]
    got = raw(s, start, iterations=3)
    assert (got['status'] == 3).all()
    assert all(np.isfinite(got[k]).all() for k in ALL)
    user = s.get_relaxation(subspace=6, iterations=3, start=start)
    assert (user['status'] == 3).all() and np.isnan(user['rates']).all() and not user['converged'].any() and all(v is None for v in user['stable'])


def test_a_small_pivot_is_reported_for_its_lane_only():
    """The pivot monitor on data (tests/response_cases.py: small_pivot): status 1 in lane 2, whose neighbours equal those of a batch
    in which lane 2 holds another uniform state"""
    case, cbs = RC.small_pivot()
    plain = RC.Case('small pivot: the state', case.D, case.q, case.cb, case.x, 0.0)
    start = _modes.default_start(8, 2, case.nx, 0)
    results = []
    for lane2 in (cbs[RC.SMALL_PIVOT_LANE], cbs[0]):
        levels = list(cbs)
        levels[RC.SMALL_PIVOT_LANE] = lane2
        with open_solver(plain, B) as s:
            states = [(np.full((2, case.nx), cb), np.zeros(case.nx)) for cb in levels]
            load(s, plain, np.zeros(B), states, np.zeros((B, 2)))
            assert (s.solve_stationary() == 0).all()
            s.set_lanes(list(range(B)), np.stack([c for c, _ in states]), np.stack([phi for _, phi in states]))
            s.set_reactions(case.reactions)
            results.append(raw(s, start, iterations=3))
    got, clean = results
    want = np.zeros(B, np.int32)
    want[RC.SMALL_PIVOT_LANE] = 1
    assert np.array_equal(got['status'], want) and (clean['status'] == 0).all()
    for k in ALL:
        assert np.array_equal(np.delete(got[k], RC.SMALL_PIVOT_LANE, axis=0), np.delete(clean[k], RC.SMALL_PIVOT_LANE, axis=0)), k


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def slowest_mode():
    """N = 3, nx = 48, Stern wall, steric ions: (case, c*, phi*, lambda_1, dc, dphi) of the slowest converged real mode of the device's
    own stationary state, scaled so that the largest relative change of a concentration is 1"""
    case = RC.small(3, 48, stern=True, steric=True)
    with open_solver(case, 1, tol=1e-12) as s:
        load(s, case, [case.phiM], [case.bulk_state()], np.zeros((1, 3)))
        assert (s.solve_stationary() == 0).all()
        c, phi = s.get_state(derived=False)
        res = s.get_relaxation(nmodes=8, profiles=True)
        LAUNCHED.add(s._mode_solver.last_kernel)
        assert res['status'][0] == 0 and res['stable'][0] is True
        j = [j for j in range(8) if res['converged'][0, j] and res['rates'][0, j].imag == 0.0][0]
        lam = res['rates'][0, j].real
        dc, dphi = res['dc'][0, j].real, res['dphi'][0, j].real
        scale = np.abs(dc / c[0]).max()
        poles = s.get_response(omega=[abs(lam), 0.1 * abs(lam)])
    return case, c[0], phi[0], lam, dc / scale, dphi / scale, poles


def test_one_backward_euler_step_of_the_solver_halves_the_slowest_mode(slowest_mode):
    """The solver itself, with dt = 1 / lambda_1: from u* + eps mode_1 (set_lanes) one step leaves u* + eps mode_1 / 2 up to the
    second-order term, which is linear in eps: the deviation at eps = 1e-4 lies between 1/12 and 1/8 of that at eps = 1e-3 (the window
    of tests/test_modes_abi.py, where the oracle's step gives 3.6e-5 and 3.6e-6)."""
    case, c, phi, lam, dc, dphi, _ = slowest_mode
    assert lam > 0
    eps = np.array([1e-3, 1e-4])
    s = PnpSolver(case.N, case.nx, case.dx, 1.0 / lam, RC.BETA, RC.EPS, case.D, case.q, method='Newton', batch_capacity=2)
    with s:
        s.set_newton(wall_bc='stern', stern_capacitance=case.CS, mpb_radius=case.radii, tol=1e-12, maxit=50)
        s.set_grid(case.x)
        load(s, case, [case.phiM] * 2, [(c, phi)] * 2, np.zeros((2, 3)))
        s.set_lanes([0, 1], np.stack([c + e * dc for e in eps]), np.stack([phi + e * dphi for e in eps]))
        s.step(1)
        assert (s.get_status() == 0).all()
        c1, _ = s.get_state(derived=False)
    dev = [np.abs((c1[i] - c) - 0.5 * e * dc).max() / np.abs(0.5 * e * dc).max() for i, e in enumerate(eps)]
    print('lambda_1 = %.6e 1/s: deviation from one half %.3e at eps = 1e-3, %.3e at eps = 1e-4, ratio %.2f' % (lam, dev[0], dev[1], dev[0] / dev[1]))
    assert 1.0 / 12.0 <= dev[1] / dev[0] <= 1.0 / 8.0, dev
    assert dev[0] < 1e-2


def test_the_admittance_is_finite_and_moves_between_the_pole_and_a_tenth_of_it(slowest_mode):
    """Qualitative only: at omega = |lambda_1| and 0.1 |lambda_1| the response of the charge is finite and the admittance differs"""
    poles = slowest_mode[-1]
    assert (poles['status'] == 0).all()
    assert np.isfinite(np.abs(poles['dsigma'])).all() and np.isfinite(np.abs(poles['admittance'])).all()
    assert poles['admittance'][0, 0] != poles['admittance'][0, 1]
