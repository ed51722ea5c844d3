"""libcatint_sens on the device (PnpSolver.get_sensitivities) against the NumPy restatement of include/catint_sens.h in
tests/sens_ref.py, which tests/test_sens_abi.py pins to the oracle (the method of tests/test_gpu_couple.py).

For every case the oracle's converged states of B = 5 operating points (the case's phiM times 1, 0.75, 0.5, 0.25, 0.1) are uploaded, one
solve_stationary runs, the device's own state is downloaded and the reference is linearised AT THAT STATE.  The small cases run with
prescribed wall fluxes 0.02 D_k c_bulk,k / L (-1)^k: without a flux, a reaction or a velocity the state does not depend on D at all.
The parameter list of a case holds every kind the case supports and a direction in bulk composition.

Tolerance: per output and system, 10 x the disagreement of the reference's two methods (banded LU with all columns; the Schur recursion
with reduced right-hand sides) on that system -- the largest over the columns -- not below 1e-11: the project's rule from
tests/test_gpu_response.py.  That disagreement must itself stay below 1e-8 (asserted).  The error of a column is its max-norm relative to
the column's maximum.  Every test prints the worst ratio of device error to tolerance.  Measured on the
MI355X for the general reaction and wall tables of cases G and G8: G 0.12 / 0.15 at nx = 5 / 21, G8 0.14 / 0.29 at nx = 7 / 34, with
reference disagreements up to 2.4e-11 (G) and 4.7e-12 (G8).  Everything that can be exact is asserted bit for bit."""
import numpy as np
import pytest

from catint_amd import PnpSolver, _sens          # fails without the feature
from tests import couple_ref as CR
from tests import response_cases as RC
from tests import sens_ref as SR
from tests.test_sens_abi import INSTANCES

pytestmark = pytest.mark.gpu

B = len(RC.SCALES)
ALL = list(_sens.FIELDS)
PC = _sens.CHUNK
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


def load(s, case, phis, states, flux, wall_k=None):
    n = len(phis)
    pb = np.zeros((n, 4))
    pb[:, 0] = phis
    s.set_batch(np.stack([c for c, _ in states]), pb, np.zeros(n), flux)
    s.set_lanes(list(range(n)), np.stack([c for c, _ in states]), np.stack([phi for _, phi in states]))
    if case.wall is not None:
        sp, nu, k, al, sat = case.wall
        s.set_wall_kinetics(sp, nu, np.tile(np.asarray(k, float), (n, 1)) if wall_k is None else wall_k, al, sat)


def small_flux(case):
    """[N] 2 % of D c_bulk / L, alternating in sign"""
    L = case.x[-1] - case.x[0]
    return 0.02 * case.D * case.cb / L * (-1.0) ** np.arange(case.N)


def every_kind(case):
    specs = ['phiM', 'velocity'] + [(kind, j) for kind in ('flux', 'c_bulk', 'D') for j in range(case.N)]
    if case.CS is not None:
        specs.append('stern_capacitance')
    for r in range(len(case.reactions)):
        specs += [('kf', r), ('kr', r)]
    if case.wall is not None:
        specs += [('wall_k', r) for r in range(len(case.wall[0]))]
    return specs


def prepared(case, flux):
    """(solver, phis, flux [B][N], [(problem, c, phi)] at the device's own state), solved once per session"""
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
        _cache[case.name] = (s, phis, fl, [(case.make(phis[b], fl[b]), c[b], phi[b]) for b in range(B)])
    return _cache[case.name]


def from_the_bulk(case, phis, flux):
    """a handle whose lanes the device itself solved from the bulk state (small potentials)"""
    key = (case.name, len(phis), flux is None)
    if key not in _cache:
        n = len(phis)
        s = open_solver(case, n)
        fl = np.tile(np.zeros(case.N) if flux is None else flux, (n, 1))
        load(s, case, phis, [case.bulk_state()] * n, fl)
        assert (s.solve_stationary() == 0).all()
        _cache[key] = (s, np.asarray(phis, float), fl, None)
    return _cache[key][0]


@pytest.fixture(scope='module', autouse=True)
def close_all():
    yield
    for entry in _cache.values():
        entry[0].close()
    _cache.clear()


def call(s, specs, **kw):
    out = s.get_sensitivities(specs, **kw)
    LAUNCHED.add(s._sensitizer.last_kernel)
    assert s._sensitizer.last_kernel_ms > 0.0
    return out


def raw(s, specs, lanes=None, flux=None, **kw):
    """catsens_solve with the parameter list exactly as given (get_sensitivities solves every distinct column once)"""
    o = s._obs
    if getattr(s, '_sensitizer', None) is None:
        s._sensitizer = _sens.Sensitizer(o['device'])
    idx = np.arange(s.B) if lanes is None else np.asarray(lanes)
    fl = (o['flux'] if flux is None else flux)[idx]
    out = s._sensitizer.solve(s.device_view(), o['D'], o['charges'], o['x'], o['beta'], o['eps'], o['dx'], o['phiM'], fl, specs, lanes=idx,
                              mpb_radius=o['mpb_radius'], wall_bc=o['wall_bc'], stern_capacitance=o['stern_capacitance'], phi_pzc=o['phi_pzc'],
                              velocity=o['velocity'], reactions=o['reactions'], wall=o['wall'], **kw)
    LAUNCHED.add(s._sensitizer.last_kernel)
    return out


def pieces(specs, N):
    """`specs` in order, cut where a call would exceed the _sens.MAX_PARAMS distinct columns it takes (a direction in bulk composition
    counts the single-species columns it weighs)"""
    out, cols = [[]], set()
    for spec in specs:
        if isinstance(spec, str):
            new = {(spec, 0)}
        elif np.ndim(spec[1]) > 0:
            new = {('c_bulk', k) for k in range(N) if spec[1][k] != 0.0}
        else:
            new = {(spec[0], int(spec[1]))}
        if len(cols | new) > _sens.MAX_PARAMS:
            out.append([])
            cols = set()
        out[-1].append(spec)
        cols |= new
    return out


def call_all(s, specs):
    """get_sensitivities over a list of any length (case G8 has 67 distinct columns): one call per piece, the results joined"""
    parts = [call(s, part) for part in pieces(specs, s.N)]
    got = {k: np.concatenate([g[k] for g in parts], axis=1) for k in ALL}
    got['elasticity'] = {k: np.concatenate([g['elasticity'][k] for g in parts], axis=1) for k in parts[0]['elasticity']}
    got['parameters'] = [spec for g in parts for spec in g['parameters']]
    got['status'] = np.max([g['status'] for g in parts], axis=0)
    return got


def check(case, flux):
    """The device against the reference linearised at the device's state: the worst error / tolerance over points, outputs, columns"""
    s, phis, fl, lin = prepared(case, flux)
    specs = every_kind(case) + [('c_bulk', case.cb.copy())]
    got = call_all(s, specs)
    assert (got['status'] == 0).all(), got['status']
    assert got['parameters'] == specs and sorted(got['elasticity']) == ['dcurrent', 'dwall_flux']
    worst, worst_dis, where = 0.0, 0.0, ''
    for b, (p, c, phi) in enumerate(lin):
        ra, rb = SR.sensitivities(p, c, phi, specs, fl[b], 'banded'), SR.sensitivities(p, c, phi, specs, fl[b], 'schur')
        dis = SR.disagreement(ra, rb)
        err = SR.disagreement({k: got[k][b] for k in SR.FIELDS}, ra)
        for k in SR.FIELDS:
            assert dis[k].max() < 1e-8, (case.name, b, k, dis[k])
            tol = max(10.0 * dis[k].max(), 1e-11)
            m = int(np.argmax(err[k]))
            if err[k][m] / tol > worst:
                where = 'point %d, %s of %s: error %.2e, reference disagreement %.2e' % (b, k, specs[m], err[k][m], dis[k].max())
            worst, worst_dis = max(worst, err[k][m] / tol), max(worst_dis, dis[k].max())
    print('%s: worst device error / tolerance %.3f (reference disagreement up to %.1e; %s)' % (case.name, worst, worst_dis, where))
    assert worst <= 1.0, (case.name, worst, where)
    return got, specs


def same(a, b, keys=None):
    for k in (keys or a):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- against the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', range(1, 9))
@pytest.mark.parametrize('nx', [3, 4, 19])
def test_every_block_size_at_the_smallest_grids_and_a_short_one(N, nx):
    """nx = 3: the bulk right-hand side feeds the only interior row; nx = 4: the first grid on which first_row enters a point"""
    case = RC.small(N, nx)
    got, specs = check(case, small_flux(case))
    assert all(np.abs(got['dc_surface'][:, m]).max() > 0 for m in range(len(specs)))          # no column is zero once the fluxes are on


@pytest.mark.parametrize('N', [2, 4, 8])
def test_stern_and_steric_variants(N):
    for stern, steric in ((True, True), (True, False), (False, True)):
        case = RC.small(N, 19, stern=stern, steric=steric)
        check(case, small_flux(case))


def test_case_F_every_term_of_the_physics_with_its_wall_table():
    got, specs = check(RC.case_F(), np.array([0.0, -1e-6, 1e-6]))
    # the elasticities: d ln|y| / d ln p from the outputs, the recorded parameters and the flux into the domain
    s, phis, fl, lin = prepared(RC.case_F(), None)
    for b, (p, c, phi) in enumerate(lin):
        jw = SR.wall_flux(p, c, phi, fl[b])
        m = specs.index(('kf', 0))
        want = got['dcurrent'][b, m] * p.reactions[0]['kf'] / (p.q * jw).sum()
        assert np.isclose(got['elasticity']['dcurrent'][b, m], want, rtol=1e-12)
        m = specs.index(('wall_k', 0))
        assert np.allclose(got['elasticity']['dwall_flux'][b, m, 1:], got['dwall_flux'][b, m, 1:] * p.wall_kinetics[0]['k'] / jw[1:], rtol=1e-12)
        assert np.isnan(got['elasticity']['dwall_flux'][b, m, 0])          # species 0 carries no flux: y = 0
        assert np.isnan(got['elasticity']['dcurrent'][b, specs.index(('flux', 0))])          # p = 0


def test_case_E_block_size_nine():
    check(RC.case_E(34), None)


FLUX_G = np.array([0.0, -1e-6, 1e-6, 0.0])
G_CASES = {'G nx=5': lambda: (RC.case_G(5), FLUX_G), 'G nx=21': lambda: (RC.case_G(21), FLUX_G),
           'G8 nx=7': lambda: (RC.case_G8(7), None), 'G8 nx=34': lambda: (RC.case_G8(34), None)}


@pytest.mark.parametrize('name', sorted(G_CASES))
def test_general_reaction_and_wall_tables(name):
    """Cases G and G8 (tests/response_cases.py): every shape of an entry of the reaction and wall tables, in the rows of the Jacobian and
    in the 'kf', 'kr' and 'wall_k' columns of every reaction (G8: 16 reactions and 8 wall reactions, 67 parameters and a direction in
    bulk composition; a call takes 64 columns: one call of eight chunks and one of two)"""
    case, flux = G_CASES[name]()
    got, specs = check(case, flux)
    assert len(specs) == {4: 27, 8: 68}[case.N] and len(specs) > PC
    # a column is zero exactly where net is: no reaction of these tables cancels, so every rate constant moves the surface
    for m, spec in enumerate(specs):
        if not isinstance(spec, str) and spec[0] in ('kf', 'kr', 'wall_k'):
            assert np.abs(got['dc_surface'][:, m]).max() > 0, spec


def test_table_entries_without_effect_change_no_bit_and_a_dropped_reaction_does():
    """tests/response_cases.py: table_properties, over the parameter list of case G"""
    case = RC.case_G(21)
    s, phis, fl, lin = prepared(case, FLUX_G)
    specs = every_kind(case) + [('c_bulk', case.cb.copy())]
    # without its first reaction the table has three: the columns of reaction 3 do not exist then
    specs = [sp for sp in specs if sp not in (('kf', 3), ('kr', 3))]
    RC.table_properties(s, case, lambda: {k: v for k, v in call(s, specs).items() if k in ALL + ['status']}, ALL)


def test_the_cases_reach_every_instance():
    """(after the cases above in file order: LAUNCHED collects last_kernel of every call)"""
    assert LAUNCHED == INSTANCES, sorted(LAUNCHED ^ INSTANCES)


def test_a_diffusion_coefficient_without_flux_reaction_or_velocity_has_no_effect():
    """exactly 0: every entry of the right-hand side is"""
    case = RC.small(3, 19, stern=True)
    s = from_the_bulk(case, -0.1 * np.linspace(0.2, 1.0, 4), None)
    got = call(s, [('D', 0), 'phiM', ('D', 2), ('D', 1)])
    assert (got['status'] == 0).all()
    for m in (0, 2, 3):
        for k in ALL:
            assert (got[k][:, m] == 0.0).all(), (k, m)
    assert (got['dphi_surface'][:, 1] != 0.0).all()


# ---- against the other libraries ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['F', 'E', 'N=4'])
def test_the_control_columns_are_those_of_libcatint_response_and_libcatint_couple(name):
    """The PHIM and ('flux', j) columns against get_response(omega = [0]) and, without a wall table, get_coupling's T_c / T_phi: within
    the tolerance of the parity checks.  The kernels form the rows of the Jacobian with the same functions (csrc/pnp_team.h) and put a
    column through the same operations in the same order: bit-identical on the MI355X, which is asserted."""
    case, flux = {'F': lambda: (RC.case_F(), np.array([0.0, -1e-6, 1e-6])), 'E': lambda: (RC.case_E(34), None),
                  'N=4': lambda: (RC.small(4, 19, True, True), small_flux(RC.small(4, 19, True, True)))}[name]()
    s, phis, fl, lin = prepared(case, flux)
    specs = ['phiM'] + [('flux', j) for j in range(case.N)]
    got = call(s, specs)
    pairs = {'dphi_surface': 'dphi_surface', 'dc_surface': 'dc_surface', 'dsigma': 'dsigma', 'dwall_flux': 'dwall_flux', 'dcurrent': 'admittance'}
    worst, exact = 0.0, True
    tols = []
    for b, (p, c, phi) in enumerate(lin):
        dis = SR.disagreement(SR.sensitivities(p, c, phi, specs, fl[b], 'banded'), SR.sensitivities(p, c, phi, specs, fl[b], 'schur'))
        tols.append({k: max(10.0 * dis[k].max(), 1e-11) for k in SR.FIELDS})
    for m, spec in enumerate(specs):
        r = s.get_response(omega=[0.0], perturbation=spec)
        assert (r['status'] == 0).all() and (r['dc_surface'].imag == 0).all()
        for k, rk in pairs.items():
            for b in range(B):
                worst = max(worst, SR.rel_columns(np.atleast_1d(got[k][b, m])[None], np.atleast_1d(r[rk][b, 0].real)[None])[0] / tols[b][k])
            exact = exact and np.array_equal(got[k][:, m], r[rk][:, 0].real)
    if case.wall is None:
        zero = {'flux': np.zeros((B, case.N)), 'dflux_dc': np.zeros((B, case.N, case.N)), 'dflux_dphi': np.zeros((B, case.N, 2))}
        T = s.get_coupling(fl, zero, fields=['T_c', 'T_phi'])
        for b in range(B):
            worst = max(worst, CR.rel_T(got['dc_surface'][b, 1:].T, T['T_c'][b]) / tols[b]['dc_surface'],
                        CR.rel(got['dphi_surface'][b, 1:], T['T_phi'][b]) / tols[b]['dphi_surface'])
        exact = exact and np.array_equal(got['dc_surface'][:, 1:].transpose(0, 2, 1), T['T_c']) and np.array_equal(got['dphi_surface'][:, 1:], T['T_phi'])
    print('%s: control columns against libcatint_response%s: worst difference / tolerance %.3f, bit-identical: %s'
          % (case.name, '' if case.wall is not None else ' and libcatint_couple', worst, exact))
    assert worst <= 1.0
    assert exact


# ---- bit for bit -------------------------------------------------------------------------------------------------------------------
def bitwise_handle(N, n):
    case = RC.small(N, 19, stern=(N == 4), steric=(N == 8))
    s = from_the_bulk(case, -0.1 * np.linspace(0.1, 1.0, n), small_flux(case))
    return s, every_kind(case)


@pytest.mark.parametrize('N, n', [(2, 23), (4, 13), (8, 8)])
def test_waves_lanes_lists_chunks_and_requested_outputs_do_not_change_the_bits(N, n):
    """Batches beyond one wave's teams (21, 12, 7) that are no multiples of them"""
    s, specs = bitwise_handle(N, n)
    P = len(specs)
    before = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    want = raw(s, specs)
    assert (want['status'] == 0).all() and all(np.isfinite(want[k]).all() for k in ALL)
    assert all(np.abs(want['dc_surface'][:, m]).max() > 0 for m in range(P))
    same(raw(s, specs, max_waves=1), want)
    same(raw(s, specs, max_waves=2), want)
    same({k: v for k, v in call(s, specs).items() if k in ALL + ['status']}, want)
    rng = np.random.RandomState(N)
    for lanes in (rng.permutation(n), np.array([n - 1, 0, 0, n // 2, n - 1]), np.array([n // 2]), np.arange(n - 1)):
        got = raw(s, specs, lanes=lanes, max_waves=int(rng.randint(0, 3)))
        for k in ALL + ['status']:
            assert np.array_equal(got[k], want[k][lanes]), (k, lanes)
    # permuted and repeated lists; lists of PC + 1 and 2 PC + 3 parameters against the same parameters asked one at a time
    alone = [raw(s, [spec]) for spec in specs]
    for m in range(P):
        for k in ALL:
            assert np.array_equal(alone[m][k][:, 0], want[k][:, m]), (k, specs[m])
    for order in (rng.permutation(P), np.arange(PC + 1) % P, (3 + np.arange(2 * PC + 3)) % P, np.array([P - 1, 0, 0, P - 1]), np.array([P // 2])):
        got = raw(s, [specs[m] for m in order], max_waves=int(rng.randint(0, 3)))
        assert np.array_equal(got['status'], want['status'])
        for k in ALL:
            assert np.array_equal(got[k], want[k][:, order]), (k, order)
    for fields in (['dcurrent'], ['dsigma', 'dphi_surface'], ['dc_surface'], ['dwall_flux', 'dcurrent']):
        got = raw(s, specs, fields=fields)
        assert sorted(got) == sorted(fields + ['status'])
        same(got, want, fields + ['status'])
    # outputs not asked for stay untouched: room for n + 1 points, and rows the call does not name
    out = {k: np.full((n + 1, P) + _sens.FIELDS[k](N), 7.0) for k in ALL}
    out['status'] = np.full(n + 1, 77, np.int32)
    named = ['dc_surface', 'dsigma']
    part = {k: out[k][:n] for k in named + ['status']}
    raw(s, specs, fields=named, out=part)
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
    specs = ['phiM', ('c_bulk', 0), ('D', 1), 'velocity', ('flux', 1)]
    flux = np.tile(small_flux(case), (B, 1))
    results = []
    for phis in (np.zeros(B), np.array([0.0, 0.0, -0.8, 0.0, 0.0])):
        with open_solver(case, B, maxit=1) as s:
            load(s, case, phis, [case.bulk_state()] * B, np.zeros((B, 2)))
            status = s.solve_stationary()
            results.append((status, call(s, specs, flux=flux)))
            if not phis.any():
                bad = flux.copy()
                bad[3, 1] = np.nan
                nan_in = call(s, specs, flux=bad)
                bad = flux.copy()
                bad[0, 0] = np.inf
                inf_in = call(s, specs, flux=bad)
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
    specs = ['phiM', ('kf', 0), ('D', 0), ('c_bulk', 1)]
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
            results.append(call(s, specs))
    got, clean = results
    want = np.zeros(B, np.int32)
    want[RC.SMALL_PIVOT_LANE] = 1
    assert np.array_equal(got['status'], want) and (clean['status'] == 0).all()
    for k in ALL:
        assert np.array_equal(np.delete(got[k], RC.SMALL_PIVOT_LANE, axis=0), np.delete(clean[k], RC.SMALL_PIVOT_LANE, axis=0)), k


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_central_differences_of_the_device_s_own_states():
    """One handle holds the lanes p, p + h, p - h for the parameters a handle takes per lane -- phiM, the wall flux of species 1, the rate
    constant of the wall reaction -- of case F; one stationary solve; the central differences of the device's own surface states
    against get_sensitivities of the middle lane.  Bound: 5 x the error of the same difference formed with the oracle on the CPU at
    that step (computed here), not below 1e-7."""
    case = RC.case_F()
    base_flux = np.array([0.0, -1e-6, 1e-6])
    p0, c0, phi0 = case.solve(flux=base_flux)
    k0 = float(case.wall[2][0])
    steps = {'phiM': 1e-3 * abs(case.phiM), ('flux', 1): 1e-2 * abs(base_flux[1]), ('wall_k', 0): 1e-2 * k0}
    specs = list(steps)
    n = 1 + 2 * len(specs)
    phis, flux, wk = np.full(n, case.phiM), np.tile(base_flux, (n, 1)), np.full((n, 1), k0)
    for m, spec in enumerate(specs):
        for sgn, lane in ((1.0, 1 + 2 * m), (-1.0, 2 + 2 * m)):
            if spec == 'phiM':
                phis[lane] += sgn * steps[spec]
            elif spec[0] == 'flux':
                flux[lane, spec[1]] += sgn * steps[spec]
            else:
                wk[lane, 0] += sgn * steps[spec]
    with open_solver(case, n, tol=1e-12) as s:
        load(s, case, phis, [(c0, phi0)] * n, flux, wall_k=wk)
        assert (s.solve_stationary() == 0).all()
        cs, vs, _ = s.get_surface()
        got = call(s, specs, lanes=[0])
    assert got['status'][0] == 0
    ref = SR.sensitivities(p0, c0, phi0, specs, base_flux)
    import copy
    from oracle import pnp_physical as PH
    worst = 0.0
    for m, spec in enumerate(specs):
        dev = np.concatenate([got['dc_surface'][0, m], [got['dphi_surface'][0, m]]])
        fd = (np.concatenate([cs[1 + 2 * m], [vs[1 + 2 * m]]]) - np.concatenate([cs[2 + 2 * m], [vs[2 + 2 * m]]])) / (2 * steps[spec])
        err = np.abs(fd - dev).max() / np.abs(dev).max()
        ends = []
        for sgn in (1.0, -1.0):
            pp = case.make(flux=base_flux.copy())
            pp.wall_kinetics = copy.deepcopy(pp.wall_kinetics)
            if spec == 'phiM':
                pp.phiM += sgn * steps[spec]
            elif spec[0] == 'flux':
                pp.flux[spec[1]] += sgn * steps[spec]
            else:
                pp.wall_kinetics[0]['k'] += sgn * steps[spec]
            c2, phi2, it, _ = PH.newton_step(pp, c0, phi0, c0, np.inf, tol=1e-12, maxit=80)
            assert it <= 80
            ends.append(np.concatenate([c2[:, 0], [phi2[0]]]))
        mine = np.concatenate([ref['dc_surface'][m], [ref['dphi_surface'][m]]])
        cpu = np.abs((ends[0] - ends[1]) / (2 * steps[spec]) - mine).max() / np.abs(mine).max()
        bound = max(5.0 * cpu, 1e-7)
        print('%s: device difference against get_sensitivities %.2e, the oracle\'s difference against the reference %.2e, bound %.1e'
              % (spec, err, cpu, bound))
        worst = max(worst, err / bound)
    assert worst <= 1.0, worst
