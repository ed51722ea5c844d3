"""libcatint_response on the device (PnpSolver.get_response) against the NumPy restatement of include/catint_response.h in
tests/response_ref.py, which tests/test_response_abi.py pins to known answers.

For every case the oracle's converged states of B = 5 operating points (the case's phiM times 1, 0.75, 0.5, 0.25, 0.1) are uploaded, one
solve_stationary runs, the device's own state is downloaded and the reference is linearised AT THAT STATE.  Frequencies: 0, 1 / tau_D,
1 / tau_DL, 100 / tau_DL (tau_D = L^2 / D_min, tau_DL = lambda_D L / D_max).

Tolerance.  Neither the conditioning of a case nor the device's rounding can be derived in advance, so the tolerance per case,
operating point and frequency is measured on the reference side: 10 x the disagreement between the reference's two solution methods
(LAPACK banded LU with pivoting; block elimination from the bulk) on that system, not below 1e-11, in the per-unknown max-norm (every
unknown's profile, and every scalar, scaled by its own maximum).  The factor 10 covers a third backward-stable elimination of the same
matrix in another order.  That disagreement must itself stay below 1e-8, or the case tests nothing (asserted).  The worst ratios
device error / tolerance are printed by every test.  Measured on the MI355X (also in DESIGN.md section 7g): case F 0.59 (phiM) and 0.65
(flux), case E 0.32 / 0.36 / 0.67 at nx = 34 / 130 / 514 with reference disagreements up to 3.8e-10 (F) and 3.1e-9 (E), the small cases
of every block size at most 0.37, Debye-Hueckel at most 0.005; the general reaction and wall tables of cases G and G8: G 0.24 / 0.11
at nx = 5 / 21, G8 0.40 / 0.76 at nx = 7 / 34 (point 2, omega = 8.1e5 / s: 7.95e-12 against 1.05e-11), with reference disagreements
up to 4.9e-11 (G) and 2.2e-10 (G8).
Everything that can be exact is asserted bit for bit."""
import os

import numpy as np
import pytest

from catint_amd import PnpSolver, _response          # fails without the feature
from tests import response_cases as RC
from tests import response_ref as RR
from tests.test_response_abi import INSTANCES

pytestmark = pytest.mark.gpu

B = len(RC.SCALES)
LAUNCHED = set()
_cache = {}


def open_solver(case, phis, maxit=50, tol=1e-10):
    s = PnpSolver(case.N, case.nx, case.dx, 1.0, RC.BETA, RC.EPS, case.D, case.q, method='Newton', batch_capacity=len(phis))
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
    flux = np.zeros((n, case.N)) if case.flux is None else np.repeat(case.flux[None], n, axis=0)
    s.set_batch(np.stack([c for c, _ in states]), pb, np.zeros(n), flux)
    s.set_lanes(list(range(n)), np.stack([c for c, _ in states]), np.stack([phi for _, phi in states]))
    if case.wall is not None:
        sp, nu, k, al, sat = case.wall
        s.set_wall_kinetics(sp, nu, np.repeat(np.asarray(k, float)[None], n, axis=0), al, sat)


def prepared(case):
    """(solver, phis, [(problem, c, phi)] at the device's own state) of a case, solved once per session"""
    if case.name not in _cache:
        phis = case.phiM * np.array(RC.SCALES)
        states, st = [None] * B, None
        for b in np.argsort(np.abs(phis)):                    # continuation from the smallest potential up
            if phis[b] == 0.0:
                states[b] = case.bulk_state()
            else:
                _, c, phi = case.solve(phis[b], start=st, tol=1e-11) if st is not None else case.solve(phis[b], tol=1e-11)
                states[b] = st = (c, phi)
        s = open_solver(case, phis)
        load(s, case, phis, states)
        status = s.solve_stationary()
        assert (status == 0).all(), (case.name, status)
        c, phi = s.get_state(derived=False)
        _cache[case.name] = (s, phis, [(case.make(phis[b]), c[b], phi[b]) for b in range(B)])
    return _cache[case.name]


@pytest.fixture(scope='module', autouse=True)
def close_all():
    yield
    for s, _, _ in _cache.values():
        s.close()
    _cache.clear()


def call(s, **kw):
    out = s.get_response(**kw)
    LAUNCHED.add(s._responder.last_kernel)
    return out


def same(a, b, keys=None):
    keys = [k for k in a if k != 'omega'] if keys is None else keys
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def check(case, perturbation='phiM', omega=None, profiles=True, lanes=None):
    """The device against the reference linearised at the device's state: the worst error / tolerance over points and frequencies"""
    s, phis, lin = prepared(case)
    omega = case.omegas() if omega is None else np.asarray(omega, float)
    got = call(s, omega=omega, perturbation=perturbation, profiles=profiles, lanes=lanes)
    idx = range(B) if lanes is None else lanes
    assert (got['status'] == 0).all(), got['status']
    worst, worst_dis, where = 0.0, 0.0, ''
    for i, b in enumerate(idx):
        p, c, phi = lin[b]
        for f, w in enumerate(omega):
            ra, rb = RR.response(p, c, phi, w, perturbation, 'banded'), RR.response(p, c, phi, w, perturbation, 'elimination')
            if not profiles:                       # the disagreement on what is compared: the scalars alone
                ra, rb = {k: ra[k] for k in RR.SCALARS}, {k: rb[k] for k in RR.SCALARS}
            dis = RR.disagreement(ra, rb)
            assert dis < 1e-8, (case.name, b, w, dis)
            tol = max(10.0 * dis, 1e-11)
            dev = {k: got[k][i, f] for k in RR.SCALARS}
            if profiles:
                dev['dc'], dev['dphi'] = got['dc'][i, f], got['dphi'][i, f]
            err = RR.disagreement(dev, ra)
            if err / tol > worst:
                where = 'point %d, omega %.3g: error %.2e, reference disagreement %.2e' % (b, w, err, dis)
            worst, worst_dis = max(worst, err / tol), max(worst_dis, dis)
            if w == 0.0:
                assert all(np.all(np.asarray(v).imag == 0.0) for v in dev.values()), (case.name, b)
    print('%s %s: worst device error / tolerance %.3f (reference disagreement up to %.1e; %s)' % (case.name, perturbation, worst, worst_dis, where))
    assert worst <= 1.0, (case.name, worst)
    return got


# ---- against the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('perturbation', ['phiM', ('flux', 1)], ids=['phiM', 'flux'])
def test_case_F_every_term_of_the_physics(perturbation):
    check(RC.case_F(), perturbation)


@pytest.mark.parametrize('nx', [34, 130, 514])
def test_case_E_block_size_nine(nx):
    check(RC.case_E(nx))
    if nx == 34:
        check(RC.case_E(nx), ('flux', 3), profiles=False)


G_CASES = {'G nx=5': lambda: RC.case_G(5), 'G nx=21': lambda: RC.case_G(21), 'G8 nx=7': lambda: RC.case_G8(7), 'G8 nx=34': lambda: RC.case_G8(34)}


@pytest.mark.parametrize('name', sorted(G_CASES))
def test_general_reaction_and_wall_tables(name):
    """Cases G and G8 (tests/response_cases.py): repeated reactants, up to four entries per side, empty sides, sides without a rate,
    a catalyst, several reactions into one dR[j], both tables full; wall reactions that share a driving species, of zeroth order, without
    a potential dependence, with a saturation.  nx = 5: the first grid on which every step of the row walk runs with reactions; nx = 7:
    the smallest that gives G8 several interior block rows.  Real and complex instances, with and without profiles, both perturbations.
    tests/test_response_abi.py shows that every entry of the tables moves these results by at least 1e6 tolerances."""
    case = G_CASES[name]()
    for perturbation in ('phiM', ('flux', 1)):
        for omega in ([0.0], case.omegas()):
            full = check(case, perturbation, omega=omega, profiles=True)
            scal = check(case, perturbation, omega=omega, profiles=False)
            assert same(scal, full, list(RR.SCALARS) + ['status'])


@pytest.mark.parametrize('N, nx, stern, steric', [(1, 3, False, False), (2, 4, True, False), (2, 66, False, True), (3, 9, True, True),
                                                  (4, 12, False, False), (5, 11, True, True), (6, 10, False, True), (7, 13, True, False),
                                                  (8, 7, False, False)])
def test_small_ends_and_every_block_size(N, nx, stern, steric):
    """Every block size with its four instances: real and complex, scalars only and profiles"""
    case = RC.small(N, nx, stern, steric)
    for omega in ([0.0], case.omegas()):
        full = check(case, omega=omega, profiles=True)
        scal = check(case, omega=omega, profiles=False)
        assert same(scal, full, list(RR.SCALARS) + ['status'])      # a scalars-only call and a profiles call return the same scalars


def test_debye_hueckel_orders_on_the_device():
    for stern, lo, hi in ((False, 3.6, 4.4), (True, 1.8, 2.2)):
        errs = []
        for nx in (41, 81):
            case = RC.debye_hueckel(nx, stern)
            got = check(case, omega=[0.0], profiles=False)
            want = RC.EPS / case.lam if not stern else 1.0 / (1.0 / 0.2 + case.lam / RC.EPS)
            errs.append(got['differential_capacitance'][0] / want - 1.0)
        print('Debye-Hueckel on the device, %s wall: %+.3e %+.3e' % ('Stern' if stern else 'Dirichlet', errs[0], errs[1]))
        assert lo <= errs[0] / errs[1] <= hi


def test_system_counts_that_do_not_fill_the_last_wave():
    case = RC.case_E(34)
    w = case.omegas()
    full = check(case, omega=w[:3], profiles=False)                  # 5 x 3 = 15 systems on 7 teams per wave
    one = check(case, omega=w[2:3], profiles=False, lanes=[3])       # one point x one frequency
    assert same({k: one[k][0, 0] for k in RR.SCALARS}, {k: full[k][3, 2] for k in RR.SCALARS})


def test_the_cases_reach_every_instance():
    """(after the cases above in file order: LAUNCHED collects last_kernel of every call)"""
    assert LAUNCHED == INSTANCES, sorted(LAUNCHED ^ INSTANCES)


# ---- exact properties --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['F', 'E'])
def test_any_number_of_waves_gives_the_same_bits(name):
    case = RC.case_F() if name == 'F' else RC.case_E(34)
    s, _, _ = prepared(case)
    want = call(s, omega=case.omegas(), profiles=True)
    for waves in (1, 2, 3):
        assert same(call(s, omega=case.omegas(), profiles=True, max_waves=waves), want), waves
    want = call(s, omega=[0.0], profiles=False)
    for waves in (1, 2):
        assert same(call(s, omega=[0.0], profiles=False, max_waves=waves), want), waves


def test_table_entries_without_effect_change_no_bit_and_a_dropped_reaction_does():
    """tests/response_cases.py: table_properties, in the complex instance with profiles and the real one without, for both perturbations"""
    case = RC.case_G(21)
    s, _, _ = prepared(case)

    def outputs():
        out = {}
        for pert in ('phiM', ('flux', 1)):
            cx = call(s, omega=case.omegas(), perturbation=pert, profiles=True)
            re = call(s, omega=[0.0], perturbation=pert)
            out.update({'%s complex %s' % (pert, k): v for k, v in cx.items()})
            out.update({'%s real %s' % (pert, k): v for k, v in re.items()})
        return out
    moves = ['%s %s %s' % (pert, inst, k) for pert in ('phiM', ('flux', 1)) for inst in ('complex', 'real') for k in RR.SCALARS]
    moves += ['%s complex %s' % (pert, k) for pert in ('phiM', ('flux', 1)) for k in ('dc', 'dphi')]
    RC.table_properties(s, case, outputs, moves)


def test_lane_subsets_permutations_and_permuted_frequencies():
    case = RC.case_F()
    s, _, _ = prepared(case)
    w = case.omegas()
    want = call(s, omega=w, profiles=True)
    lanes = [4, 0, 0, 2, 4, 3]
    got = call(s, omega=w, profiles=True, lanes=lanes)
    for k in list(RR.SCALARS) + ['dc', 'dphi', 'status']:
        assert np.array_equal(got[k], want[k][lanes]), k
    assert np.array_equal(got['differential_capacitance'], want['differential_capacitance'][lanes])
    perm = [2, 0, 3, 1]
    got = call(s, omega=w[perm], profiles=True)
    for k in list(RR.SCALARS) + ['dc', 'dphi', 'status']:
        assert np.array_equal(got[k], want[k][:, perm]), k
    # the first omega = 0 of the list gives the differential capacitance, wherever it stands
    assert np.array_equal(got['differential_capacitance'], want['differential_capacitance'])


def test_a_chunked_profiles_call_equals_an_unchunked_one():
    case = RC.case_E(34)
    s, _, _ = prepared(case)
    want = call(s, omega=case.omegas(), profiles=True)
    os.environ['CATRESP_WORKSPACE_BYTES'] = '4096'       # below one wave's records: one wave walks every system
    try:
        got = call(s, omega=case.omegas(), profiles=True)
    finally:
        del os.environ['CATRESP_WORKSPACE_BYTES']
    assert same(got, want)


def test_untouched_outputs_and_the_handle_s_state_stay_as_they_were():
    case = RC.case_F()
    s, _, _ = prepared(case)
    before = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    view = s.device_view()
    o = s._obs
    wall = o['wall']
    N, nx = case.N, case.nx
    out = {k: np.full((3, 2) + _response.SCALARS[k](N, nx), 7.0 + 7.0j) for k in _response.SCALARS}
    out.update({k: np.full((3, 2) + _response.PROFILES[k](N, nx), 7.0 + 7.0j) for k in _response.PROFILES}, status=np.full((3, 2), 77, np.int32))
    # two lanes of room for three: the third lane's entries are not the library's to touch
    view_out = {k: v[:2] for k, v in out.items()}
    s._responder.solve(view, o['D'], o['charges'], o['x'], o['beta'], o['eps'], o['dx'], o['phiM'], omega=[0.0, 1.0 / case.tau_DL], lanes=[1, 3],
                       mpb_radius=o['mpb_radius'], wall_bc=o['wall_bc'], stern_capacitance=o['stern_capacitance'], velocity=o['velocity'],
                       reactions=o['reactions'], wall=wall, profiles=True, out=view_out)
    for k, v in out.items():
        assert (v[2] == (77 if k == 'status' else 7.0 + 7.0j)).all() and not (v[:2] == (77 if k == 'status' else 7.0 + 7.0j)).any(), k
    # a call that asks for one row writes that row alone
    only = s._responder.solve(view, o['D'], o['charges'], o['x'], o['beta'], o['eps'], o['dx'], o['phiM'], lanes=[1, 3], fields=['dsigma'],
                              mpb_radius=o['mpb_radius'], wall_bc=o['wall_bc'], stern_capacitance=o['stern_capacitance'],
                              velocity=o['velocity'], reactions=o['reactions'], wall=wall)
    # (the real instance against omega = 0 of the complex one: the same numbers up to the rounding of the pivots' reciprocals)
    assert sorted(only) == ['dsigma', 'status'] and np.allclose(only['dsigma'][:, 0], out['dsigma'][:2, 0], rtol=1e-8, atol=0.0)
    after = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


# ---- status ------------------------------------------------------------------------------------------------------------------------
def test_an_unconverged_lane_reports_2_and_its_neighbours_are_untouched():
    case = RC.Case('unconverged', RC.D2, RC.Q2, [100.0, 100.0], RC.kornyshev().x, -0.8, radii=[4e-10, 4e-10])
    results = []
    for phis in (np.zeros(B), np.array([0.0, 0.0, -0.8, 0.0, 0.0])):
        with open_solver(case, phis, maxit=1) as s:
            load(s, case, phis, [case.bulk_state()] * B)
            status = s.solve_stationary()
            results.append((status, call(s, omega=[0.0, 1.0 / case.tau_DL], profiles=True)))
    (st0, clean), (st1, got) = results
    assert (st0 == 0).all() and st1[2] != 0 and (np.delete(st1, 2) == 0).all()
    assert (clean['status'] == 0).all() and (got['status'][2] == 2).all() and (np.delete(got['status'], 2, axis=0) == 0).all()
    for k in list(RR.SCALARS) + ['dc', 'dphi']:
        assert np.isnan(got[k][2].real).all() and np.isnan(got[k][2].imag).all(), k
        assert np.array_equal(np.delete(got[k], 2, axis=0), np.delete(clean[k], 2, axis=0)), k
    assert np.isnan(got['differential_capacitance'][2])


def test_a_small_pivot_is_reported_for_its_lane_only():
    """The pivot monitor on data (tests/response_cases.py: small_pivot): in lane 2 the reaction term cancels the diagonal of species 0 to
    6e-14 while the Poisson row holds 5.6e-4 in that column -- partial pivoting would exchange the rows, the kernel must say status 1,
    at omega = 0 only (at omega = 1e6 / s the storage term i omega S restores the pivot), in the real and in the complex instance."""
    from oracle import pnp_physical as PH
    case, cbs = RC.small_pivot()
    plain = RC.Case('small pivot: the state', case.D, case.q, case.cb, case.x, 0.0)
    zeros = np.zeros(B)
    with open_solver(plain, zeros) as s:
        states = [(np.full((2, case.nx), cb), np.zeros(case.nx)) for cb in cbs]
        load(s, plain, zeros, states)
        assert (s.solve_stationary() == 0).all()           # uniform neutral states are stationary: status 0
        # (the solve may move a state by a rounding; set_lanes puts the exact numbers back and leaves the flags alone)
        s.set_lanes(list(range(B)), np.stack([c for c, _ in states]), np.stack([phi for _, phi in states]))
        s.set_reactions(case.reactions)                    # ... and this is what the response linearises
        c, phi = s.get_state(derived=False)
        assert (s.get_status() == 0).all() and all((c[b] == cbs[b]).all() for b in range(B)) and (phi == 0.0).all()
        for b in range(B):                                 # the precondition, on the oracle's Jacobian at the device's state
            case.cb = np.array([cbs[b]] * 2)
            M = PH.residual_and_jacobian(case.make(0.0), c[b], phi[b], c[b], np.inf)[2][case.nx - 2]
            ratio = abs(M[2, 0] / M[0, 0])
            assert ratio > 1e9 if b == RC.SMALL_PIVOT_LANE else ratio < 1.0, (b, ratio)
        cx = call(s, omega=[0.0, 1e6], profiles=True)
        re = call(s, omega=[0.0])
        want = np.zeros((B, 2), np.int32)
        want[RC.SMALL_PIVOT_LANE, 0] = 1
        assert np.array_equal(cx['status'], want) and np.array_equal(re['status'], want[:, :1])
        for b in range(B):
            if b != RC.SMALL_PIVOT_LANE:                   # the neighbours are answered, and rightly
                case.cb = np.array([cbs[b]] * 2)
                ref = RR.response(case.make(0.0), c[b], phi[b], 0.0)
                assert abs(re['dsigma'][b, 0] - ref['dsigma']) <= 1e-8 * abs(ref['dsigma']), b
                assert abs(cx['dsigma'][b, 0] - ref['dsigma']) <= 1e-8 * abs(ref['dsigma']), b


def test_a_nan_in_one_lane_s_state_shows_in_that_lane_only():
    case = RC.small(3, 9, True, True)
    s, phis, lin = prepared(case)
    want = call(s, omega=case.omegas(), profiles=True)
    c, phi = s.get_state(derived=False)
    bad = c[1].copy()
    bad[2, 4] = np.nan
    s.set_lanes([1], bad[None], phi[1][None])
    try:
        got = call(s, omega=case.omegas(), profiles=True)
    finally:
        s.set_lanes([1], c[1][None], phi[1][None])
    assert np.isin(got['status'][1], (1, 2)).all() and (np.delete(got['status'], 1, axis=0) == 0).all()
    for k in list(RR.SCALARS) + ['dc', 'dphi']:
        assert np.array_equal(np.delete(got[k], 1, axis=0), np.delete(want[k], 1, axis=0)), k


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_calculator_response_on_the_co2r_sweep():
    """tp.newton['response'] on the small CO2R sweep of the equil and balance tests (examples/co2r_physical_sweep.py), with the Tafel
    kinetics in the Butler-Volmer form the response can see (a rate constant and alpha = -0.5 F beta: a rate given as a function K(phiM)
    is a constant per lane to the library).  Every lane is status 0 with a finite positive differential capacitance, and the slope of
    the device's own wall flux along the sweep (get_balance), by central differences of neighbouring lanes of spacing h, agrees with
    dwall_flux.  Bound: the central difference is off by h^2 f''' / 6; the potential enters the flux f through exp(alpha (phiM - phi_0))
    alone, so |f'''| <= |alpha|^3 |f|; a factor 2 for the terms beyond h^2: |FD - dwall_flux| <= 2 h^2 |alpha|^3 |f| / 6."""
    import importlib.util
    from catint_amd.calculator import Calculator
    from catint_amd.units import unit_F, unit_R
    spec = importlib.util.spec_from_file_location('co2r_physical_sweep', os.path.join(os.path.dirname(__file__), '..', 'examples',
                                                                                       'co2r_physical_sweep.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    tp, _ = ex.build(5, 96, phimin=-0.70, phimax=-0.72)
    calc = Calculator(transport=tp, calc='comsol', balance_on_device=True)
    tp.newton = {'tol': 1e-10, 'maxit': 80, 'response': {'omega': [0.0, 1e3]}}
    alpha = -0.5 * unit_F / (unit_R * tp.system['temperature'])
    k0 = float(ex.tafel_rate(tp)(np.array([0.0]))[0])          # the rate constant at phiM = 0; the potential dependence goes to alpha
    calc.set_surface_kinetics([{'species': 'CO2', 'rate': lambda phiM: np.full(np.shape(phiM), k0), 'alpha': alpha,
                                'stoichiometry': {'CO2': -1.0, 'CO': 1.0, 'OH-': 2.0}}])
    calc.run()
    assert np.all(calc.status == 0)
    res = calc.response
    assert (res['status'] == 0).all() and res['admittance'].shape == (5, 2)
    cd = np.array([tp.alldata[b]['system']['differential_capacitance'] for b in range(5)])
    assert np.isfinite(cd).all() and (cd > 0).all()
    assert np.array_equal(tp.alldata[0]['system']['response_omega'], [0.0, 1e3])
    assert np.allclose(tp.alldata[2]['system']['impedance'] * tp.alldata[2]['system']['admittance'], 1.0)
    names = list(tp.species.keys())
    phis = np.array(tp.descriptors['phiM'], float)
    h = abs(phis[1] - phis[0])
    assert np.allclose(np.abs(np.diff(phis)), h)
    worst = 0.0
    for sp in ('CO2', 'CO', 'OH-'):
        k = names.index(sp)
        f = calc.balance['wall_flux'][:, k]
        for b in (1, 2, 3):
            fd = (f[b + 1] - f[b - 1]) / (phis[b + 1] - phis[b - 1])
            bound = 2.0 * h * h * abs(alpha) ** 3 * abs(f[b]) / 6.0
            got = res['dwall_flux'][b, 0, k]
            assert got.imag == 0.0
            worst = max(worst, abs(fd - got.real) / bound)
            assert abs(fd - got.real) <= bound, (sp, b, fd, got.real, bound)
    print('slope of the wall flux along the sweep against dwall_flux: worst difference / h^2 bound %.3f' % worst)
