"""libcatint_kintrans on the device against tests/kintrans_ref.py (the method of tests/test_gpu_kinetics.py).

Agreement: every case of tests/kintrans_cases.py takes the same accepted steps, rejected steps and Newton iterations as the NumPy
restatement and ends with the same status; ln theta agrees to LN_THETA_TOL = 6.1e-13 where theta > 1e-200 and the fluxes to
FLUX_TOL = 1.8e-13 of flux_scale.  Both are ten times what moving every ln kf and ln kb by +-4 ulp does to the restatement itself
(6.1e-14, 1.8e-14; tests/test_kintrans_ref.py measures and guards them, and guards that no decision of a case sits within 1e-6 of its
threshold): the device's exp and log differ from NumPy's by ulps, and that is the size of what such ulps do.
Bit for bit: batches of 1, 63, 64, 65 and 130 points, any max_waves, the view path against the host-surface path, outputs not asked
for; S = 1 with N = 0 and S = 8 with N = 8.  Per lane: CATKT_INPUT and its confinement, CATKT_STEPS, CATKT_STEADY in some lanes of a
wave and not in others.  The rescue of PnpSolver.get_kinetics on the three networks the Newton iteration fails on."""
import numpy as np
import pytest

from catint_amd import _kintrans          # fails without the feature
from tests import kinetics_ref as KR
from tests import kintrans_cases as C
from tests import kintrans_ref as KT
from tests.test_kintrans_ref import FLUX_TOL, LN_THETA_TOL

pytestmark = pytest.mark.gpu

ALL = list(_kintrans.FIELDS)
SIZES = (1, 63, 64, 65, 130)
MAX_STEPS = 5000


@pytest.fixture(scope='module')
def ts():
    with _kintrans.TransientKinetics(0) as o:
        yield o


def kw_of(case):
    k = case.kw
    return dict(potential_drop='stern' if k['w'] else 'full', stern_capacitance=k['CS'], phi_pzc=k['phi_pzc'])


def run(ts, case, n=None, fields=ALL, poke=None, **kw):
    """the case's points (n: repeated to n of them) on the device; poke(phiM) edits the potentials in place"""
    idx = np.arange(len(case.phiM) if n is None else n) % len(case.phiM)
    pm = case.phiM[idx].copy()
    if poke is not None:
        poke(pm)
    args = dict(kw_of(case), max_steps=MAX_STEPS, **case.opts)
    args.update(kw)
    out = ts.solve(None, case.tables, pm, case.t_out, csurf=case.csurf[idx], phi_surface=case.phi_surface[idx],
                   theta0=None if case.theta0 is None else case.theta0[idx], fields=fields, **args)
    assert ts.last_kernel == 'catkt::transient_kernel' and ts.last_kernel_ms > 0.0
    return out


def same(a, b, keys=None, rows=None):
    for k in (keys or a):
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert np.array_equal(x, y, equal_nan=True), k


def n0_case():
    """* <-> X <-> *: S = 1 and no species at all; three starts"""
    from tests.test_kinetics_abi import chain
    th = np.array([[0.9, 0.1], [0.3, 0.7], [0.5, 0.5]])
    return C.Case('n0', chain(N=0, S=1), np.zeros(3), np.zeros((3, 0)), np.zeros(3), dict(w=0, CS=0.0, phi_pzc=0.0), th, (0.1, 1.0, 5.0),
                  dict(rtol=C.RTOL))


# ---- agreement with the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', C.CASE_NAMES)
def test_agreement_with_the_restatement(ts, name):
    case, ref = C.case(name), C.reference(name)
    out = run(ts, case)
    assert np.array_equal(out['status'], ref['status']), (out['status'], ref['status'])
    assert np.array_equal(out['steps'], ref['steps']), (out['steps'].tolist(), ref['steps'].tolist())
    assert np.array_equal(np.isnan(out['theta']), np.isnan(ref['theta']))
    ok = np.isfinite(ref['theta']) & (ref['theta'] > 1e-200)
    dy = np.abs(np.log(out['theta'][ok]) - np.log(ref['theta'][ok])).max()
    with np.errstate(invalid='ignore', divide='ignore'):
        df = np.abs(out['flux'] - ref['flux']) / ref['flux_scale']
    df = df[np.isfinite(df)]
    dt = np.abs(out['t_reached'] / ref['t_reached'] - 1.0).max()
    print(name, 'ln theta %.1e / %.1e; flux %.1e / %.1e of flux_scale; t_reached relative %.1e; steps %s'
          % (dy, LN_THETA_TOL, df.max() if df.size else 0.0, FLUX_TOL, dt, out['steps'].tolist()))
    assert dy <= LN_THETA_TOL
    assert (df <= FLUX_TOL).all()
    assert np.allclose(out['flux_scale'], ref['flux_scale'], rtol=1e-11, atol=0, equal_nan=True)
    done = ref['status'] == KT.DONE
    assert (out['t_reached'][done] == case.t_out[-1]).all()
    bal = np.abs((out['theta'] * np.asarray(case.tables['site_count'])).sum(axis=-1) - 1.0)
    assert bal.max() <= 4 * np.spacing(1.0)


# ---- bit for bit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['co2r_two_site', 'random_S8', 'n0'])
def test_any_batch_size_and_any_number_of_waves_give_the_same_bits(ts, name):
    """S = 3 with three points that take different numbers of steps; S = 8 with N = 8; S = 1 with N = 0"""
    case = n0_case() if name == 'n0' else C.case(name)
    base = run(ts, case, 130)
    assert (base['status'] == KT.DONE).all()
    k = len(case.phiM)
    for key in base:                          # every copy of a point has the bits of the first
        assert np.array_equal(base[key], base[key][np.arange(130) % k], equal_nan=True), key
    assert k == 1 or len({tuple(r) for r in base['steps'][:k].tolist()}) > 1
    for waves in (1, 2):
        same(base, run(ts, case, 130, max_waves=waves))
    for n in SIZES:
        got = run(ts, case, n)
        for key in got:
            assert np.array_equal(got[key], base[key][:n], equal_nan=True), (n, key)


def test_outputs_not_asked_for_change_no_bit(ts):
    case = C.case('co2r_two_site')
    full = run(ts, case, 65)
    only_status = run(ts, case, 65, fields=())
    assert set(only_status) == {'status', 'steps'}
    same(only_status, full, keys=('status', 'steps'))
    theta = run(ts, case, 65, fields=('theta',))
    same(theta, full, keys=('theta', 'status', 'steps'))
    rest = run(ts, case, 65, fields=('flux', 'drift', 't_reached'))
    same(rest, full, keys=('flux', 'drift', 't_reached'))


def test_the_view_path_gives_the_bits_of_the_host_surface_path(ts):
    from tests.kinetics_cases import co2r_model
    from tests.test_gpu_kinetics import open_handle
    phis = np.linspace(-0.12, 0.06, 65)
    t_out = (1e-9, 1e-6, 1e-3)
    model = co2r_model('two_site')
    with open_handle(phis) as s:
        assert (s.solve_stationary() == 0).all()
        before = s.get_state(derived=False) + (s.get_status(),)
        cs, vs, _ = s.get_surface()
        kw = dict(rtol=C.RTOL, max_steps=MAX_STEPS, fields=ALL)
        from_view = s.get_kinetics_transient(model, t_out, **kw)
        assert s._transient.last_kernel == 'catkt::transient_kernel'
        from_host = s.get_kinetics_transient(model, t_out, csurf=cs, phi_surface=vs, **kw)
        alone = ts.solve(None, model.tables(), phis, t_out, csurf=cs, phi_surface=vs, potential_drop='stern', stern_capacitance=0.2, phi_pzc=0.0, **kw)
        same(from_view, from_host)
        same(from_view, alone)
        assert np.isin(from_view['status'], (KT.DONE, KT.STEADY)).all() and np.isfinite(from_view['theta']).all()
        # a subset of the lanes, permuted, with a repeat
        idx = np.array([64, 3, 3, 17])
        sub = s.get_kinetics_transient(model, t_out, lanes=idx, **kw)
        for k in sub:
            assert np.array_equal(sub[k], from_view[k][idx], equal_nan=True), k
        after = s.get_state(derived=False) + (s.get_status(),)
        for a, b in zip(before, after):
            assert np.array_equal(a, b)


# ---- per-lane statuses ---------------------------------------------------------------------------------------------------------------
def test_a_bad_input_is_confined_to_its_lane(ts):
    case = C.case('co2r_one_site')
    clean = run(ts, case, 65)

    def poke(pm):
        pm[7] = np.nan
    out = run(ts, case, 65, poke=poke)
    assert out['status'][7] == KT.INPUT and not out['steps'][7].any()
    for k in ALL:
        assert np.isnan(out[k][7]).all(), k
    rest = np.arange(65) != 7
    same(out, clean, rows=rest)
    # a start that leaves no free site, and a start that is not finite
    th = case.theta0[np.arange(65) % 3].copy()
    th[5, 1:] = [0.5, 0.4, 0.3]
    th[9, 2] = np.inf
    th[11, 0] = np.nan          # the free-site entry is ignored
    out = ts.solve(None, case.tables, case.phiM[np.arange(65) % 3], case.t_out, csurf=case.csurf[np.arange(65) % 3],
                   phi_surface=case.phi_surface[np.arange(65) % 3], theta0=th, fields=ALL, max_steps=MAX_STEPS, **kw_of(case), **case.opts)
    assert list(out['status'][[5, 9, 11]]) == [KT.INPUT, KT.INPUT, KT.DONE]
    assert np.isnan(out['theta'][[5, 9]]).all() and np.isnan(out['t_reached'][[5, 9]]).all()
    same(out, clean, rows=~np.isin(np.arange(65), (5, 9)))


def test_a_step_budget_ends_a_lane_with_nan_in_the_rows_it_did_not_reach(ts):
    case, ref = C.case('random_S3'), C.reference('random_S3')
    out = run(ts, case, 2, max_steps=5)
    assert (out['status'] == KT.STEPS).all() and (out['steps'][:, :2].sum(axis=1) == 5).all()
    assert np.isnan(out['theta']).all() and np.isnan(out['flux']).all() and np.isnan(out['drift']).all()
    assert (out['t_reached'] > 0.0).all() and (out['t_reached'] < case.t_out[0]).all()
    # a budget that ends between two output times, against the restatement with the same budget
    t = KR._arrays(case.tables)
    want = KT.solve_point(t, case.phiM[0], case.csurf[0], case.phi_surface[0], case.t_out, max_steps=150, **case.kw, **case.opts)
    out = run(ts, case, max_steps=150)
    reached = np.isfinite(want['drift'])
    assert 0 < reached.sum() < len(case.t_out)
    assert out['status'][0] == KT.STEPS == want['status'] and np.array_equal(out['steps'][0], want['steps'])
    assert np.array_equal(np.isfinite(out['theta'][0]).all(axis=1), reached) and np.array_equal(np.isfinite(out['drift'][0]), reached)
    assert np.abs(np.log(out['theta'][0][reached]) - np.log(ref['theta'][0][reached])).max() <= LN_THETA_TOL
    assert abs(out['t_reached'][0] / want['t_reached'] - 1.0) <= 1e-9


def test_steady_tol_stops_some_lanes_of_a_wave_and_not_others(ts):
    """The two points of the single-step case relax at different rates.  steady_tol is the geometric mean of their drifts at the last
    output time in the restatement without it: the faster one stops before that time, the slower one does not"""
    case, ref = C.case('langmuir'), C.reference('langmuir')
    d = ref['drift'][:, -1]
    assert d.min() > 0.0 and d.max() / d.min() > 10.0
    tol = float(np.sqrt(d.min() * d.max()))
    want = C.run(case, steady_tol=tol)
    assert sorted(want['status']) == [KT.DONE, KT.STEADY]
    out = run(ts, case, 64, steady_tol=tol)
    assert np.array_equal(out['status'], want['status'][np.arange(64) % 2]) and np.array_equal(out['steps'], want['steps'][np.arange(64) % 2])
    i = int(np.flatnonzero(want['status'] == KT.STEADY)[0])
    assert out['t_reached'][i] < case.t_out[-1] and abs(out['t_reached'][i] / want['t_reached'][i] - 1.0) <= 1e-9
    filled = np.array(case.t_out) >= out['t_reached'][i]
    assert filled.sum() >= 1 and (out['theta'][i][filled] == out['theta'][i][-1]).all() and (out['drift'][i][filled] < tol).all()
    assert (out['flux'][i][filled] == out['flux'][i][-1]).all()
    ok = np.isfinite(want['theta'])
    assert np.abs(np.log(out['theta'][:2][ok]) - np.log(want['theta'][ok])).max() <= LN_THETA_TOL


# ---- the rescue ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def any_solver():
    from tests.test_gpu_kinetics import open_handle
    with open_handle(np.zeros(1)) as s:
        yield s


@pytest.mark.parametrize('name', C.RESCUE_NAMES)
def test_get_kinetics_rescues_the_points_its_newton_iteration_fails_at(any_solver, name):
    case, ref, plain_cpu = C.case(name), C.reference(name), C.plain_newton(name)
    s = any_solver
    args = dict(phiM=case.phiM, csurf=case.csurf, phi_surface=case.phi_surface, fields=('theta', 'rate', 'flux', 'flux_scale'), **kw_of(case))
    plain = s.get_kinetics(case.tables, **args)
    off = s.get_kinetics(case.tables, rescue=False, **args)
    assert set(plain) == set(off) and 'rescued' not in off
    same(plain, off)
    failed = plain['status'] != 0
    assert failed.any() and np.array_equal(failed, plain_cpu['status'] != 0)
    out = s.get_kinetics(case.tables, rescue=True, **args)
    assert s._transient.last_kernel == 'catkt::transient_kernel'
    assert (out['status'] == 0).all() and out['rescued'].dtype == bool and np.array_equal(out['rescued'], failed)
    same(out, plain, keys=('theta', 'rate', 'flux', 'flux_scale', 'iterations'), rows=~failed)
    # against the CPU's Newton iteration started from the restatement's stationary state, at 60 digits (the tolerance of
    # tests/test_gpu_kinetics.py for y: ten times the error of the fp64 reference, floor 1e-13)
    warm = KR.solve_fp64(case.tables, case.phiM, case.csurf, case.phi_surface, theta_guess=ref['theta'][:, 0], sens=False, **case.kw)
    assert (warm['status'] == 0).all()
    mp = KR.solve_mp(case.tables, case.phiM, case.csurf, case.phi_surface, warm, sens=False, **case.kw)
    tol = max(10.0 * KR.mp_err(mp['y'], warm['y']).max(), 1e-13)
    err = KR.mp_err(mp['y'], np.log(out['theta']))
    print(name, 'rescued', out['rescued'].tolist(), 'iterations', out['iterations'].tolist(), 'y error %.1e / %.1e' % (err.max(), tol))
    assert err.max() <= tol
    assert (out['iterations'][failed] <= 3).all()


def test_rescue_excludes_a_guess_and_the_device_loop(any_solver):
    case = C.case('rescue_S3')
    with pytest.raises(ValueError, match='theta_guess'):
        any_solver.get_kinetics(case.tables, phiM=case.phiM, csurf=case.csurf, phi_surface=case.phi_surface, rescue=True,
                                theta_guess=np.full((4, 4), 0.1), **kw_of(case))
    from catint_amd.calculator import Calculator, CalculatorError
    from tests.test_kinetics_abi import scf_parts
    tp, model, _ = scf_parts()
    with pytest.raises(CalculatorError, match='device loop'):
        Calculator(transport=tp, calc='comsol').set_microkinetics(model, rescue=True, device_loop=True)
