"""libcatint_voltam on the device against tests/voltam_ref.py (the method of tests/test_gpu_kintrans.py).

Agreement: every case of tests/voltam_cases.py takes the same accepted steps, rejected steps, Newton iterations and not-extrapolated
steps as the NumPy restatement and ends with the same status; ln theta agrees to LN_THETA_TOL where theta > 1e-200, the current to
CURRENT_TOL of current_scale, the fluxes to FLUX_TOL of flux_scale and the charge to CHARGE_TOL of its scale.  Each is ten times what
moving every ln kf and ln kb by +-4 ulp does to the restatement itself (tests/test_voltam_ref.py measures and guards them, and guards
that no decision of a case sits within 1e-6 of its threshold): the device's exp and log differ from NumPy's by ulps, and that is the
size of what such ulps do.
Bit for bit: batches of 1, 63, 64, 65 and 130 points, any max_waves, the view path against the host-surface path and a permuted lane
subset, outputs not asked for; S = 1 with N = 0 and S = 8 with N = 8.  Per lane: CATVM_INPUT (a NaN vertex, an empty program, a start
that does not converge) and its confinement, CATVM_STEPS.  The steady state of libcatint_kinetics along a slow sweep.
PnpSolver.get_voltammogram against Voltammetry.sweep."""
import numpy as np
import pytest

from catint_amd import voltammetry          # fails without the feature
from tests import kinetics_ref as KR
from tests import voltam_cases as C
from tests import voltam_ref as VR
from tests.test_voltam_ref import CHARGE_TOL, CURRENT_TOL, FLUX_TOL, LN_THETA_TOL, SLOW_SWEEP, SLOW_SWEEP_LN_THETA, charge_scale, slow_sweep_case

pytestmark = pytest.mark.gpu

ALL = list(voltammetry.FIELDS)
SIZES = (1, 63, 64, 65, 130)
MAX_STEPS = 20000


@pytest.fixture(scope='module')
def vm():
    with voltammetry.Voltammetry(0) as o:
        yield o


def kw_of(case):
    k = case.kw
    return dict(potential_drop='stern' if k['w'] else 'full', stern_capacitance=k['CS'], phi_pzc=k['phi_pzc'])


def run(vm, case, n=None, fields=ALL, poke=None, **kw):
    """the case's points (n: repeated to n of them) on the device; poke(args) edits the per-point arrays in place"""
    idx = np.arange(len(case.E_start) if n is None else n) % len(case.E_start)
    pp = dict(E_start=case.E_start[idx].copy(), E_vertex=case.E_vertex[idx].copy(), scan_rate=case.scan_rate[idx].copy(), csurf=case.csurf[idx].copy(),
              phi_surface=case.phi_surface[idx].copy(), theta0=None if case.theta0 is None else case.theta0[idx].copy())
    if poke is not None:
        poke(pp)
    args = dict(kw_of(case), max_steps=MAX_STEPS, **case.opts)
    args.update(kw)
    out = vm.sweep(None, case.tables, case.electrons, pp.pop('E_start'), pp.pop('E_vertex'), pp.pop('scan_rate'), fields=fields, **pp, **args)
    assert vm.last_kernel == 'catvm::sweep_kernel' and vm.last_kernel_ms > 0.0
    return out


def same(a, b, keys=None, rows=None):
    for k in (keys or a):
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert np.array_equal(x, y, equal_nan=True), k


def compare(out, ref, case, label, rows=slice(None)):
    """the device's rows against the restatement's: NaN in the same places, and the four tolerances where there is a number"""
    assert np.array_equal(np.isnan(out['theta'][rows]), np.isnan(ref['theta'][rows]))
    for k in ('current', 'charge', 'E_out', 'current_scale'):
        assert np.array_equal(np.isnan(out[k][rows]), np.isnan(ref[k][rows])), k
    ok = np.isfinite(ref['theta'][rows]) & (ref['theta'][rows] > 1e-200)
    dy = np.abs(np.log(out['theta'][rows][ok]) - np.log(ref['theta'][rows][ok])).max()
    with np.errstate(invalid='ignore', divide='ignore'):
        di = np.abs(out['current'][rows] - ref['current'][rows]) / ref['current_scale'][rows]
        dq = np.abs(out['charge'][rows] - ref['charge'][rows]) / charge_scale(case, ref)[rows]
        df = np.abs(out['flux'][rows] - ref['flux'][rows]) / ref['flux_scale'][rows]
    di, dq, df = di[np.isfinite(di)], dq[np.isfinite(dq)], df[np.isfinite(df)]
    print(label, 'ln theta %.1e / %.1e; current %.1e / %.1e of current_scale; charge %.1e / %.1e of its scale; flux %.1e / %.1e of flux_scale'
          % (dy, LN_THETA_TOL, di.max(), CURRENT_TOL, dq.max(), CHARGE_TOL, df.max() if df.size else 0.0, FLUX_TOL))
    assert dy <= LN_THETA_TOL and (di <= CURRENT_TOL).all() and (dq <= CHARGE_TOL).all() and (df <= FLUX_TOL).all()
    assert np.allclose(out['current_scale'][rows], ref['current_scale'][rows], rtol=1e-9, atol=0, equal_nan=True)
    assert np.allclose(out['flux_scale'][rows], ref['flux_scale'][rows], rtol=1e-9, atol=0, equal_nan=True)
    assert np.allclose(out['E_out'][rows], ref['E_out'][rows], rtol=1e-12, atol=0, equal_nan=True)


# ---- agreement with the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', C.CASE_NAMES)
def test_agreement_with_the_restatement(vm, name):
    case, ref = C.case(name), C.reference(name)
    out = run(vm, case)
    print(name, 'steps', out['steps'].tolist(), 'kernel %.2f ms' % vm.last_kernel_ms)
    assert np.array_equal(out['status'], ref['status']), (out['status'], ref['status'])
    assert np.array_equal(out['steps'], ref['steps']), (out['steps'].tolist(), ref['steps'].tolist())
    compare(out, ref, case, name)
    assert np.allclose(out['t_reached'], ref['t_reached'], rtol=1e-12, atol=0)
    assert np.array_equal(out['t_reached'], case.opts['n_segments'] * C.tau(case))
    bal = np.abs((out['theta'] * np.asarray(case.tables['site_count'])).sum(axis=-1) - 1.0)
    assert bal.max() <= 4 * np.spacing(1.0)
    assert np.array_equal(out['mean_current'], VR.mean_current(out['charge'], C.tau(case), case.opts['samples']))


# ---- bit for bit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['langmuir_quasi', 'co2r_two_site', 'random_S8', 'n0'])
def test_any_batch_size_and_any_number_of_waves_give_the_same_bits(vm, name):
    """points of one wave that take different numbers of steps; S = 3 with a two-site adsorbate; S = 8 with N = 8; S = 1 with N = 0"""
    case = C.case(name)
    base = run(vm, case, 130)
    assert (base['status'] == VR.DONE).all()
    k = len(case.E_start)
    for key in base:                          # every copy of a point has the bits of the first
        assert np.array_equal(base[key], base[key][np.arange(130) % k], equal_nan=True), key
    assert len({tuple(r) for r in base['steps'][:k].tolist()}) > 1
    for waves in (1, 2):
        same(base, run(vm, case, 130, max_waves=waves))
    for n in SIZES:
        got = run(vm, case, n)
        for key in got:
            assert np.array_equal(got[key], base[key][:n], equal_nan=True), (n, key)


def test_outputs_not_asked_for_change_no_bit(vm):
    case = C.case('co2r_two_site')
    full = run(vm, case, 65)
    only_status = run(vm, case, 65, fields=())
    assert set(only_status) == {'status', 'steps'}
    same(only_status, full, keys=('status', 'steps'))
    theta = run(vm, case, 65, fields=('theta',))
    same(theta, full, keys=('theta', 'status', 'steps'))
    rest = run(vm, case, 65, fields=('current', 'flux', 'charge', 't_reached'))
    same(rest, full, keys=('current', 'flux', 'charge', 't_reached', 'mean_current'))
    rest = run(vm, case, 65, fields=('current_scale', 'E_out', 'flux_scale'))
    same(rest, full, keys=('current_scale', 'E_out', 'flux_scale'))


VIEW_SWEEP = dict(E_vertex=-0.9, n_segments=2, samples=8, rtol=C.RTOL, atol=C.ATOL, max_steps=MAX_STEPS, fields=ALL)


def test_the_view_path_gives_the_bits_of_the_host_surface_path(vm):
    from tests.kinetics_cases import co2r_model
    from tests.test_gpu_kinetics import open_handle
    phis = np.linspace(-0.12, 0.06, 65)
    model = co2r_model('two_site')
    E_start = np.linspace(-0.55, -0.65, 65)
    rates = np.geomspace(0.01, 10.0, 65)
    with open_handle(phis) as s:
        assert (s.solve_stationary() == 0).all()
        before = s.get_state(derived=False) + (s.get_status(),)
        cs, vs, _ = s.get_surface()
        from_view = s.get_voltammogram(model, E_start, scan_rate=rates, **VIEW_SWEEP)
        from_host = s.get_voltammogram(model, E_start, scan_rate=rates, csurf=cs, phi_surface=vs, **VIEW_SWEEP)
        alone = vm.sweep(None, model, None, E_start, np.full(65, VIEW_SWEEP['E_vertex']), rates, csurf=cs, phi_surface=vs, potential_drop='stern',
                         stern_capacitance=0.2, phi_pzc=0.0, **{k: v for k, v in VIEW_SWEEP.items() if k != 'E_vertex'})
        held = vm.sweep(s.device_view(), model.tables(), model.electrons(), E_start, VIEW_SWEEP['E_vertex'], rates, kT=model.kT,
                        potential_drop='stern', stern_capacitance=0.2, phi_pzc=0.0, **{k: v for k, v in VIEW_SWEEP.items() if k != 'E_vertex'})
        same(from_view, from_host)
        same(from_view, alone)
        same(from_view, held)
        # the start is the steady state at E_start: a lane ends CATVM_INPUT exactly where the Newton iteration of the kinetics library
        # with the same tolerance and iteration count does not converge there (it is not globally convergent), and DONE elsewhere
        kin = s.get_kinetics(model, phiM=E_start, tol=voltammetry.DEFAULT_NEWTON_TOL, maxit=VR.START_MAXIT, fields=('theta',))
        done = from_view['status'] == VR.DONE
        assert np.array_equal(done, kin['status'] == 0) and np.array_equal(~done, from_view['status'] == VR.INPUT)
        assert done.sum() >= 20 and np.isfinite(from_view['theta'][done]).all() and np.isnan(from_view['theta'][~done]).all()
        # a subset of the lanes, permuted, with a repeat
        idx = np.array([64, 3, 3, 17])
        sub = s.get_voltammogram(model, E_start[idx], scan_rate=rates[idx], lanes=idx, **VIEW_SWEEP)
        for k in sub:
            assert np.array_equal(sub[k], from_view[k][idx], equal_nan=True), k
        after = s.get_state(derived=False) + (s.get_status(),)
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        # the context of the call was closed: the solver holds none, and a second solver opened after the call works
        assert not hasattr(s, '_voltammetry') and len(s.SATELLITES) == 13
        mc = from_view['mean_current']
        tau = np.abs(VIEW_SWEEP['E_vertex'] - E_start) / rates
        assert np.allclose(np.cumsum(mc * (tau / VIEW_SWEEP['samples'])[:, None], axis=1), from_view['charge'], rtol=1e-12, atol=0, equal_nan=True)
    with open_handle(phis[:2]) as s2:
        assert (s2.solve_stationary() == 0).all()
        again = s2.get_voltammogram(model, E_start[:2], scan_rate=rates[:2], **VIEW_SWEEP)
        cs2, vs2, _ = s2.get_surface()
        alone2 = vm.sweep(None, model, None, E_start[:2], VIEW_SWEEP['E_vertex'], rates[:2], csurf=cs2, phi_surface=vs2, potential_drop='stern',
                          stern_capacitance=0.2, phi_pzc=0.0, **{k: v for k, v in VIEW_SWEEP.items() if k != 'E_vertex'})
        same(again, alone2)
        assert (again['status'] == VR.DONE).all()


# ---- per-lane statuses ---------------------------------------------------------------------------------------------------------------
def test_a_bad_program_or_start_is_confined_to_its_lane(vm):
    case = C.case('co2r_two_site')
    clean = run(vm, case, 65)
    R = len(case.electrons)
    off = np.zeros((65, R, 2))
    off[20] = 800.0          # exp(800) overflows: the steady solve at E_start meets a pivot that is not a number

    def poke(pp):
        pp['E_vertex'][7] = np.nan
        pp['E_start'][9] = np.inf
        pp['E_vertex'][11] = pp['E_start'][11]
    out = run(vm, case, 65, poke=poke, off=off)
    bad = [7, 9, 11, 20]
    assert (out['status'][bad] == VR.INPUT).all() and not out['steps'][bad].any()
    for k in ALL:
        assert np.isnan(out[k][bad]).all(), k
    assert np.isnan(out['mean_current'][bad]).all()
    same(out, clean, rows=~np.isin(np.arange(65), bad))
    # the restatement calls the same four points CATVM_INPUT
    t = KR._arrays(case.tables)
    for i, over in ((7, dict(E_vertex=np.nan)), (9, dict(E_start=np.inf)), (11, dict(E_vertex=case.E_start[11 % 3])), (20, dict(off=off[20]))):
        p = i % 3
        a = dict(E_start=case.E_start[p], E_vertex=case.E_vertex[p])
        a.update({k: over.pop(k) for k in list(over) if k in a})
        o = VR.solve_point(t, case.electrons, a['E_start'], a['E_vertex'], case.scan_rate[p], case.csurf[p], case.phi_surface[p], **case.kw,
                           **case.opts, **over)
        assert o['status'] == VR.INPUT, i
    # a start that leaves no free site, and one that is not finite; the free-site entry is ignored
    th = np.tile([0.7, 0.1, 0.05, 0.1], (65, 1))
    given = run(vm, case._replace(theta0=np.tile([0.7, 0.1, 0.05, 0.1], (3, 1))), 65)
    assert (given['status'] == VR.DONE).all() and not np.array_equal(given['theta'][:3], clean['theta'][:3])
    th[5, 1:] = [0.5, 0.4, 0.3]
    th[9, 2] = np.inf
    th[11, 0] = np.nan
    out = run(vm, case, 65, poke=lambda pp: pp.__setitem__('theta0', th))
    assert list(out['status'][[5, 9, 11]]) == [VR.INPUT, VR.INPUT, VR.DONE]
    assert np.isnan(out['theta'][[5, 9]]).all() and np.isnan(out['t_reached'][[5, 9]]).all()
    same(out, given, rows=~np.isin(np.arange(65), (5, 9)))


def test_a_step_budget_ends_a_lane_with_nan_in_the_rows_it_did_not_reach(vm):
    case, ref = C.case('n0'), C.reference('n0')
    out = run(vm, case, max_steps=5)
    assert (out['status'] == VR.STEPS).all() and (out['steps'][:, :2].sum(axis=1) == 5).all()
    for k in ('theta', 'current', 'current_scale', 'charge', 'E_out', 'mean_current'):
        assert np.isnan(out[k]).all(), k
    assert (out['t_reached'] > 0.0).all() and (out['t_reached'] < C.tau(case) / case.opts['samples']).all()
    # a budget that ends between two output times, against the restatement with the same budget
    want = C.run(case, points=[0], max_steps=150)
    out = run(vm, case, max_steps=150)
    reached = np.isfinite(want['current'][0])
    assert 0 < reached.sum() < len(reached)
    assert out['status'][0] == VR.STEPS == want['status'][0] and np.array_equal(out['steps'][0], want['steps'][0])
    assert np.array_equal(np.isfinite(out['theta'][0]).all(axis=1), reached) and np.array_equal(np.isfinite(out['charge'][0]), reached)
    compare(out, want, case, 'n0 with 150 steps', rows=slice(0, 1))
    assert abs(out['t_reached'][0] / want['t_reached'][0] - 1.0) <= 1e-12
    # the other two points finish within that budget or not, as in the restatement
    assert np.array_equal(out['status'], [VR.STEPS if s.sum() > 150 else VR.DONE for s in ref['steps'][:, :2]])


# ---- cross-library -----------------------------------------------------------------------------------------------------------------------
def test_a_slow_sweep_follows_the_steady_state_of_the_kinetics_library(vm):
    """co2r_two_site at SLOW_SWEEP V/s: the coverages at the outputs against PnpSolver.get_kinetics at E_out.  The restatement is
    SLOW_SWEEP_LN_THETA away from its own steady state (tests/test_voltam_ref.py measures it); the device stays within twice that"""
    from tests.test_gpu_kinetics import open_handle
    case = slow_sweep_case()
    out = run(vm, case, fields=('theta', 'E_out'))
    assert (out['status'] == VR.DONE).all()
    n, K = out['E_out'].shape
    with open_handle(np.zeros(1)) as s:
        kin = s.get_kinetics(case.tables, phiM=out['E_out'].reshape(-1), csurf=np.repeat(case.csurf, K, axis=0),
                             phi_surface=np.repeat(case.phi_surface, K), fields=('theta',), **kw_of(case))
    assert (kin['status'] == 0).all()
    d = np.abs(np.log(out['theta'].reshape(n * K, -1)) - np.log(kin['theta'])).max()
    print('slow sweep against get_kinetics: max |d ln theta| %.2e, restatement %.2e' % (d, SLOW_SWEEP_LN_THETA))
    assert d <= 2.0 * SLOW_SWEEP_LN_THETA
