"""libcatint_iasweep on the device against tests/iasweep_ref.py (the method of tests/test_gpu_voltam.py).

Agreement: every case of tests/iasweep_cases.py takes the same accepted steps, rejected steps, Newton iterations and not-extrapolated
steps as the NumPy restatement and ends with the same status; ln theta agrees to LN_THETA_TOL where theta > 1e-200, the current to
CURRENT_TOL of current_scale, the fluxes to FLUX_TOL of flux_scale, the charge to CHARGE_TOL of its scale and the shifts to SHIFT_TOL
kT.  Each is ten times what moving every ln kf and ln kb by +-4 ulp does to the restatement itself (tests/test_iasweep_ref.py measures
and guards them, and guards that no decision of a case sits within 1e-6 of its threshold).
Bit for bit: batches of 1, 63, 64, 65 and 130 points, any max_waves, outputs not asked for, the view path against the host-surface
path and a permuted lane subset; G = 1, 2; T = 9 with N = 8.  Reduction: with G = 1 and strength 0 every output has the bits of
libcatint_voltam.  Per lane: CATIS_INPUT (a NaN vertex, an equal vertex without hold_time, a start that does not converge, a theta0
that leaves a type without a free site) and its confinement, CATIS_STEPS.  PnpSolver.get_voltammogram against
InteractingVoltammetry.sweep."""
import numpy as np
import pytest

from catint_amd import iasweep          # fails without the feature
from tests import iasweep_cases as C
from tests import iasweep_ref as SR
from tests import interact_ref as IR
from tests import voltam_cases as VC
from tests.test_iasweep_ref import CHARGE_TOL, CURRENT_TOL, FLUX_TOL, LN_THETA_TOL, SHIFT_TOL, charge_scale

pytestmark = pytest.mark.gpu

ALL = list(iasweep.FIELDS)
SIZES = (1, 63, 64, 65, 130)
MAX_STEPS = 20000


@pytest.fixture(scope='module')
def iv():
    with iasweep.InteractingVoltammetry(0) as o:
        yield o


def kw_of(case):
    k = case.kw
    return dict(potential_drop='stern' if k['w'] else 'full', stern_capacitance=k['CS'], phi_pzc=k['phi_pzc'])


def run(iv, case, n=None, fields=ALL, poke=None, **kw):
    """the case's points (n: repeated to n of them) on the device; poke(args) edits the per-point arrays in place"""
    idx = np.arange(len(case.E_start) if n is None else n) % len(case.E_start)
    pp = dict(E_start=case.E_start[idx].copy(), E_vertex=case.E_vertex[idx].copy(), scan_rate=case.scan_rate[idx].copy(), csurf=case.csurf[idx].copy(),
              phi_surface=case.phi_surface[idx].copy(), theta0=None if case.theta0 is None else case.theta0[idx].copy(),
              hold_time=None if case.hold_time is None else case.hold_time[idx].copy())
    if poke is not None:
        poke(pp)
    args = dict(kw_of(case), max_steps=MAX_STEPS, **case.opts)
    args.update(kw)
    out = iv.sweep(None, case.tables, case.electrons, pp.pop('E_start'), pp.pop('E_vertex'), pp.pop('scan_rate'), fields=fields, **pp, **args)
    assert iv.last_kernel == 'catis::sweep_kernel' and iv.last_kernel_ms > 0.0
    return out


def same(a, b, keys=None, rows=None):
    for k in (keys or a):
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert np.array_equal(x, y, equal_nan=True), k


def compare(out, ref, case, label, rows=slice(None)):
    """the device's rows against the restatement's: NaN in the same places, and the five tolerances where there is a number"""
    assert np.array_equal(np.isnan(out['theta'][rows]), np.isnan(ref['theta'][rows]))
    for k in ('current', 'charge', 'E_out', 'current_scale', 'energy_shift'):
        assert np.array_equal(np.isnan(out[k][rows]), np.isnan(ref[k][rows])), k
    ok = np.isfinite(ref['theta'][rows]) & (ref['theta'][rows] > 1e-200)
    dy = np.abs(np.log(out['theta'][rows][ok]) - np.log(ref['theta'][rows][ok])).max()
    with np.errstate(invalid='ignore', divide='ignore'):
        di = np.abs(out['current'][rows] - ref['current'][rows]) / ref['current_scale'][rows]
        dq = np.abs(out['charge'][rows] - ref['charge'][rows]) / charge_scale(case, ref)[rows]
        df = np.abs(out['flux'][rows] - ref['flux'][rows]) / ref['flux_scale'][rows]
        de = np.abs(out['energy_shift'][rows] - ref['energy_shift'][rows])
    di, dq, df, de = di[np.isfinite(di)], dq[np.isfinite(dq)], df[np.isfinite(df)], de[np.isfinite(de)]
    print(label, 'ln theta %.1e / %.1e; current %.1e / %.1e of current_scale; charge %.1e / %.1e of its scale; flux %.1e / %.1e of flux_scale; '
          'shift %.1e / %.1e kT' % (dy, LN_THETA_TOL, di.max(), CURRENT_TOL, dq.max(), CHARGE_TOL, df.max() if df.size else 0.0, FLUX_TOL,
                                    de.max(), SHIFT_TOL))
    assert dy <= LN_THETA_TOL and (di <= CURRENT_TOL).all() and (dq <= CHARGE_TOL).all() and (df <= FLUX_TOL).all() and (de <= SHIFT_TOL).all()
    assert np.allclose(out['current_scale'][rows], ref['current_scale'][rows], rtol=1e-9, atol=0, equal_nan=True)
    assert np.allclose(out['flux_scale'][rows], ref['flux_scale'][rows], rtol=1e-9, atol=0, equal_nan=True)
    assert np.allclose(out['E_out'][rows], ref['E_out'][rows], rtol=1e-12, atol=0, equal_nan=True)


# ---- agreement with the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', C.CASE_NAMES)
def test_agreement_with_the_restatement(iv, name):
    case, ref = C.case(name), C.reference(name)
    out = run(iv, case)
    print(name, 'steps', out['steps'].tolist(), 'kernel %.2f ms' % iv.last_kernel_ms)
    assert np.array_equal(out['status'], ref['status']), (out['status'], ref['status'])
    assert np.array_equal(out['steps'], ref['steps']), (out['steps'].tolist(), ref['steps'].tolist())
    compare(out, ref, case, name)
    assert np.allclose(out['t_reached'], ref['t_reached'], rtol=1e-12, atol=0)
    assert np.array_equal(out['t_reached'], case.opts['n_segments'] * C.tau(case))
    t = IR._arrays(case.tables)
    for g in range(t['G']):
        bal = np.abs((out['theta'] * t['ns'])[:, :, t['site_of'] == g].sum(axis=-1) / t['x'][g] - 1.0)
        assert bal.max() <= 4 * np.spacing(1.0), (g, bal.max() / np.spacing(1.0))
    from tests.voltam_ref import mean_current
    assert np.array_equal(out['mean_current'], mean_current(out['charge'], C.tau(case), case.opts['samples']))


# ---- bit for bit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['frumkin_quasi', 'co2r_weak', 'terrace_step', 'random_S7_G2_piecewise', 'hold_relax'])
def test_any_batch_size_and_any_number_of_waves_give_the_same_bits(iv, name):
    """points of one wave that take different numbers of steps; the ramped start; G = 2 from theta0; T = 9 with N = 8; a hold"""
    case = C.case(name)
    base = run(iv, case, 130)
    assert (base['status'] == SR.DONE).all()
    k = len(case.E_start)
    for key in base:                          # every copy of a point has the bits of the first
        assert np.array_equal(base[key], base[key][np.arange(130) % k], equal_nan=True), key
    assert len({tuple(r) for r in base['steps'][:k].tolist()}) > 1
    for waves in (1, 2):
        same(base, run(iv, case, 130, max_waves=waves))
    for n in SIZES:
        got = run(iv, case, n)
        for key in got:
            assert np.array_equal(got[key], base[key][:n], equal_nan=True), (n, key)


def test_outputs_not_asked_for_change_no_bit(iv):
    case = C.case('terrace_step')
    full = run(iv, case, 65)
    only_status = run(iv, case, 65, fields=())
    assert set(only_status) == {'status', 'steps'}
    same(only_status, full, keys=('status', 'steps'))
    theta = run(iv, case, 65, fields=('theta',))
    same(theta, full, keys=('theta', 'status', 'steps'))
    rest = run(iv, case, 65, fields=('current', 'flux', 'charge', 't_reached'))
    same(rest, full, keys=('current', 'flux', 'charge', 't_reached', 'mean_current'))
    rest = run(iv, case, 65, fields=('current_scale', 'E_out', 'flux_scale', 'energy_shift'))
    same(rest, full, keys=('current_scale', 'E_out', 'flux_scale', 'energy_shift'))


VIEW_SWEEP = dict(E_vertex=-0.9, n_segments=2, samples=8, rtol=C.RTOL, atol=C.ATOL, max_steps=MAX_STEPS, fields=ALL)


def test_the_view_path_and_the_solver_s_call_give_the_bits_of_the_host_surface_path(iv):
    from tests.interact_cases import co2r_model
    from tests.test_gpu_kinetics import open_handle
    phis = np.linspace(-0.12, 0.06, 65)
    model = co2r_model('one_site', 0.3, 0.15)
    E_start = np.linspace(-0.55, -0.65, 65)
    rates = np.geomspace(0.01, 10.0, 65)
    rest = {k: v for k, v in VIEW_SWEEP.items() if k != 'E_vertex'}
    with open_handle(phis) as s:
        assert (s.solve_stationary() == 0).all()
        before = s.get_state(derived=False) + (s.get_status(),)
        cs, vs, _ = s.get_surface()
        from_view = s.get_voltammogram(model, E_start, scan_rate=rates, **VIEW_SWEEP)
        from_host = s.get_voltammogram(model, E_start, scan_rate=rates, csurf=cs, phi_surface=vs, **VIEW_SWEEP)
        alone = iv.sweep(None, model, None, E_start, np.full(65, VIEW_SWEEP['E_vertex']), rates, csurf=cs, phi_surface=vs, potential_drop='stern',
                         stern_capacitance=0.2, phi_pzc=0.0, **rest)
        held = iv.sweep(s.device_view(), model.tables(), model.electrons(), E_start, VIEW_SWEEP['E_vertex'], rates, kT=model.kT,
                        potential_drop='stern', stern_capacitance=0.2, phi_pzc=0.0, **rest)
        same(from_view, from_host)
        same(from_view, alone)
        same(from_view, held)
        assert set(from_view) == set(ALL) | {'status', 'steps', 'mean_current'} and from_view['energy_shift'].shape[:2] == (65, 16)
        done = from_view['status'] == SR.DONE
        assert np.array_equal(~done, from_view['status'] == SR.INPUT)
        assert done.sum() >= 20 and np.isfinite(from_view['theta'][done]).all() and np.isnan(from_view['theta'][~done]).all()
        assert np.abs(from_view['energy_shift'][done]).max() > 0.0
        # a subset of the lanes, permuted, with a repeat
        idx = np.array([64, 3, 3, 17])
        sub = s.get_voltammogram(model, E_start[idx], scan_rate=rates[idx], lanes=idx, **VIEW_SWEEP)
        for k in sub:
            assert np.array_equal(sub[k], from_view[k][idx], equal_nan=True), k
        after = s.get_state(derived=False) + (s.get_status(),)
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        # the context of the call was closed: the solver holds none
        assert not [k for k in vars(s) if 'iasweep' in k or 'voltam' in k] and len(s.SATELLITES) == 13
        # start_ramp and hold_time pass through: a theta0 from the sweep's own start, held at E_start
        th0 = from_view['theta'][done][:, -1][:2]
        lanes = np.flatnonzero(done)[:2]
        hold = s.get_voltammogram(model, E_start[lanes], E_start[lanes], rates[lanes], lanes=lanes, theta0=th0, hold_time=[1.0, 10.0],
                                  n_segments=1, samples=4, rtol=C.RTOL, atol=C.ATOL, fields=('theta', 'E_out', 't_reached'))
        assert (hold['status'] == SR.DONE).all() and np.array_equal(hold['t_reached'], [1.0, 10.0])
        assert np.array_equal(hold['E_out'], np.repeat(E_start[lanes][:, None], 4, axis=1))
        with pytest.raises(ValueError, match='hold_time and start_ramp'):
            from tests.kinetics_cases import co2r_model as mean_field
            s.get_voltammogram(mean_field('one_site'), E_start, scan_rate=rates, hold_time=1.0, **VIEW_SWEEP)


# ---- the reduction -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['co2r_two_site', 'langmuir_quasi', 'random_S8'])
def test_one_site_type_without_interactions_has_the_bits_of_the_mean_field_library(iv, name):
    from catint_amd import voltammetry
    c = VC.case(name)
    idx = np.arange(65) % len(c.E_start)
    k = c.kw
    args = dict(potential_drop='stern' if k['w'] else 'full', stern_capacitance=k['CS'], phi_pzc=k['phi_pzc'], max_steps=MAX_STEPS,
                csurf=c.csurf[idx], phi_surface=c.phi_surface[idx], **c.opts)
    with voltammetry.Voltammetry(0) as vm:
        want = vm.sweep(None, c.tables, c.electrons, c.E_start[idx], c.E_vertex[idx], c.scan_rate[idx], fields=list(voltammetry.FIELDS), **args)
    got = iv.sweep(None, SR.mean_field_tables(c.tables), c.electrons, c.E_start[idx], c.E_vertex[idx], c.scan_rate[idx], fields=ALL, start_ramp=1,
                   **args)
    assert (want['status'] == SR.DONE).all()
    same(want, got, keys=list(want))
    assert not got['energy_shift'].any()


# ---- per-lane statuses ---------------------------------------------------------------------------------------------------------------
def test_a_bad_program_or_start_is_confined_to_its_lane(iv):
    case = C.case('co2r_weak')
    clean = run(iv, case, 65)
    R = len(case.electrons)
    off = np.zeros((65, R, 2))
    off[20] = 800.0          # exp(800) overflows: the steady solve at E_start meets a pivot that is not a number
    hold = np.full(65, np.nan)
    hold[12] = 2.0

    def poke(pp):
        pp['E_vertex'][7] = np.nan
        pp['E_start'][9] = np.inf
        pp['E_vertex'][11] = pp['E_start'][11]          # an equal vertex whose hold_time is not a time
        pp['E_vertex'][12] = pp['E_start'][12]          # and one that holds
        pp['hold_time'] = hold
    out = run(iv, case, 65, poke=poke, off=off)
    bad = [7, 9, 11, 20]
    assert (out['status'][bad] == SR.INPUT).all() and not out['steps'][bad].any()
    for k in ALL:
        assert np.isnan(out[k][bad]).all(), k
    assert out['status'][12] == SR.DONE and out['t_reached'][12] == 2.0 * case.opts['n_segments']
    same(out, clean, rows=~np.isin(np.arange(65), bad + [12]))
    # an equal vertex without any hold_time
    out = run(iv, case, 65, poke=lambda pp: pp['E_vertex'].__setitem__(11, pp['E_start'][11]))
    assert out['status'][11] == SR.INPUT and np.isnan(out['theta'][11]).all()
    same(out, clean, rows=np.arange(65) != 11)
    # a ramped start that does not converge (the terrace-and-step model at strength 0), as the restatement says
    ts = C.case('terrace_step')
    E_bad, c_bad, p_bad = C.unconverged_start()

    def unconverged(pp):
        pp['E_start'][20], pp['E_vertex'][20], pp['csurf'][20], pp['phi_surface'][20] = E_bad, E_bad - 0.1, c_bad, p_bad
    ramped = run(iv, ts._replace(theta0=None), 65, start_ramp=10)
    out = run(iv, ts._replace(theta0=None), 65, poke=unconverged, start_ramp=10)
    assert (ramped['status'] == SR.DONE).all() and out['status'][20] == SR.INPUT and np.isnan(out['theta'][20]).all() and not out['steps'][20].any()
    same(out, ramped, rows=np.arange(65) != 20)
    # a theta0 that leaves the step sites (x = 0.1) without a free site, and one that is not finite; the free-site entries are ignored
    given = run(iv, ts, 65)
    th = ts.theta0[np.arange(65) % 2].copy()
    t = IR._arrays(ts.tables)
    on_step = np.flatnonzero((t['site_of'] == 1) & (np.arange(t['T']) >= 2))
    th[5, on_step[0]] = 0.2
    th[9, 3] = np.inf
    th[11, :2] = np.nan
    out = run(iv, ts, 65, poke=lambda pp: pp.__setitem__('theta0', th))
    assert list(out['status'][[5, 9, 11]]) == [SR.INPUT, SR.INPUT, SR.DONE]
    assert np.isnan(out['theta'][[5, 9]]).all() and np.isnan(out['t_reached'][[5, 9]]).all()
    same(out, given, rows=~np.isin(np.arange(65), (5, 9)))


def test_a_step_budget_ends_a_lane_with_nan_in_the_rows_it_did_not_reach(iv):
    case, ref = C.case('frumkin_quasi'), C.reference('frumkin_quasi')
    out = run(iv, case, max_steps=5)
    assert (out['status'] == SR.STEPS).all() and (out['steps'][:, :2].sum(axis=1) == 5).all()
    for k in ('theta', 'current', 'current_scale', 'charge', 'E_out', 'energy_shift', 'mean_current'):
        assert np.isnan(out[k]).all(), k
    assert (out['t_reached'] > 0.0).all() and (out['t_reached'] < C.tau(case) / case.opts['samples']).all()
    # a budget that ends between two output times, against the restatement with the same budget
    want = C.run(case, points=[0], max_steps=150)
    out = run(iv, case, max_steps=150)
    reached = np.isfinite(want['current'][0])
    assert 0 < reached.sum() < len(reached)
    assert out['status'][0] == SR.STEPS == want['status'][0] and np.array_equal(out['steps'][0], want['steps'][0])
    assert np.array_equal(np.isfinite(out['theta'][0]).all(axis=1), reached) and np.array_equal(np.isfinite(out['charge'][0]), reached)
    compare(out, want, case, 'frumkin_quasi with 150 steps', rows=slice(0, 1))
    assert abs(out['t_reached'][0] / want['t_reached'][0] - 1.0) <= 1e-12
    assert np.array_equal(out['status'], [SR.STEPS if s.sum() > 150 else SR.DONE for s in ref['steps'][:, :2]])
