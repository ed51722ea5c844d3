"""The NumPy restatement of include/catint_iasweep.h (tests/iasweep_ref.py, which tests/test_gpu_iasweep.py compares the device with)
against things it shares no code with: tests/voltam_ref.py at G = 1 and strength 0 (bit for bit), the closed form of the Frumkin
adsorption peak, scipy's Radau on d theta / dt = G(theta, E(t)) of the interacting model, central differences of the implicit Euler
residual, the discrete charge identity, and the steady state of tests/interact_ref.py at the end of a long hold.  No GPU.

Measured with the restatement (x86-64, NumPy 2.x, scipy 1.15); every constant below is what the run printed:
  Radau          the largest |i - i_Radau| over the outputs and the points of a case, over the point's largest |i_Radau|:
                   case            rtol 1e-3   rtol 1e-4
                   frumkin_rep     6.42e-04    7.24e-05
                   frumkin_att     5.53e-04    6.95e-05
                   frumkin_quasi   8.42e-04    1.02e-04
                   co2r_weak       4.18e-05    1.55e-06
  Frumkin        at 0.05 V/s, 1 mV between outputs, rtol 1e-4, relative to the closed form, against a bound of 10 v / (kT k0) = 1.9e-3:
                   eps = +2: turnover on the forward branch 4.0e-5, peak height 1.1e-5;   eps = -2: 1.9e-4, 1.3e-4
  identity       max |sum dq - sum_s w_s (theta_s - theta_s(0))| over all outputs, in monolayers: frumkin_rep 5.8e-12, frumkin_att
                 1.3e-12, frumkin_quasi 3.1e-15
  Jacobian       the analytic implicit Euler Jacobian against central differences of the residual (step 1e-6 in y), largest
                 difference over the largest entry, over all cases and the piecewise case inside its smoothing window: 2.0e-9
  hold           hold_relax followed for 500 s per segment: max |ln theta - ln theta_steady| = 2.2e-16
  ulp shifts     every ln kf, ln kb of the step loop moved by +-4 ulp: the same four counters and statuses on every case; ln theta
                 moves by at most 8.59e-12 (frumkin_att), the current by at most 4.29e-12 of current_scale (frumkin_att), the fluxes
                 by 4.29e-12 of flux_scale (frumkin_att), the charge by 4.27e-12 of its scale (frumkin_rep), energy_shift by
                 9.27e-15 kT (frumkin_att).  The five tolerances are ten times that.
  margins        the smallest distance of a decision from its threshold over all cases: err 4.2e-5, Newton exit 1.6e-4,
                 theta_e against 0 0.99, landing 8.6e-5, Ga branch 9.4e-5: all above the 1e-6 the guard asks for."""
import functools

import numpy as np
import pytest

from tests import iasweep_cases as C
from tests import iasweep_ref as SR
from tests import interact_ref as IR
from tests import kinetics_ref as KR
from tests import voltam_cases as VC
from tests import voltam_ref as VR

RADAU_CASES = ['frumkin_rep', 'frumkin_att', 'frumkin_quasi', 'co2r_weak']
RADAU_ERR = {('frumkin_rep', 1e-3): 6.42e-4, ('frumkin_rep', 1e-4): 7.24e-5, ('frumkin_att', 1e-3): 5.53e-4, ('frumkin_att', 1e-4): 6.95e-5,
             ('frumkin_quasi', 1e-3): 8.42e-4, ('frumkin_quasi', 1e-4): 1.02e-4, ('co2r_weak', 1e-3): 4.18e-5, ('co2r_weak', 1e-4): 1.55e-6}
IDENTITY_ERR = {'frumkin_rep': 5.8e-12, 'frumkin_att': 1.3e-12, 'frumkin_quasi': 3.1e-15}
LN_THETA_TOL = 8.59e-11
CURRENT_TOL = 4.29e-11         # of current_scale
CHARGE_TOL = 4.27e-11          # of charge_scale(): F site_density + the point's largest |charge|
FLUX_TOL = 4.29e-11            # of flux_scale
SHIFT_TOL = 9.27e-14           # kT, on energy_shift
GPU_CASES = C.CASE_NAMES       # every case runs on the device
OUTPUTS = ('theta', 'current', 'current_scale', 'charge', 'E_out', 'flux', 'flux_scale', 't_reached', 'status', 'steps', 'dq', 'theta_start')


# ---- the reduction -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', VC.CASE_NAMES)
def test_one_site_type_without_interactions_has_the_bits_of_the_mean_field_restatement(name):
    c, ref = VC.case(name), VC.reference(name)
    got = SR.solve(SR.mean_field_tables(c.tables), c.electrons, c.E_start, c.E_vertex, c.scan_rate, c.csurf, c.phi_surface, theta0=c.theta0,
                   start_ramp=1, **c.kw, **c.opts)
    for k in OUTPUTS:
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
    assert not np.nan_to_num(got['energy_shift']).any()


# ---- the Frumkin peak --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['frumkin_rep', 'frumkin_att'])
def test_the_reversible_peak_is_the_frumkin_isotherm_s(name):
    """theta / (1 - theta) = exp(-(E - E0) / kT - eps theta) at unit activity, so on the forward branch the turnover is
    (v / kT) theta (1 - theta) / (1 + eps theta (1 - theta)) at the restatement's own theta, and its peak, at theta = 1/2, is
    v / ((4 + eps) kT).  Both within 10 v / (kT k0), the size of the finite-rate correction.  One forward segment at 0.05 V/s with
    1 mV between the outputs; the height from the parabola through the three highest outputs"""
    c = C.case(name)
    eps, v, k0, kT = C.FRUMKIN_EPS[name], c.scan_rate[0], VC.LANGMUIR_K0['langmuir_rev'], C.KT_EV
    samples = int(round(abs(c.E_vertex[0] - c.E_start[0]) / 1e-3))
    r = C.run(c, points=[0], n_segments=1, samples=samples, rtol=1e-4)
    assert r['status'][0] == SR.DONE
    i = -r['current'][0] / (SR.FARADAY * c.tables['site_density'])
    th = r['theta'][0, :, 1]
    assert (i > 0).all()
    closed = v / kT * th * (1.0 - th) / (1.0 + eps * th * (1.0 - th))
    j = int(i.argmax())
    assert 2 < j < len(i) - 3
    E = r['E_out'][0]
    p = np.polyfit(E[j - 1:j + 2] - E[j], i[j - 1:j + 2], 2)
    height = p[2] - p[1] ** 2 / (4.0 * p[0])
    peak = v / ((4.0 + eps) * kT)
    bound = 10.0 * v / (kT * k0)
    ei, eh = float(np.abs(i - closed).max() / peak), abs(height / peak - 1.0)
    print(name, 'turnover off the closed form by %.2e of the peak, peak height by %.2e, bound %.1e; theta at the peak %.4f' % (ei, eh, bound, th[j]))
    assert ei <= bound and eh <= bound
    assert abs(th[j] - 0.5) <= 0.03


# ---- scipy's Radau on the same equation ---------------------------------------------------------------------------------------------
def radau_current(c, p):
    """i(t_out) [n_out] of point p of case c: d theta_s / dt = G_s(theta, E(t)) for the adsorbates, the free site of every type from
    its balance, restarted at every vertex; the start is the restatement's"""
    from scipy.integrate import solve_ivp
    t = IR._arrays(c.tables)
    G = t['G']
    Es, Ev, v = c.E_start[p], c.E_vertex[p], c.scan_rate[p]
    tau = VR.program(Es, Ev, v)
    K, nseg = c.opts['samples'], c.opts['n_segments']
    a = np.maximum(c.csurf[p], 0.0) / t['cref']
    w, CS, pzc = c.kw['w'], c.kw['CS'], c.kw['phi_pzc']
    off = np.zeros((t['R'], 2))

    def rates(theta_ads, E):
        theta = np.concatenate([np.zeros(G), theta_ads])
        for g in range(G):
            theta[g] = t['x'][g] - (t['ns'] * theta)[(t['site_of'] == g) & (np.arange(t['T']) >= G)].sum()
        y = np.log(np.maximum(theta, 1e-300))
        V, sg = KR.potential_and_charge(E, c.phi_surface[p], w, CS, pzc, None)
        th, wv, _, _ = IR.surface_state(t, y)
        lf, lb = IR.step_constants(t, V, sg, off, t['strength'], th, wv)[:2]
        rf, rb, _, _ = IR.rates(t, y, a, lf, lb)
        return rf, rb

    start = C.run(c, points=[p], n_segments=1, samples=1, max_steps=1)['theta_start'][0]
    theta = start[G:].copy()
    out = []
    for k in range(nseg):
        def rhs(tt, th, k=k):
            rf, rb = rates(th, VR.potential_at(Es, Ev, tau, k, tt))
            return (t['m'].T @ (rf - rb))[G:]
        times = np.array([VR.output_time(tau, K, k * K + m) for m in range(K)])
        sol = solve_ivp(rhs, (k * tau, times[-1]), theta, method='Radau', rtol=1e-11, atol=1e-15, t_eval=times)
        assert sol.success and sol.y.shape[1] == K
        for m in range(K):
            rf, rb = rates(sol.y[:, m], VR.potential_at(Es, Ev, tau, k, times[m]))
            out.append(float(c.electrons @ (rf - rb)))
        theta = sol.y[:, -1]
    return np.array(out)


@functools.lru_cache(maxsize=None)
def radau(name):
    c = C.case(name)
    return np.array([radau_current(c, p) for p in range(len(c.E_start))])


def current_error(name, rtol):
    """largest |i - i_Radau| over the point's largest |i_Radau|, over the points"""
    c = C.case(name)
    r = C.reference(name) if rtol == C.RTOL else C.run(c, rtol=rtol)
    assert (r['status'] == SR.DONE).all()
    i = -r['current'] / (SR.FARADAY * c.tables['site_density'])
    ref = radau(name)
    return float((np.abs(i - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())


@pytest.mark.parametrize('name', RADAU_CASES)
def test_the_current_against_radau(name):
    e3, e4 = current_error(name, 1e-3), current_error(name, 1e-4)
    print(name, 'current error over the peak height: %.2e at rtol 1e-3 (recorded %.2e), %.2e at 1e-4 (recorded %.2e)'
          % (e3, RADAU_ERR[name, 1e-3], e4, RADAU_ERR[name, 1e-4]))
    assert e3 <= 3.0 * RADAU_ERR[name, 1e-3]
    assert e4 <= 3.0 * RADAU_ERR[name, 1e-4]
    assert e4 < e3


# ---- the analytic Jacobian ---------------------------------------------------------------------------------------------------------------
def jacobian_error(c, p, y, E, h):
    """the implicit Euler Jacobian at y against central differences of the residual with the row scales w held (as the header holds
    them within an iteration): the largest difference over the largest entry"""
    t = IR._arrays(c.tables)
    log = dict(branch_margin=np.inf)
    a = np.maximum(c.csurf[p], 0.0) / t['cref']
    P = SR._Point(t, a, np.asarray(c.electrons, float), np.zeros((t['R'], 2)), c.kw['w'], c.phi_surface[p], c.kw['CS'], c.kw['phi_pzc'], None,
                  t['strength'], 0, log)
    P.at(E)
    th_old = np.exp(y) * 0.9
    A, F = SR.be_system(P, y, th_old, h)
    w = np.exp(y) + h * P.rows(y)[1]
    G = t['G']

    def residual(yy):
        G_, _, _ = P.rows(yy)
        th = np.exp(yy)
        F_ = ((th - th_old) - h * G_) / w
        nth = t['ns'] * th
        for g in range(G):
            F_[g] = nth[t['site_of'] == g].sum() / t['x'][g] - 1.0
        return F_
    num = np.zeros_like(A)
    d = 1e-6
    for v in range(t['T']):
        e = np.zeros(t['T'])
        e[v] = d
        num[:, v] = (residual(y + e) - residual(y - e)) / (2.0 * d)
    return float(np.abs(A - num).max() / np.abs(A).max())


@pytest.mark.parametrize('name', C.CASE_NAMES)
def test_the_jacobian_is_the_derivative_of_the_residual(name):
    c, r = C.case(name), C.reference(name)
    K = r['y'].shape[1]
    worst = 0.0
    for p in range(len(c.E_start)):
        for k in (0, K // 2, K - 1):
            h = C.tau(c)[p] / c.opts['samples'] / 10.0
            worst = max(worst, jacobian_error(c, p, r['y'][p, k].copy(), r['E_out'][p, k], h))
    print(name, 'Jacobian against central differences: %.1e of the largest entry' % worst)
    assert worst <= 1e-6


def test_the_jacobian_inside_the_smoothing_window_of_the_piecewise_response():
    """coverages that put the crowding of both types inside (c - s, c + s), where f' is not 0 or 1"""
    c = C.case('random_S7_G2_piecewise')
    t = IR._arrays(c.tables)
    theta = np.zeros(t['T'])
    for g in range(t['G']):
        ads = np.flatnonzero((t['site_of'] == g) & (np.arange(t['T']) >= t['G']))
        crowd = t['cutoff'][g] + 0.3 * t['smooth'][g]
        theta[ads] = crowd * t['x'][g] / (t['ns'][ads] * len(ads))
        theta[g] = t['x'][g] * (1.0 - crowd)
    y = np.log(theta)
    f, fp = IR.surface_state(t, y)[2:]
    assert ((fp > 0.0) & (fp < 1.0)).all() and (f > 0.0).all()
    err = jacobian_error(c, 0, y, -0.35, 1e-3)
    print('Jacobian inside the smoothing window: %.1e of the largest entry (f = %s, f\' = %s)' % (err, f, fp))
    assert err <= 1e-6


# ---- the charge identity ------------------------------------------------------------------------------------------------------------------
def identity_error(name):
    c, r = C.case(name), C.reference(name)
    w = np.array(C.IDENTITY_W[name])
    m = IR._arrays(c.tables)['m']
    assert np.array_equal(m @ w, c.electrons)          # ne_r = sum_s w_s m[r][s]
    return float(np.abs(r['dq'] - (r['theta'] - r['theta_start'][:, None, :]) @ w).max())


@pytest.mark.parametrize('name', sorted(C.IDENTITY_W))
def test_the_charge_is_the_change_of_the_coverages(name):
    err = identity_error(name)
    print(name, 'max |sum dq - sum w (theta - theta(0))| = %.1e (recorded %.1e)' % (err, IDENTITY_ERR[name]))
    assert err <= 10.0 * IDENTITY_ERR[name]


# ---- the hold ------------------------------------------------------------------------------------------------------------------------------
def test_a_long_hold_ends_in_the_steady_state_of_the_interacting_model():
    c = C.case('hold_relax')
    r = C.run(c, points=[0], hold_time=np.array([500.0]))
    assert r['status'][0] == SR.DONE and np.array_equal(r['E_out'][0], np.full(c.opts['samples'], c.E_start[0]))
    st = IR.solve_fp64(c.tables, c.E_start[:1], c.csurf[:1], c.phi_surface[:1], sens=False, tol=1e-12, **c.kw)
    assert st['status'][0] == 0
    d = float(np.abs(r['y'][0, -1] - st['y'][0]).max())
    print('hold: max |ln theta - ln theta_steady| after 500 s = %.1e (Newton tolerance %.0e)' % (d, SR.DEFAULTS['newton_tol']))
    assert d <= SR.DEFAULTS['newton_tol']
    # the case itself: the coverage rises from theta0 = 0.1 towards the steady 0.337; the longer hold gets there
    ref = C.reference('hold_relax')
    assert (np.diff(ref['theta'][0, :, 1]) > 0.0).all() and 0.1 < ref['theta'][0, 0, 1] < ref['theta'][1, 0, 1]
    assert abs(ref['theta'][1, -1, 1] - st['theta'][0, 1]) <= 1e-8 and np.array_equal(ref['t_reached'], c.hold_time)


# ---- what the device comparison rests on ----------------------------------------------------------------------------------------------------
def test_the_cases_end_done_and_stay_within_the_limits_of_the_solve():
    for name in C.CASE_NAMES:
        c, r = C.case(name), C.reference(name)
        G = len(c.tables['site_fraction'])
        assert 2 <= len(c.E_start) <= 3 and c.opts['samples'] <= 12
        assert len(set(c.scan_rate)) > 1 or len(set(c.hold_time)) > 1
        assert (r['status'] == SR.DONE).all(), (name, r['status'])
        assert len({tuple(s) for s in r['steps'].tolist()}) == len(c.E_start), (name, r['steps'].tolist())
        assert np.array_equal(r['t_reached'], c.opts['n_segments'] * C.tau(c))
        assert r['theta'][:, :, :G].min() >= 1e-5, (name, r['theta'][:, :, :G].min())
    c = C.case('random_S7_G2_piecewise')
    assert np.asarray(c.tables['order_f']).shape[1] == 8 + 9 and len(c.tables['site_fraction']) == 2 and c.tables['response'] == 'piecewise'
    assert np.abs(C.reference('random_S7_G2_piecewise')['energy_shift']).max() > 0.0


@pytest.mark.parametrize('name', C.CASE_NAMES)
def test_site_balance_of_every_type_at_every_output(name):
    c, r = C.case(name), C.reference(name)
    t = IR._arrays(c.tables)
    for g in range(t['G']):
        bal = np.abs((r['theta'] * t['ns'])[:, :, t['site_of'] == g].sum(axis=-1) / t['x'][g] - 1.0)
        assert np.isfinite(bal).all() and bal.max() <= 4 * np.spacing(1.0), (g, bal.max() / np.spacing(1.0))


def test_statuses_of_a_point():
    c = C.case('frumkin_quasi')
    t = IR._arrays(c.tables)
    kw = dict(c.kw, **c.opts)
    base = dict(E_start=c.E_start[0], E_vertex=c.E_vertex[0])
    for bad in (dict(E_vertex=np.nan), dict(E_vertex=c.E_start[0]), dict(E_vertex=c.E_start[0], hold_time=0.0),
                dict(E_vertex=c.E_start[0], hold_time=np.inf), dict(theta0=np.array([0.0, 1.5])), dict(theta0=np.array([0.5, np.nan])),
                dict(off=np.full((1, 2), 800.0))):
        a = dict(base, **{k: bad.pop(k) for k in list(bad) if k in base})
        o = SR.solve_point(t, c.electrons, a['E_start'], a['E_vertex'], c.scan_rate[0], c.csurf[0], c.phi_surface[0], **kw, **bad)
        assert o['status'] == SR.INPUT and np.isnan(o['theta']).all() and np.isnan(o['t_reached']) and not o['steps'].any()
    # a hold_time beside a sweep changes nothing
    o = SR.solve_point(t, c.electrons, c.E_start[1], c.E_vertex[1], c.scan_rate[1], c.csurf[1], c.phi_surface[1], hold_time=3.0, **kw)
    assert np.array_equal(o['theta'], C.reference('frumkin_quasi')['theta'][1])
    # the terrace-and-step start does not converge without the repulsion: the ramp's first stage ends the point
    ts = C.case('terrace_step')
    E_bad, c_bad, p_bad = C.unconverged_start()
    tt = IR._arrays(ts.tables)
    kw = dict(ts.kw, **dict(ts.opts, start_ramp=10))
    o = SR.solve_point(tt, ts.electrons, E_bad, E_bad - 0.1, 1.0, c_bad, p_bad, **kw)
    assert o['status'] == SR.INPUT and np.isnan(o['theta']).all()
    o = SR.solve_point(tt, ts.electrons, ts.E_start[0], ts.E_vertex[0], ts.scan_rate[0], ts.csurf[0], ts.phi_surface[0], **kw)
    assert o['status'] == SR.DONE          # the case's own points do start with the ramp


def charge_scale(case, ref):
    """[n][1]: what a charge error is stated relative to -- one electron per site plus the largest charge the point passes"""
    return SR.FARADAY * case.tables['site_density'] + np.nanmax(np.abs(ref['charge']), axis=1, keepdims=True)


@pytest.mark.parametrize('name', GPU_CASES)
def test_no_decision_of_a_device_case_sits_on_its_threshold(name):
    """The guard of the device comparison: no accept / reject decision, Newton exit, sign of an extrapolated coverage, landing or Ga
    branch within 1e-6 (relative) of its threshold; and moving the rate constants by +-4 ulp changes no counter and moves ln theta,
    current, charge, fluxes and shifts by at most a tenth of the device tolerances"""
    c, r = C.case(name), C.reference(name)
    for key in ('err_margin', 'newton_margin', 'extrap_margin', 'land_margin', 'branch_margin'):
        assert r[key].min() >= 1e-6, (key, r[key].min())
    worst = np.zeros(5)
    for ulp in (4, -4):
        s = C.shifted(name, ulp)
        assert np.array_equal(s['steps'], r['steps']) and np.array_equal(s['status'], r['status'])
        ok = r['theta'] > 1e-200
        worst[0] = max(worst[0], np.abs(np.log(s['theta'][ok]) - np.log(r['theta'][ok])).max())
        worst[1] = max(worst[1], (np.abs(s['current'] - r['current']) / r['current_scale']).max())
        worst[2] = max(worst[2], (np.abs(s['charge'] - r['charge']) / charge_scale(c, r)).max())
        if r['flux'].size:
            used = r['flux_scale'] > 0.0          # (an idle species has no flux and no scale)
            worst[3] = max(worst[3], (np.abs(s['flux'] - r['flux'])[used] / r['flux_scale'][used]).max())
        worst[4] = max(worst[4], np.abs(s['energy_shift'] - r['energy_shift']).max())
    print(name, '+-4 ulp move ln theta by %.2e, the current by %.2e of current_scale, the charge by %.2e of its scale, the fluxes by %.2e of '
          'flux_scale, the shifts by %.2e kT; margins err %.1e newton %.1e extrap %.1e land %.1e branch %.1e'
          % (tuple(worst) + tuple(r[k].min() for k in ('err_margin', 'newton_margin', 'extrap_margin', 'land_margin', 'branch_margin'))))
    assert worst[0] <= LN_THETA_TOL / 10 * 1.01 and worst[1] <= CURRENT_TOL / 10 * 1.01 and worst[2] <= CHARGE_TOL / 10 * 1.01
    assert worst[3] <= FLUX_TOL / 10 * 1.01 and worst[4] <= SHIFT_TOL / 10 * 1.01
