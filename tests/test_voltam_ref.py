"""The NumPy restatement of include/catint_voltam.h (tests/voltam_ref.py, which tests/test_gpu_voltam.py compares the device with)
against things it shares no code with: scipy's Radau on d theta / dt = G(theta, E(t)), the closed form of the reversible adsorption
peak, and the discrete charge identity of the header.  No GPU.

Measured with the restatement (x86-64, NumPy 2.x, scipy 1.15); every constant below is what the run printed:
  Radau          the largest |i - i_Radau| over the outputs and the points of a case, over the point's largest |i_Radau|:
                   case            rtol 1e-3   rtol 1e-4
                   langmuir_rev    4.48e-04    6.49e-05
                   langmuir_quasi  6.34e-04    8.01e-05
                   langmuir_slow   4.14e-04    5.59e-05
                   two_peak        4.56e-04    6.78e-05
                 About sevenfold per decade of rtol on every case: the accepted state is second order.
  reversible     langmuir_rev at 0.05 V/s, 1 mV between outputs, rtol 1e-4: peak height 6.4e-05 and width 2.5e-05 relative to the
                 closed form, against a bound of 10 v / (kT k0) = 1.9e-3.
  identity       max |sum dq - sum_s w_s (theta_s - theta_s(0))| over all outputs, in monolayers: langmuir_rev 1.4e-12,
                 langmuir_quasi 3.0e-15, langmuir_slow 2.8e-15, two_peak 5.8e-15.  (langmuir_rev: 900 steps, each with a Newton
                 residual that the gross rate of 1e4 /s times h turns into charge.)
  ulp shifts     every ln kf, ln kb moved by +-4 ulp: the same four counters and statuses on every case; ln theta moves by at most
                 4.99e-11, the current by at most 2.77e-11 of current_scale and the fluxes by the same 2.77e-11 of flux_scale (all
                 langmuir_quasi), the charge by at most 3.82e-13 of F site_density + max |charge| of the point (langmuir_rev).  The four tolerances are ten times that.  They are
                 a thousand times those of tests/test_kintrans_ref.py because here the step size follows an error estimate that is
                 itself a difference of currents, each a difference of gross rates: rounding moves h by parts in 1e9, and a
                 solution with a global error of 1e-3 moves with it.
  slow sweep     co2r_two_site at 1 and 2 mV/s: theta at the outputs is 1.30e-11 (in ln theta) from the steady state at E_out.
  margins        the smallest distance of a decision from its threshold over all cases: err 1.1e-3, Newton exit 7.9e-4, theta_e
                 against 0 0.99, landing 2.6e-3, Ga branch 3.7e-5: all above the 1e-6 the guard asks for."""
import functools

import numpy as np
import pytest

from tests import kinetics_ref as KR
from tests import voltam_cases as C
from tests import voltam_ref as VR

RADAU_CASES = ['langmuir_rev', 'langmuir_quasi', 'langmuir_slow', 'two_peak']
RADAU_ERR = {('langmuir_rev', 1e-3): 4.48e-4, ('langmuir_rev', 1e-4): 6.49e-5, ('langmuir_quasi', 1e-3): 6.34e-4, ('langmuir_quasi', 1e-4): 8.01e-5,
             ('langmuir_slow', 1e-3): 4.14e-4, ('langmuir_slow', 1e-4): 5.59e-5, ('two_peak', 1e-3): 4.56e-4, ('two_peak', 1e-4): 6.78e-5}
IDENTITY_ERR = {'langmuir_rev': 1.4e-12, 'langmuir_quasi': 3.0e-15, 'langmuir_slow': 2.8e-15, 'two_peak': 5.8e-15}
LN_THETA_TOL = 4.99e-10
CURRENT_TOL = 2.77e-10         # of current_scale
CHARGE_TOL = 3.82e-12          # of charge_scale(): F site_density + the point's largest |charge|
FLUX_TOL = 2.77e-10            # of flux_scale
SLOW_SWEEP = (1e-3, 2e-3)      # V/s: co2r_two_site follows its steady state
SLOW_SWEEP_LN_THETA = 1.30e-11 # the restatement's largest |ln theta - ln theta_steady| at the outputs of that sweep
GPU_CASES = C.CASE_NAMES       # every case runs on the device


# ---- scipy's Radau on the same equation ---------------------------------------------------------------------------------------------
def radau_current(c, p):
    """i(t_out) [n_out] of point p of case c: d theta_s / dt = G_s(theta, E(t)), s >= 1, the free site from the balance, restarted at
    every vertex; the start is the restatement's (the steady state at E_start)"""
    from scipy.integrate import solve_ivp
    t = KR._arrays(c.tables)
    Es, Ev, v = c.E_start[p], c.E_vertex[p], c.scan_rate[p]
    tau = VR.program(Es, Ev, v)
    K, nseg = c.opts['samples'], c.opts['n_segments']
    a = np.maximum(c.csurf[p], 0.0) / t['cref']
    w, CS, pzc = c.kw['w'], c.kw['CS'], c.kw['phi_pzc']
    off = np.zeros((t['R'], 2))

    def rates(theta_ads, E):
        theta = np.concatenate([[1.0 - (t['ns'][1:] * theta_ads).sum()], theta_ads])
        y = np.log(np.maximum(theta, 1e-300))
        V, sg = KR.potential_and_charge(E, c.phi_surface[p], w, CS, pzc, None)
        lf, lb, _ = KR.rate_constants(t, V, sg, off)
        rf, rb, _, _ = KR.rates(t, y, a, lf, lb)
        return rf, rb

    start = C.run(c, points=[p], n_segments=1, samples=1, max_steps=1)['theta_start'][0]
    theta = start[1:].copy()
    out = []
    for k in range(nseg):
        def rhs(tt, th, k=k):
            rf, rb = rates(th, VR.potential_at(Es, Ev, tau, k, tt))
            return (t['m'].T @ (rf - rb))[1:]
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
    assert (r['status'] == VR.DONE).all()
    i = -r['current'] / (VR.FARADAY * c.tables['site_density'])
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


# ---- the reversible peak ----------------------------------------------------------------------------------------------------------------
def test_the_reversible_peak_has_the_height_and_the_width_of_its_closed_form():
    """i = (v / kT) e^x / (1 + e^x)^2, x = (E - E0) / kT at unit activity: height v / (4 kT), full width at half maximum
    2 ln(3 + 2 sqrt 2) kT = 3.53 kT.  Both within 10 v / (kT k0), the size of the finite-rate correction.  One forward segment at
    0.05 V/s with 1 mV between the outputs; the height from the parabola through the three highest outputs, the width from the two
    linear crossings of half of it"""
    c = C.case('langmuir_rev')
    v, k0, kT = c.scan_rate[0], C.LANGMUIR_K0['langmuir_rev'], C.KT_EV
    r = C.run(c, points=[0], n_segments=1, samples=600, rtol=1e-4)
    assert r['status'][0] == VR.DONE
    i = -r['current'][0] / (VR.FARADAY * c.tables['site_density'])
    E = r['E_out'][0]
    assert (i > 0).all()          # a reduction: electrons on the reactant side are consumed
    j = int(i.argmax())
    assert 2 < j < len(i) - 3
    p = np.polyfit(E[j - 1:j + 2] - E[j], i[j - 1:j + 2], 2)
    height = p[2] - p[1] ** 2 / (4.0 * p[0])
    half = 0.5 * height

    def crossing(rng):
        for q in rng:
            if (i[q] - half) * (i[q + 1] - half) <= 0.0:
                return E[q] + (half - i[q]) * (E[q + 1] - E[q]) / (i[q + 1] - i[q])
        raise AssertionError('no crossing')
    width = abs(crossing(range(j, len(i) - 1)) - crossing(range(j - 1, -1, -1)))
    bound = 10.0 * v / (kT * k0)
    eh, ew = abs(height / (v / (4.0 * kT)) - 1.0), abs(width / (2.0 * np.log(3.0 + 2.0 * np.sqrt(2.0)) * kT) - 1.0)
    print('reversible peak: height off by %.1e, width by %.1e, bound %.1e; E_peak - E0 = %.2e V' % (eh, ew, bound, E[j] - C.E0))
    assert eh <= bound and ew <= bound
    assert abs(E[j] - C.E0) <= 1.5e-3          # one output spacing and a half


# ---- the charge identity ------------------------------------------------------------------------------------------------------------------
def identity_error(name, r=None):
    c, r = C.case(name), C.reference(name) if r is None else r
    w = np.array(C.IDENTITY_W[name])
    m = KR._arrays(c.tables)['m']
    assert np.array_equal(m @ w, c.electrons)          # ne_r = sum_s w_s m[r][s]
    return float(np.abs(r['dq'] - (r['theta'] - r['theta_start'][:, None, :]) @ w).max())


@pytest.mark.parametrize('name', sorted(C.IDENTITY_W))
def test_the_charge_is_the_change_of_the_coverages(name):
    err = identity_error(name)
    print(name, 'max |sum dq - sum w (theta - theta(0))| = %.1e (recorded %.1e)' % (err, IDENTITY_ERR[name]))
    assert err <= 10.0 * IDENTITY_ERR[name]


def test_the_mean_current_of_a_full_cycle_carries_the_charge_the_coverages_changed_by():
    """mean_current times the distance of the output times, summed over the cycle, is the charge at its end, and that is F
    site_density w (theta(end) - theta(0)) within the bound of the identity: the cycle of the reversible couple returns what it took
    up to the lag of the coverage behind its equilibrium, 1e-9 of a monolayer at 0.05 V/s"""
    from catint_amd.voltammetry import mean_current
    name = 'langmuir_rev'
    c, r = C.case(name), C.reference(name)
    Fsd = VR.FARADAY * c.tables['site_density']
    mc = mean_current(r['charge'], c.E_start, c.E_vertex, c.scan_rate, c.opts['samples'])
    assert np.array_equal(mc, VR.mean_current(r['charge'], C.tau(c), c.opts['samples']))
    total = (mc * (C.tau(c) / c.opts['samples'])[:, None]).sum(axis=1)
    assert np.allclose(total, r['charge'][:, -1], rtol=1e-12, atol=1e-14 * Fsd)
    net = -total / Fsd
    change = (r['theta'][:, -1, :] - r['theta_start']) @ np.array(C.IDENTITY_W[name])
    print('net charge of the cycle (monolayers)', net, 'coverage change', change)
    assert np.abs(net - change).max() <= 10.0 * IDENTITY_ERR[name]
    assert abs(net[0]) <= 1e-8 and np.abs(r['charge'][0]).max() / Fsd > 0.99


def charge_scale(case, ref):
    """[n][1]: what a charge error is stated relative to -- one electron per site plus the largest charge the point passes"""
    return VR.FARADAY * case.tables['site_density'] + np.nanmax(np.abs(ref['charge']), axis=1, keepdims=True)


# ---- what the device comparison rests on ----------------------------------------------------------------------------------------------------
def test_the_cases_end_done_and_extrapolate():
    """every point DONE; per case at most one point in three has more than 10 % of its accepted steps on the fallback; the points of
    a case take different numbers of steps"""
    for name in C.CASE_NAMES:
        c, r = C.case(name), C.reference(name)
        assert 2 <= len(c.E_start) <= 3 and len(set(c.scan_rate)) > 1
        assert c.opts['n_segments'] in (1, 2, 3) and c.opts['samples'] in (8, 12)
        assert (r['status'] == VR.DONE).all(), (name, r['status'])
        heavy = (r['steps'][:, 3] > 0.1 * r['steps'][:, 0]).sum()
        assert 3 * heavy <= len(c.E_start), (name, r['steps'].tolist())
        assert len({tuple(s) for s in r['steps'].tolist()}) == len(c.E_start), (name, r['steps'].tolist())
        assert np.array_equal(r['t_reached'], c.opts['n_segments'] * C.tau(c))
    assert {c.opts['n_segments'] for c in map(C.case, C.CASE_NAMES)} == {1, 2, 3}
    # langmuir_slow runs on the Ea branch over the whole sweep
    c = C.case('langmuir_slow')
    t = KR._arrays(c.tables)
    for E in np.linspace(c.E_vertex[0], c.E_start[0], 50):
        assert KR.rate_constants(t, E, 0.0, np.zeros((1, 2)))[2][0] == 0


@pytest.mark.parametrize('name', C.CASE_NAMES)
def test_site_balance_at_every_output(name):
    c, r = C.case(name), C.reference(name)
    bal = np.abs((r['theta'] * np.asarray(c.tables['site_count'])).sum(axis=-1) - 1.0)
    assert np.isfinite(bal).all() and bal.max() <= 4 * np.spacing(1.0), bal.max() / np.spacing(1.0)


def test_statuses_nan_rows_and_the_program():
    c = C.case('n0')
    r = C.reference('n0')
    # E_out: down and back, every vertex an output
    K = c.opts['samples']
    assert np.allclose(r['E_out'][:, K - 1], c.E_vertex, rtol=1e-14) and np.allclose(r['E_out'][:, 2 * K - 1], c.E_start, rtol=1e-14)
    assert (np.diff(r['E_out'][:, :K], axis=1) < 0).all() and (np.diff(r['E_out'][:, K - 1:], axis=1) > 0).all()
    # a budget that ends between two outputs
    b = C.run(c, points=[0], max_steps=150)
    reached = np.isfinite(b['current'][0])
    assert b['status'][0] == VR.STEPS and b['steps'][0, :2].sum() == 150 and 0 < reached.sum() < 2 * K and not reached[reached.argmin():].any()
    k = reached.sum()
    assert np.array_equal(b['theta'][0, :k], r['theta'][0, :k]) and np.isnan(b['theta'][0, k:]).all() and np.isnan(b['charge'][0, k:]).all()
    # bad programs and inputs: CATVM_INPUT, everything NaN, no step
    t = KR._arrays(c.tables)
    for bad in (dict(E_start=np.nan), dict(E_vertex=np.inf), dict(E_vertex=c.E_start[0]), dict(off=np.full((1, 2), 800.0)),
                dict(theta0=np.array([0.0, 1.5])), dict(theta0=np.array([0.5, np.nan]))):
        args = dict(E_start=c.E_start[0], E_vertex=c.E_vertex[0])
        kw = dict(c.kw, **c.opts)
        for key in list(bad):
            if key in args:
                args[key] = bad.pop(key)
        o = VR.solve_point(t, c.electrons, args['E_start'], args['E_vertex'], c.scan_rate[0], c.csurf[0], c.phi_surface[0], **kw, **bad)
        assert o['status'] == VR.INPUT and np.isnan(o['theta']).all() and np.isnan(o['E_out']).all() and np.isnan(o['t_reached']) and not o['steps'].any()
    # a given start is used as it is: no steady solve
    o = VR.solve_point(t, c.electrons, c.E_start[0], c.E_vertex[0], c.scan_rate[0], c.csurf[0], c.phi_surface[0], theta0=np.array([np.nan, 0.25]),
                       **c.kw, **c.opts)
    assert o['status'] == VR.DONE and np.array_equal(o['theta_start'], [0.75, 0.25])


@pytest.mark.parametrize('name', GPU_CASES)
def test_no_decision_of_a_device_case_sits_on_its_threshold(name):
    """The guard of the device comparison: no accept / reject decision, Newton exit, sign of an extrapolated coverage, landing or Ga
    branch within 1e-6 (relative) of its threshold (a case that violates it is replaced by other potentials, never skipped); and
    moving the rate constants by +-4 ulp changes no counter and moves ln theta, current and charge by at most a tenth of the device
    tolerances"""
    c, r = C.case(name), C.reference(name)
    for key in ('err_margin', 'newton_margin', 'extrap_margin', 'land_margin', 'branch_margin'):
        assert r[key].min() >= 1e-6, (key, r[key].min())
    worst = np.zeros(4)
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
    print(name, '+-4 ulp move ln theta by %.2e, the current by %.2e of current_scale, the charge by %.2e of its scale, the fluxes by %.2e of '
          'flux_scale' % tuple(worst))
    assert worst[0] <= LN_THETA_TOL / 10 * 1.01 and worst[1] <= CURRENT_TOL / 10 * 1.01 and worst[2] <= CHARGE_TOL / 10 * 1.01
    assert worst[3] <= FLUX_TOL / 10 * 1.01


def slow_sweep_case():
    return C.co2r_case(rates=SLOW_SWEEP, n_segments=1, samples=8)


def test_a_slow_sweep_follows_the_steady_state():
    """co2r_two_site at 1 and 2 mV/s: theta at the outputs is the steady state of tests/kinetics_ref.py at E_out to 1e-6 (in ln
    theta); the figure is what tests/test_gpu_voltam.py holds the device and PnpSolver.get_kinetics to, twice over"""
    c = slow_sweep_case()
    r = C.run(c)
    assert (r['status'] == VR.DONE).all()
    n, K = r['E_out'].shape
    st = KR.solve_fp64(c.tables, r['E_out'].reshape(-1), np.repeat(c.csurf, K, axis=0), np.repeat(c.phi_surface, K), sens=False, **c.kw)
    assert (st['status'] == 0).all()
    d = float(np.abs(np.log(r['theta'].reshape(n * K, -1)) - st['y']).max())
    print('slow sweep: max |ln theta - ln theta_steady| = %.2e (recorded %.2e), steps %s' % (d, SLOW_SWEEP_LN_THETA, r['steps'].tolist()))
    assert d <= 1e-6
    assert SLOW_SWEEP_LN_THETA / 3.0 <= d <= 3.0 * SLOW_SWEEP_LN_THETA
