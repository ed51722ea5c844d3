"""The NumPy restatement of include/catint_kintrans.h (tests/kintrans_ref.py, which tests/test_gpu_kintrans.py compares the device
with) against things it shares no code with: two closed forms, the site balance, the steady state of the Newton iteration of
tests/kinetics_ref.py, and the rescue of the networks that iteration fails on.  No GPU.

Measured with the restatement (x86-64, NumPy 2.x):
  closed forms   max |theta - exact| / rtol: A + * <-> A* 3.49 (rtol 1e-3), 11.44 (1e-4); the ring 2.48, 8.10.  The step control bounds
                 the local error, so the global one in units of rtol grows with the step count, about as rtol^-1/2.  K = 23 is twice
                 the largest value seen.
  ulp shifts     every ln kf, ln kb moved by +-4 ulp: the same steps and statuses on every case; ln theta moves by at most 6.1e-14
                 (random_S3), the fluxes by at most 1.8e-14 of flux_scale (random_S8).  LN_THETA_TOL and FLUX_TOL are ten times that.
  margins        the smallest |err - 1| over all accept / reject decisions is 1.6e-4 (rescue_S8), the smallest
                 |max|dy| / newton_tol - 1| over all Newton iterations 4.8e-3 (rescue_S8): far above the 1e-6 the guard asks for."""
import numpy as np
import pytest

from tests import kinetics_ref as KR
from tests import kintrans_cases as C
from tests import kintrans_ref as KT

K_GLOBAL = 23.0
LN_THETA_TOL = 6.1e-13
FLUX_TOL = 1.8e-13
GPU_CASES = C.CASE_NAMES          # every case runs on the device


@pytest.mark.parametrize('rtol', [1e-3, 1e-4])
def test_single_step_against_its_closed_form(rtol):
    """theta_inf + (theta_0 - theta_inf) exp(-(kf a + kb) t), desorption and adsorption: the global error is at most K rtol, K = 23
    (measured: 3.49 rtol at 1e-3, 11.44 rtol at 1e-4; twice the largest)"""
    c = C.langmuir_case(rtol)
    r = C.run(c)
    exact = C.langmuir_exact(c)
    err = np.abs(r['theta'][:, :, 1] - exact).max()
    print('langmuir rtol %g: %.2f rtol, steps %s' % (rtol, err / rtol, r['steps'].tolist()))
    assert (r['status'] == KT.DONE).all()
    assert err <= K_GLOBAL * rtol
    assert np.abs(r['theta'][:, :, 0] - (1.0 - exact)).max() <= K_GLOBAL * rtol


@pytest.mark.parametrize('rtol', [1e-3, 1e-4])
def test_first_order_ring_against_the_matrix_exponential(rtol):
    """expm(K t) theta_0 (scipy): at most K rtol (measured: 2.48 rtol at 1e-3, 8.10 rtol at 1e-4); the free site, which takes no part,
    keeps its coverage to rounding"""
    c = C.ring_case(rtol)
    r = C.run(c)
    exact = C.ring_exact(c)
    err = np.abs(r['theta'][:, :, 1:] - exact).max()
    print('ring rtol %g: %.2f rtol, steps %s' % (rtol, err / rtol, r['steps'].tolist()))
    assert (r['status'] == KT.DONE).all()
    assert err <= K_GLOBAL * rtol
    assert np.abs(r['theta'][0, :, 0] - c.theta0[0, 0]).max() <= 4 * np.spacing(1.0)


@pytest.mark.parametrize('name', C.CASE_NAMES)
def test_site_balance_at_every_output(name):
    c, r = C.case(name), C.reference(name)
    bal = np.abs((r['theta'] * np.asarray(c.tables['site_count'])).sum(axis=-1) - 1.0)
    assert np.isfinite(bal).all() and bal.max() <= 4 * np.spacing(1.0), bal.max() / np.spacing(1.0)


@pytest.mark.parametrize('name', ['co2r_one_site', 'co2r_two_site', 'random_S1', 'random_S3', 'random_S8'])
def test_the_stationary_state_is_the_newton_iteration_s(name):
    """steady_tol = 1e-9: the state reached, handed to the Newton iteration as its guess, converges in <= 3 iterations to the y the
    plain iteration finds from the uniform start"""
    c = C.case(name)
    r = C.run(c._replace(t_out=(1e12,)), steady_tol=1e-9)
    assert (r['status'] == KT.STEADY).all() and (r['drift'][:, 0] < 1e-9).all()
    assert (r['t_reached'] < 1e12).all() and (r['steps'][:, 0] <= 5000).all()
    warm = KR.solve_fp64(c.tables, c.phiM, c.csurf, c.phi_surface, theta_guess=r['theta'][:, 0], sens=False, **c.kw)
    plain = C.plain_newton(name)
    assert (warm['status'] == 0).all() and warm['iterations'].max() <= 3, warm['iterations']
    assert (plain['status'] == 0).all()
    ok = np.exp(plain['y']) > 1e-200
    print(name, 'steps', r['steps'][:, 0].tolist(), 'warm iterations', warm['iterations'].tolist(), 'max |dy| %.1e' % np.abs(warm['y'] - plain['y'])[ok].max())
    assert np.abs(warm['y'] - plain['y'])[ok].max() <= 1e-12


@pytest.mark.parametrize('name', C.RESCUE_NAMES)
def test_the_rescue(name):
    """At every point of the three rescue networks where the Newton iteration stops at maxit from the uniform start, the integration
    with the rescue's settings (rtol 1e-2, steady_tol 1e-6, t_out 1e12) ends CATKT_STEADY and the Newton iteration from that state
    converges"""
    c, r, plain = C.case(name), C.reference(name), C.plain_newton(name)
    failed = plain['status'] == 1
    assert failed.any()
    assert (r['status'][failed] == KT.STEADY).all(), r['status']
    warm = KR.solve_fp64(c.tables, c.phiM, c.csurf, c.phi_surface, theta_guess=r['theta'][:, 0], sens=False, **c.kw)
    print(name, 'plain', plain['status'].tolist(), 'steps', r['steps'].tolist(), 'warm iterations', warm['iterations'].tolist())
    assert (warm['status'][failed] == 0).all()
    # where the plain iteration does converge, the rescue's route ends at the same state
    both = ~failed
    if both.any():
        ok = np.exp(plain['y'][both]) > 1e-200
        assert np.abs(warm['y'][both] - plain['y'][both])[ok].max() <= 1e-12


def test_statuses_nan_rows_and_t_reached():
    c = C.case('random_S3')
    t = KR._arrays(c.tables)
    args = (t, c.phiM[0], c.csurf[0], c.phi_surface[0])
    ref = C.reference('random_S3')
    # a step budget that ends between two output times: CATKT_STEPS, the rows behind it NaN, t_reached where it got to
    r = KT.solve_point(*args, c.t_out, max_steps=150, **c.kw, **c.opts)
    assert r['status'] == KT.STEPS and r['steps'][0] + r['steps'][1] == 150
    reached = np.isfinite(r['drift'])
    assert 0 < reached.sum() < len(c.t_out) and not reached[reached.argmin():].any()
    k = reached.sum()
    assert np.array_equal(r['theta'][:k], ref['theta'][0, :k]) and np.isnan(r['theta'][k:]).all() and np.isnan(r['flux'][k:]).all()
    assert c.t_out[k - 1] <= r['t_reached'] < c.t_out[k]
    # bad inputs: CATKT_INPUT, everything NaN
    for bad in (dict(phiM=np.nan), dict(theta0=np.array([0.0, 0.5, 0.6, 0.2])), dict(theta0=np.array([0.1, np.nan, 0.1, 0.1]))):
        kw = dict(c.kw, **c.opts)
        phiM = bad.pop('phiM', c.phiM[0])
        r = KT.solve_point(t, phiM, c.csurf[0], c.phi_surface[0], c.t_out, **kw, **bad)
        assert r['status'] == KT.INPUT and np.isnan(r['theta']).all() and np.isnan(r['t_reached']) and not r['steps'].any()
    # the free-site entry of theta0 is ignored
    a = KT.solve_point(*args, c.t_out[:1], theta0=np.array([0.7, 0.1, 0.1, 0.1]), **c.kw, **c.opts)
    b = KT.solve_point(*args, c.t_out[:1], theta0=np.array([np.nan, 0.1, 0.1, 0.1]), **c.kw, **c.opts)
    assert a['status'] == KT.DONE and np.array_equal(a['theta'], b['theta'])
    # CATKT_DONE: t_reached is the last output time, exactly
    assert ref['status'][0] == KT.DONE and ref['t_reached'][0] == c.t_out[-1]
    # CATKT_STEADY: the remaining rows hold the state the lane stopped at
    s = KT.solve_point(*args, list(c.t_out) + [1e3, 1e6], steady_tol=1e-7, **c.kw, **c.opts)
    assert s['status'] == KT.STEADY and s['t_reached'] < 1e3
    first = int(np.searchsorted(np.array(list(c.t_out) + [1e3, 1e6]), s['t_reached'], side='left'))
    assert first < len(s['theta']) - 1 and (s['theta'][first:] == s['theta'][-1]).all() and (s['drift'][first:] < 1e-7).all()


def test_shortened_steps_land_on_the_output_times_exactly():
    """t_out that no step size sequence would hit: every row is written, the state at a time does not depend on the times behind it,
    and a single output time works"""
    c = C.case('ring')
    t = KR._arrays(c.tables)
    args = (t, c.phiM[0], c.csurf[0], c.phi_surface[0])
    times = [0.0123, 0.0124, 0.7, 0.7000001, 2.9]
    r = KT.solve_point(*args, times, theta0=c.theta0[0], **c.kw, **c.opts)
    assert r['status'] == KT.DONE and r['t_reached'] == times[-1] and np.isfinite(r['theta']).all()
    one = KT.solve_point(*args, times[:1], theta0=c.theta0[0], **c.kw, **c.opts)
    assert one['status'] == KT.DONE and one['theta'].shape == (1, 4) and np.array_equal(one['theta'][0], r['theta'][0])
    exact = C.ring_exact(c._replace(t_out=tuple(times)))
    assert np.abs(r['theta'][:, 1:] - exact[0]).max() <= K_GLOBAL * c.opts['rtol']


@pytest.mark.parametrize('name', GPU_CASES)
def test_no_decision_of_a_device_case_sits_on_its_threshold(name):
    """The guard of the device comparison: no accept / reject decision with |err - 1| < 1e-6 and no Newton exit with
    |max|dy| / newton_tol - 1| < 1e-6 (a case that violates it is replaced by another potential or seed, never skipped); and moving
    the rate constants by +-4 ulp changes no step count"""
    r = C.reference(name)
    assert r['err_margin'].min() >= 1e-6 and r['newton_margin'].min() >= 1e-6, (r['err_margin'].min(), r['newton_margin'].min())
    worst = 0.0
    for ulp in (4, -4):
        s = C.shifted(name, ulp)
        assert np.array_equal(s['steps'], r['steps']) and np.array_equal(s['status'], r['status'])
        ok = np.isfinite(r['theta']) & (r['theta'] > 1e-200)
        d = np.abs(np.log(s['theta'][ok]) - np.log(r['theta'][ok])).max()
        worst = max(worst, d)
        with np.errstate(invalid='ignore', divide='ignore'):
            df = np.abs(s['flux'] - r['flux']) / r['flux_scale']
        assert d <= LN_THETA_TOL / 10 * 1.01 and (df[np.isfinite(df)] <= FLUX_TOL / 10 * 1.01).all()
    print(name, 'ln theta moves by %.2e under +-4 ulp' % worst)
