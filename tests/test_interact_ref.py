"""tests/interact_ref.py pinned to known answers on the CPU, before anything on the device is compared with it: without interactions
on one site type it is tests/kinetics_ref.py number for number; its analytic Jacobian and sensitivities agree with central differences;
a single adsorbate with a self-interaction reproduces the Frumkin isotherm; two site types without cross terms are two independent
Langmuir isotherms."""
import numpy as np
import pytest

from tests import interact_cases as IC
from tests import interact_ref as IR
from tests import kinetics_cases as KC
from tests import kinetics_ref as KR


def with_zero_interactions(tab):
    T = len(tab['site_count'])
    return dict(tab, site_of=np.zeros(T, np.int32), site_fraction=np.ones(1), eps=np.zeros((T - 1, T - 1)))


@pytest.mark.parametrize('name', ['co2r_one_site', 'co2r_two_site', 'random_S4', 'random_S8'])
def test_without_interactions_on_one_site_type_it_is_the_mean_field_reference(name):
    c = KC.case(name)
    want = KR.solve_fp64(c.tables, c.phiM, c.csurf, c.phi_surface, **c.kw)
    got = IR.solve_fp64(with_zero_interactions(c.tables), c.phiM, c.csurf, c.phi_surface, **c.kw)
    # the same iteration in another order of summation (kinetics_ref sums the steps by matrix products): equal counts, and values within
    # what two fp64 evaluations of one iteration stopped at max|dy| < 1e-12 can differ by
    assert np.array_equal(want['status'], got['status']) and np.array_equal(want['iterations'], got['iterations']) and (got['status'] == 0).all()
    assert np.abs(want['y'] - got['y']).max() <= 1e-12
    assert (np.abs(want['rate'] - got['rate']) <= 1e-12 * want['rate_gross']).all() and (np.abs(want['flux'] - got['flux']) <= 1e-12 * want['flux_scale']).all()
    N = want['flux'].shape[1]
    assert (np.abs(want['dflux_dc'] - got['dflux_dc']) <= 1e-10 * want['dflux_scale'][:, :, :N]).all()
    assert (np.abs(want['dflux_dphi'] - got['dflux_dphi']) <= 1e-10 * want['dflux_scale'][:, :, N:]).all()
    assert (got['energy_shift'] == 0.0).all() and (got['ramp_reached'] == 0).all()
    # every further stage of a ramp finds the state it starts from: one iteration each
    more = IR.solve_fp64(with_zero_interactions(c.tables), c.phiM, c.csurf, c.phi_surface, ramp=3, sens=False, **c.kw)
    assert np.array_equal(more['iterations'], want['iterations'] + 2) and (more['ramp_reached'] == 2).all() and (more['status'] == 0).all()
    assert np.abs(more['y'] - want['y']).max() <= 1e-12


def point_args(c, i):
    t = IR._arrays(c.tables)
    V, sg = KR.potential_and_charge(c.phiM[i], c.phi_surface[i], c.kw['w'], c.kw['CS'], c.kw['phi_pzc'], None)
    a = np.maximum(c.csurf[i], 0.0) / t['cref']
    return t, a, V, sg, np.zeros((t['R'], 2))


@pytest.mark.parametrize('name', ['co2r_two_site_strong', 'terrace_step', 'random_S8_G1_piecewise', 'random_S5_G2_piecewise', 'random_S3_G3_linear'])
def test_the_analytic_jacobian_agrees_with_central_differences(name):
    """The rows of F at fixed row scales D and a fixed branch of Ga, away from the solution (a point of the iteration's path) and at it.
    Central differences with h = 1e-6 in y: truncation h^2 |F'''| / 6 ~ 1e-12 of the row's entries of order 1, rounding 1e-16 / h =
    1e-10 relative to the row's terms, which are scaled to <= 1: 1e-8 absolute leaves two orders of margin."""
    c = IC.case(name)
    fp = IC.fp64(name)
    rng = np.random.RandomState(3)
    for i in (0, len(c.phiM) - 1):
        t, a, V, sg, off = point_args(c, i)
        for y0 in (fp['y'][i] + rng.uniform(-0.3, 0.3, t['T']), fp['y'][i].copy()):
            y0 = np.maximum(y0, -30.0)          # (far below, a difference in y resolves nothing of exp(y))
            J, F, D = IR.system(t, y0.copy(), a, V, sg, off, 1.0)[:3]
            if (D[t['G']:] == 0.0).any():
                continue
            num = np.zeros_like(J)
            for k in range(t['T']):
                Fs = []
                for sign in (1.0, -1.0):
                    y = y0.copy()
                    y[k] += sign * 1e-6
                    Jk, Fk, Dk = IR.system(t, y, a, V, sg, off, 1.0)[:3]
                    Fk[t['G']:] *= Dk[t['G']:] / D[t['G']:]          # back to the row scales of the centre
                    Fs.append(Fk)
                num[:, k] = (Fs[0] - Fs[1]) / 2e-6
            assert np.abs(J - num).max() <= 1e-8, (name, i, np.abs(J - num).max())


@pytest.mark.parametrize('name', ['co2r_one_site_strong', 'random_S2_G2_linear', 'random_S5_G2_piecewise'])
def test_the_sensitivities_agree_with_central_differences_of_solves(name):
    """d flux / d phiM and d flux / d phi_0 against differences of converged solves, h = 1e-5 V: truncation h^2 f''' / 6 with f''' ~
    (40 / V)^3 f gives 1e-6 f, rounding 1e-13 flux_scale / h of the solve's own accuracy: 1e-5 of the sum of the terms (dflux_terms)."""
    c = IC.case(name)
    fp = IC.fp64(name)
    h = 1e-5
    N = fp['flux'].shape[1]
    for q, (dm, d0) in enumerate(((h, 0.0), (0.0, h))):
        up = IR.solve_fp64(c.tables, c.phiM + dm, c.csurf, c.phi_surface + d0, theta_guess=fp['theta'], sens=False, **c.kw)
        dn = IR.solve_fp64(c.tables, c.phiM - dm, c.csurf, c.phi_surface - d0, theta_guess=fp['theta'], sens=False, **c.kw)
        assert (up['status'] == 0).all() and (dn['status'] == 0).all()
        num = (up['flux'] - dn['flux']) / (2 * h)
        scale = fp['dflux_terms'][:, :, N + q] + 1e-13 * fp['flux_scale'] / h
        assert (np.abs(num - fp['dflux_dphi'][:, :, q]) <= 1e-5 * scale + 1e-300).all(), (name, q)


def one_adsorbate(eps_kT, K_log, G=1, x=(1.0,)):
    """A_g + * <-> A* on each of G types, no transition state: theta / (x - theta) = K a exp(-eps theta) per type"""
    N, S = 1, G
    T = G + S
    of, ob = np.zeros((G, N + T), np.int32), np.zeros((G, N + T), np.int32)
    for g in range(G):
        of[g, 0] = of[g, N + g] = 1
        ob[g, N + G + g] = 1
    return {'order_f': of, 'order_b': ob, 'nu': -np.ones((G, 1)), 'cref': np.ones(1), 'site_count': np.ones(T),
            'dG': np.array([[-k, 0.0, 0.0, 0.0] for k in K_log]), 'Ea': np.array([[-np.inf, 0.0, 0.0, 0.0]] * G), 'lnA': np.full(G, 29.0),
            'site_density': 1e-5, 'site_of': np.concatenate([np.arange(G), np.arange(G)]).astype(np.int32), 'site_fraction': np.array(x),
            'eps': np.diag(np.atleast_1d(eps_kT).astype(float)), 'eps_ts': np.zeros((G, S)), 'response': 'linear', 'strength': 1.0}


def bisect(fun, lo, hi):
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if fun(mid) > 0 else (lo, mid)
    return 0.5 * (lo + hi)


@pytest.mark.parametrize('eps', [0.0, 4.0, 12.0, -1.5])
def test_a_single_adsorbate_with_self_interaction_is_the_frumkin_isotherm(eps):
    acts = np.array([1e-3, 0.1, 1.0, 30.0])
    tab = one_adsorbate([eps], [2.0])
    got = IR.solve_fp64(tab, np.zeros(4), acts[:, None], np.zeros(4), sigma=np.zeros(4), ramp=4, sens=False)
    assert (got['status'] == 0).all()
    for a, th, shift in zip(acts, got['theta'][:, 1], got['energy_shift'][:, 0]):
        want = bisect(lambda v: np.exp(2.0) * a * np.exp(-eps * v) * (1.0 - v) - v, 0.0, 1.0)
        assert abs(th - want) <= 1e-12 and abs(shift - eps * want) <= 1e-11, (eps, a, th, want)


def test_two_site_types_without_cross_terms_are_two_langmuir_isotherms():
    x = (0.8, 0.2)
    tab = one_adsorbate([0.0, 0.0], [1.0, 4.0], G=2, x=x)
    acts = np.array([1e-3, 0.1, 1.0, 30.0])
    got = IR.solve_fp64(tab, np.zeros(4), acts[:, None], np.zeros(4), sigma=np.zeros(4), sens=False)
    assert (got['status'] == 0).all()
    for g, k in enumerate((1.0, 4.0)):
        Ka = np.exp(k) * acts
        assert np.allclose(got['theta'][:, 2 + g], x[g] * Ka / (1.0 + Ka), rtol=1e-12, atol=0)
        assert np.allclose(got['theta'][:, g], x[g] / (1.0 + Ka), rtol=1e-12, atol=0)
    # with a self-interaction on the step sites alone the terrace keeps its Langmuir isotherm and the steps follow Frumkin's
    tab = one_adsorbate([0.0, 5.0], [1.0, 4.0], G=2, x=x)
    got = IR.solve_fp64(tab, np.zeros(4), acts[:, None], np.zeros(4), sigma=np.zeros(4), ramp=3, sens=False)
    assert (got['status'] == 0).all()
    assert np.allclose(got['theta'][:, 2], x[0] * np.exp(1.0) * acts / (1.0 + np.exp(1.0) * acts), rtol=1e-12, atol=0)
    for a, th in zip(acts, got['theta'][:, 3]):
        want = bisect(lambda v: np.exp(4.0) * a * np.exp(-5.0 * v) * (x[1] - v) - v, 0.0, x[1])
        assert abs(th - want) <= 1e-12
