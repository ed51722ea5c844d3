"""The cases of tests/test_kintrans_ref.py and tests/test_gpu_kintrans.py (test infrastructure, no tests of its own).  Every case is a
few operating points with the arguments of one catkt_solve; reference(name) integrates it once per session with the NumPy
restatement (tests/kintrans_ref.py) and every test shares the result and leaves it unchanged.

  co2r_one_site, co2r_two_site   the four-step CO2 reduction mechanism of tests/kinetics_cases.py at 30 mol/m^3 CO2 and three
                                 potentials, started from the steady state of the neighbouring potential: the potential step
  random_S1, random_S3, random_S8  random_network(S, KC.SEEDS[S]), point 0, from the uniform start
  rescue_S3, rescue_S5, rescue_S8  random_network(3, 105), (5, 101), (8, 107): networks on which the damped Newton iteration of the
                                 steady state stops at maxit from the uniform start; all four points, integrated with the settings
                                 of get_kinetics(rescue=True)
  langmuir                       A + * <-> A*: theta(t) = theta_inf + (theta_0 - theta_inf) exp(-(kf a + kb) t)
  ring                           X1 <-> X2 <-> X3 <-> X1, first order, no free site taking part: theta(t) = expm(K t) theta_0
"""
import functools
from collections import namedtuple

import numpy as np

from tests import kinetics_cases as KC
from tests import kinetics_ref as KR
from tests import kintrans_ref as KT

Case = namedtuple('Case', 'name tables phiM csurf phi_surface kw theta0 t_out opts')

RTOL = 1e-3
CO2R_POINTS = (2, 5, 8)              # indices into KC.POTENTIALS: -0.6, -0.9, -1.2 V, each started from the next more negative one
CO2R_T_OUT = (1e-9, 1e-6, 1e-3, 1.0)
RANDOM_T_OUT = (1e-13, 1e-12, 1e-10, 1e-6)
RESCUE = {3: 105, 5: 101, 8: 107}
RESCUE_OPTS = dict(rtol=1e-2, steady_tol=1e-6)      # catint_amd._kintrans.RESCUE_RTOL, RESCUE_STEADY_TOL
RESCUE_T_OUT = (1e12,)


def _tables(of, ob, nu, ns, dG, lnA):
    of, ob = np.asarray(of, np.int32), np.asarray(ob, np.int32)
    R, N = of.shape[0], of.shape[1] - len(ns)
    return {'order_f': of, 'order_b': ob, 'nu': np.asarray(nu, float).reshape(R, N), 'cref': np.ones(N), 'site_count': np.asarray(ns, float),
            'dG': np.asarray(dG, float).reshape(R, 4), 'Ea': np.tile([-np.inf, 0.0, 0.0, 0.0], (R, 1)), 'lnA': np.asarray(lnA, float),
            'site_density': 1e-5}


def co2r_case(variant):
    c = KC.co2r_case(variant)
    n_lv = len(KC.CO2_LEVELS)
    at = np.array([j * n_lv for j in CO2R_POINTS])            # the 30 mol/m^3 points
    before = at + n_lv                                         # the same at the next potential
    fp = KR.solve_fp64(c.tables, c.phiM[before], c.csurf[before], c.phi_surface[before], sens=False, **c.kw)
    assert (fp['status'] == 0).all()
    return Case('co2r_' + variant, c.tables, c.phiM[at], c.csurf[at], c.phi_surface[at], dict(c.kw), fp['theta'], CO2R_T_OUT, dict(rtol=RTOL))


def random_case(S):
    c = KC.random_network(S, KC.SEEDS[S])
    return Case('random_S%d' % S, c.tables, c.phiM[:1], c.csurf[:1], c.phi_surface[:1], dict(c.kw), None, RANDOM_T_OUT, dict(rtol=RTOL))


def rescue_case(S):
    c = KC.random_network(S, RESCUE[S])
    return Case('rescue_S%d' % S, c.tables, c.phiM, c.csurf, c.phi_surface, dict(c.kw), None, RESCUE_T_OUT, dict(RESCUE_OPTS))


LANGMUIR = dict(lnK=1.5, lnA=2.0, a=(0.3, 2.0), theta0=(0.9, 0.05))


def langmuir_case(rtol=RTOL):
    """A + * <-> A*; columns: A | *, A*.  kf = exp(lnA), kb = kf exp(-lnK); two points: desorption from 0.9, adsorption from 0.05"""
    L = LANGMUIR
    tab = _tables([[1, 1, 0]], [[0, 0, 1]], [[-1.0]], [1.0, 1.0], [[-L['lnK'], 0.0, 0.0, 0.0]], [L['lnA']])
    a = np.array(L['a'])
    th0 = np.array([[1.0 - v, v] for v in L['theta0']])
    rate = np.exp(L['lnA']) * a + np.exp(L['lnA'] - L['lnK'])
    t_out = tuple(np.array([0.1, 0.5, 1.0, 3.0, 8.0]) / rate.max())
    return Case('langmuir', tab, np.zeros(2), a[:, None], np.zeros(2), dict(w=0, CS=0.0, phi_pzc=0.0), th0, t_out, dict(rtol=rtol))


def langmuir_exact(case):
    L = LANGMUIR
    kf, kb = np.exp(L['lnA']), np.exp(L['lnA'] - L['lnK'])
    a = np.array(L['a'])[:, None]
    t = np.array(case.t_out)[None, :]
    inf = kf * a / (kf * a + kb)
    return inf + (np.array(L['theta0'])[:, None] - inf) * np.exp(-(kf * a + kb) * t)          # theta of A* [n][n_out]


RING = dict(dG=(-1.0, 0.7, 0.3), lnA=(0.0, 1.0, -0.5), theta0=(0.6, 0.2, 0.1))


def ring_case(rtol=RTOL):
    """X1 <-> X2 <-> X3 <-> X1; columns: *, X1, X2, X3 (N = 0).  The free site keeps its 0.1"""
    R = RING
    of = [[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    ob = [[0, 0, 1, 0], [0, 0, 0, 1], [0, 1, 0, 0]]
    tab = _tables(of, ob, np.zeros((3, 0)), [1.0, 1.0, 1.0, 1.0], [[g, 0.0, 0.0, 0.0] for g in R['dG']], R['lnA'])
    th0 = np.array([[1.0 - sum(R['theta0'])] + list(R['theta0'])])
    return Case('ring', tab, np.zeros(1), np.zeros((1, 0)), np.zeros(1), dict(w=0, CS=0.0, phi_pzc=0.0), th0, (0.05, 0.2, 0.5, 1.0, 3.0),
                dict(rtol=rtol))


def ring_exact(case):
    from scipy.linalg import expm
    R = RING
    dG, lnA = np.array(R['dG']), np.array(R['lnA'])
    kf = np.exp(lnA - np.maximum(dG, 0.0))
    kb = kf * np.exp(dG)
    K = np.zeros((3, 3))
    for r, (i, j) in enumerate(((0, 1), (1, 2), (2, 0))):          # step r: X_i <-> X_j
        K[i, i] -= kf[r]
        K[j, i] += kf[r]
        K[j, j] -= kb[r]
        K[i, j] += kb[r]
    return np.array([expm(K * t) @ np.array(R['theta0']) for t in case.t_out])[None]          # [1][n_out][3]


BUILDERS = {'co2r_one_site': lambda: co2r_case('one_site'), 'co2r_two_site': lambda: co2r_case('two_site'),
            'random_S1': lambda: random_case(1), 'random_S3': lambda: random_case(3), 'random_S8': lambda: random_case(8),
            'rescue_S3': lambda: rescue_case(3), 'rescue_S5': lambda: rescue_case(5), 'rescue_S8': lambda: rescue_case(8),
            'langmuir': langmuir_case, 'ring': ring_case}
CASE_NAMES = list(BUILDERS)
RESCUE_NAMES = ['rescue_S3', 'rescue_S5', 'rescue_S8']


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def run(c, **over):
    """the restatement on a case, with `over` in the place of its options"""
    opts = dict(c.opts)
    opts.update(over)
    return KT.solve(c.tables, c.phiM, c.csurf, c.phi_surface, c.t_out, theta0=c.theta0, **c.kw, **opts)


@functools.lru_cache(maxsize=None)
def reference(name):
    return run(case(name))


@functools.lru_cache(maxsize=None)
def shifted(name, ulp):
    """the restatement with every ln kf and ln kb moved by `ulp` ulp: what a few ulp in exp and log do to the result"""
    return run(case(name), lnk_shift=ulp)


@functools.lru_cache(maxsize=None)
def plain_newton(name):
    """KR.solve_fp64 on the case's points from the uniform start (no sensitivities)"""
    c = case(name)
    return KR.solve_fp64(c.tables, c.phiM, c.csurf, c.phi_surface, sens=False, **c.kw)
