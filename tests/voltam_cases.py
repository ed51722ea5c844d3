"""The cases of tests/test_voltam_ref.py and tests/test_gpu_voltam.py (test infrastructure, no tests of its own).  Every case is two
or three operating points with the arguments of one catvm_solve, the points at different scan rates so that the lanes of a wave take
different numbers of steps; reference(name) integrates it once per session with the NumPy restatement (tests/voltam_ref.py) and every
test shares the result and leaves it unchanged.

  langmuir_rev, langmuir_quasi   A + * + e- <-> A* without a transition state: kf = k0 min(1, exp(-(E - E0) / kT)), kb = kf exp((E - E0) / kT);
                                 k0 = 1e4 /s (reversible at these scan rates) and 10 /s
  langmuir_slow                  the same step behind a transition state, beta = 0.5, with a barrier high enough that the Ea branch holds
                                 over the whole sweep (Butler-Volmer): k0 = 0.1 /s
  two_peak                       * + e- <-> X1, X1 + e- <-> X2 with formal potentials 0.15 V apart, N = 0: two peaks per branch
  co2r_two_site                  the four-step CO2 reduction mechanism of tests/kinetics_cases.py between -0.6 and -1.0 V
  random_S8                      random_network(8, KC.SEEDS[8]): S = 8, N = 8; an electron on every step whose dG depends on the potential
  n0                             * + e- <-> X, S = 1 and no species at all

The sweeps start positive of the formal potentials, where the steady state is the empty surface, and go negative first.  They turn
before the free site falls below 1e-5: the site row resolves ln theta_0 to 1e-16 / theta_0, and a Newton iteration whose tolerance is
below that cannot converge (the limit of include/catint_kintrans.h's implicit Euler solve, which this library shares)."""
import functools
from collections import namedtuple

import numpy as np

from catint_amd.units import unit_e, unit_kB
from tests import kinetics_cases as KC
from tests import kinetics_ref as KR
from tests import voltam_ref as VR

Case = namedtuple('Case', 'name tables electrons E_start E_vertex scan_rate csurf phi_surface kw theta0 opts')

KT_EV = unit_kB * 298.15 / unit_e          # kT / e in V
RATE_FLOOR = 1.0 / (4.0 * KT_EV)           # catint_amd.voltammetry's default: the peak turnover per V/s of a reversible one-electron monolayer
RTOL = 1e-3
ATOL = 1e-8                                # coverages below atol / rtol = 1e-5 are not resolved relatively: their exponential tails would set the step
FLAT = dict(w=0, CS=0.0, phi_pzc=0.0)
E0 = 0.1                                   # formal potential of the single-step cases, V
LANGMUIR_K0 = {'langmuir_rev': 1e4, 'langmuir_quasi': 10.0, 'langmuir_slow': 0.1}
SLOW_LNA = np.log(1e5)                     # prefactor of langmuir_slow: the barrier at E0 is ln(1e5 / 0.1) = 13.8 kT
TWO_PEAK = dict(E1=0.175, E2=0.025, k0=100.0)


def _tables(of, ob, nu, ns, dG, lnA, Ea=None):
    of, ob = np.asarray(of, np.int32), np.asarray(ob, np.int32)
    R, N = of.shape[0], of.shape[1] - len(ns)
    return {'order_f': of, 'order_b': ob, 'nu': np.asarray(nu, float).reshape(R, N), 'cref': np.ones(N), 'site_count': np.asarray(ns, float),
            'dG': np.asarray(dG, float).reshape(R, 4), 'Ea': np.tile([-np.inf, 0.0, 0.0, 0.0], (R, 1)) if Ea is None else np.asarray(Ea, float),
            'lnA': np.asarray(lnA, float), 'site_density': 1e-5}


def _opts(n_segments, samples, **kw):
    return dict(dict(n_segments=n_segments, samples=samples, rate_floor=RATE_FLOOR, rtol=RTOL, atol=ATOL), **kw)


def langmuir_case(name, rates, n_segments, samples, rtol=RTOL):
    """columns: A | *, A*.  dG = (E - E0) / kT for one electron on the reactant side"""
    k0 = LANGMUIR_K0[name]
    dG = [[-E0 / KT_EV, 1.0 / KT_EV, 0.0, 0.0]]
    if name == 'langmuir_slow':
        barrier = SLOW_LNA - np.log(k0)
        tab = _tables([[1, 1, 0]], [[0, 0, 1]], [[-1.0]], [1.0, 1.0], dG, [SLOW_LNA], Ea=[[barrier - 0.5 * E0 / KT_EV, 0.5 / KT_EV, 0.0, 0.0]])
    else:
        tab = _tables([[1, 1, 0]], [[0, 0, 1]], [[-1.0]], [1.0, 1.0], dG, [np.log(k0)])
    n = len(rates)
    return Case(name, tab, np.array([1.0]), np.full(n, E0 + 0.31), np.full(n, E0 - 0.29), np.array(rates, float), np.ones((n, 1)), np.zeros(n),
                dict(FLAT), None, _opts(n_segments, samples, rtol=rtol))


def two_peak_case(rates=(0.05, 1.0), n_segments=3, samples=8, rtol=RTOL):
    """columns: *, X1, X2 (N = 0)"""
    P = TWO_PEAK
    tab = _tables([[1, 0, 0], [0, 1, 0]], [[0, 1, 0], [0, 0, 1]], np.zeros((2, 0)), [1.0, 1.0, 1.0],
                  [[-P['E1'] / KT_EV, 1.0 / KT_EV, 0.0, 0.0], [-P['E2'] / KT_EV, 1.0 / KT_EV, 0.0, 0.0]], [np.log(P['k0'])] * 2)
    n = len(rates)
    return Case('two_peak', tab, np.array([1.0, 1.0]), np.full(n, 0.41), np.full(n, -0.04), np.array(rates, float), np.zeros((n, 0)), np.zeros(n),
                dict(FLAT), None, _opts(n_segments, samples, rtol=rtol))


def n0_case():
    tab = _tables([[1, 0]], [[0, 1]], np.zeros((1, 0)), [1.0, 1.0], [[-E0 / KT_EV, 1.0 / KT_EV, 0.0, 0.0]], [np.log(50.0)])
    return Case('n0', tab, np.array([1.0]), np.array([0.41, 0.35, 0.41]), np.array([-0.2, -0.1, -0.2]), np.array([0.1, 2.0, 20.0]), np.zeros((3, 0)),
                np.zeros(3), dict(FLAT), None, _opts(2, 8))


CO2R_RATES = (0.02, 0.5, 10.0)


def co2r_case(rates=CO2R_RATES, E_start=-0.6, E_vertex=-1.0, n_segments=2, samples=8):
    """30 mol/m^3 CO2 at the surface, the surface potential constant at -0.08 V"""
    model = KC.co2r_model('two_site')
    n = len(rates)
    csurf = np.tile([30.0, 1e-3, 0.1], (n, 1))
    return Case('co2r_two_site', model.tables(), np.array([float(s['electrons']) for s in model.steps]), np.full(n, float(E_start)),
                np.full(n, float(E_vertex)), np.array(rates, float), csurf, np.full(n, -0.08), dict(KC.STERN), None, _opts(n_segments, samples))


def random_case():
    c = KC.random_network(8, KC.SEEDS[8])
    ne = (c.tables['dG'][:, 1] != 0.0).astype(float)
    return Case('random_S8', c.tables, ne, np.array([-0.2, -0.2]), np.array([-0.5, -0.5]), np.array([0.1, 5.0]), c.csurf[[0, 3]],
                np.array([-0.04, -0.04]), dict(c.kw), None, _opts(1, 8))


BUILDERS = {'langmuir_rev': lambda: langmuir_case('langmuir_rev', (0.05, 0.5, 5.0), 2, 12),
            'langmuir_quasi': lambda: langmuir_case('langmuir_quasi', (0.05, 1.0), 2, 8),
            'langmuir_slow': lambda: langmuir_case('langmuir_slow', (0.01, 0.04, 0.2), 1, 12),
            'two_peak': two_peak_case, 'co2r_two_site': co2r_case, 'random_S8': random_case, 'n0': n0_case}
CASE_NAMES = list(BUILDERS)
IDENTITY_W = {'langmuir_rev': (0.0, 1.0), 'langmuir_quasi': (0.0, 1.0), 'langmuir_slow': (0.0, 1.0), 'two_peak': (0.0, 1.0, 2.0)}


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def run(c, points=None, **over):
    """the restatement on a case (points: a subset), with `over` in the place of its options"""
    opts = dict(c.opts)
    opts.update(over)
    idx = np.arange(len(c.E_start)) if points is None else np.asarray(points)
    return VR.solve(c.tables, c.electrons, c.E_start[idx], c.E_vertex[idx], c.scan_rate[idx], c.csurf[idx], c.phi_surface[idx],
                    theta0=None if c.theta0 is None else c.theta0[idx], **c.kw, **opts)


@functools.lru_cache(maxsize=None)
def reference(name):
    return run(case(name))


@functools.lru_cache(maxsize=None)
def shifted(name, ulp):
    """the restatement with every ln kf and ln kb moved by `ulp` ulp: what a few ulp in exp and log do to the result"""
    return run(case(name), lnk_shift=ulp)


def tau(c):
    return np.abs(c.E_vertex - c.E_start) / c.scan_rate
