"""The cases of tests/test_iasweep_ref.py and tests/test_gpu_iasweep.py (test infrastructure, no tests of its own).  Every case is two
or three operating points with the arguments of one catis_solve, the points at different scan rates (hold times) so that the lanes of a
wave take different numbers of steps; reference(name) integrates it once per session with the NumPy restatement (tests/iasweep_ref.py)
and every test shares the result and leaves it unchanged.

  frumkin_rep, frumkin_att   the step of voltam_cases' langmuir_rev (A + * + e- <-> A*, k0 = 1e4 /s) with a self-interaction of +2 and
                             -2 kT: the Frumkin isotherm, peak v / ((4 + eps) kT)
  frumkin_quasi              the same with k0 = 10 /s and +2 kT
  co2r_weak                  interact_cases' one-site CO2 reduction model with the weak interaction between -0.6 and -1.0 V
  terrace_step               interact_cases' two site types, started with theta0 = the steady state at full strength (its ramped start
                             does not converge at strength 0)
  random_S7_G2_piecewise     interact_cases.random_network(7, 2, 'piecewise') with three inert species added: T = 9, N = 8, the largest
                             shape, with the piecewise response
  hold_relax                 frumkin_quasi's model held at its formal potential from theta0 = (0.9, 0.1), for 0.5 s and 5 s per segment

As in voltam_cases the sweeps turn before a free site falls below 1e-5; with attraction that is 70 mV earlier."""
import functools
from collections import namedtuple

import numpy as np

from tests import iasweep_ref as SR
from tests import interact_cases as IC
from tests import interact_ref as IR
from tests import kinetics_cases as KC
from tests import voltam_cases as VC

Case = namedtuple('Case', 'name tables electrons E_start E_vertex scan_rate csurf phi_surface kw theta0 hold_time opts')

KT_EV, RATE_FLOOR, RTOL, ATOL, E0 = VC.KT_EV, VC.RATE_FLOOR, VC.RTOL, VC.ATOL, VC.E0
FRUMKIN_EPS = {'frumkin_rep': 2.0, 'frumkin_att': -2.0, 'frumkin_quasi': 2.0}
FRUMKIN_VERTEX = {'frumkin_rep': E0 - 0.29, 'frumkin_att': E0 - 0.22, 'frumkin_quasi': E0 - 0.29}
RANDOM_SEED = 107


def _opts(n_segments, samples, start_ramp, **kw):
    return dict(dict(n_segments=n_segments, samples=samples, rate_floor=RATE_FLOOR, rtol=RTOL, atol=ATOL, start_ramp=start_ramp), **kw)


def frumkin_tables(eps, k0_case='langmuir_rev'):
    """columns: A | *, A*.  dG = (E - E0) / kT + eps theta"""
    tab = dict(VC.langmuir_case(k0_case, (1.0,), 1, 1).tables)
    tab.update(site_of=np.zeros(2, np.int32), site_fraction=np.ones(1), eps=np.array([[float(eps)]]), eps_ts=None, response='linear', strength=1.0)
    return tab


def frumkin_case(name, rates, n_segments=2, samples=12, rtol=RTOL):
    n = len(rates)
    tab = frumkin_tables(FRUMKIN_EPS[name], 'langmuir_quasi' if name == 'frumkin_quasi' else 'langmuir_rev')
    return Case(name, tab, np.array([1.0]), np.full(n, E0 + 0.31), np.full(n, FRUMKIN_VERTEX[name]), np.array(rates, float), np.ones((n, 1)),
                np.zeros(n), dict(VC.FLAT), None, None, _opts(n_segments, samples, 3, rtol=rtol))


def co2r_case(rates=(0.5, 1e6, 1e7)):
    """Below some 1e5 V/s this model follows its steady state and every step is as long as the outputs allow, whatever rtol is; the
    two fast points are where the step control works (56 and 228 accepted steps at rtol 1e-3 and 1e-4)"""
    model = IC.co2r_model('one_site', 0.3, 0.15)
    n = len(rates)
    return Case('co2r_weak', model.tables(), model.electrons(), np.full(n, -0.6), np.full(n, -1.0), np.array(rates, float),
                np.tile([30.0, 1e-3, 0.1], (n, 1)), np.full(n, -0.08), dict(KC.STERN), None, None, _opts(2, 8, 5))


def terrace_step_case(rates=(0.1, 5.0)):
    model = IC.terrace_step_model()
    tab = model.tables()
    n = len(rates)
    es, csurf, phis = np.full(n, -0.6), np.tile([30.0, 1e-3, 0.1], (n, 1)), np.full(n, -0.08)
    start = IR.solve_fp64(tab, es, csurf, phis, ramp=1, sens=False, **KC.STERN)
    assert (start['status'] == 0).all(), start['status']
    return Case('terrace_step', tab, model.electrons(), es, np.full(n, -0.9), np.array(rates, float), csurf, phis, dict(KC.STERN),
                start['theta'].copy(), None, _opts(2, 8, 1))


def unconverged_start():
    """(E_start, csurf [N], phi_surface) of the last point of interact_cases.terrace_step_case: without the repulsion CO saturates the
    step sites there and the first stage of a ramped start from the uniform surface does not converge"""
    c = IC.terrace_step_case()
    return float(c.phiM[-1]), c.csurf[-1].copy(), float(c.phi_surface[-1])


def random_case():
    """S = 7 on G = 2 types, piecewise, padded with inert species to N = 8"""
    c = IC.random_network(7, 2, 'piecewise', RANDOM_SEED)
    tab = dict(c.tables)
    of, ob = np.asarray(tab['order_f']), np.asarray(tab['order_b'])
    R, N, pad = of.shape[0], of.shape[1] - 9, 8 - (of.shape[1] - 9)
    z = np.zeros((R, pad), of.dtype)
    tab['order_f'], tab['order_b'] = np.hstack([of[:, :N], z, of[:, N:]]), np.hstack([ob[:, :N], z, ob[:, N:]])
    tab['nu'], tab['cref'] = np.hstack([tab['nu'], np.zeros((R, pad))]), np.full(8, 1000.0)
    ne = (tab['dG'][:, 1] != 0.0).astype(float)
    csurf = np.hstack([c.csurf[[0, 3]], np.ones((2, pad))])
    return Case('random_S7_G2_piecewise', tab, ne, np.array([-0.2, -0.2]), np.array([-0.5, -0.5]), np.array([0.1, 5.0]), csurf,
                np.array([-0.04, -0.04]), dict(c.kw), None, None, _opts(1, 8, 4))


def hold_case(holds=(0.5, 5.0)):
    n = len(holds)
    tab = frumkin_tables(2.0, 'langmuir_quasi')
    return Case('hold_relax', tab, np.array([1.0]), np.full(n, E0), np.full(n, E0), np.ones(n), np.ones((n, 1)), np.zeros(n), dict(VC.FLAT),
                np.tile([0.9, 0.1], (n, 1)), np.array(holds, float), _opts(1, 8, 1))


BUILDERS = {'frumkin_rep': lambda: frumkin_case('frumkin_rep', (0.05, 0.4, 4.0)), 'frumkin_att': lambda: frumkin_case('frumkin_att', (0.05, 1.0)),
            'frumkin_quasi': lambda: frumkin_case('frumkin_quasi', (0.05, 1.0), samples=8), 'co2r_weak': co2r_case,
            'terrace_step': terrace_step_case, 'random_S7_G2_piecewise': random_case, 'hold_relax': hold_case}
CASE_NAMES = list(BUILDERS)
IDENTITY_W = {'frumkin_rep': (0.0, 1.0), 'frumkin_att': (0.0, 1.0), 'frumkin_quasi': (0.0, 1.0)}


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def run(c, points=None, **over):
    """the restatement on a case (points: a subset), with `over` in the place of its options"""
    opts = dict(c.opts)
    opts.update(over)
    idx = np.arange(len(c.E_start)) if points is None else np.asarray(points)
    hold = opts.pop('hold_time', None if c.hold_time is None else c.hold_time[idx])
    return SR.solve(c.tables, c.electrons, c.E_start[idx], c.E_vertex[idx], c.scan_rate[idx], c.csurf[idx], c.phi_surface[idx],
                    theta0=None if c.theta0 is None else c.theta0[idx], hold_time=hold, **c.kw, **opts)


@functools.lru_cache(maxsize=None)
def reference(name):
    return run(case(name))


@functools.lru_cache(maxsize=None)
def shifted(name, ulp):
    """the restatement with every ln kf and ln kb of the step loop moved by `ulp` ulp: what a few ulp in exp and log do to the result"""
    return run(case(name), lnk_shift=ulp)


def tau(c):
    t = np.abs(c.E_vertex - c.E_start) / c.scan_rate
    return t if c.hold_time is None else np.where(c.E_vertex == c.E_start, c.hold_time, t)
