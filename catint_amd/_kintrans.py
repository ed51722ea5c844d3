"""ctypes binding of ``include/catint_kintrans.h``: the transient of a mean-field surface microkinetic model per operating point --
implicit Euler with step doubling, every point with its own step size -- integrated on the device
(``catint_amd/lib/libcatint_kintrans.so``, built by ``catint_amd.build.build_kintrans_library()``), and the rescue of steady-state solves
that rests on it.  No fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _devlib, _microkin
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _dptr  # noqa: F401  (part of this module's interface)
from ._microkin import DROP, _PD, _PI, _PL, _f64, _iptr  # noqa: F401  (the same)

LIB_PATH = _devlib.lib_path('kintrans')

# every symbol include/catint_kintrans.h declares (tests/test_kintrans_abi.py)
SYMBOLS = _devlib.symbols('catkt_', 'solve')

DONE, STEADY, INPUT, STEPS = 0, 1, 2, 3
MAX_STEPS = 1000000
DEFAULT_RTOL, DEFAULT_ATOL, DEFAULT_NEWTON_TOL, DEFAULT_NEWTON_MAXIT, DEFAULT_MAX_STEPS = 1e-4, 1e-12, 1e-10, 8, 20000
# output rows: name -> shape of one operating point from (N, S, R, n_out)
FIELDS = {'theta': lambda N, S, R, K: (K, S + 1), 'flux': lambda N, S, R, K: (K, N), 'flux_scale': lambda N, S, R, K: (K, N),
          'drift': lambda N, S, R, K: (K,), 't_reached': lambda N, S, R, K: ()}
DEFAULT_FIELDS = ('theta', 'flux', 'flux_scale', 'drift', 't_reached')
# what get_kinetics(rescue=True) integrates the points its Newton iteration failed at with
RESCUE_T_OUT, RESCUE_RTOL, RESCUE_STEADY_TOL = 1e12, 1e-2, 1e-6


class KintransError(_devlib.LibraryError):
    library = 'catint_kintrans'


class CatktParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('nspecies', C.c_int32), ('nadsorbates', C.c_int32),
                ('nsteps', C.c_int32), ('newton_maxit', C.c_int32), ('potential_drop', C.c_int32), ('max_steps', C.c_int32),
                ('n', C.c_int64), ('lanes', _PL), ('order_f', _PI), ('order_b', _PI), ('nu', _PD), ('cref', _PD), ('site_count', _PD),
                ('dG', _PD), ('Ea', _PD), ('lnA', _PD), ('site_density', C.c_double), ('stern_capacitance', C.c_double),
                ('phi_pzc', C.c_double), ('phiM', _PD), ('sigma', _PD), ('off', _PD), ('gamma', _PD), ('theta0', _PD), ('csurf', _PD),
                ('phi_surface', _PD), ('t_out', _PD), ('n_out', C.c_int64), ('rtol', C.c_double), ('atol', C.c_double),
                ('newton_tol', C.c_double), ('steady_tol', C.c_double), ('h0', C.c_double)]


class CatktOutputs(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('theta', _PD), ('flux', _PD), ('flux_scale', _PD), ('drift', _PD),
                ('t_reached', _PD), ('status', _PI), ('steps', _PI)]


load_library = _devlib.loader(globals(), 'catkt_', 'solve', CatktParams, CatktOutputs, KintransError)


class TransientKinetics(_devlib.Handle):
    """One ``catkt_ctx``.  No device call is made before the first ``solve`` that passes validation with at least one point."""
    _prefix, _error, _load = 'catkt_', KintransError, staticmethod(load_library)

    def solve(self, view, tables, phiM, t_out, lanes=None, csurf=None, phi_surface=None, potential_drop='stern', stern_capacitance=0.0,
              phi_pzc=0.0, sigma=None, off=None, gamma=None, theta0=None, rtol=DEFAULT_RTOL, atol=DEFAULT_ATOL, steady_tol=0.0, h0=0.0,
              newton_tol=DEFAULT_NEWTON_TOL, newton_maxit=DEFAULT_NEWTON_MAXIT, max_steps=DEFAULT_MAX_STEPS, fields=None, max_waves=0,
              struct_size=None, out_struct_size=None, out=None):
        """catkt_solve.  view, tables, phiM, lanes, csurf, phi_surface, potential_drop, stern_capacitance, phi_pzc, sigma, off, gamma: those
        of KineticsSolver.solve; the surface state is constant over the integration.  t_out [n_out]: the output times in s, positive and
        increasing, the same for every point; theta0 [n][S+1]: the coverages at t = 0 (the free-site entry is recomputed from the site
        balance), None: the uniform start of the steady-state solve.  rtol, atol: on the coverages, per step; steady_tol > 0: a point
        whose scaled residual max |G_s| / D_s falls below it stops, status STEADY, and its remaining rows hold that state; h0 <= 0: the
        first step size is chosen.  fields: names out of FIELDS (None: DEFAULT_FIELDS).  Returns a dict of the requested arrays
        ('theta' [n][n_out][S+1], 'flux', 'flux_scale' [n][n_out][N], 'drift' [n][n_out], 't_reached' [n]) and 'status' [n] (DONE,
        STEADY, INPUT: NaN rows, STEPS: max_steps attempted steps were not enough, the rows not reached are NaN), 'steps' [n][3]
        (accepted, rejected, Newton iterations), both int32.  out: arrays to write into (tests)."""
        tt = None if t_out is None else _f64(np.atleast_1d(np.asarray(t_out, float))).reshape(-1)
        K = 0 if tt is None else len(tt)
        known = {name: (lambda N, S, R, f=f: f(N, S, R, K)) for name, f in FIELDS.items()}
        per_point = {'sigma': sigma, 'off': off, 'gamma': gamma, 'theta0': theta0, 'csurf': csurf, 'phi_surface': phi_surface}
        call = _microkin.Call(tables, phiM, lanes, per_point, fields, known, DEFAULT_FIELDS, potential_drop, stern_capacitance, phi_pzc, max_waves)
        p = CatktParams(struct_size=_devlib.size_of(CatktParams, struct_size), newton_maxit=int(newton_maxit),
                        max_steps=int(max_steps), t_out=_dptr(tt), n_out=K, rtol=float(rtol), atol=float(atol), newton_tol=float(newton_tol),
                        steady_tol=float(steady_tol), h0=float(h0), **call.members)
        res = call.results(known, out)
        res.setdefault('status', np.zeros(call.n, np.int32))
        res.setdefault('steps', np.zeros((call.n, 3), np.int32))
        o = CatktOutputs(struct_size=_devlib.size_of(CatktOutputs, out_struct_size),
                         status=_iptr(res['status']), steps=_iptr(res['steps']), **{name: _dptr(a) for name, a in res.items() if name in FIELDS})
        self._call('solve', view, p, o)
        return res


def rescue(kinetics, transient, view, tables, phiM, res, lanes=None, per_point=None, **solve_kw):
    """The points of `res` (what kinetics.solve(view, tables, phiM, lanes=lanes, **per_point, **solve_kw) returned from the uniform
    start) that ended MAXIT or PIVOT, once more: integrated from the uniform start to RESCUE_T_OUT with RESCUE_RTOL and
    RESCUE_STEADY_TOL, and those that end STEADY solved again by kinetics.solve with that state as theta_guess.  The rows of the points
    whose second solve converges replace the failed ones in `res` (in place), and res['rescued'] [n] (bool) marks them; a point whose
    second solve fails too keeps its first rows and status.  per_point: the arrays that have one row per point ('csurf',
    'phi_surface', 'sigma', 'off', 'gamma'; None entries allowed).  Returns res."""
    from . import _kinetics
    status = np.asarray(res['status'])
    n = len(status)
    res['rescued'] = np.zeros(n, bool)
    failed = np.flatnonzero((status == _kinetics.MAXIT) | (status == _kinetics.PIVOT))
    if not len(failed):
        return res
    per_point = {k: v for k, v in (per_point or {}).items() if v is not None}
    if view is not None and lanes is None:
        lanes = np.arange(n, dtype=np.int64)

    def rows(idx):
        sub = {}
        for k, v in per_point.items():
            a = np.asarray(v, float)
            sub[k] = (a if a.shape[:1] == (n,) else a.reshape(n, -1))[idx]
        if lanes is not None:
            sub['lanes'] = np.asarray(lanes, np.int64).reshape(-1)[idx]
        return sub
    pm = np.asarray(phiM, float).reshape(-1)
    common = {k: solve_kw[k] for k in ('potential_drop', 'stern_capacitance', 'phi_pzc', 'max_waves') if k in solve_kw}
    tr = transient.solve(view, tables, pm[failed], [RESCUE_T_OUT], rtol=RESCUE_RTOL, steady_tol=RESCUE_STEADY_TOL, fields=('theta',), **common,
                         **rows(failed))
    steady = np.flatnonzero(tr['status'] == STEADY)
    if not len(steady):
        return res
    again = failed[steady]
    second = kinetics.solve(view, tables, pm[again], theta_guess=tr['theta'][steady, 0, :], **solve_kw, **rows(again))
    good = np.flatnonzero(second['status'] == _kinetics.CONVERGED)
    for name, a in second.items():
        if name in res:
            res[name][again[good]] = a[good]
    res['rescued'][again[good]] = True
    return res
