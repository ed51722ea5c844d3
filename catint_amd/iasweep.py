"""Voltammetry of a surface microkinetic model with lateral interactions and several site types: ctypes binding of
``include/catint_iasweep.h``.  The model is that of ``catint_amd.interactions.InteractingModel`` (``include/catint_interact.h``), the
method that of ``catint_amd.voltammetry`` (``include/catint_voltam.h``): the coverages are integrated on the device along a linear
potential program, or held at a constant potential, every operating point with its own program and step size, the rate constants
following the coverages at every rate evaluation (``catint_amd/lib/libcatint_iasweep.so``, built by
``catint_amd.build.build_iasweep_library()``).  No fallback: a missing library raises.

An ``InteractingVoltammetry`` is a context the user owns (``with InteractingVoltammetry() as iv: iv.sweep(...)``);
``PnpSolver.get_voltammogram`` opens one for the call when its model has interactions, and closes it."""
import ctypes as C

import numpy as np

from . import _devlib, _microkin
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _dptr  # noqa: F401  (part of this module's interface)
from ._interact import MAX_COLUMNS, MAX_SITE_TYPES, RESPONSE, SCF_RAMP  # noqa: F401  (the same)
from ._microkin import DROP, _PD, _PI, _PL, _f64, _i32, _iptr  # noqa: F401  (the same)
from .voltammetry import (DEFAULT_ATOL, DEFAULT_MAX_STEPS, DEFAULT_NEWTON_MAXIT, DEFAULT_NEWTON_TOL, DEFAULT_RTOL, DEFAULT_SAMPLES,  # noqa: F401
                          DEFAULT_SEGMENTS, FARADAY, MAX_SAMPLES, MAX_SEGMENTS, MAX_STEPS, default_rate_floor, mean_current)

LIB_PATH = _devlib.lib_path('iasweep')

# every symbol include/catint_iasweep.h declares (tests/test_iasweep_abi.py)
SYMBOLS = _devlib.symbols('catis_', 'solve')

DONE, INPUT, STEPS = 0, 2, 3
START_RAMP = SCF_RAMP          # the stages of the steady solve at E_start from the uniform start
# output rows: name -> shape of one operating point from (N, T - 1, R, n_out) and G
FIELDS = {'theta': lambda N, S, R, K, G=1: (K, S + 1), 'current': lambda N, S, R, K, G=1: (K,), 'current_scale': lambda N, S, R, K, G=1: (K,),
          'charge': lambda N, S, R, K, G=1: (K,), 'E_out': lambda N, S, R, K, G=1: (K,), 'flux': lambda N, S, R, K, G=1: (K, N),
          'flux_scale': lambda N, S, R, K, G=1: (K, N), 't_reached': lambda N, S, R, K, G=1: (),
          'energy_shift': lambda N, S, R, K, G=1: (K, S + 1 - G)}
DEFAULT_FIELDS = ('theta', 'current', 'current_scale', 'charge', 'E_out', 't_reached')


class IasweepError(_devlib.LibraryError):
    library = 'catint_iasweep'


class CatisParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('nspecies', C.c_int32), ('nadsorbates', C.c_int32),
                ('nsteps', C.c_int32), ('newton_maxit', C.c_int32), ('potential_drop', C.c_int32), ('max_steps', C.c_int32),
                ('nsitetypes', C.c_int32), ('response', C.c_int32), ('start_ramp', C.c_int32), ('reserved', C.c_int32),
                ('n', C.c_int64), ('lanes', _PL), ('order_f', _PI), ('order_b', _PI), ('nu', _PD), ('cref', _PD), ('site_count', _PD),
                ('site_of', _PI), ('site_fraction', _PD), ('dG', _PD), ('Ea', _PD), ('lnA', _PD), ('eps', _PD), ('eps_ts', _PD),
                ('cutoff', _PD), ('smoothing', _PD), ('electrons', _PD), ('site_density', C.c_double), ('stern_capacitance', C.c_double),
                ('phi_pzc', C.c_double), ('strength', C.c_double), ('E_start', _PD), ('E_vertex', _PD), ('scan_rate', _PD),
                ('hold_time', _PD), ('sigma', _PD), ('off', _PD), ('gamma', _PD), ('theta0', _PD), ('csurf', _PD), ('phi_surface', _PD),
                ('n_segments', C.c_int32), ('samples', C.c_int32), ('rate_floor', C.c_double), ('rtol', C.c_double), ('atol', C.c_double),
                ('newton_tol', C.c_double), ('h0', C.c_double)]


class CatisOutputs(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('theta', _PD), ('current', _PD), ('current_scale', _PD), ('charge', _PD),
                ('E_out', _PD), ('flux', _PD), ('flux_scale', _PD), ('t_reached', _PD), ('energy_shift', _PD), ('status', _PI), ('steps', _PI)]


load_library = _devlib.loader(globals(), 'catis_', 'solve', CatisParams, CatisOutputs, IasweepError)


def _per_point(name, a, n):
    """a [n] (a scalar: the same for every point) as the contiguous array the library takes, None as it is"""
    if a is None:
        return None
    a = np.asarray(a, float).reshape(-1)
    a = _f64(np.broadcast_to(a, (n,)) if a.size == 1 else a)
    if len(a) != n:
        raise ValueError('%s has %d values, E_start %d' % (name, len(a), n))
    return a


class InteractingVoltammetry(_devlib.Handle):
    """One ``catis_ctx``.  No device call is made before the first ``sweep`` that passes validation with at least one point.  Hold one
    for repeated sweeps: its device buffers are kept between calls."""
    _prefix, _error, _load = 'catis_', IasweepError, staticmethod(load_library)

    def sweep(self, view, tables, electrons, E_start, E_vertex, scan_rate, n_segments=DEFAULT_SEGMENTS, samples=DEFAULT_SAMPLES, lanes=None,
              csurf=None, phi_surface=None, potential_drop='stern', stern_capacitance=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None,
              theta0=None, rate_floor=None, kT=None, rtol=DEFAULT_RTOL, atol=DEFAULT_ATOL, h0=0.0, newton_tol=DEFAULT_NEWTON_TOL,
              newton_maxit=DEFAULT_NEWTON_MAXIT, max_steps=DEFAULT_MAX_STEPS, fields=None, max_waves=0, struct_size=None, out_struct_size=None,
              out=None, hold_time=None, start_ramp=None, strength=None):
        """catis_solve.  The arguments and the result of catint_amd.voltammetry.Voltammetry.sweep, with: tables a
        catint_amd.interactions.InteractingModel or the dict of its tables() (the keys InteractingKinetics.solve takes; a dict of
        MeanFieldModel.tables() alone is one site type without interactions); theta0 and 'theta' are [n][T] and [n][n_out][T], T = G + S
        columns with the free sites first, the free site of every type recomputed from its balance; fields may also name
        'energy_shift' [n][n_out][S]: the shift of every adsorbate's energy at the output state, in kT.
        hold_time [n] in s (a scalar: the same for every point): a point whose E_vertex equals its E_start and whose hold_time is
        positive and finite is held at E_start, every one of the n_segments segments lasting hold_time with `samples` output times --
        the transient of the interacting model after a step of the potential, started from theta0; scan_rate is still required and
        only sets the floor of the current.  start_ramp: the stages the interaction strength is raised in by the steady solve at
        E_start (None: START_RAMP = 10 from the uniform start, 1 with theta0, which runs no steady solve); a point where a stage does
        not converge ends INPUT.  strength: overrides tables['strength']."""
        model = tables if hasattr(tables, 'tables') else None
        tables = model.tables() if model is not None else tables
        if electrons is None and model is not None:
            electrons = model.electrons()
        if rate_floor is None:
            kT = model.kT if kT is None and model is not None else kT
            if kT is None:
                raise ValueError('InteractingVoltammetry.sweep: rate_floor=None needs kT (eV) or a model that gives it')
            rate_floor = default_rate_floor(kT)
        if start_ramp is None:
            start_ramp = START_RAMP if theta0 is None else 1
        ne = None if electrons is None else _f64(np.atleast_1d(np.asarray(electrons, float))).reshape(-1)
        es = _f64(np.atleast_1d(np.asarray(E_start, float))).reshape(-1)
        n = len(es)
        ev, sr, hold = _per_point('E_vertex', E_vertex, n), _per_point('scan_rate', scan_rate, n), _per_point('hold_time', hold_time, n)
        site_of = _i32(tables['site_of']).reshape(-1) if 'site_of' in tables else np.zeros(len(tables['site_count']), np.int32)
        frac = _f64(tables['site_fraction']).reshape(-1) if 'site_fraction' in tables else np.ones(1)
        G = len(frac)
        K = max(int(n_segments), 0) * max(int(samples), 0)
        known = {name: (lambda N, S, R, f=f: f(N, S, R, K, G)) for name, f in FIELDS.items()}
        per_point = {'sigma': sigma, 'off': off, 'gamma': gamma, 'theta0': theta0, 'csurf': csurf, 'phi_surface': phi_surface}
        call = _microkin.Call(tables, es, lanes, per_point, fields, known, DEFAULT_FIELDS, potential_drop, stern_capacitance, phi_pzc, max_waves)
        N, T1, R = call.dims
        S = T1 + 1 - G
        if ne is not None and len(ne) != R:
            raise ValueError('electrons has %d values, the tables have %d steps' % (len(ne), R))
        if len(site_of) != T1 + 1:
            raise ValueError('site_of has %d values, the tables need %d' % (len(site_of), T1 + 1))
        eps = _f64(tables['eps']) if tables.get('eps') is not None else np.zeros((max(S, 0), max(S, 0)))
        eps_ts = _f64(tables['eps_ts']) if tables.get('eps_ts') is not None else None
        for name, a, size in (('eps', eps, S * S), ('eps_ts', eps_ts, R * S)):
            if a is not None and a.size != max(size, 0) and S > 0:
                raise ValueError('%s has %d values, the tables need %d' % (name, a.size, size))
        response = tables.get('response', 'linear')
        cutoff = _f64(np.broadcast_to(np.asarray(tables['cutoff'], float), (G,))) if tables.get('cutoff') is not None else None
        smoothing = _f64(np.broadcast_to(np.asarray(tables['smoothing'], float), (G,))) if tables.get('smoothing') is not None else None
        members = dict(call.members, nadsorbates=S)
        members['E_start'] = members.pop('phiM')
        p = CatisParams(struct_size=_devlib.size_of(CatisParams, struct_size), newton_maxit=int(newton_maxit), max_steps=int(max_steps),
                        nsitetypes=G, response=response if isinstance(response, int) else RESPONSE[response], start_ramp=int(start_ramp),
                        site_of=_iptr(site_of), site_fraction=_dptr(frac), eps=_dptr(eps), eps_ts=_dptr(eps_ts), cutoff=_dptr(cutoff),
                        smoothing=_dptr(smoothing), strength=float(tables.get('strength', 1.0) if strength is None else strength),
                        electrons=_dptr(ne), E_vertex=_dptr(ev), scan_rate=_dptr(sr), hold_time=_dptr(hold), n_segments=int(n_segments),
                        samples=int(samples), rate_floor=float(rate_floor), rtol=float(rtol), atol=float(atol), newton_tol=float(newton_tol),
                        h0=float(h0), **members)
        res = call.results(known, out)
        res.setdefault('status', np.zeros(call.n, np.int32))
        res.setdefault('steps', np.zeros((call.n, 4), np.int32))
        o = CatisOutputs(struct_size=_devlib.size_of(CatisOutputs, out_struct_size),
                         status=_iptr(res['status']), steps=_iptr(res['steps']), **{name: _dptr(a) for name, a in res.items() if name in FIELDS})
        self._call('solve', view, p, o)
        if 'charge' in res and ev is not None and sr is not None:
            tau = np.abs(ev - es) / sr
            if hold is not None:
                tau = np.where((ev == es) & (hold > 0.0) & np.isfinite(hold), hold, tau)
            with np.errstate(divide='ignore', invalid='ignore'):
                res['mean_current'] = np.diff(np.concatenate([np.zeros((len(es), 1)), res['charge']], axis=1), axis=1) / (tau / int(samples))[:, None]
        return res
