"""Voltammetry of a mean-field surface microkinetic model: ctypes binding of ``include/catint_voltam.h``.  The coverages are integrated
on the device along a linear potential program -- linear sweep, cyclic, several cycles -- every operating point with its own program
and step size, and the current, the charge and the wall fluxes come back along it (``catint_amd/lib/libcatint_voltam.so``, built by
``catint_amd.build.build_voltam_library()``).  No fallback: a missing library raises.

A ``Voltammetry`` is a context the user owns (``with Voltammetry() as vm: vm.sweep(...)``); ``PnpSolver.get_voltammogram`` opens one for
the call and closes it."""
import ctypes as C

import numpy as np

from . import _devlib, _microkin
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _dptr  # noqa: F401  (part of this module's interface)
from ._microkin import DROP, _PD, _PI, _PL, _f64, _iptr  # noqa: F401  (the same)

LIB_PATH = _devlib.lib_path('voltam')

# every symbol include/catint_voltam.h declares (tests/test_voltam_abi.py)
SYMBOLS = _devlib.symbols('catvm_', 'solve')

DONE, INPUT, STEPS = 0, 2, 3
MAX_STEPS, MAX_SEGMENTS, MAX_SAMPLES = 1000000, 64, 4096
FARADAY = 96485.33289
DEFAULT_RTOL, DEFAULT_ATOL, DEFAULT_NEWTON_TOL, DEFAULT_NEWTON_MAXIT, DEFAULT_MAX_STEPS = 1e-4, 1e-12, 1e-10, 8, 20000
DEFAULT_SEGMENTS, DEFAULT_SAMPLES = 2, 200
# output rows: name -> shape of one operating point from (N, S, R, n_out)
FIELDS = {'theta': lambda N, S, R, K: (K, S + 1), 'current': lambda N, S, R, K: (K,), 'current_scale': lambda N, S, R, K: (K,),
          'charge': lambda N, S, R, K: (K,), 'E_out': lambda N, S, R, K: (K,), 'flux': lambda N, S, R, K: (K, N),
          'flux_scale': lambda N, S, R, K: (K, N), 't_reached': lambda N, S, R, K: ()}
DEFAULT_FIELDS = ('theta', 'current', 'current_scale', 'charge', 'E_out', 't_reached')


class VoltamError(_devlib.LibraryError):
    library = 'catint_voltam'


class CatvmParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('nspecies', C.c_int32), ('nadsorbates', C.c_int32),
                ('nsteps', C.c_int32), ('newton_maxit', C.c_int32), ('potential_drop', C.c_int32), ('max_steps', C.c_int32),
                ('n', C.c_int64), ('lanes', _PL), ('order_f', _PI), ('order_b', _PI), ('nu', _PD), ('cref', _PD), ('site_count', _PD),
                ('dG', _PD), ('Ea', _PD), ('lnA', _PD), ('electrons', _PD), ('site_density', C.c_double), ('stern_capacitance', C.c_double),
                ('phi_pzc', C.c_double), ('E_start', _PD), ('E_vertex', _PD), ('scan_rate', _PD), ('sigma', _PD), ('off', _PD), ('gamma', _PD),
                ('theta0', _PD), ('csurf', _PD), ('phi_surface', _PD), ('n_segments', C.c_int32), ('samples', C.c_int32),
                ('rate_floor', C.c_double), ('rtol', C.c_double), ('atol', C.c_double), ('newton_tol', C.c_double), ('h0', C.c_double)]


class CatvmOutputs(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('theta', _PD), ('current', _PD), ('current_scale', _PD), ('charge', _PD),
                ('E_out', _PD), ('flux', _PD), ('flux_scale', _PD), ('t_reached', _PD), ('status', _PI), ('steps', _PI)]


load_library = _devlib.loader(globals(), 'catvm_', 'solve', CatvmParams, CatvmOutputs, VoltamError)


def default_rate_floor(kT):
    """1 / (4 kT/e) in 1/V: the peak turnover per V/s of a reversible one-electron monolayer, i_peak = v / (4 kT/e)"""
    return 1.0 / (4.0 * float(kT))


def mean_current(charge, E_start, E_vertex, scan_rate, samples):
    """charge [n][n_out] differenced between the output times, which are tau / samples apart (the first interval starts at t = 0 with
    no charge): [n][n_out] in A/m^2"""
    charge = np.asarray(charge, float)
    tau = np.abs(np.asarray(E_vertex, float).reshape(-1) - np.asarray(E_start, float).reshape(-1)) / np.asarray(scan_rate, float).reshape(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.diff(np.concatenate([np.zeros((len(charge), 1)), charge], axis=1), axis=1) / (tau / int(samples))[:, None]


class Voltammetry(_devlib.Handle):
    """One ``catvm_ctx``.  No device call is made before the first ``sweep`` that passes validation with at least one point.  Hold one
    for repeated sweeps: its device buffers are kept between calls."""
    _prefix, _error, _load = 'catvm_', VoltamError, staticmethod(load_library)

    def sweep(self, view, tables, electrons, E_start, E_vertex, scan_rate, n_segments=DEFAULT_SEGMENTS, samples=DEFAULT_SAMPLES, lanes=None,
              csurf=None, phi_surface=None, potential_drop='stern', stern_capacitance=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None,
              theta0=None, rate_floor=None, kT=None, rtol=DEFAULT_RTOL, atol=DEFAULT_ATOL, h0=0.0, newton_tol=DEFAULT_NEWTON_TOL,
              newton_maxit=DEFAULT_NEWTON_MAXIT, max_steps=DEFAULT_MAX_STEPS, fields=None, max_waves=0, struct_size=None, out_struct_size=None,
              out=None):
        """catvm_solve.  view, lanes, csurf, phi_surface, potential_drop, stern_capacitance, phi_pzc, off, gamma: those of
        KineticsSolver.solve; the surface concentrations and the surface potential are constant over the sweep (the electrolyte does
        not answer).  tables: a catint_amd.microkinetics.MeanFieldModel or the dict of its tables(); electrons [R]: the electrons on the
        reactant side of every step (None: the model's electrons()).  A model with lateral interactions or several site types is
        refused: the integrator is mean-field on one site type (catint_amd.iasweep.InteractingVoltammetry takes such a model).
        E_start, E_vertex [n] in V and scan_rate [n] in V/s: segment 0 runs from E_start to E_vertex, segment 1 back, and so on for
        n_segments segments (1: a linear sweep, 2: one cycle); every segment has `samples` equidistant output times, the last of them
        its end.  sigma [n]: a surface charge held constant over the sweep (None: it follows the potential through the Stern
        capacitance).  theta0 [n][S+1]: the coverages at t = 0 (None: the steady state at E_start).
        rtol: per step, on the coverages and on the turnover; atol: on the coverages; rate_floor in 1/V: rate_floor * scan_rate is the
        turnover below which the current is no longer resolved relatively (None: 1 / (4 kT/e) with kT in eV as given or the model's:
        the peak turnover per V/s of a reversible one-electron monolayer).
        fields: names out of FIELDS (None: DEFAULT_FIELDS; also 'flux', 'flux_scale').  Returns a dict of the requested arrays ('theta'
        [n][n_out][S+1], 'current', 'current_scale', 'charge', 'E_out' [n][n_out] with n_out = n_segments * samples: A/m^2, a reduction
        negative; A/m^2; C/m^2, cumulative; V; 'flux', 'flux_scale' [n][n_out][N], 't_reached' [n]) and 'status' [n] (DONE; INPUT: NaN
        rows -- a non-finite input, E_vertex == E_start, an unsolved lane or a start that does not converge; STEPS: max_steps attempted
        steps were not enough, the rows not reached are NaN), 'steps' [n][4] (accepted, rejected, Newton iterations, accepted without
        extrapolation), both int32.
        With 'charge' the result also holds 'mean_current' [n][n_out]: the charge passed between two output times over their
        distance, computed on the host.  Prefer it to 'current' for steps near equilibrium: there the instantaneous current is a
        small difference of large gross rates and keeps only the digits current / current_scale leaves of 16, while the charge obeys
        sum dq = sum_s w_s (theta_s(t) - theta_s(0)) to the Newton tolerance whatever the rates.  out: arrays to write into (tests)."""
        from .interactions import has_interactions
        model = tables if hasattr(tables, 'tables') else None
        tables = model.tables() if model is not None else tables
        if has_interactions(tables):
            raise ValueError('Voltammetry.sweep: the sweep integrates the mean-field model on one site type (include/catint_voltam.h); this '
                             'model has lateral interactions or several site types')
        if electrons is None and model is not None:
            electrons = model.electrons()
        if rate_floor is None:
            kT = model.kT if kT is None and model is not None else kT
            if kT is None:
                raise ValueError('Voltammetry.sweep: rate_floor=None needs kT (eV) or a model that gives it')
            rate_floor = default_rate_floor(kT)
        ne = None if electrons is None else _f64(np.atleast_1d(np.asarray(electrons, float))).reshape(-1)
        es = _f64(np.atleast_1d(np.asarray(E_start, float))).reshape(-1)
        n = len(es)
        ev = None if E_vertex is None else _f64(np.broadcast_to(np.asarray(E_vertex, float).reshape(-1), (n,)) if np.size(E_vertex) == 1 else
                                                np.asarray(E_vertex, float).reshape(-1))
        sr = None if scan_rate is None else _f64(np.broadcast_to(np.asarray(scan_rate, float).reshape(-1), (n,)) if np.size(scan_rate) == 1 else
                                                 np.asarray(scan_rate, float).reshape(-1))
        for name, a in (('E_vertex', ev), ('scan_rate', sr)):
            if a is not None and len(a) != n:
                raise ValueError('%s has %d values, E_start %d' % (name, len(a), n))
        K = max(int(n_segments), 0) * max(int(samples), 0)
        known = {name: (lambda N, S, R, f=f: f(N, S, R, K)) for name, f in FIELDS.items()}
        per_point = {'sigma': sigma, 'off': off, 'gamma': gamma, 'theta0': theta0, 'csurf': csurf, 'phi_surface': phi_surface}
        call = _microkin.Call(tables, es, lanes, per_point, fields, known, DEFAULT_FIELDS, potential_drop, stern_capacitance, phi_pzc, max_waves)
        if ne is not None and len(ne) != call.dims[2]:
            raise ValueError('electrons has %d values, the tables have %d steps' % (len(ne), call.dims[2]))
        members = dict(call.members)
        members['E_start'] = members.pop('phiM')
        p = CatvmParams(struct_size=_devlib.size_of(CatvmParams, struct_size), newton_maxit=int(newton_maxit), max_steps=int(max_steps),
                        electrons=_dptr(ne), E_vertex=_dptr(ev), scan_rate=_dptr(sr), n_segments=int(n_segments), samples=int(samples),
                        rate_floor=float(rate_floor), rtol=float(rtol), atol=float(atol), newton_tol=float(newton_tol), h0=float(h0), **members)
        res = call.results(known, out)
        res.setdefault('status', np.zeros(call.n, np.int32))
        res.setdefault('steps', np.zeros((call.n, 4), np.int32))
        o = CatvmOutputs(struct_size=_devlib.size_of(CatvmOutputs, out_struct_size),
                         status=_iptr(res['status']), steps=_iptr(res['steps']), **{name: _dptr(a) for name, a in res.items() if name in FIELDS})
        self._call('solve', view, p, o)
        if 'charge' in res and ev is not None and sr is not None:
            res['mean_current'] = mean_current(res['charge'], es, ev, sr, samples)
        return res
