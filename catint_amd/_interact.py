"""ctypes binding of ``include/catint_interact.h``: the steady state of a surface microkinetic model with lateral interactions and several
site types per operating point, the interaction strength ramped in stages inside one launch, its wall fluxes and their sensitivities,
solved on the device (``catint_amd/lib/libcatint_interact.so``, built by ``catint_amd.build.build_interact_library()``).  No fallback: a
missing library raises."""
import ctypes as C

import numpy as np

from . import _devlib, _microkin
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _dptr  # noqa: F401  (part of this module's interface)
from ._microkin import DROP, MAX_ORDER, MAX_SITES, MAX_SPECIES, MAX_STEPS, MIN_LOG, _PD, _PI, _PL, _f64, _i32, _iptr  # noqa: F401  (the same)

LIB_PATH = _devlib.lib_path('interact')

# every symbol include/catint_interact.h declares (tests/test_interact_abi.py)
SYMBOLS = _devlib.symbols('catia_', 'solve')

MAX_SITE_TYPES, MAX_COLUMNS = 3, 9
CONVERGED, MAXIT, INPUT, PIVOT = 0, 1, 2, 3
RESPONSE = {'linear': 0, 'piecewise': 1}
DEFAULT_TOL, DEFAULT_MAXIT, DEFAULT_RAMP = 1e-12, 200, 1
SCF_RAMP = 10          # the reference's n_inter: the stages of a solve from the uniform start in the SCF loops
# output rows: name -> shape of one operating point from (N, T - 1, R) and G
FIELDS = {'theta': lambda N, S, R, G=1: (S + 1,), 'rate': lambda N, S, R, G=1: (R,), 'rate_gross': lambda N, S, R, G=1: (R,),
          'flux': lambda N, S, R, G=1: (N,), 'flux_scale': lambda N, S, R, G=1: (N,), 'dflux_dc': lambda N, S, R, G=1: (N, N),
          'dflux_dphi': lambda N, S, R, G=1: (N, 2), 'energy_shift': lambda N, S, R, G=1: (S + 1 - G,)}
DEFAULT_FIELDS = ('theta', 'rate', 'rate_gross', 'flux', 'flux_scale', 'energy_shift')
FLAGS = ('status', 'iterations', 'ramp_reached')


class InteractError(_devlib.LibraryError):
    library = 'catint_interact'


class CatiaParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('nspecies', C.c_int32), ('nadsorbates', C.c_int32),
                ('nsteps', C.c_int32), ('maxit', C.c_int32), ('potential_drop', C.c_int32), ('nsitetypes', C.c_int32),
                ('response', C.c_int32), ('ramp', C.c_int32), ('n', C.c_int64), ('lanes', _PL), ('order_f', _PI), ('order_b', _PI),
                ('nu', _PD), ('cref', _PD), ('site_count', _PD), ('site_of', _PI), ('site_fraction', _PD), ('dG', _PD), ('Ea', _PD),
                ('lnA', _PD), ('eps', _PD), ('eps_ts', _PD), ('cutoff', _PD), ('smoothing', _PD), ('site_density', C.c_double),
                ('tol', C.c_double), ('stern_capacitance', C.c_double), ('phi_pzc', C.c_double), ('strength', C.c_double), ('phiM', _PD),
                ('sigma', _PD), ('off', _PD), ('gamma', _PD), ('theta_guess', _PD), ('csurf', _PD), ('phi_surface', _PD)]


class CatiaOutputs(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('theta', _PD), ('rate', _PD), ('rate_gross', _PD), ('flux', _PD),
                ('flux_scale', _PD), ('dflux_dc', _PD), ('dflux_dphi', _PD), ('energy_shift', _PD), ('status', _PI), ('iterations', _PI),
                ('ramp_reached', _PI)]


load_library = _devlib.loader(globals(), 'catia_', 'solve', CatiaParams, CatiaOutputs, InteractError)


class InteractingKinetics(_devlib.Handle):
    """One ``catia_ctx``.  No device call is made before the first ``solve`` that passes validation with at least one point."""
    _prefix, _error, _load = 'catia_', InteractError, staticmethod(load_library)

    def solve(self, view, tables, phiM, lanes=None, csurf=None, phi_surface=None, potential_drop='stern', stern_capacitance=0.0, phi_pzc=0.0,
              sigma=None, off=None, gamma=None, theta_guess=None, tol=DEFAULT_TOL, maxit=DEFAULT_MAXIT, fields=None, max_waves=0,
              struct_size=None, out_struct_size=None, out=None, ramp=DEFAULT_RAMP, strength=None):
        """catia_solve.  The arguments and the result of KineticsSolver.solve, with: tables the dict of InteractingModel.tables()
        ('order_f', 'order_b' [R][N+T], 'site_count' [T], 'site_of' [T], 'site_fraction' [G], 'eps' [S][S], 'eps_ts' [R][S] or None,
        'response' 'linear' | 'piecewise', 'cutoff', 'smoothing' [G], 'strength'; a dict of MeanFieldModel.tables() alone is one site
        type without interactions); theta_guess [n][T]; ramp: the number of stages the strength is raised in, maxit per stage;
        strength: overrides tables['strength'].  Returns the requested arrays (FIELDS; 'energy_shift' [n][S] in kT) and 'status',
        'iterations' (summed over the stages), 'ramp_reached' [n] (int32)."""
        site_of = _i32(tables['site_of']).reshape(-1) if 'site_of' in tables else np.zeros(len(tables['site_count']), np.int32)
        frac = _f64(tables['site_fraction']).reshape(-1) if 'site_fraction' in tables else np.ones(1)
        G = len(frac)
        per_point = {'sigma': sigma, 'off': off, 'gamma': gamma, 'theta_guess': theta_guess, 'csurf': csurf, 'phi_surface': phi_surface}
        known = {k: (lambda N, S, R, f=f: f(N, S, R, G)) for k, f in FIELDS.items()}
        call = _microkin.Call(tables, phiM, lanes, per_point, fields, known, DEFAULT_FIELDS, potential_drop, stern_capacitance, phi_pzc, max_waves)
        N, T1, R = call.dims
        S = T1 + 1 - G
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
        p = CatiaParams(struct_size=_devlib.size_of(CatiaParams, struct_size), maxit=int(maxit), tol=float(tol),
                        nsitetypes=G, response=response if isinstance(response, int) else RESPONSE[response], ramp=int(ramp),
                        site_of=_iptr(site_of), site_fraction=_dptr(frac), eps=_dptr(eps), eps_ts=_dptr(eps_ts), cutoff=_dptr(cutoff),
                        smoothing=_dptr(smoothing), strength=float(tables.get('strength', 1.0) if strength is None else strength), **members)
        res = call.results(known, out)
        for k in FLAGS:
            res.setdefault(k, np.zeros(call.n, np.int32))
        o = CatiaOutputs(struct_size=_devlib.size_of(CatiaOutputs, out_struct_size),
                         **dict({k: _iptr(res[k]) for k in FLAGS}, **{name: _dptr(a) for name, a in res.items() if name in FIELDS}))
        self._call('solve', view, p, o)
        return res


_PER_POINT = ('lanes', 'csurf', 'phi_surface', 'sigma', 'off', 'gamma')


class RampedKinetics(InteractingKinetics):
    """What the SCF loops of the calculator hold in the place of a KineticsSolver when the model carries interaction keys: solve() has
    KineticsSolver.solve's signature.  A call without theta_guess (the first SCF iteration) ramps the interaction strength in `ramp`
    stages from the uniform start; a call with one (the later iterations) starts there at full strength, and a point that then ends
    with status 1 or 3 is solved once more from the uniform start with the ramp."""

    def __init__(self, device=0, ramp=SCF_RAMP):
        if int(ramp) < 1:
            raise ValueError('ramp is the number of stages, at least 1')
        InteractingKinetics.__init__(self, device)
        self.ramp = int(ramp)
        self.retried = 0          # points solved a second time so far

    def solve(self, view, tables, phiM, theta_guess=None, **kw):
        if theta_guess is None:
            return InteractingKinetics.solve(self, view, tables, phiM, ramp=self.ramp, **kw)
        out = InteractingKinetics.solve(self, view, tables, phiM, theta_guess=theta_guess, ramp=1, **kw)
        status = np.asarray(out['status'])
        again = np.flatnonzero((status == MAXIT) | (status == PIVOT))
        if len(again):
            self.retried += len(again)
            sub = {k: (np.asarray(v)[again] if k in _PER_POINT and v is not None else v) for k, v in kw.items() if k != 'out'}
            if view is not None and sub.get('lanes') is None:
                sub['lanes'] = again
            second = InteractingKinetics.solve(self, view, tables, np.asarray(phiM, float).reshape(-1)[again], ramp=self.ramp, **sub)
            for k, v in second.items():
                out[k][again] = v
        return out
