"""Degree of rate control of a surface microkinetic model with lateral interactions and several site types: ctypes binding of
``include/catint_iacontrol.h``.  The model is that of ``catint_amd.interactions.InteractingModel`` (``include/catint_interact.h``), the
method that of ``catint_amd._drc`` (``include/catint_drc.h``): the exact derivatives of the wall fluxes with respect to every rate
constant, transition state and adsorbate energy at given coverages, from the full Jacobian of the steady state with the coverage
dependence of the energies in it, and the derivative with respect to the interaction strength itself
(``catint_amd/lib/libcatint_iacontrol.so``, built by ``catint_amd.build.build_iacontrol_library()``).  No fallback: a missing library
raises.

An ``InteractingRateControl`` is a context the user owns (``with InteractingRateControl() as rc: rc.solve(...)``);
``PnpSolver.get_rate_control`` opens one for the call when its model has interactions, and closes it."""
import ctypes as C

import numpy as np

from . import _devlib, _microkin
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _dptr  # noqa: F401  (part of this module's interface)
from ._drc import DEFAULT_RESIDUAL_TOL, INPUT, OK_POINT, PIVOT, RESIDUAL, apparent, normalised  # noqa: F401  (the same)
from ._interact import MAX_COLUMNS, MAX_SITE_TYPES, RESPONSE  # noqa: F401  (the same)
from ._microkin import DROP, _PD, _PI, _PL, _f64, _i32, _iptr  # noqa: F401  (the same)

LIB_PATH = _devlib.lib_path('iacontrol')

# every symbol include/catint_iacontrol.h declares (tests/test_iacontrol_abi.py)
SYMBOLS = _devlib.symbols('catic_', 'solve')

# output rows: name -> shape of one operating point from (N, T - 1, R) and G
FIELDS = {'dflux_dlnkf': lambda N, S, R, G=1: (R, N), 'dflux_dlnkb': lambda N, S, R, G=1: (R, N), 'dflux_drc': lambda N, S, R, G=1: (R, N),
          'dy_drc': lambda N, S, R, G=1: (R, S + 1), 'drc': lambda N, S, R, G=1: (R, N), 'dflux_dG': lambda N, S, R, G=1: (S + 1 - G, N),
          'tdrc': lambda N, S, R, G=1: (S + 1 - G, N), 'dflux_dstrength': lambda N, S, R, G=1: (N,), 'dy_dstrength': lambda N, S, R, G=1: (S + 1,),
          'strength_control': lambda N, S, R, G=1: (N,), 'flux': lambda N, S, R, G=1: (N,), 'flux_scale': lambda N, S, R, G=1: (N,)}
DEFAULT_FIELDS = ('drc', 'tdrc', 'strength_control', 'dflux_drc', 'dflux_dG', 'dflux_dstrength', 'flux', 'flux_scale')


class IacontrolError(_devlib.LibraryError):
    library = 'catint_iacontrol'


class CaticParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('nspecies', C.c_int32), ('nadsorbates', C.c_int32),
                ('nsteps', C.c_int32), ('potential_drop', C.c_int32), ('nsitetypes', C.c_int32), ('response', C.c_int32), ('n', C.c_int64),
                ('lanes', _PL), ('order_f', _PI), ('order_b', _PI), ('nu', _PD), ('cref', _PD), ('site_count', _PD), ('site_of', _PI),
                ('site_fraction', _PD), ('dG', _PD), ('Ea', _PD), ('lnA', _PD), ('eps', _PD), ('eps_ts', _PD), ('cutoff', _PD),
                ('smoothing', _PD), ('site_density', C.c_double), ('residual_tol', C.c_double), ('stern_capacitance', C.c_double),
                ('phi_pzc', C.c_double), ('strength', C.c_double), ('phiM', _PD), ('sigma', _PD), ('off', _PD), ('gamma', _PD), ('theta', _PD),
                ('csurf', _PD), ('phi_surface', _PD)]


class CaticOutputs(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('dflux_dlnkf', _PD), ('dflux_dlnkb', _PD), ('dflux_drc', _PD),
                ('dy_drc', _PD), ('drc', _PD), ('dflux_dG', _PD), ('tdrc', _PD), ('dflux_dstrength', _PD), ('dy_dstrength', _PD),
                ('strength_control', _PD), ('flux', _PD), ('flux_scale', _PD), ('residual', _PD), ('status', _PI)]


load_library = _devlib.loader(globals(), 'catic_', 'solve', CaticParams, CaticOutputs, IacontrolError)


class InteractingRateControl(_devlib.Handle):
    """One ``catic_ctx``.  No device call is made before the first ``solve`` that passes validation with at least one point.  Hold one
    for repeated calls: its device buffers are kept between them."""
    _prefix, _error, _load = 'catic_', IacontrolError, staticmethod(load_library)

    def solve(self, view, tables, phiM, theta, lanes=None, csurf=None, phi_surface=None, potential_drop='stern', stern_capacitance=0.0,
              phi_pzc=0.0, sigma=None, off=None, gamma=None, residual_tol=DEFAULT_RESIDUAL_TOL, fields=None, max_waves=0, struct_size=None,
              out_struct_size=None, out=None, strength=None):
        """catic_solve.  The arguments and the result of catint_amd._drc.RateControl.solve, with: tables a
        catint_amd.interactions.InteractingModel or the dict of its tables() (the keys InteractingKinetics.solve takes; a dict of
        MeanFieldModel.tables() alone is one site type without interactions); theta [n][T], T = G + S columns with the free sites
        first: the coverages InteractingKinetics.solve returned at the same arguments and the same strength; 'dy_drc' is [n][R][T],
        'dflux_dG' and 'tdrc' are [n][S][N].  fields may also name 'dflux_dstrength' [n][N], 'dy_dstrength' [n][T] and
        'strength_control' [n][N] = strength * dflux_dstrength / flux: the share of each flux that is owed to the interactions, to first
        order (exactly 0 for a species the mechanism does not touch).  strength: overrides tables['strength']."""
        tables = tables.tables() if hasattr(tables, 'tables') else tables
        site_of = _i32(tables['site_of']).reshape(-1) if 'site_of' in tables else np.zeros(len(tables['site_count']), np.int32)
        frac = _f64(tables['site_fraction']).reshape(-1) if 'site_fraction' in tables else np.ones(1)
        G = len(frac)
        per_point = {'sigma': sigma, 'off': off, 'gamma': gamma, 'theta': theta, 'csurf': csurf, 'phi_surface': phi_surface}
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
        p = CaticParams(struct_size=_devlib.size_of(CaticParams, struct_size), residual_tol=float(residual_tol), nsitetypes=G,
                        response=response if isinstance(response, int) else RESPONSE[response], site_of=_iptr(site_of),
                        site_fraction=_dptr(frac), eps=_dptr(eps), eps_ts=_dptr(eps_ts), cutoff=_dptr(cutoff), smoothing=_dptr(smoothing),
                        strength=float(tables.get('strength', 1.0) if strength is None else strength), **dict(call.members, nadsorbates=S))
        res = call.results(known, out)
        res.setdefault('status', np.zeros(call.n, np.int32))
        res.setdefault('residual', np.zeros(call.n))
        o = CaticOutputs(struct_size=_devlib.size_of(CaticOutputs, out_struct_size), status=_iptr(res['status']),
                         residual=_dptr(res['residual']), **{name: _dptr(a) for name, a in res.items() if name in FIELDS})
        self._call('solve', view, p, o)
        return res
