"""ctypes binding of ``include/catint_eis.h``: the small-signal response of the microkinetic electrode -- the linearised surface kinetics
with adsorbate storage, the transport transfer functions at the same frequency and the Stern layer, closed at the wall -- formed on the
device (``catint_amd/lib/libcatint_eis.so``, built by ``catint_amd.build.build_eis_library()``).  No fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _devlib, _microkin
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _dptr  # noqa: F401  (part of this module's interface)
from ._devlib import _PD, _PI, _PL, _f64, _iptr  # noqa: F401  (the same)
from ._medium import WALL, Medium, reaction_table  # noqa: F401  (the same)
from ._microkin import DROP  # noqa: F401  (the same)

LIB_PATH = _devlib.lib_path('eis')

# every symbol include/catint_eis.h declares (tests/test_eis_abi.py)
SYMBOLS = _devlib.symbols('cateis_', 'kinetic') + ['cateis_solve']

MAX_FREQ, MAX_NX = 256, 4098
PIVOT_GROWTH_LIMIT, SINGULAR = 1e8, 1e-12
OK, PIVOT, INPUT, SINGULAR_A, RESIDUAL = 0, 1, 2, 3, 4
# output rows: name -> (shape of one (point, frequency) pair from (N, S), complex?); 'residual' is per point
KINETIC_FIELDS = {'Kc': lambda N, S: (N, N), 'Kphi': lambda N, S: (N, 2), 'dy': lambda N, S: (S + 1, N + 2)}
ELECTRODE_FIELDS = {'admittance': lambda N, S: (), 'faradaic': lambda N, S: (), 'double_layer': lambda N, S: (), 'dflux': lambda N, S: (N,),
                    'dc_surface': lambda N, S: (N,), 'dphi_surface': lambda N, S: (), 'dsigma': lambda N, S: (), 'Tc': lambda N, S: (N, N),
                    'Tphi': lambda N, S: (N,), 'tc': lambda N, S: (N,), 'tphi': lambda N, S: ()}
FIELDS = dict(KINETIC_FIELDS, **ELECTRODE_FIELDS)
FIELDS['residual'] = None
DEFAULT_KINETIC_FIELDS = ('Kc', 'Kphi', 'residual')
DEFAULT_FIELDS = ('admittance', 'faradaic', 'double_layer', 'dflux', 'dc_surface', 'dphi_surface', 'dsigma', 'residual')


class EisError(_devlib.LibraryError):
    library = 'catint_eis'


class CateisParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('nspecies', C.c_int32), ('nadsorbates', C.c_int32),
                ('nsteps', C.c_int32), ('potential_drop', C.c_int32), ('nfreq', C.c_int32), ('wall_bc', C.c_int32),
                ('nreactions', C.c_int32), ('reserved', C.c_int32), ('n', C.c_int64), ('lanes', _PL), ('order_f', _PI), ('order_b', _PI),
                ('nu', _PD), ('cref', _PD), ('site_count', _PD), ('dG', _PD), ('Ea', _PD), ('lnA', _PD), ('site_density', C.c_double),
                ('stern_capacitance', C.c_double), ('phi_pzc', C.c_double), ('phiM', _PD), ('sigma', _PD), ('off', _PD), ('gamma', _PD),
                ('theta', _PD), ('csurf', _PD), ('phi_surface', _PD), ('omega', _PD), ('residual_tol', C.c_double), ('D', _PD),
                ('charges', _PD), ('mpb_radius', _PD), ('x', _PD), ('beta', C.c_double), ('eps', C.c_double), ('dx', C.c_double),
                ('velocity', C.c_double), ('n_lhs', _PI), ('lhs', _PI), ('n_rhs', _PI), ('rhs', _PI), ('kf', _PD), ('kr', _PD),
                ('rf', C.c_double)]


class CateisOutputs(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('Kc', _PD), ('Kphi', _PD), ('dy', _PD), ('residual', _PD),
                ('status', _PI), ('admittance', _PD), ('faradaic', _PD), ('double_layer', _PD), ('dflux', _PD), ('dc_surface', _PD),
                ('dphi_surface', _PD), ('dsigma', _PD), ('Tc', _PD), ('Tphi', _PD), ('tc', _PD), ('tphi', _PD)]


load_library = _devlib.loader(globals(), 'cateis_', 'kinetic', CateisParams, CateisOutputs, EisError, more=('solve',))


class Impedance(_devlib.Handle):
    """One ``cateis_ctx``.  No device call is made before the first call that passes validation with at least one point and one output."""
    _prefix, _error, _load = 'cateis_', EisError, staticmethod(load_library)

    def _run(self, entry, known, default, view, tables, phiM, theta, omega, lanes, per_point, fields, potential_drop, stern_capacitance,
             phi_pzc, residual_tol, max_waves, extra, struct_size, out_struct_size, out):
        om = None if omega is None else _f64(np.atleast_1d(np.asarray(omega, float))).reshape(-1)
        F = 0 if om is None else len(om)
        shapes = {name: None for name in known}
        pp = dict(per_point)
        pp['theta'] = theta
        call = _microkin.Call(tables, phiM, lanes, pp, fields, shapes, default, potential_drop, stern_capacitance, phi_pzc, max_waves)
        N, S, _ = (max(v, 0) for v in call.dims)
        p = CateisParams(struct_size=_devlib.size_of(CateisParams, struct_size), nfreq=F, omega=_dptr(om), residual_tol=float(residual_tol),
                         **call.members, **extra)
        res = {} if out is None else out
        for name in call.names:
            if name == 'residual':
                res.setdefault(name, np.empty(call.n))
            else:
                res.setdefault(name, np.empty((call.n, F) + FIELDS[name](N, S), np.complex128))
        res.setdefault('status', np.zeros((call.n, F), np.int32))
        o = CateisOutputs(struct_size=_devlib.size_of(CateisOutputs, out_struct_size), status=_iptr(res['status']))
        for name, a in res.items():
            if name in FIELDS:
                setattr(o, name, C.cast(a.ctypes.data, _PD))
        self._call(entry, view, p, o)
        return res

    def kinetic(self, view, tables, phiM, theta, omega, lanes=None, csurf=None, phi_surface=None, potential_drop='stern',
                stern_capacitance=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None, residual_tol=1e-8, fields=None, max_waves=0,
                struct_size=None, out_struct_size=None, out=None):
        """cateis_kinetic: the intrinsic kinetic admittance at a fixed surface state.  view, tables, phiM, lanes, csurf, phi_surface,
        potential_drop, stern_capacitance, phi_pzc, sigma, off, gamma: those of KineticsSolver.solve; theta [n][S+1]: the stationary
        coverages; omega [F] in rad/s.  fields: names out of KINETIC_FIELDS and 'residual' (None: DEFAULT_KINETIC_FIELDS).  Returns
        complex128 arrays 'Kc' [n][F][N][N], 'Kphi' [n][F][N][2], 'dy' [n][F][S+1][N+2], 'residual' [n] (float64) and 'status' [n][F]
        (int32)."""
        known = dict(KINETIC_FIELDS, residual=None)
        return self._run('kinetic', known, DEFAULT_KINETIC_FIELDS, view, tables, phiM, theta, omega, lanes,
                         {'sigma': sigma, 'off': off, 'gamma': gamma, 'csurf': csurf, 'phi_surface': phi_surface}, fields, potential_drop,
                         stern_capacitance, phi_pzc, residual_tol, max_waves, {}, struct_size, out_struct_size, out)

    def solve(self, view, tables, phiM, theta, omega, D, charges, x, beta, eps, dx, rf=1.0, lanes=None, mpb_radius=None, wall_bc='stern',
              stern_capacitance=0.0, velocity=0.0, reactions=(), potential_drop='stern', phi_pzc=0.0, sigma=None, off=None, gamma=None,
              residual_tol=1e-8, fields=None, max_waves=0, struct_size=None, out_struct_size=None, out=None):
        """cateis_solve: the coupled electrode about the state behind `view`.  The medium (D, charges, x, beta, eps, dx, mpb_radius,
        wall_bc, stern_capacitance, velocity, reactions) is that of Coupler.solve, the kinetic arguments those of `kinetic`; rf: the
        roughness factor (0: the blocking electrode).  fields: names out of FIELDS (None: DEFAULT_FIELDS).  Returns complex128 arrays
        [n][F]..., 'residual' [n] and 'status' [n][F] (0; 1 failed pivot check in the transport elimination; 2 unsolved lane or
        non-finite input, NaN; 3 singular A(omega); 4 the coverages are not stationary)."""
        medium = Medium(view, D, charges, x, beta, mpb_radius, velocity, reactions, eps=eps, dx=dx, wall_bc=wall_bc)
        medium.check('the call needs')
        extra = dict(medium.members, rf=float(rf))
        return self._run('solve', FIELDS, DEFAULT_FIELDS, view, tables, phiM, theta, omega, lanes, {'sigma': sigma, 'off': off, 'gamma': gamma},
                         fields, potential_drop, stern_capacitance, phi_pzc, residual_tol, max_waves, extra, struct_size, out_struct_size, out)
