"""ctypes binding of ``include/catint_drc.h``: the degree of rate control of a microkinetic steady state per operating point -- the
derivatives of the wall fluxes with respect to every rate constant, transition state and adsorbate energy, computed on the device
(``catint_amd/lib/libcatint_drc.so``, built by ``catint_amd.build.build_drc_library()``).  No fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _devlib, _microkin
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _dptr  # noqa: F401  (part of this module's interface)
from ._microkin import DROP, MAX_ADSORBATES, MAX_ORDER, MAX_SITES, MAX_SPECIES, MAX_STEPS, MIN_LOG, _PD, _PI, _PL, _iptr  # noqa: F401  (the same)

LIB_PATH = _devlib.lib_path('drc')

# every symbol include/catint_drc.h declares (tests/test_drc_abi.py)
SYMBOLS = _devlib.symbols('catdrc_', 'solve')

OK_POINT, RESIDUAL, INPUT, PIVOT = 0, 1, 2, 3
DEFAULT_RESIDUAL_TOL = 1e-8
# output rows: name -> shape of one operating point from (N, S, R)
FIELDS = {'dflux_dlnkf': lambda N, S, R: (R, N), 'dflux_dlnkb': lambda N, S, R: (R, N), 'dflux_drc': lambda N, S, R: (R, N),
          'dy_drc': lambda N, S, R: (R, S + 1), 'drc': lambda N, S, R: (R, N), 'dflux_dG': lambda N, S, R: (S, N),
          'tdrc': lambda N, S, R: (S, N), 'flux': lambda N, S, R: (N,), 'flux_scale': lambda N, S, R: (N,)}
DEFAULT_FIELDS = ('drc', 'tdrc', 'dflux_drc', 'dflux_dG', 'flux', 'flux_scale')


class DrcError(_devlib.LibraryError):
    library = 'catint_drc'


class CatdrcParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('nspecies', C.c_int32), ('nadsorbates', C.c_int32),
                ('nsteps', C.c_int32), ('potential_drop', C.c_int32), ('n', C.c_int64), ('lanes', _PL), ('order_f', _PI), ('order_b', _PI),
                ('nu', _PD), ('cref', _PD), ('site_count', _PD), ('dG', _PD), ('Ea', _PD), ('lnA', _PD), ('site_density', C.c_double),
                ('residual_tol', C.c_double), ('stern_capacitance', C.c_double), ('phi_pzc', C.c_double), ('phiM', _PD), ('sigma', _PD),
                ('off', _PD), ('gamma', _PD), ('theta', _PD), ('csurf', _PD), ('phi_surface', _PD)]


class CatdrcOutputs(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('dflux_dlnkf', _PD), ('dflux_dlnkb', _PD), ('dflux_drc', _PD),
                ('dy_drc', _PD), ('drc', _PD), ('dflux_dG', _PD), ('tdrc', _PD), ('flux', _PD), ('flux_scale', _PD), ('residual', _PD),
                ('status', _PI)]


load_library = _devlib.loader(globals(), 'catdrc_', 'solve', CatdrcParams, CatdrcOutputs, DrcError)


class RateControl(_devlib.Handle):
    """One ``catdrc_ctx``.  No device call is made before the first ``solve`` that passes validation with at least one point."""
    _prefix, _error, _load = 'catdrc_', DrcError, staticmethod(load_library)

    def solve(self, view, tables, phiM, theta, lanes=None, csurf=None, phi_surface=None, potential_drop='stern', stern_capacitance=0.0,
              phi_pzc=0.0, sigma=None, off=None, gamma=None, residual_tol=DEFAULT_RESIDUAL_TOL, fields=None, max_waves=0, struct_size=None,
              out_struct_size=None, out=None):
        """catdrc_solve.  view: a PnpDeviceView, or None when csurf [n][N] and phi_surface [n] give the surface state.  tables: the dict
        of MeanFieldModel.tables().  theta [n][S+1]: the coverages of the steady state (KineticsSolver.solve's 'theta' at the same
        arguments).  phiM [n] and every other per-point array are indexed by the position in the call; lanes [n]: indices into the
        handle's batch on the view path (None: 0 .. n-1).  sigma [n], off [n][R][2], gamma [n][N] optional, as in KineticsSolver.solve.
        fields: names out of FIELDS (None: DEFAULT_FIELDS).  Returns a dict of the requested arrays and 'status' [n] (int32: 0; 1 the
        residual of the state is above residual_tol, numbers as computed; 2 non-finite input or unsolved lane, NaN; 3 bad pivot) and
        'residual' [n].  'drc' = 'dflux_drc' / 'flux' and 'tdrc' = 'dflux_dG' / 'flux' (exactly 0 for a species the mechanism does not
        touch): their number of digits is what flux / flux_scale leaves of 16.  out: arrays to write into (tests)."""
        per_point = {'sigma': sigma, 'off': off, 'gamma': gamma, 'theta': theta, 'csurf': csurf, 'phi_surface': phi_surface}
        call = _microkin.Call(tables, phiM, lanes, per_point, fields, FIELDS, DEFAULT_FIELDS, potential_drop, stern_capacitance, phi_pzc, max_waves)
        p = CatdrcParams(struct_size=_devlib.size_of(CatdrcParams, struct_size), residual_tol=float(residual_tol),
                         **call.members)
        res = call.results(FIELDS, out)
        res.setdefault('status', np.zeros(call.n, np.int32))
        res.setdefault('residual', np.zeros(call.n))
        o = CatdrcOutputs(struct_size=_devlib.size_of(CatdrcOutputs, out_struct_size),
                          status=_iptr(res['status']), residual=_dptr(res['residual']),
                          **{name: _dptr(a) for name, a in res.items() if name in FIELDS})
        self._call('solve', view, p, o)
        return res


def apparent(raw, kin, coupling, rf=1.0):
    """The derivative of the wall fluxes of the COUPLED electrode (kinetics plus mass transport) from the intrinsic one, per point on the
    host: raw [n][P][N] = d flux_k / dp at a fixed surface state; kin 'dflux_dc' [n][N][N] (K_c), 'dflux_dphi' [n][N][2] (its column
    d/d phi_0: K_phi); coupling 'T_c' [n][N][N] = d c_k(0) / d g_j, 'T_phi' [n][N] = d phi(0) / d g_j with g the flux the transport is
    given.  M = I - rf (K_c T_c + K_phi (x) T_phi) is the matrix of include/catint_couple.h; returns M^-1 (rf raw) [n][P][N], the
    derivative of g.  A singular M gives NaN for the point."""
    raw = np.asarray(raw, float)
    n, P, N = raw.shape
    Kc = np.asarray(kin['dflux_dc'], float).reshape(n, N, N)
    Kphi = np.asarray(kin['dflux_dphi'], float).reshape(n, N, 2)[:, :, 1]
    Tc = np.asarray(coupling['T_c'], float).reshape(n, N, N)
    Tphi = np.asarray(coupling['T_phi'], float).reshape(n, N)
    out = np.full((n, P, N), np.nan)
    for i in range(n):
        M = np.eye(N) - rf * (Kc[i] @ Tc[i] + np.outer(Kphi[i], Tphi[i]))
        if not (np.isfinite(M).all() and np.isfinite(raw[i]).all()):
            continue
        try:
            with np.errstate(all='ignore'):
                x = np.linalg.solve(M, rf * raw[i].T).T
        except np.linalg.LinAlgError:
            continue
        if np.isfinite(x).all():
            out[i] = x
    return out


def normalised(dflux, flux, nu):
    """dflux [n][P][N] / flux [n][N], exactly 0 for a species whose column of nu is all zero"""
    idle = ~(np.asarray(nu, float).reshape(-1, flux.shape[1]) != 0.0).any(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        out = np.asarray(dflux, float) / np.asarray(flux, float)[:, None, :]
    out[:, :, idle] = 0.0
    return out
