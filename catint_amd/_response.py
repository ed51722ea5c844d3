"""ctypes binding of ``include/catint_response.h``: the linear response of a stationary state of the physical mode -- differential
capacitance, slope of the currents, admittance spectrum -- solved on the device (``catint_amd/lib/libcatint_response.so``, built by
``catint_amd.build.build_response_library()``).  No fallback: a missing library raises."""
import ctypes as C
import os

import numpy as np

from . import _devlib
from ._capi import flatten_reactions as reaction_table      # the arrays of pnp_set_reactions: catresp_params takes the same form
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _dptr  # noqa: F401  (part of this module's interface)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CATINT_RESPONSE_LIB') or os.path.join(_HERE, 'lib', 'libcatint_response.so')

# every symbol include/catint_response.h declares (tests/test_response_abi.py)
SYMBOLS = _devlib.symbols('catresp_', 'solve')

MAX_SPECIES, MAX_NX, MAX_FREQ = 8, 4098, 256
WALL = {'dirichlet': 0, 'stern': 1}
PHIM, WALL_FLUX = 0, 1
# complex output rows: name -> shape of one (operating point, frequency) from (N, nx)
SCALARS = {'dphi_surface': lambda N, nx: (), 'dc_surface': lambda N, nx: (N,), 'dsigma': lambda N, nx: (), 'dwall_flux': lambda N, nx: (N,),
           'admittance': lambda N, nx: ()}
PROFILES = {'dc': lambda N, nx: (N, nx), 'dphi': lambda N, nx: (nx,)}


class ResponseError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('catint_response error %d: %s' % (code, msg))
        self.code = code


_PD, _PI, _PL = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


class CatrespParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('wall_bc', C.c_int32), ('perturbation', C.c_int32),
                ('species', C.c_int32), ('nfreq', C.c_int32), ('nreactions', C.c_int32), ('n_wall', C.c_int32),
                ('nlanes', C.c_int64), ('lanes', _PL), ('D', _PD), ('charges', _PD), ('mpb_radius', _PD), ('x', _PD),
                ('beta', C.c_double), ('eps', C.c_double), ('dx', C.c_double), ('velocity', C.c_double), ('stern_capacitance', C.c_double),
                ('n_lhs', _PI), ('lhs', _PI), ('n_rhs', _PI), ('rhs', _PI), ('kf', _PD), ('kr', _PD),
                ('wall_species', _PI), ('nu', _PD), ('k', _PD), ('alpha', _PD), ('saturation', _PD), ('phiM', _PD), ('omega', _PD)]


class CatrespOutputs(C.Structure):
    _fields_ = [('dphi_surface', _PD), ('dc_surface', _PD), ('dsigma', _PD), ('dwall_flux', _PD), ('admittance', _PD), ('status', _PI),
                ('dc', _PD), ('dphi', _PD)]


_lib = None


def load_library():
    global _lib
    if _lib is None:
        _lib = _devlib.load(LIB_PATH, 'catresp_', 'solve', CatrespParams, CatrespOutputs, ResponseError)
    return _lib


def _iptr(a):
    return a.ctypes.data_as(_PI) if a is not None else None


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _cptr(a):
    """complex128 array as the (re, im) pairs of doubles the library writes"""
    return a.ctypes.data_as(_PD) if a is not None else None


class Responder(_devlib.Handle):
    """One ``catresp_ctx``.  No device call is made before the first ``solve`` that passes validation with at least one lane."""
    _prefix, _error, _load = 'catresp_', ResponseError, staticmethod(load_library)

    def solve(self, view, D, charges, x, beta, eps, dx, phiM, omega=(0.0,), perturbation='phiM', lanes=None, mpb_radius=None,
              wall_bc='dirichlet', stern_capacitance=0.0, velocity=0.0, reactions=(), wall=None, fields=None, profiles=False,
              max_waves=0, struct_size=None, out=None):
        """catresp_solve about the state behind `view` (a PnpDeviceView).  perturbation: 'phiM' or ('flux', k); lanes: indices into
        the batch (None: all, in order; repeats allowed); omega [F] rad/s; reactions: [(lhs indices, rhs indices, kf, kr)]; wall: None
        or a dict {'species' [n], 'nu' [n][N], 'k' [B][n], 'alpha' [n] or None, 'saturation' [n] or None}; phiM [B].
        fields: names out of SCALARS (None: all); profiles: also 'dc' [n][F][N][nx] and 'dphi' [n][F][nx].  Returns a dict of
        complex128 arrays [n][F]... and 'status' [n][F] (int32).  out: arrays to write into instead of fresh ones (tests)."""
        B, N, nx = max(int(view.batch), 0), max(int(view.nspecies), 0), max(int(view.nx), 0)
        names = list(SCALARS) if fields is None else list(fields)
        for n in names:
            if n not in SCALARS:
                raise ValueError('unknown field %r (known: %s)' % (n, ', '.join(SCALARS)))
        if isinstance(perturbation, str):
            if perturbation != 'phiM':
                raise ValueError("perturbation is 'phiM' or ('flux', k)")
            pert, sp = PHIM, 0
        elif isinstance(perturbation, int):
            pert, sp = int(perturbation), 0          # (raw code: the library validates it)
        else:
            if perturbation[0] != 'flux':
                raise ValueError("perturbation is 'phiM' or ('flux', k)")
            pert, sp = WALL_FLUX, int(perturbation[1])
        R, n_lhs, lhs, n_rhs, rhs, kf, kr = reaction_table(list(reactions))
        W = 0 if not wall else len(wall['species'])
        keep = [_f64(a) for a in (D, charges, x, mpb_radius, phiM)]
        om = _f64(np.atleast_1d(np.asarray(omega, float)).reshape(-1))
        F = len(om)
        wk = [None] * 5
        if W:
            wk = [np.ascontiguousarray(wall['species'], dtype=np.int32), _f64(wall['nu']), _f64(wall.get('k')), _f64(wall.get('alpha')),
                  _f64(wall.get('saturation'))]
        for name, a, n in (('phiM', keep[4], B), ('wall k', wk[2], B * W), ('wall nu', wk[1], W * N), ('wall alpha', wk[3], W),
                           ('wall saturation', wk[4], W), ('mpb_radius', keep[3], N)):
            if a is not None and a.size != n:
                raise ValueError('%s has %d values, the view needs %d' % (name, a.size, n))
        if keep[0].size < N or keep[1].size < N or keep[2].size < nx:
            raise ValueError('D, charges or x shorter than the view')
        idx = None if lanes is None else np.ascontiguousarray(lanes, dtype=np.int64).reshape(-1)
        n = B if idx is None else len(idx)
        p = CatrespParams(C.sizeof(CatrespParams) if struct_size is None else int(struct_size), int(max_waves),
                          wall_bc if isinstance(wall_bc, int) else WALL[wall_bc], pert, sp, F, R, W, n,
                          None if idx is None else idx.ctypes.data_as(_PL), _dptr(keep[0]), _dptr(keep[1]), _dptr(keep[3]), _dptr(keep[2]),
                          float(beta), float(eps), float(dx), float(velocity), float(stern_capacitance),
                          _iptr(n_lhs), _iptr(lhs), _iptr(n_rhs), _iptr(rhs), _dptr(kf), _dptr(kr),
                          _iptr(wk[0]), _dptr(wk[1]), _dptr(wk[2]), _dptr(wk[3]), _dptr(wk[4]), _dptr(keep[4]), _dptr(om))
        Fs = max(F, 0)
        res = {} if out is None else out
        for name in names:
            res.setdefault(name, np.empty((n, Fs) + SCALARS[name](N, nx), np.complex128))
        if profiles:
            for name in PROFILES:
                res.setdefault(name, np.empty((n, Fs) + PROFILES[name](N, nx), np.complex128))
        res.setdefault('status', np.zeros((n, Fs), np.int32))
        o = CatrespOutputs(status=_iptr(res['status']), **{name: _cptr(a) for name, a in res.items() if name != 'status'})
        self._call('solve', view, p, o)
        return res
