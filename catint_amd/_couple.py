"""ctypes binding of ``include/catint_couple.h``: one Newton step of the self-consistency between electrode kinetics and electrolyte
transport per operating point -- the transport tangent d(surface state) / d(wall flux) from one block elimination, the Newton matrix,
the damped step -- formed on the device (``catint_amd/lib/libcatint_couple.so``, built by ``catint_amd.build.build_couple_library()``).
No fallback: a missing library raises."""
import ctypes as C
import os

import numpy as np

from . import _devlib
from ._capi import flatten_reactions as reaction_table      # the arrays of pnp_set_reactions: catcpl_params takes the same form
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _dptr  # noqa: F401  (part of this module's interface)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CATINT_COUPLE_LIB') or os.path.join(_HERE, 'lib', 'libcatint_couple.so')

# every symbol include/catint_couple.h declares (tests/test_couple_abi.py)
SYMBOLS = _devlib.symbols('catcpl_', 'solve')

MAX_SPECIES, MAX_NX = 8, 4098
PIVOT_GROWTH_LIMIT, SINGULAR = 1e8, 1e-12
WALL = {'dirichlet': 0, 'stern': 1}
OK, PIVOT, UNSOLVED, SINGULAR_A = 0, 1, 2, 3
# output rows: name -> shape of one operating point from N
FIELDS = {'T_c': lambda N: (N, N), 'T_phi': lambda N: (N,), 'dflux': lambda N: (N,), 'lambda': lambda N: (), 'flux_new': lambda N: (N,),
          'dc_surface': lambda N: (N,), 'dphi_surface': lambda N: ()}


class CoupleError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('catint_couple error %d: %s' % (code, msg))
        self.code = code


_PD, _PI, _PL = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


class CatcplParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('wall_bc', C.c_int32), ('nreactions', C.c_int32),
                ('nlanes', C.c_int64), ('lanes', _PL), ('D', _PD), ('charges', _PD), ('mpb_radius', _PD), ('x', _PD),
                ('beta', C.c_double), ('eps', C.c_double), ('dx', C.c_double), ('velocity', C.c_double), ('stern_capacitance', C.c_double),
                ('n_lhs', _PI), ('lhs', _PI), ('n_rhs', _PI), ('rhs', _PI), ('kf', _PD), ('kr', _PD),
                ('rf', C.c_double), ('dphi_max', C.c_double), ('flux', _PD), ('K', _PD), ('Kc', _PD), ('Kphi', _PD)]


class CatcplOutputs(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('T_c', _PD), ('T_phi', _PD), ('dflux', _PD), ('lambda', _PD),
                ('flux_new', _PD), ('dc_surface', _PD), ('dphi_surface', _PD), ('status', _PI)]


_lib = None


def load_library():
    global _lib
    if _lib is None:
        _lib = _devlib.load(LIB_PATH, 'catcpl_', 'solve', CatcplParams, CatcplOutputs, CoupleError)
    return _lib


def _iptr(a):
    return a.ctypes.data_as(_PI) if a is not None else None


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


class Coupler(_devlib.Handle):
    """One ``catcpl_ctx``.  No device call is made before the first ``solve`` that passes validation with at least one lane."""
    _prefix, _error, _load = 'catcpl_', CoupleError, staticmethod(load_library)

    def solve(self, view, D, charges, x, beta, eps, dx, flux, K, Kc, Kphi, rf=1.0, dphi_max=0.05, lanes=None, mpb_radius=None,
              wall_bc='dirichlet', stern_capacitance=0.0, velocity=0.0, reactions=(), fields=None, max_waves=0, struct_size=None,
              out_struct_size=None, out=None):
        """catcpl_solve about the state behind `view` (a PnpDeviceView).  lanes: indices into the batch (None: 0 .. n-1; repeats
        allowed); flux, K, Kphi [n][N] and Kc [n][N][N] are indexed by the position in the call, n = len(lanes) (None: the number of
        rows of flux); reactions: [(lhs indices, rhs indices, kf, kr)].  fields: names out of FIELDS (None: all).  Returns a dict of
        float64 arrays [n]... and 'status' [n] (int32).  out: arrays to write into instead of fresh ones (tests)."""
        N = max(int(view.nspecies), 0)
        names = list(FIELDS) if fields is None else list(fields)
        for nm in names:
            if nm not in FIELDS:
                raise ValueError('unknown field %r (known: %s)' % (nm, ', '.join(FIELDS)))
        R, n_lhs, lhs, n_rhs, rhs, kf, kr = reaction_table(list(reactions))
        keep = [_f64(a) for a in (D, charges, x, mpb_radius)]
        idx = None if lanes is None else np.ascontiguousarray(lanes, dtype=np.int64).reshape(-1)
        g, k, kc, kp = (_f64(a) for a in (flux, K, Kc, Kphi))
        n = len(idx) if idx is not None else (0 if g is None else g.size // max(N, 1))
        for name, a, size in (('flux', g, n * N), ('K', k, n * N), ('Kc', kc, n * N * N), ('Kphi', kp, n * N), ('mpb_radius', keep[3], N)):
            if a is not None and a.size != size:
                raise ValueError('%s has %d values, the call needs %d' % (name, a.size, size))
        if keep[0].size < N or keep[1].size < N or keep[2].size < max(int(view.nx), 0):
            raise ValueError('D, charges or x shorter than the view')
        p = CatcplParams(C.sizeof(CatcplParams) if struct_size is None else int(struct_size), int(max_waves),
                         wall_bc if isinstance(wall_bc, int) else WALL[wall_bc], R, n, None if idx is None else idx.ctypes.data_as(_PL),
                         _dptr(keep[0]), _dptr(keep[1]), _dptr(keep[3]), _dptr(keep[2]), float(beta), float(eps), float(dx), float(velocity),
                         float(stern_capacitance), _iptr(n_lhs), _iptr(lhs), _iptr(n_rhs), _iptr(rhs), _dptr(kf), _dptr(kr), float(rf),
                         float(dphi_max), _dptr(g), _dptr(k), _dptr(kc), _dptr(kp))
        res = {} if out is None else out
        for name in names:
            res.setdefault(name, np.empty((n,) + FIELDS[name](N)))
        res.setdefault('status', np.zeros(n, np.int32))
        o = CatcplOutputs(struct_size=C.sizeof(CatcplOutputs) if out_struct_size is None else int(out_struct_size),
                          status=_iptr(res['status']), **{name: _dptr(a) for name, a in res.items() if name in FIELDS})
        self._call('solve', view, p, o)
        return res
