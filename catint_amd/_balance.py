"""ctypes binding of ``include/catint_balance.h``: species fluxes, reaction rates, wall terms and the discrete mass balance of the
physical mode derived on the device (``catint_amd/lib/libcatint_balance.so``, built by ``catint_amd.build.build_balance_library()``).
No fallback: a missing library raises."""
import ctypes as C
import os

import numpy as np

from . import _devlib
from ._capi import flatten_reactions as reaction_table      # the arrays of pnp_set_reactions: catbal_params takes the same form
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _dptr  # noqa: F401  (part of this module's interface)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CATINT_BALANCE_LIB') or os.path.join(_HERE, 'lib', 'libcatint_balance.so')

# every symbol include/catint_balance.h declares (tests/test_balance_abi.py)
SYMBOLS = _devlib.symbols('catbal_', 'species')

MAX_SPECIES, MAX_NX = 8, 4098
MAX_REACTIONS, MAX_REACTANTS, MAX_WALL_REACTIONS = 16, 4, 8          # PNP_MAX_* of catint_pnp.h
SCALARS = ('wall_flux', 'bulk_flux', 'source_integral', 'defect', 'max_imbalance_rel', 'inventory')
NSCALARS = len(SCALARS)
# output rows: name -> shape of one operating point's part from (N, nx, R = nreactions, W = n_wall)
FIELDS = {'flux': lambda N, nx, R, W: (N, nx - 1), 'reaction_rate': lambda N, nx, R, W: (R, nx), 'source': lambda N, nx, R, W: (N, nx),
          'wall_rate': lambda N, nx, R, W: (W,), 'wall_flux': lambda N, nx, R, W: (N,), 'imbalance': lambda N, nx, R, W: (N, nx)}


class BalanceError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('catint_balance error %d: %s' % (code, msg))
        self.code = code


_PD, _PI = C.POINTER(C.c_double), C.POINTER(C.c_int32)


class CatbalParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('nreactions', C.c_int32), ('n_wall', C.c_int32),
                ('D', _PD), ('charges', _PD), ('mpb_radius', _PD), ('x', _PD), ('beta', C.c_double), ('velocity', C.c_double),
                ('n_lhs', _PI), ('lhs', _PI), ('n_rhs', _PI), ('rhs', _PI), ('kf', _PD), ('kr', _PD),
                ('species', _PI), ('nu', _PD), ('k', _PD), ('alpha', _PD), ('saturation', _PD), ('flux', _PD), ('phiM', _PD)]


class CatbalOutputs(C.Structure):
    _fields_ = [(n, _PD) for n in tuple(FIELDS) + ('scalars',)]


_lib = None


def load_library():
    global _lib
    if _lib is None:
        _lib = _devlib.load(LIB_PATH, 'catbal_', 'species', CatbalParams, CatbalOutputs, BalanceError)
    return _lib


def _iptr(a):
    return a.ctypes.data_as(_PI) if a is not None else None


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


class Balancer(_devlib.Handle):
    """One ``catbal_ctx``.  No device call is made before the first ``species`` that passes validation."""
    _prefix, _error, _load = 'catbal_', BalanceError, staticmethod(load_library)

    def species(self, view, D, charges, x, beta, flux, phiM, mpb_radius=None, velocity=0.0, reactions=(), wall=None, fields=None,
                scalars=True, max_waves=0, struct_size=None):
        """catbal_species on the state behind `view` (a PnpDeviceView).  reactions: [(lhs indices, rhs indices, kf, kr)]; wall: None or
        a dict {'species' [n], 'nu' [n][N], 'k' [B][n], 'alpha' [n] or None, 'saturation' [n] or None}; flux [B][N], phiM [B].
        fields: names out of FIELDS (None: all); returns a dict of the requested rows and, with scalars, 'scalars' [B][N][NSCALARS]
        (columns: SCALARS)."""
        B, N, nx = max(int(view.batch), 0), max(int(view.nspecies), 0), max(int(view.nx), 0)
        names = list(FIELDS) if fields is None else list(fields)
        for n in names:
            if n not in FIELDS:
                raise ValueError('unknown field %r (known: %s)' % (n, ', '.join(FIELDS)))
        R, n_lhs, lhs, n_rhs, rhs, kf, kr = reaction_table(list(reactions))
        W = 0 if not wall else len(wall['species'])
        keep = [_f64(a) for a in (D, charges, x, mpb_radius, flux, phiM)]
        wk = [None] * 5
        if W:
            wk = [np.ascontiguousarray(wall['species'], dtype=np.int32), _f64(wall['nu']), _f64(wall.get('k')), _f64(wall.get('alpha')),
                  _f64(wall.get('saturation'))]
        for name, a, n in (('flux', keep[4], B * N), ('phiM', keep[5], B), ('wall k', wk[2], B * W), ('wall nu', wk[1], W * N),
                           ('wall alpha', wk[3], W), ('wall saturation', wk[4], W), ('mpb_radius', keep[3], N)):
            if a is not None and a.size != n:
                raise ValueError('%s has %d values, the view needs %d' % (name, a.size, n))
        if keep[0].size < N or keep[1].size < N or keep[2].size < nx:
            raise ValueError('D, charges or x shorter than the view')
        p = CatbalParams(C.sizeof(CatbalParams) if struct_size is None else int(struct_size), int(max_waves), R, W,
                         _dptr(keep[0]), _dptr(keep[1]), _dptr(keep[3]), _dptr(keep[2]), float(beta), float(velocity),
                         _iptr(n_lhs), _iptr(lhs), _iptr(n_rhs), _iptr(rhs), _dptr(kf), _dptr(kr),
                         _iptr(wk[0]), _dptr(wk[1]), _dptr(wk[2]), _dptr(wk[3]), _dptr(wk[4]), _dptr(keep[4]), _dptr(keep[5]))
        dims = (N, nx, max(R, 0), max(W, 0))
        out = {n: np.empty((B,) + tuple(max(d, 0) for d in FIELDS[n](*dims))) for n in names}
        if scalars:
            out['scalars'] = np.empty((B, N, NSCALARS))
        o = CatbalOutputs(**{n: _dptr(a) for n, a in out.items()})
        self._call('species', view, p, o)
        return out
