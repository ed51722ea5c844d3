"""ctypes binding of ``include/catint_balance.h``: species fluxes, reaction rates, wall terms and the discrete mass balance of the
physical mode derived on the device (``catint_amd/lib/libcatint_balance.so``, built by ``catint_amd.build.build_balance_library()``).
No fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _devlib
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _PD, _PI, _PL, _dptr, _f64, _iptr  # noqa: F401  (part of this module's interface)
from ._medium import Medium, reaction_table  # noqa: F401  (the same)

LIB_PATH = _devlib.lib_path('balance')

# every symbol include/catint_balance.h declares (tests/test_balance_abi.py)
SYMBOLS = _devlib.symbols('catbal_', 'species')

MAX_SPECIES, MAX_NX = 8, 4098
MAX_REACTIONS, MAX_REACTANTS, MAX_WALL_REACTIONS = 16, 4, 8          # PNP_MAX_* of catint_pnp.h
SCALARS = ('wall_flux', 'bulk_flux', 'source_integral', 'defect', 'max_imbalance_rel', 'inventory')
NSCALARS = len(SCALARS)
# output rows: name -> shape of one operating point's part from (N, nx, R = nreactions, W = n_wall)
FIELDS = {'flux': lambda N, nx, R, W: (N, nx - 1), 'reaction_rate': lambda N, nx, R, W: (R, nx), 'source': lambda N, nx, R, W: (N, nx),
          'wall_rate': lambda N, nx, R, W: (W,), 'wall_flux': lambda N, nx, R, W: (N,), 'imbalance': lambda N, nx, R, W: (N, nx)}


class BalanceError(_devlib.LibraryError):
    library = 'catint_balance'


class CatbalParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('nreactions', C.c_int32), ('n_wall', C.c_int32),
                ('D', _PD), ('charges', _PD), ('mpb_radius', _PD), ('x', _PD), ('beta', C.c_double), ('velocity', C.c_double),
                ('n_lhs', _PI), ('lhs', _PI), ('n_rhs', _PI), ('rhs', _PI), ('kf', _PD), ('kr', _PD),
                ('species', _PI), ('nu', _PD), ('k', _PD), ('alpha', _PD), ('saturation', _PD), ('flux', _PD), ('phiM', _PD)]


class CatbalOutputs(C.Structure):
    _fields_ = [(n, _PD) for n in tuple(FIELDS) + ('scalars',)]


load_library = _devlib.loader(globals(), 'catbal_', 'species', CatbalParams, CatbalOutputs, BalanceError)


class Balancer(_devlib.Handle):
    """One ``catbal_ctx``.  No device call is made before the first ``species`` that passes validation."""
    _prefix, _error, _load = 'catbal_', BalanceError, staticmethod(load_library)

    def species(self, view, D, charges, x, beta, flux, phiM, mpb_radius=None, velocity=0.0, reactions=(), wall=None, fields=None,
                scalars=True, max_waves=0, struct_size=None):
        """catbal_species on the state behind `view` (a PnpDeviceView).  reactions: [(lhs indices, rhs indices, kf, kr)]; wall: None or
        a dict {'species' [n], 'nu' [n][N], 'k' [B][n], 'alpha' [n] or None, 'saturation' [n] or None}; flux [B][N], phiM [B].
        fields: names out of FIELDS (None: all); returns a dict of the requested rows and, with scalars, 'scalars' [B][N][NSCALARS]
        (columns: SCALARS)."""
        names = _devlib.field_names(fields, FIELDS)
        medium = Medium(view, D, charges, x, beta, mpb_radius, velocity, reactions, max_waves=max_waves, wall=wall)
        B, N, nx = medium.dims
        g, pm = _f64(flux), _f64(phiM)
        medium.check('the view needs', [('flux', g, B * N), ('phiM', pm, B)])
        members = dict(medium.members)
        members['species'] = members.pop('wall_species')          # (catbal_params has no other `species`)
        p = CatbalParams(struct_size=_devlib.size_of(CatbalParams, struct_size), flux=_dptr(g), phiM=_dptr(pm), **members)
        dims = (N, nx, members['nreactions'], members['n_wall'])
        out = _devlib.results(None, {n: tuple(max(d, 0) for d in FIELDS[n](*dims)) for n in names}, (B,))
        if scalars:
            out['scalars'] = np.empty((B, N, NSCALARS))
        o = CatbalOutputs(**{n: _dptr(a) for n, a in out.items()})
        self._call('species', view, p, o)
        return out
