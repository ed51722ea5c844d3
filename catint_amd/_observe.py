"""ctypes binding of ``include/catint_observe.h``: electrolyte observables of the physical mode derived on the device
(``catint_amd/lib/libcatint_observe.so``, built by ``catint_amd.build.build_observe_library()``).  No fallback: a missing library raises."""
import ctypes as C
import os

import numpy as np

from . import _devlib
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _dptr  # noqa: F401  (part of this module's interface)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CATINT_OBSERVE_LIB') or os.path.join(_HERE, 'lib', 'libcatint_observe.so')

# every symbol include/catint_observe.h declares (tests/test_observe_abi.py)
SYMBOLS = _devlib.symbols('catobs_', 'electrolyte')

MAX_SPECIES, MAX_NX = 8, 4098
SCALARS = ('surface_potential', 'surface_efield', 'surface_activity_coefficient', 'surface_pH', 'delta_phi_iR_inf', 'delta_phi_diff_inf',
           'delta_phi_inf', 'delta_phi_inf_min_iR', 'wall_current_density', 'bulk_conductivity')
NSCALARS = len(SCALARS)
# output rows: name -> length of a row relative to nx
FIELDS = {'efield': 0, 'charge_density': 0, 'gamma': 0, 'pH': 0, 'conductivity': -1, 'current_density': -1, 'dphi_iR': 0, 'dphi_diff': 0}


class ObserveError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('catint_observe error %d: %s' % (code, msg))
        self.code = code


class CatobsParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('species_H', C.c_int32), ('species_OH', C.c_int32), ('max_waves', C.c_int32),
                ('D', C.POINTER(C.c_double)), ('charges', C.POINTER(C.c_double)), ('mpb_radius', C.POINTER(C.c_double)),
                ('x', C.POINTER(C.c_double)), ('beta', C.c_double), ('velocity', C.c_double)]


class CatobsOutputs(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_double)) for n in tuple(FIELDS) + ('scalars',)]


_lib = None


def load_library():
    global _lib
    if _lib is None:
        _lib = _devlib.load(LIB_PATH, 'catobs_', 'electrolyte', CatobsParams, CatobsOutputs, ObserveError)
    return _lib


class Observer(_devlib.Handle):
    """One ``catobs_ctx``.  No device call is made before the first ``electrolyte`` that passes validation."""
    _prefix, _error, _load = 'catobs_', ObserveError, staticmethod(load_library)

    def electrolyte(self, view, D, charges, x, beta, mpb_radius=None, velocity=0.0, species_H=-1, species_OH=-1, fields=None,
                    scalars=True, max_waves=0, struct_size=None):
        """catobs_electrolyte on the state behind `view` (a PnpDeviceView).  fields: names out of FIELDS (None: all); returns a dict
        of the requested rows ([B][nx] or [B][nx-1]) and, with scalars, 'scalars' [B][NSCALARS] (columns: SCALARS)."""
        B, nx = int(view.batch), int(view.nx)
        names = list(FIELDS) if fields is None else list(fields)
        for n in names:
            if n not in FIELDS:
                raise ValueError('unknown field %r (known: %s)' % (n, ', '.join(FIELDS)))
        keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (D, charges, x)]
        rad = None if mpb_radius is None else np.ascontiguousarray(mpb_radius, dtype=np.float64)
        p = CatobsParams(C.sizeof(CatobsParams) if struct_size is None else int(struct_size), int(species_H), int(species_OH), int(max_waves),
                         _dptr(keep[0]), _dptr(keep[1]), _dptr(rad), _dptr(keep[2]), float(beta), float(velocity))
        out = {n: np.empty((max(B, 0), max(nx + FIELDS[n], 0))) for n in names}
        if scalars:
            out['scalars'] = np.empty((max(B, 0), NSCALARS))
        o = CatobsOutputs(**{n: _dptr(a) for n, a in out.items()})
        self._call('electrolyte', view, p, o)
        return out
