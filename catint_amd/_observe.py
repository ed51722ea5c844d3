"""ctypes binding of ``include/catint_observe.h``: electrolyte observables of the physical mode derived on the device
(``catint_amd/lib/libcatint_observe.so``, built by ``catint_amd.build.build_observe_library()``).  No fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _devlib
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _PD, _PI, _PL, _dptr, _f64, _iptr  # noqa: F401  (part of this module's interface)

LIB_PATH = _devlib.lib_path('observe')

# every symbol include/catint_observe.h declares (tests/test_observe_abi.py)
SYMBOLS = _devlib.symbols('catobs_', 'electrolyte')

MAX_SPECIES, MAX_NX = 8, 4098
SCALARS = ('surface_potential', 'surface_efield', 'surface_activity_coefficient', 'surface_pH', 'delta_phi_iR_inf', 'delta_phi_diff_inf',
           'delta_phi_inf', 'delta_phi_inf_min_iR', 'wall_current_density', 'bulk_conductivity')
NSCALARS = len(SCALARS)
# output rows: name -> length of a row relative to nx
FIELDS = {'efield': 0, 'charge_density': 0, 'gamma': 0, 'pH': 0, 'conductivity': -1, 'current_density': -1, 'dphi_iR': 0, 'dphi_diff': 0}


class ObserveError(_devlib.LibraryError):
    library = 'catint_observe'


class CatobsParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('species_H', C.c_int32), ('species_OH', C.c_int32), ('max_waves', C.c_int32),
                ('D', _PD), ('charges', _PD), ('mpb_radius', _PD),
                ('x', _PD), ('beta', C.c_double), ('velocity', C.c_double)]


class CatobsOutputs(C.Structure):
    _fields_ = [(n, _PD) for n in tuple(FIELDS) + ('scalars',)]


load_library = _devlib.loader(globals(), 'catobs_', 'electrolyte', CatobsParams, CatobsOutputs, ObserveError)


class Observer(_devlib.Handle):
    """One ``catobs_ctx``.  No device call is made before the first ``electrolyte`` that passes validation."""
    _prefix, _error, _load = 'catobs_', ObserveError, staticmethod(load_library)

    def electrolyte(self, view, D, charges, x, beta, mpb_radius=None, velocity=0.0, species_H=-1, species_OH=-1, fields=None,
                    scalars=True, max_waves=0, struct_size=None):
        """catobs_electrolyte on the state behind `view` (a PnpDeviceView).  fields: names out of FIELDS (None: all); returns a dict
        of the requested rows ([B][nx] or [B][nx-1]) and, with scalars, 'scalars' [B][NSCALARS] (columns: SCALARS)."""
        B, nx = int(view.batch), int(view.nx)
        names = _devlib.field_names(fields, FIELDS)
        keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (D, charges, x)]
        rad = _f64(mpb_radius)
        p = CatobsParams(struct_size=_devlib.size_of(CatobsParams, struct_size), species_H=int(species_H), species_OH=int(species_OH),
                         max_waves=int(max_waves), D=_dptr(keep[0]), charges=_dptr(keep[1]), mpb_radius=_dptr(rad), x=_dptr(keep[2]),
                         beta=float(beta), velocity=float(velocity))
        out = {n: np.empty((max(B, 0), max(nx + FIELDS[n], 0))) for n in names}
        if scalars:
            out['scalars'] = np.empty((max(B, 0), NSCALARS))
        o = CatobsOutputs(**{n: _dptr(a) for n, a in out.items()})
        self._call('electrolyte', view, p, o)
        return out
