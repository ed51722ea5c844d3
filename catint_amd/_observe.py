"""ctypes binding of ``include/catint_observe.h``: electrolyte observables of the physical mode derived on the device
(``catint_amd/lib/libcatint_observe.so``, built by ``catint_amd.build.build_observe_library()``).  No fallback: a missing library raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CATINT_OBSERVE_LIB') or os.path.join(_HERE, 'lib', 'libcatint_observe.so')

# every symbol include/catint_observe.h declares (tests/test_observe_abi.py)
SYMBOLS = ['catobs_create', 'catobs_destroy', 'catobs_last_error', 'catobs_last_kernel', 'catobs_last_kernel_ms', 'catobs_electrolyte']

EINVAL, ENOMEM, EDEVICE = -1, -2, -3
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


class PnpDeviceView(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('method', C.c_int32), ('nspecies', C.c_int32), ('nx', C.c_int32), ('row_pitch', C.c_int32),
                ('reserved', C.c_int32), ('batch', C.c_int64), ('c_dev', C.c_void_p), ('phi_dev', C.c_void_p), ('status_dev', C.c_void_p),
                ('stream', C.c_void_p)]


class CatobsParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('species_H', C.c_int32), ('species_OH', C.c_int32), ('max_waves', C.c_int32),
                ('D', C.POINTER(C.c_double)), ('charges', C.POINTER(C.c_double)), ('mpb_radius', C.POINTER(C.c_double)),
                ('x', C.POINTER(C.c_double)), ('beta', C.c_double), ('velocity', C.c_double)]


class CatobsOutputs(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_double)) for n in tuple(FIELDS) + ('scalars',)]


_lib = None


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ObserveError(EDEVICE, 'HIP extension %s is missing: run `python -c "import __graft_entry__ as g; g.build()"`' % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    lib.catobs_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
    lib.catobs_create.restype = C.c_int
    lib.catobs_destroy.argtypes = [C.c_void_p]
    lib.catobs_destroy.restype = None
    lib.catobs_last_error.argtypes = [C.c_void_p]
    lib.catobs_last_error.restype = C.c_char_p
    lib.catobs_last_kernel.argtypes = [C.c_void_p]
    lib.catobs_last_kernel.restype = C.c_char_p
    lib.catobs_last_kernel_ms.argtypes = [C.c_void_p]
    lib.catobs_last_kernel_ms.restype = C.c_float
    lib.catobs_electrolyte.argtypes = [C.c_void_p, C.POINTER(PnpDeviceView), C.POINTER(CatobsParams), C.POINTER(CatobsOutputs)]
    lib.catobs_electrolyte.restype = C.c_int
    _lib = lib
    return lib


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


class Observer(object):
    """One ``catobs_ctx``.  No device call is made before the first ``electrolyte`` that passes validation."""

    def __init__(self, device=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        rc = self._lib.catobs_create(int(device), C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise ObserveError(rc, self._lib.catobs_last_error(None).decode())

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self._lib.catobs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def last_kernel(self):
        return self._lib.catobs_last_kernel(self._h).decode()

    @property
    def last_kernel_ms(self):
        """Device time of the last call's kernel alone, without the copies (HIP events), in ms"""
        return float(self._lib.catobs_last_kernel_ms(self._h))

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
        rc = self._lib.catobs_electrolyte(self._h, C.byref(view), C.byref(p), C.byref(o))
        if rc != 0:
            raise ObserveError(rc, self._lib.catobs_last_error(self._h).decode())
        return out
