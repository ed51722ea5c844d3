"""ctypes binding of ``include/catint_regrid.h``: a device-resident state of the physical mode resampled onto another grid with the
Scharfetter-Gummel interpolant (``catint_amd/lib/libcatint_regrid.so``, built by ``catint_amd.build.build_regrid_library()``).
No fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _devlib
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _PD, _PI, _PL, _dptr, _f64, _iptr  # noqa: F401  (part of this module's interface)

LIB_PATH = _devlib.lib_path('regrid')

# every symbol include/catint_regrid.h declares (tests/test_regrid_abi.py)
SYMBOLS = _devlib.symbols('catgrid_', 'resample')

MAX_SPECIES, MAX_NX, MAX_U = 8, 4098, 500.0


class RegridError(_devlib.LibraryError):
    library = 'catint_regrid'


class CatgridParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('D', _PD), ('charges', _PD), ('mpb_radius', _PD),
                ('beta', C.c_double), ('velocity', C.c_double), ('x', _PD), ('nx_target', C.c_int32), ('reserved', C.c_int32),
                ('x_target', _PD), ('nlanes', C.c_int64), ('lanes', _PL)]


class CatgridOutputs(C.Structure):
    _fields_ = [('c', _PD), ('phi', _PD), ('c_dev', C.POINTER(C.c_void_p)), ('phi_dev', C.POINTER(C.c_void_p))]


load_library = _devlib.loader(globals(), 'catgrid_', 'resample', CatgridParams, CatgridOutputs, RegridError)


def row_pitch(nx):
    """Row pitch (doubles) of a handle of nx points, and of the device result of a resample onto such a grid"""
    return (int(nx) + 15) // 16 * 16


class Regridder(_devlib.Handle):
    """One ``catgrid_ctx``.  No device call is made before the first ``resample`` that passes validation."""
    _prefix, _error, _load = 'catgrid_', RegridError, staticmethod(load_library)

    def resample(self, view, D, charges, x, beta, x_target, mpb_radius=None, velocity=0.0, lanes=None, to_host=True, device=False,
                 max_waves=0, struct_size=None):
        """catgrid_resample of the state behind `view` (a PnpDeviceView) from the grid x onto x_target; lanes: source operating
        points in the order wanted (None: all).  Returns a dict: with to_host 'c' [n][N][nx_target] and 'phi' [n][nx_target]; with
        device 'c_dev' and 'phi_dev', the integer device addresses of [n][N][pitch] and [n][pitch] (pitch = row_pitch(nx_target)),
        valid until the next call on this context or its close."""
        B, N, nx = max(int(view.batch), 0), max(int(view.nspecies), 0), max(int(view.nx), 0)
        keep = [_f64(a) for a in (D, charges, x, mpb_radius)]
        xt = _f64(x_target)
        nxt = 0 if xt is None else int(xt.size)
        if keep[0].size < N or keep[1].size < N or keep[2].size < nx:
            raise ValueError('D, charges or x shorter than the view')
        if keep[3] is not None and keep[3].size != N:
            raise ValueError('mpb_radius has %d values, the view needs %d' % (keep[3].size, N))
        idx = _devlib.lane_list(lanes)
        n = B if idx is None else len(idx)
        p = CatgridParams(struct_size=_devlib.size_of(CatgridParams, struct_size), max_waves=int(max_waves), D=_dptr(keep[0]),
                          charges=_dptr(keep[1]), mpb_radius=_dptr(keep[3]), beta=float(beta), velocity=float(velocity), x=_dptr(keep[2]),
                          nx_target=nxt, x_target=_dptr(xt), nlanes=n, lanes=_devlib._lptr(idx))
        out = {}
        if to_host:
            out['c'], out['phi'] = np.empty((n, N, nxt)), np.empty((n, nxt))
        cd, pd = C.c_void_p(), C.c_void_p()
        o = CatgridOutputs(_dptr(out.get('c')), _dptr(out.get('phi')), C.pointer(cd) if device else None, C.pointer(pd) if device else None)
        self._call('resample', view, p, o)
        if device:
            out['c_dev'], out['phi_dev'] = cd.value, pd.value
        return out
