"""ctypes binding of ``include/catint_equil.h``: the zero-flux state of the physical mode solved on the device as a discrete size-modified
Poisson-Boltzmann problem (``catint_amd/lib/libcatint_equil.so``, built by ``catint_amd.build.build_equil_library()``).
No fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _devlib
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _PD, _PI, _PL, _dptr, _f64, _iptr  # noqa: F401  (part of this module's interface)
from ._medium import WALL  # noqa: F401  (the same)

LIB_PATH = _devlib.lib_path('equil')

# every symbol include/catint_equil.h declares (tests/test_equil_abi.py)
SYMBOLS = _devlib.symbols('cateq_', 'solve')

MAX_SPECIES, MAX_NX, MAX_EXPONENT, MAX_ITERATIONS = 8, 4098, 500.0, 1000


class EquilError(_devlib.LibraryError):
    library = 'catint_equil'


class CateqParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('charges', _PD), ('mpb_radius', _PD), ('x', _PD),
                ('beta', C.c_double), ('eps', C.c_double), ('dx', C.c_double), ('wall_bc', C.c_int32), ('maxit', C.c_int32),
                ('stern_capacitance', C.c_double), ('phi_pzc', C.c_double), ('tol', C.c_double), ('phiM', _PD), ('phi_bulk', _PD),
                ('c_bulk', _PD), ('nlanes', C.c_int64)]


class CateqOutputs(C.Structure):
    _fields_ = [('c', _PD), ('phi', _PD), ('status', _PI), ('iterations', _PI), ('c_dev', C.POINTER(C.c_void_p)),
                ('phi_dev', C.POINTER(C.c_void_p))]


load_library = _devlib.loader(globals(), 'cateq_', 'solve', CateqParams, CateqOutputs, EquilError)


class Equilibrator(_devlib.Handle):
    """One ``cateq_ctx``.  No device call is made before the first ``solve`` that passes validation."""
    _prefix, _error, _load = 'cateq_', EquilError, staticmethod(load_library)

    def solve(self, view, charges, x, beta, eps, dx, phiM, phi_bulk, c_bulk, mpb_radius=None, wall_bc='dirichlet', stern_capacitance=0.0,
              phi_pzc=0.0, tol=1e-10, maxit=100, to_host=True, device=False, max_waves=0, struct_size=None):
        """cateq_solve on the grid x of the handle behind `view` (a PnpDeviceView): one operating point per entry of phiM [n], with
        phi_bulk [n] and c_bulk [n][N].  Returns a dict with 'status' and 'iterations' [n]; with to_host 'c' [n][N][nx] and 'phi'
        [n][nx]; with device 'c_dev' and 'phi_dev', the integer device addresses of [n][N][pitch] and [n][pitch] (the view's row
        pitch, pads zero), valid until the next call on this context or its close."""
        N, nx = max(int(view.nspecies), 0), max(int(view.nx), 0)
        keep = [_f64(a) for a in (charges, x, mpb_radius)]
        if keep[0].size < N or keep[1].size < nx:
            raise ValueError('charges or x shorter than the view')
        if keep[2] is not None and keep[2].size != N:
            raise ValueError('mpb_radius has %d values, the view needs %d' % (keep[2].size, N))
        pm = _f64(phiM).reshape(-1)
        n = len(pm)
        pbk = np.ascontiguousarray(np.broadcast_to(_f64(phi_bulk), (n,)))
        cb = np.ascontiguousarray(np.broadcast_to(_f64(c_bulk), (n, N)))
        p = CateqParams(struct_size=_devlib.size_of(CateqParams, struct_size), max_waves=int(max_waves), charges=_dptr(keep[0]),
                        mpb_radius=_dptr(keep[2]), x=_dptr(keep[1]), beta=float(beta), eps=float(eps), dx=float(dx),
                        wall_bc=wall_bc if isinstance(wall_bc, int) else WALL[wall_bc], maxit=int(maxit),
                        stern_capacitance=float(stern_capacitance), phi_pzc=float(phi_pzc), tol=float(tol), phiM=_dptr(pm), phi_bulk=_dptr(pbk),
                        c_bulk=_dptr(cb), nlanes=n)
        out = {'status': np.zeros(n, np.int32), 'iterations': np.zeros(n, np.int32)}
        if to_host:
            out['c'], out['phi'] = np.empty((n, N, nx)), np.empty((n, nx))
        cd, pd = C.c_void_p(), C.c_void_p()
        o = CateqOutputs(_dptr(out.get('c')), _dptr(out.get('phi')), out['status'].ctypes.data_as(_PI), out['iterations'].ctypes.data_as(_PI),
                         C.pointer(cd) if device else None, C.pointer(pd) if device else None)
        self._call('solve', view, p, o)
        if device:
            out['c_dev'], out['phi_dev'] = cd.value, pd.value
        return out
