"""ctypes binding of ``include/catint_couple.h``: one Newton step of the self-consistency between electrode kinetics and electrolyte
transport per operating point -- the transport tangent d(surface state) / d(wall flux) from one block elimination, the Newton matrix,
the damped step -- formed on the device (``catint_amd/lib/libcatint_couple.so``, built by ``catint_amd.build.build_couple_library()``).
No fallback: a missing library raises."""
import ctypes as C

from . import _devlib
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _PD, _PI, _PL, _dptr, _f64, _iptr  # noqa: F401  (part of this module's interface)
from ._medium import WALL, Medium, reaction_table  # noqa: F401  (the same)

LIB_PATH = _devlib.lib_path('couple')

# every symbol include/catint_couple.h declares (tests/test_couple_abi.py)
SYMBOLS = _devlib.symbols('catcpl_', 'solve')

MAX_SPECIES, MAX_NX = 8, 4098
PIVOT_GROWTH_LIMIT, SINGULAR = 1e8, 1e-12
OK, PIVOT, UNSOLVED, SINGULAR_A = 0, 1, 2, 3
# output rows: name -> shape of one operating point from N
FIELDS = {'T_c': lambda N: (N, N), 'T_phi': lambda N: (N,), 'dflux': lambda N: (N,), 'lambda': lambda N: (), 'flux_new': lambda N: (N,),
          'dc_surface': lambda N: (N,), 'dphi_surface': lambda N: ()}


class CoupleError(_devlib.LibraryError):
    library = 'catint_couple'


class CatcplParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('wall_bc', C.c_int32), ('nreactions', C.c_int32),
                ('nlanes', C.c_int64), ('lanes', _PL), ('D', _PD), ('charges', _PD), ('mpb_radius', _PD), ('x', _PD),
                ('beta', C.c_double), ('eps', C.c_double), ('dx', C.c_double), ('velocity', C.c_double), ('stern_capacitance', C.c_double),
                ('n_lhs', _PI), ('lhs', _PI), ('n_rhs', _PI), ('rhs', _PI), ('kf', _PD), ('kr', _PD),
                ('rf', C.c_double), ('dphi_max', C.c_double), ('flux', _PD), ('K', _PD), ('Kc', _PD), ('Kphi', _PD)]


class CatcplOutputs(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('T_c', _PD), ('T_phi', _PD), ('dflux', _PD), ('lambda', _PD),
                ('flux_new', _PD), ('dc_surface', _PD), ('dphi_surface', _PD), ('status', _PI)]


load_library = _devlib.loader(globals(), 'catcpl_', 'solve', CatcplParams, CatcplOutputs, CoupleError)


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
        names = _devlib.field_names(fields, FIELDS)
        medium = Medium(view, D, charges, x, beta, mpb_radius, velocity, reactions, eps=eps, dx=dx, wall_bc=wall_bc,
                        stern_capacitance=stern_capacitance, max_waves=max_waves, lanes=lanes)
        N = medium.dims[1]
        g, k, kc, kp = (_f64(a) for a in (flux, K, Kc, Kphi))
        if medium.idx is None:
            medium.rows(0 if g is None else g.size // max(N, 1))
        n = medium.n
        medium.check('the call needs', [('flux', g, n * N), ('K', k, n * N), ('Kc', kc, n * N * N), ('Kphi', kp, n * N)])
        p = CatcplParams(struct_size=_devlib.size_of(CatcplParams, struct_size), rf=float(rf), dphi_max=float(dphi_max), flux=_dptr(g),
                         K=_dptr(k), Kc=_dptr(kc), Kphi=_dptr(kp), **medium.members)
        res = _devlib.results(out, {name: FIELDS[name](N) for name in names}, (n,), status=n)
        o = CatcplOutputs(struct_size=_devlib.size_of(CatcplOutputs, out_struct_size), status=_iptr(res['status']),
                          **{name: _dptr(a) for name, a in res.items() if name in FIELDS})
        self._call('solve', view, p, o)
        return res
