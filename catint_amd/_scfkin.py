"""ctypes binding of ``include/catint_scfkin.h``: the wall fluxes of a mean-field surface microkinetic model inside the device SCF loop
(``catint_amd/lib/libcatint_scfkin.so``, built by ``catint_amd.build.build_scfkin_library()``).  ``ScfKinetics.flux_fn`` and
``ScfKinetics.user`` are the two addresses ``PnpSolver.scf_cycle(..., flux_fn=, user=)`` takes.  No fallback: a missing library raises."""
import ctypes as C
import os

import numpy as np

from . import _devlib, _microkin
from ._devlib import EDEVICE, EINVAL, ENOMEM, _dptr  # noqa: F401  (part of this module's interface)
from ._microkin import DROP, MAX_ADSORBATES, MAX_SPECIES, MAX_STEPS, MIN_LOG, _PD, _PI, _iptr  # noqa: F401  (the same)

LIB_PATH = _devlib.lib_path('scfkin')

# every symbol include/catint_scfkin.h declares (tests/test_scfkin_abi.py)
SYMBOLS = ['catsk_' + n for n in ('create', 'destroy', 'last_error', 'last_kernel', 'begin', 'flux_fn', 'step_host', 'end')]

CONVERGED, MAXIT, INPUT, PIVOT = 0, 1, 2, 3
DEFAULT_TOL, DEFAULT_MAXIT = 1e-12, 200
# what catsk_end reads back: name -> (shape of one lane from (N, S), dtype)
FIELDS = {'theta': (lambda N, S: (S + 1,), np.float64), 'flux_scale': (lambda N, S: (N,), np.float64),
          'flux_last': (lambda N, S: (N,), np.float64), 'status': (lambda N, S: (), np.int32),
          'iterations_last': (lambda N, S: (), np.int32), 'iterations_total': (lambda N, S: (), np.int32),
          'calls': (lambda N, S: (), np.int32)}


class ScfKineticsError(_devlib.LibraryError):
    library = 'catint_scfkin'


class CatskParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('nspecies', C.c_int32), ('nadsorbates', C.c_int32),
                ('nsteps', C.c_int32), ('maxit', C.c_int32), ('potential_drop', C.c_int32), ('reserved', C.c_int32),
                ('batch', C.c_int64), ('order_f', _PI), ('order_b', _PI), ('nu', _PD), ('cref', _PD), ('site_count', _PD),
                ('dG', _PD), ('Ea', _PD), ('lnA', _PD), ('site_density', C.c_double), ('tol', C.c_double), ('stern_capacitance', C.c_double),
                ('phi_pzc', C.c_double), ('phiM', _PD), ('gamma', _PD), ('theta_guess', _PD)]


class CatskOutputs(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('theta', _PD), ('flux_scale', _PD), ('flux_last', _PD), ('status', _PI),
                ('iterations_last', _PI), ('iterations_total', _PI), ('calls', _PI)]


_lib = None


def load_library():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ScfKineticsError(EDEVICE, 'HIP extension %s is missing: run `python -c "import __graft_entry__ as g; g.build()"`' % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        for name, argtypes, restype in (('create', [C.c_int32, C.POINTER(vp)], C.c_int), ('destroy', [vp], None),
                                        ('last_error', [vp], C.c_char_p), ('last_kernel', [vp], C.c_char_p),
                                        ('begin', [vp, C.POINTER(CatskParams)], C.c_int), ('flux_fn', [], vp),
                                        ('step_host', [vp, _PD, _PD, _PI, _PD], C.c_int), ('end', [vp, C.POINTER(CatskOutputs)], C.c_int)):
            f = getattr(lib, 'catsk_' + name)
            f.argtypes, f.restype = argtypes, restype
        _lib = lib
    return _lib


class ScfKinetics(_devlib.Handle):
    """One ``catsk_ctx``.  No device call is made before the first ``begin`` that passes validation."""
    _prefix, _error, _load = 'catsk_', ScfKineticsError, staticmethod(load_library)

    def _check(self, rc):
        if rc != 0:
            raise ScfKineticsError(rc, self._sym('last_error')(self._h).decode())

    @property
    def flux_fn(self):
        """address of the library's pnp_scf_flux_fn"""
        return int(self._sym('flux_fn')())

    @property
    def user(self):
        """address of the context: the `user` argument of flux_fn"""
        return int(self._h.value)

    @property
    def last_error(self):
        return self._sym('last_error')(self._h).decode()

    def begin(self, tables, phiM, potential_drop='stern', stern_capacitance=0.0, phi_pzc=0.0, gamma=None, theta_guess=None, tol=DEFAULT_TOL,
              maxit=DEFAULT_MAXIT, max_waves=0, struct_size=None):
        """catsk_begin for the lanes of phiM [B].  tables: the dict of MeanFieldModel.tables(); gamma [B][N], theta_guess [B][S+1]
        optional.  The per-lane buffers stay on the device until end()."""
        call = _microkin.Call(tables, phiM, None, {'gamma': gamma, 'theta_guess': theta_guess}, (), {}, (), potential_drop, stern_capacitance,
                              phi_pzc, max_waves)
        members = dict(call.members)
        members.pop('lanes')
        p = CatskParams(struct_size=_devlib.size_of(CatskParams, struct_size), maxit=int(maxit), tol=float(tol),
                        batch=members.pop('n'), **members)
        self._check(self._sym('begin')(self._h, C.byref(p)))
        self.B, self.dims = call.n, call.dims

    def step_host(self, csurf, phi_surface, active=None, flux=None):
        """catsk_step_host: the fluxes [B][N] at csurf [B][N], phi_surface [B] for the lanes with active[b] != 0 (None: all); rows of
        inactive lanes come back as `flux` had them (None: zeros)."""
        B, N = self.B, max(self.dims[0], 0)
        cs = np.ascontiguousarray(np.asarray(csurf, float).reshape(B, N))
        ps = np.ascontiguousarray(np.asarray(phi_surface, float).reshape(B))
        act = np.ones(B, np.int32) if active is None else np.ascontiguousarray(np.asarray(active).reshape(B), dtype=np.int32)
        fx = np.zeros((B, N)) if flux is None else np.array(np.asarray(flux, float).reshape(B, N), order='C')
        self._check(self._sym('step_host')(self._h, _dptr(cs), _dptr(ps), _iptr(act), _dptr(fx)))
        return fx

    def end(self, fields=None, out_struct_size=None):
        """catsk_end: a dict of the requested arrays (names out of FIELDS, None: all)"""
        N, S = max(self.dims[0], 0), self.dims[1]
        names = _devlib.field_names(fields, FIELDS)
        res = {}
        for name in names:
            shape, dtype = FIELDS[name]
            res[name] = np.zeros((self.B,) + shape(N, S), dtype)
        o = CatskOutputs(struct_size=_devlib.size_of(CatskOutputs, out_struct_size),
                         **{name: (_dptr(a) if a.dtype == np.float64 else _iptr(a)) for name, a in res.items()})
        self._check(self._sym('end')(self._h, C.byref(o)))
        return res
