"""ctypes binding of ``include/catint_response.h``: the linear response of a stationary state of the physical mode -- differential
capacitance, slope of the currents, admittance spectrum -- solved on the device (``catint_amd/lib/libcatint_response.so``, built by
``catint_amd.build.build_response_library()``).  No fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _devlib
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _PD, _PI, _PL, _cptr, _dptr, _f64, _iptr  # noqa: F401  (part of this module's interface)
from ._medium import WALL, Medium, reaction_table  # noqa: F401  (the same)

LIB_PATH = _devlib.lib_path('response')

# every symbol include/catint_response.h declares (tests/test_response_abi.py)
SYMBOLS = _devlib.symbols('catresp_', 'solve')

MAX_SPECIES, MAX_NX, MAX_FREQ = 8, 4098, 256
PHIM, WALL_FLUX = 0, 1
# complex output rows: name -> shape of one (operating point, frequency) from (N, nx)
SCALARS = {'dphi_surface': lambda N, nx: (), 'dc_surface': lambda N, nx: (N,), 'dsigma': lambda N, nx: (), 'dwall_flux': lambda N, nx: (N,),
           'admittance': lambda N, nx: ()}
PROFILES = {'dc': lambda N, nx: (N, nx), 'dphi': lambda N, nx: (nx,)}


class ResponseError(_devlib.LibraryError):
    library = 'catint_response'


class CatrespParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('wall_bc', C.c_int32), ('perturbation', C.c_int32),
                ('species', C.c_int32), ('nfreq', C.c_int32), ('nreactions', C.c_int32), ('n_wall', C.c_int32),
                ('nlanes', C.c_int64), ('lanes', _PL), ('D', _PD), ('charges', _PD), ('mpb_radius', _PD), ('x', _PD),
                ('beta', C.c_double), ('eps', C.c_double), ('dx', C.c_double), ('velocity', C.c_double), ('stern_capacitance', C.c_double),
                ('n_lhs', _PI), ('lhs', _PI), ('n_rhs', _PI), ('rhs', _PI), ('kf', _PD), ('kr', _PD),
                ('wall_species', _PI), ('nu', _PD), ('k', _PD), ('alpha', _PD), ('saturation', _PD), ('phiM', _PD), ('omega', _PD)]


class CatrespOutputs(C.Structure):
    _fields_ = [('dphi_surface', _PD), ('dc_surface', _PD), ('dsigma', _PD), ('dwall_flux', _PD), ('admittance', _PD), ('status', _PI),
                ('dc', _PD), ('dphi', _PD)]


load_library = _devlib.loader(globals(), 'catresp_', 'solve', CatrespParams, CatrespOutputs, ResponseError)


class Responder(_devlib.Handle):
    """One ``catresp_ctx``.  No device call is made before the first ``solve`` that passes validation with at least one lane."""
    _prefix, _error, _load = 'catresp_', ResponseError, staticmethod(load_library)

    def solve(self, view, D, charges, x, beta, eps, dx, phiM, omega=(0.0,), perturbation='phiM', lanes=None, mpb_radius=None,
              wall_bc='dirichlet', stern_capacitance=0.0, velocity=0.0, reactions=(), wall=None, fields=None, profiles=False,
              max_waves=0, struct_size=None, out=None):
        """catresp_solve about the state behind `view` (a PnpDeviceView).  perturbation: 'phiM' or ('flux', k); lanes: indices into
        the batch (None: all, in order; repeats allowed); omega [F] rad/s; reactions: [(lhs indices, rhs indices, kf, kr)]; wall: None
        or a dict {'species' [n], 'nu' [n][N], 'k' [B][n], 'alpha' [n] or None, 'saturation' [n] or None}; phiM [B].
        fields: names out of SCALARS (None: all); profiles: also 'dc' [n][F][N][nx] and 'dphi' [n][F][nx].  Returns a dict of
        complex128 arrays [n][F]... and 'status' [n][F] (int32).  out: arrays to write into instead of fresh ones (tests)."""
        names = _devlib.field_names(fields, SCALARS)
        if isinstance(perturbation, str):
            if perturbation != 'phiM':
                raise ValueError("perturbation is 'phiM' or ('flux', k)")
            pert, sp = PHIM, 0
        elif isinstance(perturbation, int):
            pert, sp = int(perturbation), 0          # (raw code: the library validates it)
        else:
            if perturbation[0] != 'flux':
                raise ValueError("perturbation is 'phiM' or ('flux', k)")
            pert, sp = WALL_FLUX, int(perturbation[1])
        medium = Medium(view, D, charges, x, beta, mpb_radius, velocity, reactions, eps=eps, dx=dx, wall_bc=wall_bc,
                        stern_capacitance=stern_capacitance, max_waves=max_waves, wall=wall, lanes=lanes)
        B, N, nx = medium.dims
        pm, om = _f64(phiM), _f64(np.atleast_1d(np.asarray(omega, float)).reshape(-1))
        F = len(om)
        medium.check('the view needs', [('phiM', pm, B)])
        p = CatrespParams(struct_size=_devlib.size_of(CatrespParams, struct_size), perturbation=pert, species=sp, nfreq=F, phiM=_dptr(pm),
                          omega=_dptr(om), **medium.members)
        shapes = {name: SCALARS[name](N, nx) for name in names}
        if profiles:
            shapes.update((name, f(N, nx)) for name, f in PROFILES.items())
        res = _devlib.results(out, shapes, (medium.n, max(F, 0)), np.complex128, status=(medium.n, max(F, 0)))
        o = CatrespOutputs(status=_iptr(res['status']), **{name: _cptr(a) for name, a in res.items() if name != 'status'})
        self._call('solve', view, p, o)
        return res
