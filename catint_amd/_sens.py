"""ctypes binding of ``include/catint_sens.h``: the sensitivities of a stationary state of the physical mode to its model parameters --
bulk concentrations, diffusion coefficients, rate constants of the homogeneous and of the wall reactions, Stern capacitance, convection
velocity, next to the electrode potential and the prescribed wall fluxes -- from block eliminations with carried right-hand sides on the
device (``catint_amd/lib/libcatint_sens.so``, built by ``catint_amd.build.build_sens_library()``).  No fallback: a missing library
raises."""
import ctypes as C

import numpy as np

from . import _devlib
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _PD, _PI, _PL, _dptr, _f64, _iptr  # noqa: F401  (part of this module's interface)
from ._medium import WALL, Medium, reaction_table  # noqa: F401  (the same)

LIB_PATH = _devlib.lib_path('sens')

# every symbol include/catint_sens.h declares (tests/test_sens_abi.py)
SYMBOLS = _devlib.symbols('catsens_', 'solve')

MAX_SPECIES, MAX_NX, MAX_PARAMS, CHUNK = 8, 4098, 64, 8
PIVOT_GROWTH_LIMIT = 1e8
OK, PIVOT, UNSOLVED = 0, 1, 2
# kinds of parameter: name -> CATSENS_* code
KINDS = {'phiM': 0, 'flux': 1, 'c_bulk': 2, 'D': 3, 'kf': 4, 'kr': 5, 'wall_k': 6, 'stern_capacitance': 7, 'velocity': 8}
INDEXED = ('flux', 'c_bulk', 'D', 'kf', 'kr', 'wall_k')      # the kinds that name a species, a reaction or a wall reaction
# output rows: name -> shape of one (operating point, parameter) from N
FIELDS = {'dphi_surface': lambda N: (), 'dc_surface': lambda N: (N,), 'dsigma': lambda N: (), 'dwall_flux': lambda N: (N,),
          'dcurrent': lambda N: ()}


class SensError(_devlib.LibraryError):
    library = 'catint_sens'


class CatsensParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('wall_bc', C.c_int32), ('nreactions', C.c_int32),
                ('n_wall', C.c_int32), ('nparams', C.c_int32), ('nlanes', C.c_int64), ('lanes', _PL),
                ('D', _PD), ('charges', _PD), ('mpb_radius', _PD), ('x', _PD),
                ('beta', C.c_double), ('eps', C.c_double), ('dx', C.c_double), ('velocity', C.c_double), ('stern_capacitance', C.c_double),
                ('phi_pzc', C.c_double),
                ('n_lhs', _PI), ('lhs', _PI), ('n_rhs', _PI), ('rhs', _PI), ('kf', _PD), ('kr', _PD),
                ('wall_species', _PI), ('nu', _PD), ('k', _PD), ('alpha', _PD), ('saturation', _PD), ('phiM', _PD), ('flux', _PD),
                ('kind', _PI), ('index', _PI)]


class CatsensOutputs(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('dphi_surface', _PD), ('dc_surface', _PD), ('dsigma', _PD),
                ('dwall_flux', _PD), ('dcurrent', _PD), ('status', _PI)]


load_library = _devlib.loader(globals(), 'catsens_', 'solve', CatsensParams, CatsensOutputs, SensError)


def encode(parameters):
    """(kind [P], index [P]) int32 from a list of 'phiM' / 'stern_capacitance' / 'velocity' / (name, index) / raw (code, index) pairs"""
    kind, index = [], []
    for spec in parameters:
        if isinstance(spec, str):
            if spec not in KINDS or spec in INDEXED:
                raise ValueError('unknown parameter %r (known: %s; the indexed ones as (name, index))' % (spec, ', '.join(KINDS)))
            kind.append(KINDS[spec]), index.append(0)
        else:
            name, i = spec
            if isinstance(name, str):
                if name not in INDEXED:
                    raise ValueError('parameter %r takes no index or is unknown' % (name,))
                name = KINDS[name]
            kind.append(int(name)), index.append(int(i))         # (raw code: the library validates it)
    return np.array(kind, np.int32), np.array(index, np.int32)


class Sensitizer(_devlib.Handle):
    """One ``catsens_ctx``.  No device call is made before the first ``solve`` that passes validation with at least one lane."""
    _prefix, _error, _load = 'catsens_', SensError, staticmethod(load_library)

    def solve(self, view, D, charges, x, beta, eps, dx, phiM, flux, parameters, lanes=None, mpb_radius=None, wall_bc='dirichlet',
              stern_capacitance=0.0, phi_pzc=0.0, velocity=0.0, reactions=(), wall=None, fields=None, max_waves=0, struct_size=None,
              out_struct_size=None, out=None, nparams=None):
        """catsens_solve about the state behind `view` (a PnpDeviceView).  parameters: see `encode`; lanes: indices into the batch (None:
        0 .. n-1; repeats allowed); flux [n][N] is indexed by the position in the call, n = len(lanes) (None: the number of rows of
        flux); phiM [B]; reactions: [(lhs indices, rhs indices, kf, kr)]; wall: None or a dict {'species' [n_wall], 'nu' [n_wall][N],
        'k' [B][n_wall], 'alpha' [n_wall] or None, 'saturation' [n_wall] or None}.  fields: names out of FIELDS (None: all).  Returns a
        dict of float64 arrays [n][P]... and 'status' [n] (int32).  out: arrays to write into instead of fresh ones (tests)."""
        names = _devlib.field_names(fields, FIELDS)
        kind, index = encode(parameters)
        P = len(kind) if nparams is None else int(nparams)
        medium = Medium(view, D, charges, x, beta, mpb_radius, velocity, reactions, eps=eps, dx=dx, wall_bc=wall_bc,
                        stern_capacitance=stern_capacitance, max_waves=max_waves, wall=wall, lanes=lanes)
        B, N, _ = medium.dims
        pm, g = _f64(phiM), _f64(flux)
        if medium.idx is None:
            medium.rows(0 if g is None else g.size // max(N, 1))
        n = medium.n
        medium.check('the call needs', [('flux', g, n * N), ('phiM', pm, B)])
        p = CatsensParams(struct_size=_devlib.size_of(CatsensParams, struct_size), nparams=P, phi_pzc=float(phi_pzc), phiM=_dptr(pm),
                          flux=_dptr(g), kind=_iptr(kind) if len(kind) else None, index=_iptr(index) if len(index) else None,
                          **medium.members)
        res = _devlib.results(out, {name: FIELDS[name](N) for name in names}, (n, min(max(P, 0), len(kind))), status=n)
        o = CatsensOutputs(struct_size=_devlib.size_of(CatsensOutputs, out_struct_size), status=_iptr(res['status']),
                           **{name: _dptr(a) for name, a in res.items() if name in FIELDS})
        self._call('solve', view, p, o)
        return res
