"""ctypes binding of ``include/catint_sens.h``: the sensitivities of a stationary state of the physical mode to its model parameters --
bulk concentrations, diffusion coefficients, rate constants of the homogeneous and of the wall reactions, Stern capacitance, convection
velocity, next to the electrode potential and the prescribed wall fluxes -- from block eliminations with carried right-hand sides on the
device (``catint_amd/lib/libcatint_sens.so``, built by ``catint_amd.build.build_sens_library()``).  No fallback: a missing library
raises."""
import ctypes as C
import os

import numpy as np

from . import _devlib
from ._capi import flatten_reactions as reaction_table      # the arrays of pnp_set_reactions: catsens_params takes the same form
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _dptr  # noqa: F401  (part of this module's interface)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CATINT_SENS_LIB') or os.path.join(_HERE, 'lib', 'libcatint_sens.so')

# every symbol include/catint_sens.h declares (tests/test_sens_abi.py)
SYMBOLS = _devlib.symbols('catsens_', 'solve')

MAX_SPECIES, MAX_NX, MAX_PARAMS, CHUNK = 8, 4098, 64, 8
PIVOT_GROWTH_LIMIT = 1e8
WALL = {'dirichlet': 0, 'stern': 1}
OK, PIVOT, UNSOLVED = 0, 1, 2
# kinds of parameter: name -> CATSENS_* code
KINDS = {'phiM': 0, 'flux': 1, 'c_bulk': 2, 'D': 3, 'kf': 4, 'kr': 5, 'wall_k': 6, 'stern_capacitance': 7, 'velocity': 8}
INDEXED = ('flux', 'c_bulk', 'D', 'kf', 'kr', 'wall_k')      # the kinds that name a species, a reaction or a wall reaction
# output rows: name -> shape of one (operating point, parameter) from N
FIELDS = {'dphi_surface': lambda N: (), 'dc_surface': lambda N: (N,), 'dsigma': lambda N: (), 'dwall_flux': lambda N: (N,),
          'dcurrent': lambda N: ()}


class SensError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('catint_sens error %d: %s' % (code, msg))
        self.code = code


_PD, _PI, _PL = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


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


_lib = None


def load_library():
    global _lib
    if _lib is None:
        _lib = _devlib.load(LIB_PATH, 'catsens_', 'solve', CatsensParams, CatsensOutputs, SensError)
    return _lib


def _iptr(a):
    return a.ctypes.data_as(_PI) if a is not None else None


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


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
        B, N = max(int(view.batch), 0), max(int(view.nspecies), 0)
        names = list(FIELDS) if fields is None else list(fields)
        for nm in names:
            if nm not in FIELDS:
                raise ValueError('unknown field %r (known: %s)' % (nm, ', '.join(FIELDS)))
        kind, index = encode(parameters)
        P = len(kind) if nparams is None else int(nparams)
        R, n_lhs, lhs, n_rhs, rhs, kf, kr = reaction_table(list(reactions))
        W = 0 if not wall else len(wall['species'])
        wk = [None] * 5
        if W:
            wk = [np.ascontiguousarray(wall['species'], dtype=np.int32), _f64(wall['nu']), _f64(wall.get('k')), _f64(wall.get('alpha')),
                  _f64(wall.get('saturation'))]
        keep = [_f64(a) for a in (D, charges, x, mpb_radius, phiM)]
        idx = None if lanes is None else np.ascontiguousarray(lanes, dtype=np.int64).reshape(-1)
        g = _f64(flux)
        n = len(idx) if idx is not None else (0 if g is None else g.size // max(N, 1))
        for name, a, size in (('flux', g, n * N), ('phiM', keep[4], B), ('wall k', wk[2], B * W), ('wall nu', wk[1], W * N),
                              ('wall alpha', wk[3], W), ('wall saturation', wk[4], W), ('mpb_radius', keep[3], N)):
            if a is not None and a.size != size:
                raise ValueError('%s has %d values, the call needs %d' % (name, a.size, size))
        if keep[0].size < N or keep[1].size < N or keep[2].size < max(int(view.nx), 0):
            raise ValueError('D, charges or x shorter than the view')
        p = CatsensParams(C.sizeof(CatsensParams) if struct_size is None else int(struct_size), int(max_waves),
                          wall_bc if isinstance(wall_bc, int) else WALL[wall_bc], R, W, P, n, None if idx is None else idx.ctypes.data_as(_PL),
                          _dptr(keep[0]), _dptr(keep[1]), _dptr(keep[3]), _dptr(keep[2]), float(beta), float(eps), float(dx), float(velocity),
                          float(stern_capacitance), float(phi_pzc), _iptr(n_lhs), _iptr(lhs), _iptr(n_rhs), _iptr(rhs), _dptr(kf), _dptr(kr),
                          _iptr(wk[0]), _dptr(wk[1]), _dptr(wk[2]), _dptr(wk[3]), _dptr(wk[4]), _dptr(keep[4]), _dptr(g),
                          _iptr(kind) if len(kind) else None, _iptr(index) if len(index) else None)
        Ps = min(max(P, 0), len(kind))
        res = {} if out is None else out
        for name in names:
            res.setdefault(name, np.empty((n, Ps) + FIELDS[name](N)))
        res.setdefault('status', np.zeros(n, np.int32))
        o = CatsensOutputs(struct_size=C.sizeof(CatsensOutputs) if out_struct_size is None else int(out_struct_size),
                           status=_iptr(res['status']), **{name: _dptr(a) for name, a in res.items() if name in FIELDS})
        self._call('solve', view, p, o)
        return res
