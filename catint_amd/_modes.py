"""ctypes binding of ``include/catint_modes.h``: the relaxation modes of a stationary state of the physical mode -- a subspace iteration on
J^-1 S per operating point, all passes in one launch on the device (``catint_amd/lib/libcatint_modes.so``, built by
``catint_amd.build.build_modes_library()``) -- and the small eigenproblem that stays on the host.  No fallback: a missing library
raises."""
import ctypes as C
import os

import numpy as np

from . import _devlib
from ._capi import flatten_reactions as reaction_table      # the arrays of pnp_set_reactions: catmodes_params takes the same form
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _dptr  # noqa: F401  (part of this module's interface)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CATINT_MODES_LIB') or os.path.join(_HERE, 'lib', 'libcatint_modes.so')

# every symbol include/catint_modes.h declares (tests/test_modes_abi.py)
SYMBOLS = _devlib.symbols('catmodes_', 'solve')

MAX_SPECIES, MAX_NX, MAX_SUBSPACE, MAX_ITERATIONS = 8, 4098, 8, 64
PIVOT_GROWTH_LIMIT, BREAKDOWN = 1e8, 1e-10
WALL = {'dirichlet': 0, 'stern': 1}
OK, PIVOT, UNSOLVED, BREAKDOWN_STATUS = 0, 1, 2, 3
# output rows: name -> shape of one operating point from (m, N, nx)
FIELDS = {'ritz': lambda m, N, nx: (m, m), 'gram': lambda m, N, nx: (m, m), 'basis': lambda m, N, nx: (m, N + 1, nx)}


class ModesError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('catint_modes error %d: %s' % (code, msg))
        self.code = code


_PD, _PI, _PL = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


class CatmodesParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('max_waves', C.c_int32), ('wall_bc', C.c_int32), ('nreactions', C.c_int32),
                ('n_wall', C.c_int32), ('subspace', C.c_int32), ('iterations', C.c_int32), ('reserved', C.c_int32),
                ('nlanes', C.c_int64), ('lanes', _PL),
                ('D', _PD), ('charges', _PD), ('mpb_radius', _PD), ('x', _PD),
                ('beta', C.c_double), ('eps', C.c_double), ('dx', C.c_double), ('velocity', C.c_double), ('stern_capacitance', C.c_double),
                ('n_lhs', _PI), ('lhs', _PI), ('n_rhs', _PI), ('rhs', _PI), ('kf', _PD), ('kr', _PD),
                ('wall_species', _PI), ('nu', _PD), ('k', _PD), ('alpha', _PD), ('saturation', _PD), ('phiM', _PD), ('start', _PD)]


class CatmodesOutputs(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('ritz', _PD), ('gram', _PD), ('basis', _PD), ('status', _PI)]


_lib = None


def load_library():
    global _lib
    if _lib is None:
        _lib = _devlib.load(LIB_PATH, 'catmodes_', 'solve', CatmodesParams, CatmodesOutputs, ModesError)
    return _lib


def _iptr(a):
    return a.ctypes.data_as(_PI) if a is not None else None


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def default_start(m, N, nx, seed=0):
    """[m][N+1][nx] standard normal numbers of numpy.random.RandomState(seed): a start without a symmetry the modes could be
    orthogonal to.  The same for every operating point of a call, so neighbouring points differ by their physics alone."""
    return np.random.RandomState(seed).standard_normal((m, N + 1, nx))


def ritz_pairs(ritz, gram):
    """The small eigenproblem of one operating point (include/catint_modes.h): theta [m] complex and s [m][m] (columns) = eig(B),
    ordered by descending |theta| (the two members of a conjugate pair, which LAPACK returns as exact conjugates, stay together, the
    one with the positive imaginary part first), and the
    relative residuals sqrt(s_j^H G s_j) / (|theta_j| |s_j|).  Rows of NaN where B or G is not finite; a theta of exactly 0 has an
    infinite residual."""
    B, G = np.asarray(ritz, float), np.asarray(gram, float)
    m = B.shape[0]
    if not (np.isfinite(B).all() and np.isfinite(G).all()):
        return np.full(m, np.nan + 0j), np.full((m, m), np.nan + 0j), np.full(m, np.nan)
    theta, s = np.linalg.eig(B)
    order = sorted(range(m), key=lambda j: (-abs(theta[j]), -theta[j].imag))
    theta, s = theta[order], s[:, order].astype(complex)
    num = np.sqrt(np.maximum(np.real(np.einsum('aj,ab,bj->j', s.conj(), G, s)), 0.0))
    with np.errstate(divide='ignore', invalid='ignore'):
        res = np.where(np.abs(theta) > 0, num / (np.abs(theta) * np.linalg.norm(s, axis=0)), np.inf)
    return theta.astype(complex), s, res


class ModeSolver(_devlib.Handle):
    """One ``catmodes_ctx``.  No device call is made before the first ``solve`` that passes validation with at least one lane."""
    _prefix, _error, _load = 'catmodes_', ModesError, staticmethod(load_library)

    def solve(self, view, D, charges, x, beta, eps, dx, phiM, start, subspace=None, iterations=12, lanes=None, mpb_radius=None,
              wall_bc='dirichlet', stern_capacitance=0.0, velocity=0.0, reactions=(), wall=None, fields=None, max_waves=0,
              struct_size=None, out_struct_size=None, out=None):
        """catmodes_solve about the state behind `view` (a PnpDeviceView).  start [m][N+1][nx] (m = subspace; None: its first axis);
        lanes: indices into the batch (None: all of it; repeats allowed); phiM [B]; reactions: [(lhs indices, rhs indices, kf, kr)];
        wall: None or a dict {'species' [n_wall], 'nu' [n_wall][N], 'k' [B][n_wall], 'alpha' [n_wall] or None, 'saturation' [n_wall] or
        None}.  fields: names out of FIELDS (None: 'ritz' and 'gram').  Returns a dict of float64 arrays [n]... and 'status' [n] (int32).
        out: arrays to write into instead of fresh ones (tests)."""
        B, N, nx = max(int(view.batch), 0), max(int(view.nspecies), 0), max(int(view.nx), 0)
        names = ['ritz', 'gram'] if fields is None else list(fields)
        for nm in names:
            if nm not in FIELDS:
                raise ValueError('unknown field %r (known: %s)' % (nm, ', '.join(FIELDS)))
        q0 = _f64(start)
        m = int(subspace) if subspace is not None else (0 if q0 is None else int(q0.shape[0]))
        R, n_lhs, lhs, n_rhs, rhs, kf, kr = reaction_table(list(reactions))
        W = 0 if not wall else len(wall['species'])
        wk = [None] * 5
        if W:
            wk = [np.ascontiguousarray(wall['species'], dtype=np.int32), _f64(wall['nu']), _f64(wall.get('k')), _f64(wall.get('alpha')),
                  _f64(wall.get('saturation'))]
        keep = [_f64(a) for a in (D, charges, x, mpb_radius, phiM)]
        idx = None if lanes is None else np.ascontiguousarray(lanes, dtype=np.int64).reshape(-1)
        n = len(idx) if idx is not None else B
        ms = min(max(m, 0), MAX_SUBSPACE)
        for name, a, size in (('start', q0, ms * (N + 1) * nx), ('phiM', keep[4], B), ('wall k', wk[2], B * W), ('wall nu', wk[1], W * N),
                              ('wall alpha', wk[3], W), ('wall saturation', wk[4], W), ('mpb_radius', keep[3], N)):
            if a is not None and a.size != size and not (name == 'start' and not 1 <= m <= MAX_SUBSPACE):
                raise ValueError('%s has %d values, the call needs %d' % (name, a.size, size))
        if keep[0].size < N or keep[1].size < N or keep[2].size < nx:
            raise ValueError('D, charges or x shorter than the view')
        p = CatmodesParams(C.sizeof(CatmodesParams) if struct_size is None else int(struct_size), int(max_waves),
                           wall_bc if isinstance(wall_bc, int) else WALL[wall_bc], R, W, m, int(iterations), 0, n,
                           None if idx is None else idx.ctypes.data_as(_PL),
                           _dptr(keep[0]), _dptr(keep[1]), _dptr(keep[3]), _dptr(keep[2]), float(beta), float(eps), float(dx), float(velocity),
                           float(stern_capacitance), _iptr(n_lhs), _iptr(lhs), _iptr(n_rhs), _iptr(rhs), _dptr(kf), _dptr(kr),
                           _iptr(wk[0]), _dptr(wk[1]), _dptr(wk[2]), _dptr(wk[3]), _dptr(wk[4]), _dptr(keep[4]), _dptr(q0))
        res = {} if out is None else out
        for name in names:
            res.setdefault(name, np.empty((n,) + FIELDS[name](ms, N, nx)))
        res.setdefault('status', np.zeros(n, np.int32))
        o = CatmodesOutputs(struct_size=C.sizeof(CatmodesOutputs) if out_struct_size is None else int(out_struct_size),
                            status=_iptr(res['status']), **{name: _dptr(a) for name, a in res.items() if name in FIELDS})
        self._call('solve', view, p, o)
        return res
