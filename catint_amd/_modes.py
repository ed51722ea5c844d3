"""ctypes binding of ``include/catint_modes.h``: the relaxation modes of a stationary state of the physical mode -- a subspace iteration on
J^-1 S per operating point, all passes in one launch on the device (``catint_amd/lib/libcatint_modes.so``, built by
``catint_amd.build.build_modes_library()``) -- and the small eigenproblem that stays on the host.  No fallback: a missing library
raises."""
import ctypes as C

import numpy as np

from . import _devlib
from ._devlib import EDEVICE, EINVAL, ENOMEM, PnpDeviceView, _PD, _PI, _PL, _dptr, _f64, _iptr  # noqa: F401  (part of this module's interface)
from ._medium import WALL, Medium, reaction_table  # noqa: F401  (the same)

LIB_PATH = _devlib.lib_path('modes')

# every symbol include/catint_modes.h declares (tests/test_modes_abi.py)
SYMBOLS = _devlib.symbols('catmodes_', 'solve')

MAX_SPECIES, MAX_NX, MAX_SUBSPACE, MAX_ITERATIONS = 8, 4098, 8, 64
PIVOT_GROWTH_LIMIT, BREAKDOWN = 1e8, 1e-10
OK, PIVOT, UNSOLVED, BREAKDOWN_STATUS = 0, 1, 2, 3
# output rows: name -> shape of one operating point from (m, N, nx)
FIELDS = {'ritz': lambda m, N, nx: (m, m), 'gram': lambda m, N, nx: (m, m), 'basis': lambda m, N, nx: (m, N + 1, nx)}


class ModesError(_devlib.LibraryError):
    library = 'catint_modes'


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


load_library = _devlib.loader(globals(), 'catmodes_', 'solve', CatmodesParams, CatmodesOutputs, ModesError)


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
        names = _devlib.field_names(fields, FIELDS, ('ritz', 'gram'))
        q0, pm = _f64(start), _f64(phiM)
        m = int(subspace) if subspace is not None else (0 if q0 is None else int(q0.shape[0]))
        medium = Medium(view, D, charges, x, beta, mpb_radius, velocity, reactions, eps=eps, dx=dx, wall_bc=wall_bc,
                        stern_capacitance=stern_capacitance, max_waves=max_waves, wall=wall, lanes=lanes)
        B, N, nx = medium.dims
        ms = min(max(m, 0), MAX_SUBSPACE)
        # (a subspace outside 1 .. MAX_SUBSPACE is the library's to refuse: `start` has no size to be checked against then)
        medium.check('the call needs', ([('start', q0, ms * (N + 1) * nx)] if 1 <= m <= MAX_SUBSPACE else []) + [('phiM', pm, B)])
        p = CatmodesParams(struct_size=_devlib.size_of(CatmodesParams, struct_size), subspace=m, iterations=int(iterations), phiM=_dptr(pm),
                           start=_dptr(q0), **medium.members)
        res = _devlib.results(out, {name: FIELDS[name](ms, N, nx) for name in names}, (medium.n,), status=medium.n)
        o = CatmodesOutputs(struct_size=_devlib.size_of(CatmodesOutputs, out_struct_size), status=_iptr(res['status']),
                            **{name: _dptr(a) for name, a in res.items() if name in FIELDS})
        self._call('solve', view, p, o)
        return res
