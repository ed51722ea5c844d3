"""Unit tests of the shared device primitives (test infrastructure, no tests of its own).

Three parts:
  * the ctypes binding of libcatint_unittest.so (tests/csrc/primitives_harness.hip: every primitive of pnp_math.h, pnp_wave.h,
    pnp_post.h, pnp_lane_common.h and pnp_lane_cols.h, and the per-lane LU of pnp_kin.h, behind a kernel of its own),
  * multiprecision references (mpmath, 60 digits, rounded ONCE to fp64; where an error is measured in ulp the reference is the pair
    (hi, lo) with hi + lo the exact value to ~1e-32 relative, so that the error is taken against the exact value, not a rounded one),
  * the assertion helpers of tests/test_gpu_primitives.py -- pure functions of arrays -- and plain fp64 NumPy emulations of the
    operations with their mutants; tests/test_primitives_ref.py shows without a GPU that every helper passes the emulation and fails
    the mutants.
"""
import ctypes as C
import functools
import os

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.prec = 200
mpf = MP.mpf

PS = (1, 2, 4, 8, 16)
FN = {'fast_rcp': 0, 'fast_rcp2': 1, 'nrcp': 2, 'expm1_sc': 3, 'log1p_sc': 4, 'bernoulli': 5}
SYMBOLS = ('catunit_scalar', 'catunit_edge_flux', 'catunit_wave_moves', 'catunit_read_lane', 'catunit_pick_blocked', 'catunit_wave_scan',
           'catunit_blocked_scan', 'catunit_blocked_scan_sum', 'catunit_tridiag', 'catunit_row_alloc', 'catunit_win_alloc', 'catunit_load_row',
           'catunit_store_row', 'catunit_load_window', 'catunit_store_window', 'catunit_col_lanes', 'catunit_newton_rule', 'catunit_newton_accept',
           'catunit_lu')

# the bars (the header comments' own figures with the allowance of the design note, or its derivations)
RCP1_BAR = 2 * 2.2e-15          # fast_rcp, relative
RCP2_BAR = 2 * 1.1e-16          # fast_rcp2, nrcp, relative
ULP_BAR = 4.0                   # expm1_sc, log1p_sc: strictly below
B_ULP_BAR = 8.0                 # B: 4 ulp of expm1_sc, doubled for the reciprocal and the product
DB_REL_BAR = 5e-14              # B' (Jacobian only): u^7/151200 <= 5.2e-15 against |B'| >= 0.49; ulp(1)/0.025 from 1 - B - u
FAST_RCP_REL = 2.2e-15          # the unit of the tridiagonal forward-error bar
SERIES_U = 0.05


# ---- the binding ------------------------------------------------------------------------------------------------------------------
class HarnessError(RuntimeError):
    pass


_lib = None


def load_library():
    global _lib
    if _lib is None:
        from catint_amd import build
        if not os.path.exists(build.UNITTEST_LIB):
            raise HarnessError('%s is missing: run __graft_entry__.build()' % build.UNITTEST_LIB)
        _lib = C.CDLL(build.UNITTEST_LIB)
        for s in SYMBOLS:
            getattr(_lib, s).restype = C.c_int
    return _lib


def _in(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _check(rc, what):
    if rc != 0:
        raise HarnessError('%s returned HIP error %d' % (what, rc))


def scalar(name, x):
    x = _in(x)
    y = np.empty_like(x)
    _check(load_library().catunit_scalar(FN[name], _p(x), _p(y), C.c_int(x.size)), 'catunit_scalar(%s)' % name)
    return y


def edge_flux(u):
    """B(u) and B'(u) as lane_edge_flux(u, cl=1, cr=0, w=1) returns them in Bp and Ju"""
    u = _in(u)
    B, dB = np.empty_like(u), np.empty_like(u)
    _check(load_library().catunit_edge_flux(_p(u), _p(B), _p(dB), C.c_int(u.size)), 'catunit_edge_flux')
    return B, dB


def wave_moves(v, old):
    v = _in(v).reshape(-1, 64)
    prev, nxt = np.empty_like(v), np.empty_like(v)
    _check(load_library().catunit_wave_moves(_p(v), C.c_double(old), _p(prev), _p(nxt), C.c_int(v.shape[0])), 'catunit_wave_moves')
    return prev, nxt


def read_lane(v):
    v = _in(v).reshape(64)
    out = np.empty((64, 64))
    _check(load_library().catunit_read_lane(_p(v), _p(out)), 'catunit_read_lane')
    return out


def col_lanes(W, v):
    """the exchanges of pnp_lane_cols.h on one wave: bcast [W, 64], other [64], total [64]"""
    v = _in(v).reshape(64)
    bcast, other, total = np.empty((W, 64)), np.empty(64), np.empty(64)
    _check(load_library().catunit_col_lanes(W, _p(v), _p(bcast), _p(other), _p(total)), 'catunit_col_lanes')
    return bcast, other, total


def pick_blocked(P, a):
    a = _in(a).reshape(64 * P)
    out = np.empty((64 * P, 64))
    _check(load_library().catunit_pick_blocked(P, _p(a), _p(out)), 'catunit_pick_blocked')
    return out


def wave_scan(v, bc):
    v = _in(v).reshape(-1, 64)
    out = np.empty_like(v)
    _check(load_library().catunit_wave_scan(int(bc), _p(v), _p(out), C.c_int(v.shape[0])), 'catunit_wave_scan')
    return out


def blocked_scan(P, rev, x):
    x = _in(x).reshape(-1, 64 * P)
    n = x.shape[0]
    xo, total, base = np.empty_like(x), np.empty((n, 64)), np.empty((n, 64))
    _check(load_library().catunit_blocked_scan(P, int(rev), _p(x), _p(xo), _p(total), _p(base), C.c_int(n)), 'catunit_blocked_scan')
    return xo, total, base


def blocked_scan_sum(P, x, w):
    x = _in(x).reshape(-1, 64 * P)
    n = x.shape[0]
    w = _in(w).reshape(n, 64)
    xo, total, base, wtotal = np.empty_like(x), np.empty((n, 64)), np.empty((n, 64)), np.empty((n, 64))
    _check(load_library().catunit_blocked_scan_sum(P, _p(x), _p(w), _p(xo), _p(total), _p(base), _p(wtotal), C.c_int(n)), 'catunit_blocked_scan_sum')
    return xo, total, base, wtotal


def tridiag(P, G, dpp1, a, c, d):
    """a, c, d: [ncase, G, 64 P] -> x of the same shape"""
    a, c, d = (_in(t).reshape(-1, G, 64 * P) for t in (a, c, d))
    assert a.shape == c.shape == d.shape
    x = np.empty_like(d)
    _check(load_library().catunit_tridiag(P, G, int(dpp1), _p(a), _p(c), _p(d), _p(x), C.c_int(a.shape[0])), 'catunit_tridiag')
    return x


def row_alloc(P):
    return load_library().catunit_row_alloc(P)


def win_alloc(P):
    return load_library().catunit_win_alloc(P)


def load_row(P, src, ldx):
    src = _in(src)
    out = np.empty(row_alloc(P))
    _check(load_library().catunit_load_row(P, _p(src), C.c_int(src.size), C.c_int(ldx), _p(out)), 'catunit_load_row')
    return out


def store_row(P, aux, vals, dst, ldx):
    vals, dst = _in(vals), _in(dst).copy()
    assert vals.size == row_alloc(P)
    _check(load_library().catunit_store_row(P, aux, _p(vals), _p(dst), C.c_int(dst.size), C.c_int(ldx)), 'catunit_store_row')
    return dst


LOAD_WINDOW = {'load_window<P, 0>': 0, 'load_window<P, 2>': 1, 'post::load_win<P>': 2}
STORE_WINDOW = {'store_rows<P>': 0, 'post::store_blocked (point row)': 1, 'post::store_blocked (edge row)': 2}


def load_window(P, which, row, nrec):
    row = _in(row)
    w = np.empty((64, P + 2))
    _check(load_library().catunit_load_window(P, LOAD_WINDOW[which], _p(row), C.c_int(row.size), C.c_int(nrec), _p(w)), 'catunit_load_window')
    return w


def store_window(P, mode, v, dst, nrec):
    v, dst = _in(v).reshape(64, P + 2), _in(dst).copy()
    _check(load_library().catunit_store_window(P, STORE_WINDOW[mode], _p(v), _p(dst), C.c_int(dst.size), C.c_int(nrec)), 'catunit_store_window')
    return dst


def lu(T, A, b):
    """pnp_kin.h's factor and substitute on one wave: A [64, T, T], b [64, 2, T] -> the factors [64, T, T], the packed pivot rows [64]
    (uint64), the bad-pivot flags [64] (uint64: 0 / 1) and the solutions [64, 2, T]"""
    A, b = _in(A).reshape(64, T, T), _in(b).reshape(64, 2, T)
    f, meta, x = np.empty_like(A), np.empty((64, 2), np.uint64), np.empty_like(b)
    _check(load_library().catunit_lu(T, _p(A), _p(b), _p(f), meta.ctypes.data_as(C.POINTER(C.c_uint64)), _p(x)), 'catunit_lu')
    return f, meta[:, 0].copy(), meta[:, 1].copy(), x


# ---- multiprecision references ------------------------------------------------------------------------------------------------------
def _hilo(values):
    hi = np.array([float(v) for v in values])
    lo = np.array([float(v - mpf(h)) if np.isfinite(h) else 0.0 for v, h in zip(values, hi)])
    return hi, lo


def ref_rcp(x):
    return _hilo([1 / mpf(float(v)) for v in x])


def ref_expm1(u):
    return _hilo([MP.expm1(mpf(float(v))) for v in u])


def ref_log1p(x):
    return _hilo([MP.log1p(mpf(float(v))) for v in x])


def _mp_bernoulli(v):
    u = mpf(float(v))
    if u == 0:
        return mpf(1), mpf(-0.5)
    E = MP.expm1(u)
    B = u / E
    return B, (1 - B - u) / E


def ref_bernoulli(u):
    """B(u) = u / (exp(u) - 1) as (hi, lo), and B'(u) rounded once"""
    pairs = [_mp_bernoulli(v) for v in u]
    hi, lo = _hilo([p[0] for p in pairs])
    return (hi, lo), np.array([float(p[1]) for p in pairs])


def ref_prefix(x, rev=False):
    """exact prefix (rev: suffix) sums of the rows of x, rounded once"""
    x = np.atleast_2d(x)
    out = np.empty_like(x)
    for i, row in enumerate(x):
        row = row[::-1] if rev else row
        acc, res = mpf(0), []
        for v in row:
            acc += mpf(float(v))
            res.append(float(acc))
        out[i] = res[::-1] if rev else res
    return out


def ref_thomas(a, c, d, m):
    """the m real rows a[r] x[r-1] + x[r] + c[r] x[r+1] = d[r] (a[0] and c[m-1] do not enter) solved in multiprecision, rounded once"""
    a, c, d = ([mpf(float(v)) for v in t[:m]] for t in (a, c, d))
    cp, dp = [None] * m, [None] * m
    cp[0], dp[0] = c[0], d[0]
    for i in range(1, m):
        piv = 1 - a[i] * cp[i - 1]
        cp[i] = c[i] / piv
        dp[i] = (d[i] - a[i] * dp[i - 1]) / piv
    x = [None] * m
    x[m - 1] = dp[m - 1]
    for i in range(m - 2, -1, -1):
        x[i] = dp[i] - cp[i] * x[i + 1]
    return np.array([float(v) for v in x])


# ---- arguments (shared by the CPU and the GPU tests; every set stays below 2^16) ---------------------------------------------------------
def neighbours(x, n):
    """the n doubles below x, x itself and the n doubles above it"""
    lo, hi = [x], [x]
    for _ in range(n):
        lo.append(np.nextafter(lo[-1], -np.inf))
        hi.append(np.nextafter(hi[-1], np.inf))
    return np.array(lo[:0:-1] + [x] + hi[1:])


def rcp_args():
    mag = np.logspace(-150, 150, 12000)
    near = np.concatenate([np.linspace(0.5, 2.0, 2048), np.random.default_rng(11).uniform(0.5, 2.0, 2048)])
    return np.concatenate([mag, -mag, near])


def expm1_args():
    """inside the clamps: |u| in [0.05, 709] (-60 on the negative side, where the result is -1 to the last bit anyway)"""
    mag = np.logspace(np.log10(0.05), np.log10(709.0), 6000)
    mag[0], mag[-1] = 0.05, 709.0
    ties = np.concatenate([neighbours((k + 0.5) * np.log(2.0), 256) for k in range(-4, 5)])
    ties = ties[np.abs(ties) >= 0.05]
    edge = np.concatenate([neighbours(-60.0, 4), neighbours(709.0, 4)[:5], [0.05, -0.05]])
    return np.concatenate([mag, -mag, ties, edge])


EXPM1_BELOW = np.array([np.nextafter(-60.0, -np.inf), -60.5, -61.0, -100.0, -745.2, -1e4, -1e308, -np.inf])      # exactly -1.0
EXPM1_ABOVE = np.array([np.nextafter(709.0, np.inf), 709.5, 710.0, 1e3, 1e308, np.inf])                           # +inf


def log1p_args():
    """x = -f and x = -(1 - f) (volume fractions near 0 and near 1; the latter only where it is above -1), x = 1 - f, the doubles around
    the switch of the mantissa range at 1 + x = sqrt(1/2), and 0"""
    f = np.logspace(-18, -1, 6000)
    near1 = -(1.0 - f)
    near1 = near1[near1 > -1.0]
    return np.concatenate([-f, near1, 1.0 - f, -neighbours(1.0 - np.sqrt(0.5), 256), [0.0]])


def bernoulli_args():
    mag = np.logspace(-12, np.log10(700.0), 6000)
    mag[-1] = 700.0
    sw = neighbours(SERIES_U, 2048)
    return np.concatenate([mag, -mag, [0.0], sw, -sw])


# ---- assertion helpers: pure functions of arrays --------------------------------------------------------------------------------------
def ulp_error(got, ref):
    """|got - exact| in ulp of the exact value; ref = (hi, lo) with hi + lo exact, or one rounded array"""
    hi, lo = ref if isinstance(ref, tuple) else (ref, 0.0)
    got, hi = np.asarray(got, float), np.asarray(hi, float)
    with np.errstate(invalid='ignore', over='ignore'):
        err = np.abs((got - hi) - lo) / np.spacing(np.abs(hi))
    same = (got == hi) | (np.isnan(got) & np.isnan(hi))          # equal infinities
    return np.where(same & ~np.isfinite(hi), 0.0, np.where(np.isnan(err), np.inf, err))


def check_ulp(got, ref, bar, args=None, strict=False, what=''):
    """every error <= bar ulp (strict: < bar); returns (worst, its argument)"""
    err = ulp_error(got, ref)
    k = int(np.argmax(err))
    worst, at = float(err[k]), (None if args is None else float(np.asarray(args)[k]))
    ok = worst < bar if strict else worst <= bar
    assert ok, '%s: %.3f ulp at %r, bar %s%g' % (what, worst, at, '< ' if strict else '', bar)
    return worst, at


def rel_error(got, ref):
    hi, lo = ref if isinstance(ref, tuple) else (ref, 0.0)
    got, hi = np.asarray(got, float), np.asarray(hi, float)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        err = np.abs((got - hi) - lo) / np.abs(hi)
    return np.where(np.isnan(err), np.inf, err)


def check_rel(got, ref, bar, args=None, what=''):
    err = rel_error(got, ref)
    k = int(np.argmax(err))
    worst, at = float(err[k]), (None if args is None else float(np.asarray(args)[k]))
    assert worst <= bar, '%s: relative error %.3e at %r, bar %g' % (what, worst, at, bar)
    return worst, at


def check_bernoulli_switch(u, B, bar=B_ULP_BAR):
    """the last series value below |u| = 0.05 and the first value of the other branch lie within `bar` ulp of each other; returns
    {+0.05: (series value, other value, distance in ulp), -0.05: ...}"""
    u, B = np.asarray(u), np.asarray(B)
    out = {}
    for s in (1.0, -1.0):
        inner, outer = np.nextafter(s * SERIES_U, 0.0), s * SERIES_U
        (ki,), (ko,) = np.nonzero(u == inner)[0][:1], np.nonzero(u == outer)[0][:1]
        dist = abs(B[ki] - B[ko]) / np.spacing(max(B[ki], B[ko]))
        assert dist <= bar, 'B jumps by %.2f ulp at u = %+.2f (%r -> %r)' % (dist, outer, B[ki], B[ko])
        out[outer] = (float(B[ki]), float(B[ko]), float(dist))
    return out


def check_bernoulli_balance(u, B, bar=B_ULP_BAR):
    """|B(-u) - (B(u) + u)| <= bar ulp of max(B(u), B(-u)) for every u > 0 whose mirror image is among the arguments; the combination is
    formed in extended precision, so what is measured is the two function values.  Returns (worst in ulp, its u)"""
    u, B = np.asarray(u), np.asarray(B)
    index = {v: k for k, v in enumerate(u)}
    pos = [k for k, v in enumerate(u) if v > 0 and -v in index]
    neg = [index[-u[k]] for k in pos]
    assert len(pos) > 1000
    L = np.longdouble
    gap = np.abs(L(B[neg]) - (L(B[pos]) + L(u[pos]))).astype(float) / np.spacing(np.maximum(B[pos], B[neg]))
    k = int(np.argmax(gap))
    assert gap[k] <= bar, 'detailed balance: B(-u) - (B(u) + u) is %.2f ulp at u = %r' % (gap[k], u[pos[k]])
    return float(gap[k]), float(u[pos[k]])


def lane_ids():
    """what every lane feeds the column-lane exchanges: its lane id plus 0.25 (sums of four stay exact)"""
    return np.arange(64) + 0.25


def check_col_lanes(W, bcast, other, total):
    """outputs of the column-lane exchanges for the input lane_ids(), against index arithmetic on lane = 2 W point + W direction + column
    lane: bcast[Q] the lane Q of the own point and direction, other the same column lane of the other direction, total the sum over the W
    column lanes of the own direction.  Exact."""
    lane = np.arange(64)
    point, direction, col = lane // (2 * W), (lane // W) % 2, lane % W
    ident = lambda p, d, c: 2 * W * p + W * d + c
    for Q in range(W):
        want = ident(point, direction, Q) + 0.25
        bad = np.nonzero(bcast[Q] != want)[0]
        assert bad.size == 0, 'W = %d, broadcast of column lane %d: lane %d reads %r, expected %r' % (W, Q, bad[0], bcast[Q][bad[0]], want[bad[0]])
    want = ident(point, 1 - direction, col) + 0.25
    bad = np.nonzero(other != want)[0]
    assert bad.size == 0, 'W = %d, other direction: lane %d reads %r, expected %r' % (W, bad[0], other[bad[0]], want[bad[0]])
    want = sum(ident(point, direction, c) for c in range(W)) + 0.25 * W
    bad = np.nonzero(total != want)[0]
    assert bad.size == 0, 'W = %d, sum over the column lanes: lane %d holds %r, expected %r' % (W, bad[0], total[bad[0]], want[bad[0]])


def check_scan_onehot(out, rev=False):
    """out[i] = scan of the i-th unit vector: the step function from element i on (rev: up to element i), exactly"""
    n = out.shape[0]
    assert out.shape == (n, n)
    want = np.triu(np.ones((n, n))) if not rev else np.tril(np.ones((n, n)))
    bad = np.argwhere(out != want)
    assert bad.size == 0, 'input e_%d: element %d is %r' % (bad[0][0], bad[0][1], out[tuple(bad[0])])


def check_blocked_scan(x, xo, total, base, P, rev=False):
    """exact (integer-valued or one-hot input): xo the inclusive prefix (rev: suffix) sums, total the sum in every lane, base what the lane
    inherited from the lanes before (rev: after) it -- 0 in lane 0 (rev: lane 63)"""
    x = np.atleast_2d(x)
    want = np.cumsum(x[:, ::-1], axis=1)[:, ::-1] if rev else np.cumsum(x, axis=1)
    bad = np.argwhere(xo != want)
    assert bad.size == 0, 'case %d element %d: %r, expected %r' % (bad[0][0], bad[0][1], xo[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(total, np.repeat(x.sum(axis=1)[:, None], 64, axis=1)), 'total'
    lane_sum = x.reshape(x.shape[0], 64, P).sum(axis=2)
    if rev:
        wb = np.concatenate([np.cumsum(lane_sum[:, ::-1], axis=1)[:, ::-1][:, 1:], np.zeros((x.shape[0], 1))], axis=1)
    else:
        wb = np.concatenate([np.zeros((x.shape[0], 1)), np.cumsum(lane_sum, axis=1)[:, :-1]], axis=1)
    assert np.array_equal(base, wb), 'base'
    assert np.all(base[:, 63 if rev else 0] == 0.0)


def check_scan_bound(x, xo, ref, P):
    """random doubles: |xo - exact prefix sum| <= (P + 6) 2^-53 sum|x| (P serial plus 6 tree additions); returns the worst error / bar"""
    x = np.atleast_2d(x)
    bar = (P + 6) * 2.0 ** -53 * np.abs(x).sum(axis=1)[:, None]
    ratio = float((np.abs(xo - ref) / bar).max())
    assert ratio <= 1.0, 'prefix sums off by %.2f of the bound (P + 6) 2^-53 sum|x|' % ratio
    return ratio


def check_load(out, src, ldx):
    """out = what a load through a resource of ldx doubles returned: the source below ldx, 0.0 from ldx on (never what lies behind)"""
    n = out.size
    want = np.where(np.arange(n) < ldx, src[:n], 0.0)
    bad = np.nonzero(out != want)[0]
    assert bad.size == 0, 'ldx %d: element %d reads %r, expected %r' % (ldx, bad[0], out[bad[0]], want[bad[0]])


def check_store(after, before, vals, ldx):
    """after = the buffer a row of vals was stored into through a resource of ldx doubles: vals below ldx, untouched from ldx on"""
    want = before.copy()
    want[:ldx] = vals[:ldx]
    bad = np.nonzero(after != want)[0]
    assert bad.size == 0, 'ldx %d: element %d holds %r, expected %r' % (ldx, bad[0], after[bad[0]], want[bad[0]])


def check_window_load(w, row, nrec, P):
    idx = np.arange(64)[:, None] * P + np.arange(P + 2)[None, :]
    want = np.where(idx < nrec, row[np.minimum(idx, row.size - 1)], 0.0)
    bad = np.argwhere(w != want)
    assert bad.size == 0, 'resource of %d doubles: lane %d position %d reads %r, expected %r' % (nrec, bad[0][0], bad[0][1], w[tuple(bad[0])], want[tuple(bad[0])])


def window_store_expected(before, v, nrec, P, mode):
    want = before.copy()
    edge = STORE_WINDOW[mode] == 2
    for lane in range(64):
        for j in range(P):
            i = lane * P + j + (0 if edge else 1)
            if i < nrec:
                want[i] = v[lane, j + (0 if edge else 1)]
    return want


def check_window_store(after, before, v, nrec, P, mode):
    want = window_store_expected(before, v, nrec, P, mode)
    bad = np.nonzero(after != want)[0]
    assert bad.size == 0, 'resource of %d doubles: element %d holds %r, expected %r' % (nrec, bad[0], after[bad[0]], want[bad[0]])


def dense(a, c, m):
    T = np.eye(m)
    T[np.arange(1, m), np.arange(m - 1)] = a[1:m]
    T[np.arange(m - 1), np.arange(1, m)] = c[:m - 1]
    return T


def tridiag_bar(a, c, m, P):
    """kappa_inf(T) (P + 6) 2.2e-15, T the dense matrix of the m real rows"""
    return float(np.linalg.cond(dense(a, c, m), np.inf)) * (P + 6) * FAST_RCP_REL


def check_tridiag(a, c, d, x_hat, P, m=None, x_ref=None, bar=None):
    """forward error of the real rows against the multiprecision solution: max|x_hat - x| / max|x| <= kappa_inf(T) (P + 6) 2.2e-15.
    Returns error / bar.  (x_ref and bar may be handed in when they are already known: they depend on the system alone)"""
    m = 64 * P if m is None else m
    x_ref = ref_thomas(a, c, d, m) if x_ref is None else x_ref
    bar = tridiag_bar(a, c, m, P) if bar is None else bar
    err = np.abs(np.asarray(x_hat)[:m] - x_ref).max() / np.abs(x_ref).max()
    ratio = float(err / bar) if np.isfinite(err) else np.inf
    assert ratio <= 1.0, 'forward error %.3e is %.2f of the bar %.3e (P = %d, m = %d)' % (err, ratio, bar, P, m)
    return ratio


# ---- the tridiagonal systems --------------------------------------------------------------------------------------------------------
CLASSES = ('dominant', 'cn r=1', 'cn r=1e2', 'cn r=1e4', 'cn r=1 alt', 'cn r=1e2 alt', 'cn r=1e4 alt')
CN_CLASSES = CLASSES[1:]


def row_counts(P):
    return (64, 63, 3) if P == 1 else (64 * P, 64 * P - 1, 32 * P + 1)


class TriSystem(object):
    """One padded system of 64 P rows, m of them real: unit diagonal, a[0] = 0, c[m-1] = 0.  a, c, d: the padded rows continue the real
    ones, as step_kernel leaves them (its rows r >= m come out of the same stencil on finite inputs: pnp_kernels.hip); a2, c2, d2: a
    second finite filling of the rows r >= m (all three changed)."""

    def __init__(self, P, m, cls, g):
        n = 64 * P
        rng = np.random.default_rng([P, m, CLASSES.index(cls), g])
        j = np.arange(n)
        if cls == 'dominant':            # (i) |a| + |c| <= 0.5, random signs
            tot, split = rng.uniform(0.05, 0.5, n), rng.uniform(0.0, 1.0, n)
            a = tot * split * rng.choice([-1.0, 1.0], n)
            c = tot * (1.0 - split) * rng.choice([-1.0, 1.0], n)
            d = rng.uniform(-1.0, 1.0, n)
        else:                            # (ii) the Crank-Nicolson limit, r = D dt/dx^2, drift skew s varying along the row
            r = float(cls.split('=')[1].split()[0])
            s = 0.2 * np.sin(2.0 * np.pi * (1 + g) * j / n + 0.7 * g) * rng.uniform(0.5, 1.0, n)
            a = -(r / 2.0) * (1.0 - s) / (1.0 + r)
            c = -(r / 2.0) * (1.0 + s) / (1.0 + r)
            d = 1.0 + 0.5 * np.cos(2.0 * np.pi * (2 + g) * j / n) + 0.01 * rng.uniform(-1.0, 1.0, n)
            if cls.endswith('alt'):      # (iii) d of alternating sign
                d = d * np.where(j % 2, -1.0, 1.0)
        a[0] = 0.0
        c[m - 1] = 0.0
        self.P, self.m, self.cls, self.g = P, m, cls, g
        self.a, self.c, self.d = a, c, d
        self.a2, self.c2, self.d2 = a.copy(), c.copy(), d.copy()
        if m < n:
            k = n - m
            tot, split = rng.uniform(0.05, 0.5, k), rng.uniform(0.0, 1.0, k)
            self.a2[m:] = tot * split * rng.choice([-1.0, 1.0], k)
            self.c2[m:] = tot * (1.0 - split) * rng.choice([-1.0, 1.0], k)
            self.d2[m:] = rng.uniform(-3.0, 3.0, k)
            assert not np.any(self.a2[m:] == a[m:]) and not np.any(self.c2[m:] == c[m:]) and not np.any(self.d2[m:] == d[m:])
        self.x_ref = ref_thomas(a, c, d, m)
        self.bar = tridiag_bar(a, c, m, P)


@functools.lru_cache(maxsize=None)
def system(P, m, cls, g):
    return TriSystem(P, m, cls, g)


def systems(P):
    """every system of one P: the three row counts, the seven coefficient classes, three systems each (the G of a call)"""
    return [system(P, m, cls, g) for m in row_counts(P) for cls in CLASSES for g in range(3)]


# ---- plain fp64 emulations and their mutants ------------------------------------------------------------------------------------------
SEED_REL = 4.6e-8          # the bare v_rcp_f64 seed (pnp_wave.h: fast_rcp)


def emul_tridiag(a, c, d, rcp_rel=0.0):
    """fp64 Thomas solve of ALL padded rows, the way the device solves them (no row count: a non-zero c[m-1] lets the padding in);
    a, c, d: [..., n].  rcp_rel: relative error of every reciprocal, of alternating sign (the mutant: SEED_REL)"""
    a, c, d = (np.asarray(t, float) for t in (a, c, d))
    n = d.shape[-1]
    cp, dp, x = np.empty_like(d), np.empty_like(d), np.empty_like(d)
    cp[..., 0], dp[..., 0] = c[..., 0], d[..., 0]
    for i in range(1, n):
        r = (1.0 / (1.0 - a[..., i] * cp[..., i - 1])) * (1.0 + (rcp_rel if i % 2 else -rcp_rel))
        cp[..., i] = c[..., i] * r
        dp[..., i] = (d[..., i] - a[..., i] * dp[..., i - 1]) * r
    x[..., n - 1] = dp[..., n - 1]
    for i in range(n - 2, -1, -1):
        x[..., i] = dp[..., i] - cp[..., i] * x[..., i + 1]
    return x


def emul_bernoulli(u, k30240=1.0 / 30240.0):
    """the device's formulas in fp64 NumPy (libm expm1, true division); k30240: the u^6 coefficient of the series"""
    u = np.asarray(u, float)
    small = np.abs(u) < SERIES_U
    us = np.where(small, u, 0.0)
    u2 = us * us
    Bs = 1.0 - 0.5 * us + u2 * (1.0 / 12.0 + u2 * (-1.0 / 720.0 + u2 * k30240))
    dBs = -0.5 + us * (1.0 / 6.0 + u2 * (-1.0 / 180.0 + u2 * (1.0 / 5040.0)))
    ul = np.where(small, 1.0, u)
    with np.errstate(over='ignore', invalid='ignore'):
        rE = 1.0 / np.expm1(ul)
        Bl = ul * rE
        dBl = (1.0 - Bl - ul) * rE
    return np.where(small, Bs, Bl), np.where(small, dBs, dBl)


SCAN_STAGES = ('row_shr:1', 'row_shr:2', 'row_shr:4', 'row_shr:8', 'row_bcast:15', 'row_bcast:31')


def emul_wave_scan(v, skip=None, bcast31_rows=(2, 3)):
    """the six DPP stages of wave_scan_incl on [ncase, 64]; skip: index of a stage left out; bcast31_rows: the rows its last stage writes"""
    v = np.array(np.atleast_2d(v), float)
    lane = np.arange(64)
    for k, s in enumerate((1, 2, 4, 8)):
        if skip == k:
            continue
        src = np.where((lane % 16 >= s)[None, :], np.roll(v, s, axis=1), 0.0)
        v = v + src
    if skip != 4:
        add = np.zeros_like(v)
        for row in (1, 3):
            add[:, 16 * row:16 * row + 16] = v[:, 16 * row - 1][:, None]
        v = v + add
    if skip != 5:
        add = np.zeros_like(v)
        for row in bcast31_rows:
            add[:, 16 * row:16 * row + 16] = v[:, 31][:, None]
        v = v + add
    return v


def emul_blocked_scan(x, P, rev=False, skip=None):
    """blocked_scan in fp64: P - 1 serial additions per lane, six Hillis-Steele stages across the lanes (skip: one left out), the base
    added to every element.  Returns xo [ncase, 64 P], total [ncase, 64], base [ncase, 64]"""
    x = np.array(np.atleast_2d(x), float)
    n = x.shape[0]
    if rev:
        xo, total, base = emul_blocked_scan(x[:, ::-1], P, False, skip)
        return xo[:, ::-1], total, base[:, ::-1]
    b = x.reshape(n, 64, P).copy()
    for j in range(1, P):
        b[:, :, j] += b[:, :, j - 1]
    inc = b[:, :, P - 1].copy()
    for k in range(6):
        if skip == k:
            continue
        s = 1 << k
        sh = np.zeros_like(inc)
        sh[:, s:] = inc[:, :-s]
        inc = inc + sh
    base = np.concatenate([np.zeros((n, 1)), inc[:, :-1]], axis=1)
    b += base[:, :, None]
    return b.reshape(n, 64 * P), np.repeat(inc[:, 63:64], 64, axis=1), base


def emul_quad_perm(v, sel):
    """DPP quad_perm: lane i of every quad reads lane sel[i] of it"""
    v = np.asarray(v, float)
    lane = np.arange(64)
    return v[(lane & ~3) + np.asarray(sel)[lane & 3]]


COL_LANE_MUTANTS = ('bcast within the quad', 'other direction = partner lane', 'sum of one exchange')


def emul_col_lanes(W, v, mutant=None):
    """the exchanges of pnp_lane_cols.h as the moves the device makes (quad_perm, and the xor-4 shuffle of the lane quad).  Mutants: the
    pair's broadcast with the quad's control (both directions read the upward one); the other direction taken from lane ^ 1; the sum with
    its last exchange left out"""
    v = np.asarray(v, float)
    lane = np.arange(64)
    if W == 4 or mutant == COL_LANE_MUTANTS[0]:
        bcast = np.array([emul_quad_perm(v, [Q] * 4) for Q in range(W)])
    else:
        bcast = np.array([emul_quad_perm(v, [Q, Q, 2 + Q, 2 + Q]) for Q in range(W)])
    if mutant == COL_LANE_MUTANTS[1]:
        other = v[lane ^ 1]
    else:
        other = v[lane ^ 4] if W == 4 else emul_quad_perm(v, [2, 3, 0, 1])
    total = v + emul_quad_perm(v, [1, 0, 3, 2])
    if W == 4 and mutant != COL_LANE_MUTANTS[2]:
        total = total + emul_quad_perm(total, [2, 3, 0, 1])
    if W == 2 and mutant == COL_LANE_MUTANTS[2]:
        total = v.copy()
    return bcast, other, total


def emul_load(src, ldx, n, overrun=0):
    """n doubles read through a resource of ldx doubles (overrun: the range check ends that many doubles late)"""
    return np.where(np.arange(n) < ldx + overrun, src[:n], 0.0)


def emul_store(before, vals, ldx, overrun=0):
    after = before.copy()
    after[:ldx + overrun] = vals[:ldx + overrun]
    return after


def emul_window_load(row, nrec, P, overrun=0):
    idx = np.arange(64)[:, None] * P + np.arange(P + 2)[None, :]
    return np.where(idx < nrec + overrun, row[np.minimum(idx, row.size - 1)], 0.0)


CANARY = 1e300


def canaries(n, first=0):
    """distinct, non-zero, recognisable values for the slack behind a resource's end"""
    return -(CANARY + 1e285 * (first + np.arange(n)))


def distinct(n, first=1):
    """distinct non-zero source values"""
    return (first + np.arange(n)) + 0.25


# ---- the damped Newton update of the physical mode (pnp_math.h: newton_norm_species, newton_norm_phi, newton_damping, newton_floor_step, newton_free_volume,
# ---- newton_backtrack, newton_clip_row, newton_accept), written from oracle/pnp_physical.py: newton_step and at_rounding_floor -------------
RULE_NS = (1, 2, 7, 8)
RULE_TOL = 1e-10
FREE_MIN = 1e-12               # oracle/pnp_physical.py: FREE_MIN (tests/test_primitives_ref.py compares)
RULE_MUTANTS = ('no floor', 'floor at a fifth', 'no backtrack', 'backtrack always', 'no free_min', 'nan dropped (species)', 'nan dropped (potential)',
                'no damping', 'damping without the switch')
ACCEPT_MUTANTS = ('damped steps accepted', 'no tol exit', 'no estimate exit', 'estimate on the first iteration', 'estimate without contraction',
                  'no rounding floor', 'rounding floor at half', 'upd_prev kept after a damped step')


def newton_rule(N, rows):
    """the rule functions on the device: rows as newton_rule_rows returns them -> the dictionary newton_rule_twin returns (no 'free_min')"""
    c, du, cb, vol = (_in(rows[k]).reshape(-1, N) for k in ('c', 'du', 'cb', 'vol'))
    n = c.shape[0]
    lam, dphi, dphi_max = (_in(rows[k]).reshape(n) for k in ('lam', 'dphi', 'dphi_max'))
    cf, cn, row, damp = np.empty((n, N)), np.empty((n, N)), np.empty((n, 4)), np.empty(n)
    _check(load_library().catunit_newton_rule(N, n, _p(c), _p(du), _p(cb), _p(vol), _p(lam), _p(dphi), _p(dphi_max), _p(cf), _p(cn), _p(row), _p(damp)),
           'catunit_newton_rule')
    return {'cf': cf, 'cn': cn, 'floor': cf == 0.1 * c, 'back': row[:, 0] != 0.0, 'theta': row[:, 1], 'upd': row[:, 2], 'mphi': row[:, 3], 'damp': damp, 'damped': damp != 1.0}


def newton_accept(t):
    """newton_accept on the device: t [n][5] = (lam, upd, upd_prev, tol, estimate) -> accepted [n] (bool), upd_prev afterwards [n]"""
    t = _in(t).reshape(-1, 5)
    cols = [np.ascontiguousarray(t[:, k]) for k in range(5)]
    acc, prev = np.empty(t.shape[0]), np.empty(t.shape[0])
    _check(load_library().catunit_newton_accept(t.shape[0], *[_p(v) for v in cols], _p(acc), _p(prev)), 'catunit_newton_accept')
    return acc != 0.0, prev


class _FP(object):
    """fp64 as the device computes: every operation rounded once, a multiply-add where the header writes one"""
    num = staticmethod(float)

    @staticmethod
    def fma(a, b, c):
        if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
            with np.errstate(invalid='ignore', over='ignore'):
                return float(np.float64(a) * np.float64(b) + np.float64(c))
        return float(mpf(a) * mpf(b) + mpf(c))

    @staticmethod
    def div(a, b):
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            return float(np.float64(a) / np.float64(b))


class _MP(object):
    """exact arithmetic on the same doubles (200 bits)"""
    num = staticmethod(lambda v: mpf(float(v)))
    fma = staticmethod(lambda a, b, c: a * b + c)
    div = staticmethod(lambda a, b: a / b)


def _rule_row(X, c, du, cb, vol, lam, dphi, dphi_max, mutant):
    N = len(c)
    inf = X.num(np.inf)
    cf, floor = [], []
    for k in range(N):
        t = X.fma(lam, du[k], c[k])
        lo = (X.num(0.2) if mutant == 'floor at a fifth' else X.num(0.1)) * c[k]
        fl = bool(t < lo) and mutant != 'no floor'
        floor.append(fl)
        cf.append(lo if fl else t)
    f_old = f_new = X.num(0.0)
    for k in range(N):
        f_old = X.fma(vol[k], c[k], f_old)
        f_new = X.fma(vol[k], cf[k], f_new)
    free = 1 - f_old
    free_min = bool(X.num(0.1) * free < X.num(FREE_MIN)) and mutant != 'no free_min'
    target = X.num(FREE_MIN) if free_min else X.num(0.1) * free
    back = (bool((1 - f_new) < target) or mutant == 'backtrack always') and mutant != 'no backtrack'
    theta = X.div(free - target, f_new - f_old) if back else X.num(0.0)
    cn = [X.fma(theta, cf[k] - c[k], c[k]) for k in range(N)] if back else list(cf)

    upd = X.num(0.0)
    for k in range(N):
        rel = X.div(abs(du[k]), abs(c[k]) + abs(cb[k]) + X.num(1e-300))
        if du[k] != du[k] and mutant != 'nan dropped (species)':
            rel = inf
        upd = rel if rel > upd else upd            # (fmax: a NaN operand is dropped)
    mphi = abs(dphi)
    if mphi != mphi and mutant != 'nan dropped (potential)':
        mphi = inf
    damped = bool(mphi > dphi_max) and (dphi_max > 0 or mutant == 'damping without the switch') and mutant != 'no damping'
    return {'cf': cf, 'cn': cn, 'floor': floor, 'back': back, 'free_min': back and free_min, 'theta': theta, 'upd': upd, 'mphi': mphi,
            'damp': X.div(dphi_max, mphi) if damped else X.num(1.0), 'damped': damped}


RULE_VALUES = ('cf', 'cn', 'theta', 'upd', 'mphi', 'damp')
# ulp of the exact value: twice the worst error measured on the MI355X (profiles/primitives_unit.md: cf 0.500, cn 2.230, theta 10.168,
# upd 1.090, damp 0.498; mphi is |x|, exact).  theta is a quotient of two rounded sums, and cn after a backtrack carries its error
RULE_BARS = {'cf': 1.0, 'cn': 4.46, 'theta': 20.34, 'upd': 2.18, 'mphi': 0.0, 'damp': 1.0}
RULE_DECISIONS = ('floor', 'back', 'damped')


def newton_rule_twin(rows, exact=False, mutant=None):
    """the CPU twin, row by row.  exact: in multiprecision, the values as (hi, lo) pairs (rows with a non-finite input: evaluated in fp64,
    lo = 0).  Decisions: 'floor' [n][N], 'back', 'free_min' (the backtrack with 0.1 free < FREE_MIN), 'damped' [n]"""
    N = np.asarray(rows['c']).shape[1]
    out = {k: [] for k in RULE_VALUES + RULE_DECISIONS + ('free_min',)}
    for i in range(len(rows['lam'])):
        args = [rows[k][i] for k in ('c', 'du', 'cb', 'vol', 'lam', 'dphi', 'dphi_max')]
        finite = all(np.isfinite(np.asarray(a, float)).all() for a in args)
        X = _MP if exact and finite else _FP
        r = _rule_row(X, *[[X.num(v) for v in a] if np.ndim(a) else X.num(a) for a in args], mutant)
        for k in out:
            out[k].append(r[k])
    res = {k: np.array(out[k], dtype=bool).reshape(-1, N) if k == 'floor' else np.array(out[k], dtype=bool) for k in RULE_DECISIONS + ('free_min',)}
    for k in RULE_VALUES:
        flat = [v for r in out[k] for v in (r if isinstance(r, list) else [r])]
        if exact:
            hi, lo = _hilo([v if isinstance(v, mpf) else mpf(v) for v in flat])
            res[k] = (hi.reshape(-1, N), lo.reshape(-1, N)) if k in ('cf', 'cn') else (hi, lo)
        else:
            res[k] = np.array(flat, float).reshape(-1, N) if k in ('cf', 'cn') else np.array(flat, float)
    return res


def newton_rule_rows(N):
    """About 130 rows of N species: 'kind' names what each row is there for.  No comparison of the rule sits at a tie: the floor is missed
    or overshot by 5 % of c at least, the free volume left is at least four times or at most a tenth of what the backtrack allows, and
    where the 1e-12 floor of the free volume decides, the occupied fraction is exact in fp64 (dyadic volumes, concentrations powers of two)."""
    rng = np.random.default_rng(7000 + N)
    rows = {k: [] for k in ('c', 'du', 'cb', 'vol', 'lam', 'dphi', 'dphi_max', 'kind')}

    def add(kind, c, du, vol, lam, dphi=None, dphi_max=0.05):
        rows['kind'].append(kind)
        rows['c'].append(c)
        rows['du'].append(du)
        rows['cb'].append(rng.uniform(0.0, 20.0, N))
        rows['vol'].append(vol)
        rows['lam'].append(lam)
        rows['dphi'].append(rng.uniform(0.06, 0.3) * rng.choice([-1.0, 1.0]) if dphi is None else dphi)
        rows['dphi_max'].append(dphi_max)

    def filled(c, f):          # volumes with sum_k vol_k c_k = f (to rounding)
        w = rng.uniform(0.2, 1.0, N)
        return f * w / w.sum() / c
    for j in range(24):         # mild rows: no clip; the potential below and above dphi_max, dphi_max switched off
        c = rng.uniform(0.5, 50.0, N)
        add('plain', c, c * rng.uniform(-0.5, 0.5, N), filled(c, rng.uniform(0.05, 0.4)), 1.0 if j % 2 else rng.uniform(0.05, 0.95),
            dphi=rng.uniform(0.001, 0.04) * (-1.0) ** j if j % 3 == 0 else None, dphi_max=(0.05, 0.05, 0.0, -1.0)[j % 4])
    for j in range(24):         # the floor in some slots (every slot at N = 1), the others mild
        c = rng.uniform(0.5, 50.0, N)
        lam = 1.0 if j % 2 else rng.uniform(0.05, 0.95)
        hit = rng.uniform(size=N) < 0.5
        hit[rng.integers(N)] = True
        add('floor', c, np.where(hit, -c * rng.uniform(0.95, 3.0, N) / lam, c * rng.uniform(-0.5, 0.5, N)), filled(c, rng.uniform(0.05, 0.4)), lam)
    for j in range(24):         # crowded rows whose ions grow: the free volume would fall below a tenth
        c = rng.uniform(0.5, 50.0, N)
        lam = 1.0 if j % 2 else rng.uniform(0.3, 0.95)
        add('backtrack', c, c * rng.uniform(0.5, 2.0, N) / lam, filled(c, rng.uniform(0.7, 0.95)), lam)
    for j in range(12):         # ... with the floor in one slot as well (N >= 2: the others carry the growth)
        c = rng.uniform(0.5, 50.0, N)
        du = c * rng.uniform(0.8, 2.0, N)
        vol = filled(c, rng.uniform(0.7, 0.95))
        if N > 1:               # (the floored slot holds a tenth of the occupied volume)
            k = rng.integers(N)
            du[k] *= -1.5
            rest = (vol * c).sum() - vol[k] * c[k]
            vol = np.where(np.arange(N) == k, 0.1 * (vol * c).sum() / c, vol * 0.9 * (vol * c).sum() / rest)
        add('backtrack', c, du, vol, 1.0)
    for j in range(24):         # 0.1 free < 1e-12: f_old = 1 - d 2^-43 exactly, d = 36 .. 52 (free 4.1e-12 .. 5.9e-12)
        c = 2.0 ** rng.integers(-2, 4, N)
        w = rng.integers(1, 1024 // N, N) / 1024.0
        w[-1] = 1.0 - rng.integers(36, 53) * 2.0 ** -43 - w[:-1].sum()
        grow = j % 3 != 0       # two in three grow (backtrack with the 1e-12 target), the others shrink (no backtrack)
        add('free_min' if grow else 'free_min, shrinking', c, c * rng.uniform(0.1, 0.6, N) * (1.0 if grow else -1.0), w / c, 1.0)
    for bad in (np.nan, np.inf, -np.inf):       # a non-finite update in a species slot and in the potential slot
        for slot in sorted({0, N - 1}):
            c = rng.uniform(0.5, 50.0, N)
            du = c * rng.uniform(-0.5, 0.5, N)
            du[slot] = bad
            add('non-finite species', c, du, filled(c, 0.3), 1.0)
        c = rng.uniform(0.5, 50.0, N)
        add('non-finite potential', c, c * rng.uniform(-0.5, 0.5, N), filled(c, 0.3), 1.0, dphi=bad)
    return {k: (v if k == 'kind' else np.array(v)) for k, v in rows.items()}


def perturbed(rows, rel, seed):
    """every input moved by a relative `rel` of random sign"""
    rng = np.random.default_rng(seed)
    return {k: (v if k == 'kind' else v * (1.0 + rel * rng.choice([-1.0, 1.0], np.shape(v)))) for k, v in rows.items()}


def check_newton_rule(got, fp, exact, bars, kinds=None):
    """got against the twin: the decisions equal those of BOTH evaluations of the twin (fp64 and multiprecision agree: no tie), the values
    within bars[name] ulp of the multiprecision ones (non-finite rows: equal to the fp64 twin's, NaN matching NaN).  Returns the worst
    error per value in ulp"""
    for k in RULE_DECISIONS:
        assert np.array_equal(fp[k], exact[k]), 'the twin decides %r differently in fp64 and in multiprecision: an input sits at a tie' % k
        bad = np.argwhere(np.asarray(got[k]) != exact[k])
        assert bad.size == 0, '%s: row %d (%s) decides %r, the twin %r' % (k, bad[0][0], None if kinds is None else kinds[bad[0][0]], got[k][tuple(bad[0])], exact[k][tuple(bad[0])])
    worst = {}
    for k in RULE_VALUES:
        err = ulp_error(got[k], exact[k])
        err = np.where((np.asarray(got[k]) == 0.0) & (exact[k][0] == 0.0), 0.0, err)
        j = np.unravel_index(int(np.argmax(err)), err.shape)
        worst[k] = float(err[j])
        assert worst[k] <= bars[k], '%s: %.3f ulp in row %d (%s), bar %g' % (k, worst[k], j[0], None if kinds is None else kinds[j[0]], bars[k])
    return worst


# (lam, upd, upd_prev, tol, estimate) and what each tuple is there for; 'alone': exactly this exit fires
def newton_accept_tuples():
    tol, inf = RULE_TOL, np.inf
    t = [((1.0, 5e-11, inf, tol, 0), 'tol exit alone, first iteration'),
         ((1.0, 5e-11, 1e-3, tol, 0), 'tol exit alone'),
         ((1.0, 5e-11, 3e-5, tol, 1), 'below tol with the estimate as well'),
         ((1.0, 1e-8, 1e-4, tol, 1), 'estimate exit alone'),
         ((1.0, 1e-8, 1e-4, tol, 0), 'estimate switched off'),
         ((1.0, 1e-8, inf, tol, 1), 'estimate on the first iteration (upd_prev = inf)'),
         ((1.0, 3e-10, 1.5e-9, tol, 1), 'estimate below tol but contraction above a tenth'),
         ((1.0, 1e-6, 1e-4, tol, 1), 'estimate above tol'),
         ((1.0, 3.2e-9, 3e-9, tol, 0), 'rounding floor alone'),
         ((1.0, 3.2e-9, 3e-9, tol, 1), 'rounding floor alone (estimate on)'),
         ((1.0, 2.9e-9, 3e-9, tol, 0), 'inside 100 tol but shrinking'),
         ((1.0, 2e-8, 3e-9, tol, 0), 'not smaller, but above 100 tol'),
         ((1.0, 3e-9, 2e-8, tol, 0), 'previous update above 100 tol'),
         ((1.0, 3e-9, inf, tol, 0), 'inside 100 tol on the first iteration'),
         ((0.5, 1e-12, inf, tol, 0), 'damped step below tol'),
         ((0.999999, 1e-12, 1e-12, tol, 1), 'damped step below tol, every exit otherwise open'),
         ((0.25, 3.2e-9, 3e-9, tol, 1), 'damped step on the rounding floor'),
         ((1.0, 0.3, 0.9, tol, 1), 'far from the solution'),
         ((1.0, inf, 1e-9, tol, 1), 'infinite update (a NaN in the update)'),
         ((1.0, 5e-7, 1e-3, 1e-6, 0), 'another tolerance: tol exit'),
         ((1.0, 4e-5, 3e-5, 1e-6, 0), 'another tolerance: rounding floor')]
    for ratio in (0.5, 0.7, 0.9, 0.99):      # linearly converging: every update a fixed fraction of the one before, from 5e-9 down to below tol
        u = 5e-9
        while u / ratio >= tol:
            t.append(((1.0, u * ratio, u, tol, 0), 'linear sequence, ratio %g' % ratio))
            t.append(((1.0, u * ratio, u, tol, 1), 'linear sequence, ratio %g (estimate on)' % ratio))
            u *= ratio
    return np.array([a for a, _ in t], float), [w for _, w in t]


def newton_accept_twin(t, mutant=None):
    """oracle/pnp_physical.py: newton_step's exits and at_rounding_floor.  Returns accepted [n], upd_prev afterwards [n] and which of the three
    conditions held [n][3] (tol, estimate, rounding floor; all False on a damped step)"""
    acc, prev_out, fired = [], [], []
    for lam, upd, prev, tol, est in np.asarray(t, float).reshape(-1, 5):
        full = lam == 1.0 or mutant == 'damped steps accepted'
        w = 100.0 * tol
        with np.errstate(invalid='ignore', divide='ignore'):
            f = (bool(upd < tol) and mutant != 'no tol exit',
                 bool(est != 0 and (np.isfinite(prev) or mutant == 'estimate on the first iteration') and
                      (upd < 0.1 * prev or mutant == 'estimate without contraction') and upd * (upd / prev) < tol) and mutant != 'no estimate exit',
                 bool(prev < w and upd < w and (upd > 0.5 * prev if mutant == 'rounding floor at half' else upd >= prev)) and mutant != 'no rounding floor')
        f = f if full else (False, False, False)
        acc.append(any(f))
        fired.append(f)
        prev_out.append(upd if lam == 1.0 else (prev if mutant == 'upd_prev kept after a damped step' else np.inf))
    return np.array(acc), np.array(prev_out), np.array(fired)


def check_newton_accept(acc, prev_out, t, what=None):
    """the decision and the new upd_prev against the twin, exactly"""
    want, wprev, _ = newton_accept_twin(t)
    bad = np.nonzero(np.asarray(acc) != want)[0]
    assert bad.size == 0, 'tuple %d %r (%s): accepted %r, the twin %r' % (bad[0], tuple(np.asarray(t)[bad[0]]), None if what is None else what[bad[0]], acc[bad[0]], want[bad[0]])
    bad = np.nonzero(np.asarray(prev_out) != wprev)[0]
    assert bad.size == 0, 'tuple %d (%s): upd_prev becomes %r, the twin %r' % (bad[0], None if what is None else what[bad[0]], prev_out[bad[0]], wprev[bad[0]])


# ---- the per-lane LU of pnp_kin.h (factor, substitute): 64 systems of order T, one per lane ---------------------------------------------
LU_TS = (1, 2, 5, 9)
LU_SPECIAL = ('site row', 'tie', 'dead row', 'singular', 'infinite')          # lanes 0 .. 4; the other 59 are seeded random matrices
LU_NONSINGULAR = np.array([k not in (3, 4) for k in range(64)])


@functools.lru_cache(maxsize=None)
def lu_cases(T):
    """A [64, T, T], b [64, 2, T] (treat as read-only) and what the special lanes must show.  Entries of order 1 throughout.
      lane 0  the steady state's matrix with its site row on top: A[0][0] = 5e-8 against a column of order 1 -- the rows must be exchanged
      lane 1  column 0 holds its largest magnitude twice (rows i1 < i2, opposite signs): the comparison is strict, row i1 is the pivot row
      lane 2  the identity row of a dead adsorbate as the last row
      lane 3  exactly singular: upper triangular with a zero as its last diagonal entry -- the flag is set.  The entries above the diagonal
              are negative and b is positive, so every solution entry is +inf and no stored word is a NaN (IEEE 754 leaves the sign and
              payload of a generated NaN open, the equality of the test is bitwise)
      lane 4  A[0][0] = +inf: the flag is set; the multipliers of step 0 are zeros, the first solution entry is a zero, no NaN either"""
    rng = np.random.default_rng(9100 + T)
    A = rng.uniform(-1.0, 1.0, (64, T, T))
    b = rng.uniform(-1.0, 1.0, (64, 2, T))
    A[0] = rng.uniform(0.5, 1.5, (T, T)) * rng.choice([-1.0, 1.0], (T, T))
    A[0, 0, 0] = 5e-8
    i1, i2 = (0, T - 1) if T < 3 else (1, T - 1)
    A[1, :, 0] = rng.uniform(-0.5, 0.5, T)
    A[1, i1, 0], A[1, i2, 0] = 1.25, (-1.25 if i2 != i1 else 1.25)
    A[2, T - 1] = 0.0
    A[2, T - 1, T - 1] = 1.0
    A[3] = np.triu(-rng.uniform(0.5, 1.5, (T, T)), 1) + np.diag(rng.uniform(0.5, 1.5, T))
    A[3, T - 1, T - 1] = 0.0
    b[3] = rng.uniform(0.5, 1.5, (2, T))
    A[4, 0, 0] = np.inf
    return A, b, {'exchange': 0 if T == 1 else int(np.argmax(np.abs(A[0, :, 0]))), 'tie rows': (i1, i2)}


def emul_lu(A, b, strict=True, contract=False):
    """factor and substitute of pnp_kin.h replayed in fp64, lane by lane, in the header's operation order: every division and every
    multiply-subtract as separately rounded IEEE operations.  Returns what lu() returns.  Mutants: strict=False takes the LAST of equal
    magnitudes as the pivot; contract=True forms the multiply-subtracts of the elimination with one rounding"""
    A, b = np.array(A, float), np.array(b, float)
    T = A.shape[1]
    pivs, bad = np.zeros(64, np.uint64), np.zeros(64, np.uint64)

    def mulsub(c, f, v):
        return np.float64(_FP.fma(-float(f), float(v), float(c))) if contract else c - f * v
    with np.errstate(all='ignore'):
        for lane in range(64):
            J = A[lane]
            word, flag = 0, False
            for k in range(T):
                p, best = k, abs(J[k, k])
                for i in range(k + 1, T):
                    v = abs(J[i, k])
                    if v > best or (not strict and v == best):
                        p, best = i, v
                word |= p << (4 * k)
                J[[k, p]] = J[[p, k]]
                piv = J[k, k]
                flag = flag or not (piv != 0.0 and np.isfinite(piv))
                for i in range(k + 1, T):
                    f = J[i, k] / piv
                    J[i, k] = f
                    for c in range(k + 1, T):
                        J[i, c] = mulsub(J[i, c], f, J[k, c])
            pivs[lane], bad[lane] = word, int(flag)
            for x in b[lane]:
                for k in range(T):
                    p = (word >> (4 * k)) & 15
                    x[k], x[p] = x[p], x[k]
                for k in range(T):
                    for i in range(k + 1, T):
                        x[i] = x[i] - J[i, k] * x[k]
                for k in range(T - 1, -1, -1):
                    s = x[k]
                    for c in range(k + 1, T):
                        s = s - J[k, c] * x[c]
                    x[k] = s / J[k, k]
    return A, pivs, bad, b


def lu_backward_error(A, x, b):
    """the normwise backward error ||A x - b||_inf / (||A||_inf ||x||_inf + ||b||_inf) per lane and right-hand side [64, 2], the
    residual formed in extended precision"""
    L = np.longdouble
    with np.errstate(all='ignore'):          # (the singular and the infinite lane come out as inf or NaN)
        r = np.abs(np.einsum('lij,lqj->lqi', A.astype(L), x.astype(L)) - b.astype(L)).max(axis=2)
        return (r / (np.abs(A).sum(axis=2).max(axis=1)[:, None] * np.abs(x).max(axis=2) + np.abs(b).max(axis=2))).astype(float)


def lu_backward_bar(T):
    """8 T 2^(T-1) 2^-53: the textbook bound of Gaussian elimination with partial pivoting at its worst-case growth 2^(T-1)"""
    return 8.0 * T * 2.0 ** (T - 1) * 2.0 ** -53


def check_lu(got, want):
    """every stored word of the factors, the pivot words, the flags and the solutions, bit for bit.  Returns the number of words"""
    words = 0
    for name, g, w in zip(('factors', 'pivot rows', 'bad-pivot flag', 'solutions'), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, name
        gb, wb = g.view(np.uint64), w.view(np.uint64)
        bad = np.argwhere(gb != wb)
        assert bad.size == 0, '%s: lane %d%s holds %r (0x%016x), the replay %r (0x%016x); %d words differ' % (
            name, bad[0][0], '' if g.ndim == 1 else ' element %s' % (tuple(bad[0][1:]),), g[tuple(bad[0])], gb[tuple(bad[0])], w[tuple(bad[0])],
            wb[tuple(bad[0])], len(bad))
        words += g.size
    return words
