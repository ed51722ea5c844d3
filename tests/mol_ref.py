"""Multiprecision restatement of the reference's method-of-lines right-hand side (test infrastructure): ode_func, catint/calculator_old.py
:827-935, with get_potential_and_gradient (:680-819) and get_rates (:159-208), in mpmath at 60 digits.  Same equations as
oracle/pnp_ref.py mol_rhs -- the wall cell without a rate term, the bulk point zero, the Lax-Friedrichs term, migration off, the rate
table's overwrite order, the five Poisson boundary combinations (the Dirichlet-Dirichlet one by a tridiagonal elimination, the others by
the reference's prefix sums) -- evaluated from the fp64 inputs taken as exact numbers.  At 60 digits the rounding of this file is far
below one fp64 ulp of any result, so the distance of an fp64 evaluation from it is that evaluation's own error: tests/test_mol_rhs_ref.py
measures the fp64 oracle's (E_oracle), tests/test_gpu_mol_rhs.py holds the device kernels to a multiple of it.  Practical up to a few
hundred grid points (every number is an mpf)."""
import mpmath
import numpy as np

DPS = 60
ctx = mpmath.mp.clone()
ctx.dps = DPS
F = ctx.mpf


def _f(x):
    return F(float(x))


def poisson(C, p):
    """v, grad_v, lapl_v (lists of mpf) of the state C[N][nx] (mpf): oracle/pnp_ref.py poisson"""
    nx, dx, eps = p.nx, _f(p.dx), _f(p.eps)
    q = [_f(x) for x in p.charges]
    lapl = [F(0)] * nx
    for k in range(p.N):
        lapl = [l - q[k] * c / eps for l, c in zip(lapl, C[k])]
    v, g = [F(0)] * nx, [F(0)] * nx
    vw, vb, gw, gb = [None if np.isnan(x) else _f(x) for x in p.pb]
    if gw is not None and gb is not None:
        raise ValueError('Cannot use two boundary conditions for gradient')
    if vw is not None:
        v[0] = vw
    if vb is not None:
        v[-1] = vb
    if vw is not None and vb is not None:
        # v[i-1] - 2 v[i] + v[i+1] = lapl[i] dx^2 on the interior: elimination of the (1, -2, 1) system
        m = nx - 2
        b = [lapl[i + 1] * dx ** 2 for i in range(m)]
        b[0] -= v[0]
        b[-1] -= v[-1]
        cp, dp = [F(0)] * m, [F(0)] * m
        cp[0], dp[0] = F(1) / F(-2), b[0] / F(-2)
        for i in range(1, m):
            den = F(-2) - cp[i - 1]
            cp[i] = F(1) / den
            dp[i] = (b[i] - dp[i - 1]) / den
        x = [F(0)] * m
        x[-1] = dp[-1]
        for i in range(m - 2, -1, -1):
            x[i] = dp[i] - cp[i] * x[i + 1]
        v[1:nx - 1] = x
        for i in range(1, nx - 1):
            g[i] = (v[i + 1] - v[i - 1]) / (2 * dx)
        g[0] = g[1] + (g[1] - g[2])
        g[-1] = g[-2] + (g[-2] - g[-3])
        return v, g, lapl
    if gw is not None:
        g[0] = gw
        for i in range(1, nx - 1):
            g[i] = g[i - 1] + lapl[i] * dx
        g[-1] = g[-2] + (g[-2] - g[-3])
    if gb is not None:
        g[-1] = gb
        for i in range(nx - 2, 0, -1):
            g[i] = g[i + 1] - lapl[i] * dx
        g[0] = g[1] + (g[1] - g[2])
    if vw is not None:
        for i in range(1, nx - 1):
            v[i] = v[i - 1] + g[i] * dx
        v[-1] = v[-2] + (v[-2] - v[-3])
    if vb is not None:
        for i in range(nx - 2, 0, -1):
            v[i] = v[i + 1] - g[i] * dx
        v[0] = v[1] + (v[1] - v[2])
    return v, g, lapl


def get_rates(C, p):
    """rates[N][nx] (mpf) with the reference's order: every reaction OVERWRITES the rate of each species it touches (:173, :193), so a
    species keeps the contribution of the last reaction that names it (and, named twice on one side, of that reaction once)."""
    nx = len(C[0])
    rates = [[F(0)] * nx for _ in range(p.N)]
    for lhs, rhs, kf, kr in p.reactions:
        kf, kr = _f(kf), _f(kr)
        pl, pr = [F(1)] * nx, [F(1)] * nx
        for k in lhs:
            pl = [a * c for a, c in zip(pl, C[k])]
        for k in rhs:
            pr = [a * c for a, c in zip(pr, C[k])]
        for k in lhs:
            rates[k] = [b * kr - a * kf for a, b in zip(pl, pr)]
        for k in rhs:
            rates[k] = [a * kf - b * kr for a, b in zip(pl, pr)]
    return rates


def mol_rhs(c, p, use_reactions=False):
    """dc/dt of the flat fp64 state c[N*nx] as an object array of mpf [N*nx]"""
    N, nx = p.N, p.nx
    dx, dt, beta = _f(p.dx), _f(p.dt), _f(p.beta)
    C = [[_f(x) for x in row] for row in np.asarray(c, float).reshape(N, nx)]
    g = poisson(C, p)[1] if p.use_migration else [F(0)] * nx
    rates = get_rates(C, p) if use_reactions else [[F(0)] * nx for _ in range(N)]
    out = np.empty((N, nx), dtype=object)
    for k in range(N):
        D, q, c_, flux = _f(p.D[k]), _f(p.charges[k]), C[k], _f(p.flux_bound[k])
        corr = (c_[1] - c_[0]) / dt if p.lax_friedrich else F(0)
        out[k, 0] = corr + (D * ((c_[2] - c_[0]) / (2 * dx) + beta * q * c_[1] * g[1]) - flux) / dx      # wall cell: no rate term
        for i in range(1, nx - 1):
            d2 = (c_[i + 1] - 2 * c_[i] + c_[i - 1]) / dx ** 2
            dcg = (c_[i + 1] * g[i + 1] - c_[i - 1] * g[i - 1]) / (2 * dx)          # g = 0 without migration
            corr = d2 * dx ** 2 / dt / 2 if p.lax_friedrich else F(0)
            out[k, i] = corr + D * (d2 + beta * q * dcg) + rates[k][i]
        out[k, nx - 1] = F(0)                                                        # bulk point
    return out.reshape(-1)


def rates_array(c, p):
    N, nx = p.N, p.nx
    C = [[_f(x) for x in row] for row in np.asarray(c, float).reshape(N, nx)]
    return np.array(get_rates(C, p), dtype=object).reshape(-1)


def row_errors(f, ref, N):
    """[N]: per species row max |f - ref| scaled by that row's max |ref| (ref: fp64 or mpf; an all-zero reference row: absolute)."""
    f = np.asarray(f).reshape(N, -1)
    ref = np.asarray(ref).reshape(N, -1)
    out = np.zeros(N)
    for k in range(N):
        if ref.dtype == object:
            d = max(abs(_f(a) - b) for a, b in zip(f[k], ref[k]))
            s = max(abs(b) for b in ref[k])
            out[k] = float(d / s) if s != 0 else float(d)
        else:
            d, s = np.abs(f[k] - ref[k]).max(), np.abs(ref[k]).max()
            out[k] = d / s if s != 0 else d
            if not np.isfinite(f[k]).all():
                out[k] = np.inf
    return out


def assert_rows_within(f, ref, N, bar, what=''):
    """The assertion of tests/test_gpu_mol_rhs.py: every lane, every species row of f[B][N*nx] within `bar` of ref[B] (row-scaled).
    Returns the largest error seen."""
    worst = 0.0
    for b in range(len(ref)):
        e = row_errors(f[b], ref[b], N)
        k = int(np.argmax(e))
        assert e[k] <= bar, '%s lane %d species %d: error %.3e of the row maximum, bar %.3e' % (what, b, k, e[k], bar)
        worst = max(worst, float(e[k]))
    return worst
