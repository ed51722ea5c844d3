"""NumPy restatement of include/catint_sens.h (test infrastructure): the sensitivities J du = -dF/dp of a stationary state of the physical
mode to its model parameters.  The right-hand sides are the analytic ones of the header's table; the operator is the oracle's own
Jacobian (oracle.pnp_physical.residual_and_jacobian with dt = inf).  Two independent solution methods -- LAPACK's banded LU with partial
pivoting on the point-major ordering with all columns at once, and the Schur recursion from the bulk row towards the wall with reduced
right-hand sides -- whose disagreement measures what rounding does to the case; tests/test_gpu_sens.py derives its tolerance from it."""
import numpy as np
from scipy.linalg import solve_banded

from oracle import pnp_physical as PH

KINDS = ('phiM', 'flux', 'c_bulk', 'D', 'kf', 'kr', 'wall_k', 'stern_capacitance', 'velocity')
FIELDS = ('dphi_surface', 'dc_surface', 'dsigma', 'dwall_flux', 'dcurrent')


def split(spec):
    """(kind, index) of 'phiM' / ('D', 1) / ..."""
    return (spec, 0) if isinstance(spec, str) else (spec[0], int(spec[1]))


def edge_derivative(p, c, phi, k):
    """Ju [nx-1] = dJhat_e/du of species k, as oracle.pnp_physical.residual_and_jacobian forms it"""
    w, _ = PH._steric(p, c)
    u = p.q[k] * p.beta * (phi[1:] - phi[:-1]) + (w[1:] - w[:-1])
    if p.velocity != 0.0:
        u = u - p.velocity * p.dx / (p.D[k] * p.w)
    _, dB = PH.bernoulli(u)
    return -p.w * ((dB + 1.0) * c[k, 1:] - dB * c[k, :-1])


def unit_products(p, c):
    """a [R][2][nx]: the unit-rate activity products gamma^m prod c of the left and the right side of every reaction"""
    nx = c.shape[1]
    gam = 1.0 / (1.0 - (p.vol[:, None] * c).sum(axis=0)) if p.mpb else np.ones(nx)
    a = np.ones((len(p.reactions), 2, nx))
    for r, rx in enumerate(p.reactions):
        for sd, side in enumerate((rx['lhs'], rx['rhs'])):
            prod = np.ones(nx)
            for _ in side:
                prod = prod * gam
            for j in side:
                prod = prod * c[j]
            a[r, sd] = prod
    return a


def net(p, r, k):
    rx = p.reactions[r]
    return float(list(rx['rhs']).count(k) - list(rx['lhs']).count(k))


def source(p, c, k, a=None):
    """R_k [nx] = sum_r net[r][k] (kf a_f - kr a_b)"""
    a = unit_products(p, c) if a is None else a
    R = np.zeros(c.shape[1])
    for r, rx in enumerate(p.reactions):
        R = R + net(p, r, k) * (rx['kf'] * a[r, 0] - rx['kr'] * a[r, 1])
    return R


def wall_flux(p, c, phi, flux):
    """jw [N]: the flux into the domain, prescribed + wall table"""
    jw = np.array(flux, float)
    for wk in p.wall_kinetics:
        g = PH.wall_rate_law(p, wk, c, phi)[0]
        jw = jw + np.asarray(wk['nu'], float) * wk['k'] * g
    return jw


def rhs(p, c, phi, flux, kind, index=0):
    """r [(N+1), nx] = -dF/dp, analytic, from the table of include/catint_sens.h.  flux [N]: the prescribed wall fluxes (None: p.flux)"""
    N, nx, dx = p.N, p.nx, p.dx
    flux = p.flux if flux is None else np.asarray(flux, float)
    r = np.zeros((N + 1, nx))
    h = np.diff(p.x)
    v = p.v
    if kind == 'phiM':
        r[N, 0] = 1.0 if p.CS is None else -dx * p.CS / p.eps
        for wk in p.wall_kinetics:
            g, _, al = PH.wall_rate_law(p, wk, c, phi)
            for k in range(N):
                r[k, 0] += wk['nu'][k] * wk['k'] * al * g * dx / p.D[k]
    elif kind == 'flux':
        r[index, 0] = dx / p.D[index]
    elif kind == 'c_bulk':
        r[index, nx - 1] = 1.0
    elif kind == 'D':
        k, D = index, p.D[index]
        Ju = edge_derivative(p, c, phi, k)
        s = p.velocity * h / (D * D)
        q2 = dx * dx / D / D
        R = source(p, c, k)
        r[k, 1:-1] = (-(Ju[1:] * s[1:]) + Ju[:-1] * s[:-1]) - q2 * v[1:-1] * R[1:-1]
        jw = wall_flux(p, c, phi, flux)[k]
        r[k, 0] = ((-(Ju[0] * s[0]) + 0.0) - q2 * v[0] * R[0]) + -(jw * dx / (D * D))
    elif kind in ('kf', 'kr'):
        a = unit_products(p, c)
        for k in range(N):
            rsv = dx * dx / p.D[k] * v[:-1]
            if kind == 'kf':
                r[k, :-1] = rsv * net(p, index, k) * a[index, 0, :-1]
            else:
                r[k, :-1] = -(rsv * net(p, index, k) * a[index, 1, :-1])
    elif kind == 'wall_k':
        wk = p.wall_kinetics[index]
        g = PH.wall_rate_law(p, wk, c, phi)[0]
        for k in range(N):
            r[k, 0] = wk['nu'][k] * g * dx / p.D[k]
    elif kind == 'stern_capacitance':
        assert p.CS is not None, 'the Stern capacitance of a Dirichlet wall'
        r[N, 0] = -(dx / p.eps) * (p.phiM - p.phi_pzc - phi[0])
    elif kind == 'velocity':
        for k in range(N):
            Ju = edge_derivative(p, c, phi, k)
            r[k, 1:-1] = (Ju[1:] * h[1:] - Ju[:-1] * h[:-1]) / p.D[k]
            r[k, 0] = (Ju[0] * h[0] - 0.0) / p.D[k]
    else:
        raise ValueError('unknown kind %r' % (kind,))
    return r


def jacobian(p, c, phi):
    _, L, M, U = PH.residual_and_jacobian(p, c, phi, c, np.inf)
    return L, M, U


def solve_banded_lu(L, M, U, rs):
    """LAPACK banded LU (partial pivoting), all columns at once.  rs [P][(N+1)][nx]; returns (du_0 [P][N+1], du_1 [P][N+1])"""
    nx, nb, _ = M.shape
    n = nx * nb
    kl = ku = 2 * nb - 1
    ab = np.zeros((kl + ku + 1, n))
    rr, ss = np.meshgrid(np.arange(nb), np.arange(nb), indexing='ij')
    for blk, joff in ((L, -1), (M, 0), (U, 1)):
        for i in range(max(0, -joff), min(nx, nx - joff)):
            ab[ku + (i * nb + rr) - ((i + joff) * nb + ss), (i + joff) * nb + ss] = blk[i]
    b = np.stack([r.T.reshape(-1) for r in rs], axis=1)
    x = solve_banded((kl, ku), ab, b)
    return x[:nb].T.copy(), x[nb:2 * nb].T.copy()


def solve_schur(L, M, U, rs):
    """The Schur recursion from the bulk row: y_i = D'_i^-1 g'_i, T_i = D'_i^-1 L_i, D'_{i-1} = M_{i-1} - U_{i-1} T_i,
    g'_{i-1} = r_{i-1} - U_{i-1} y_i; du_0 = D'_0^-1 g'_0 and du_1 = y_1 - T_1 du_0"""
    nx, nb, _ = M.shape
    G = np.stack([r.T for r in rs], axis=2)        # [nx][nb][P]
    D = M[nx - 1].copy()
    g = G[nx - 1].copy()
    T1 = y1 = None
    for i in range(nx - 1, 0, -1):
        sol = np.linalg.solve(D, np.concatenate([L[i], g], axis=1))
        T, y = sol[:, :nb], sol[:, nb:]
        if i == 1:
            T1, y1 = T, y
        D = M[i - 1] - U[i - 1] @ T
        g = G[i - 1] - U[i - 1] @ y
    du0 = np.linalg.solve(D, g)
    du1 = y1 - T1 @ du0
    return du0.T.copy(), du1.T.copy()


METHODS = {'banded': solve_banded_lu, 'schur': solve_schur}


def outputs(p, c, phi, spec, du0, du1):
    """The header's outputs of one parameter from du_0, du_1 [N+1]"""
    N = p.N
    kind, index = split(spec)
    dphiM = 1.0 if kind == 'phiM' else 0.0
    drive = dphiM - du0[N]
    out = {'dphi_surface': du0[N], 'dc_surface': du0[:N].copy()}
    if p.CS is not None:
        out['dsigma'] = p.CS * drive
        if kind == 'stern_capacitance':
            out['dsigma'] = out['dsigma'] + (p.phiM - p.phi_pzc - phi[0])
    else:
        h0 = p.x[1] - p.x[0]
        out['dsigma'] = -p.eps / h0 * (du1[N] - du0[N]) + -0.5 * h0 * (p.q * du0[:N]).sum()
    dj = np.zeros(N)
    if kind == 'flux':
        dj[index] = 1.0
    if kind == 'wall_k':
        wk = p.wall_kinetics[index]
        dj = dj + np.asarray(wk['nu'], float) * PH.wall_rate_law(p, wk, c, phi)[0]
    for wk in p.wall_kinetics:
        g, dg, al = PH.wall_rate_law(p, wk, c, phi)
        dcs = du0[wk['species']] if wk['species'] >= 0 else 0.0
        dj = dj + np.asarray(wk['nu'], float) * wk['k'] * (dg * dcs + al * g * drive)
    out['dwall_flux'] = dj
    out['dcurrent'] = (p.q * dj).sum()
    return out


def expand(p, specs):
    """[(terms)] per spec: ('c_bulk', weights [N]) is the weighted sum of the single-species columns"""
    plan = []
    for spec in specs:
        if not isinstance(spec, str) and spec[0] == 'c_bulk' and np.ndim(spec[1]) > 0:
            plan.append([(('c_bulk', k), float(wt)) for k, wt in enumerate(spec[1]) if wt != 0.0])
        else:
            plan.append([(spec, 1.0)])
    return plan


def sensitivities(p, c, phi, specs, flux=None, method='banded'):
    """One operating point: dict of the header's outputs, each [P]... in the order of `specs`"""
    L, M, U = jacobian(p, c, phi)
    plan = expand(p, specs)
    single = []
    for terms in plan:
        for s, _ in terms:
            if s not in single:
                single.append(s)
    du0, du1 = METHODS[method](L, M, U, [rhs(p, c, phi, flux, *split(s)) for s in single])
    per = [outputs(p, c, phi, s, du0[m], du1[m]) for m, s in enumerate(single)]
    res = {}
    for name in FIELDS:
        rows = []
        for terms in plan:
            if len(terms) == 1 and terms[0][1] == 1.0:
                rows.append(np.asarray(per[single.index(terms[0][0])][name], float))
            else:
                acc = np.zeros_like(np.asarray(per[0][name], float))
                for s, wt in terms:
                    acc = acc + wt * np.asarray(per[single.index(s)][name], float)
                rows.append(acc)
        res[name] = np.array(rows)
    res['du0'] = du0
    return res


def rel_columns(a, b):
    """[P]: per column (parameter) the max-norm difference relative to the column's maximum in b; a column that is zero in b must be
    zero in a (then 0, else inf)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    scale = np.abs(b).max(axis=1)
    diff = np.abs(a - b).max(axis=1)
    return np.where(scale > 0, diff / np.where(scale > 0, scale, 1.0), np.where(diff > 0, np.inf, 0.0))


def disagreement(ra, rb):
    """per output: [P], the relative difference of two results column by column"""
    return {k: rel_columns(ra[k], rb[k]) for k in FIELDS}
