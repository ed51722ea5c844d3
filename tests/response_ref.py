"""NumPy restatement of include/catint_response.h (test infrastructure): the linear response (J + i omega S) du = r of a state of the
physical mode, built from the oracle's own Jacobian (oracle.pnp_physical.residual_and_jacobian with dt = inf) and wall_rate_law, and
solved in two independent ways -- LAPACK's banded LU with partial pivoting on the point-major ordering (the complex analogue of
oracle.pnp_physical.solve_block_tridiagonal) and a block elimination from the bulk row towards the wall.  The disagreement of the two
measures what rounding does to the case; tests/test_gpu_response.py derives its tolerance from it."""
import numpy as np
from scipy.linalg import solve_banded

from oracle import pnp_physical as PH

PHIM = 'phiM'
SCALARS = ('dphi_surface', 'dc_surface', 'dsigma', 'dwall_flux', 'admittance')


def operator(p, c, phi, omega):
    """(L, M + i omega S, U) [nx, N+1, N+1] at the state (c, phi)"""
    _, L, M, U = PH.residual_and_jacobian(p, c, phi, c, np.inf)
    M = M.astype(complex)
    if omega != 0.0:
        for k in range(p.N):
            M[:-1, k, k] += 1j * omega * (p.dx * p.dx / p.D[k]) * p.v[:-1]
    return L, M, U


def rhs(p, c, phi, perturbation):
    """r [(N+1), nx]: -dF/dphiM, or -dF/dflux_j for ('flux', j)"""
    r = np.zeros((p.N + 1, p.nx))
    if perturbation == PHIM:
        r[p.N, 0] = 1.0 if p.CS is None else -p.dx * p.CS / p.eps
        for wk in p.wall_kinetics:
            g, _, al = PH.wall_rate_law(p, wk, c, phi)
            for k in range(p.N):
                r[k, 0] += wk['nu'][k] * wk['k'] * al * g * p.dx / p.D[k]
    else:
        j = int(perturbation[1])
        r[j, 0] = p.dx / p.D[j]
    return r


def solve_banded_lu(L, M, U, r):
    """LAPACK banded LU (partial pivoting) on the point-major ordering; r, result [(N+1), nx]"""
    nx, nb, _ = M.shape
    n = nx * nb
    kl = ku = 2 * nb - 1
    ab = np.zeros((kl + ku + 1, n), dtype=M.dtype)
    rr, ss = np.meshgrid(np.arange(nb), np.arange(nb), indexing='ij')
    for blk, joff in ((L, -1), (M, 0), (U, 1)):
        for i in range(max(0, -joff), min(nx, nx - joff)):
            ab[ku + (i * nb + rr) - ((i + joff) * nb + ss), (i + joff) * nb + ss] = blk[i]
    return solve_banded((kl, ku), ab, r.T.reshape(-1).astype(M.dtype)).reshape(nx, nb).T


def solve_elimination(L, M, U, r):
    """Block Thomas from the bulk row towards the wall: [T_i | rt_i] = D'_i^-1 [L_i | r_i], D'_{i-1} = M_{i-1} - U_{i-1} T_i,
    r_{i-1} -= U_{i-1} rt_i; du_0 = D'_0^-1 r_0, du_i = rt_i - T_i du_{i-1}"""
    nx, nb, _ = M.shape
    r = r.T.astype(M.dtype).copy()
    T = np.zeros((nx, nb, nb), dtype=M.dtype)
    rt = np.zeros((nx, nb), dtype=M.dtype)
    D = M[nx - 1].copy()
    for i in range(nx - 1, 0, -1):
        sol = np.linalg.solve(D, np.concatenate([L[i], r[i][:, None]], axis=1))
        T[i], rt[i] = sol[:, :nb], sol[:, nb]
        D = M[i - 1] - U[i - 1] @ T[i]
        r[i - 1] = r[i - 1] - U[i - 1] @ rt[i]
    du = np.zeros((nx, nb), dtype=M.dtype)
    du[0] = np.linalg.solve(D, r[0])
    for i in range(1, nx):
        du[i] = rt[i] - T[i] @ du[i - 1]
    return du.T


METHODS = {'banded': solve_banded_lu, 'elimination': solve_elimination}


def outputs(p, c, phi, du, omega, perturbation):
    """The header's outputs from the solution du [(N+1), nx] (complex)"""
    N = p.N
    dphiM = 1.0 if perturbation == PHIM else 0.0
    out = {'dphi_surface': du[N, 0], 'dc_surface': du[:N, 0].copy(), 'dc': du[:N].copy(), 'dphi': du[N].copy()}
    if p.CS is not None:
        out['dsigma'] = p.CS * (dphiM - du[N, 0])
    else:
        h0 = p.x[1] - p.x[0]
        out['dsigma'] = -p.eps * (du[N, 1] - du[N, 0]) / h0 - 0.5 * h0 * (p.q * du[:N, 0]).sum()
    dj = np.zeros(N, dtype=complex)
    if perturbation != PHIM:
        dj[int(perturbation[1])] = 1.0
    for wk in p.wall_kinetics:
        g, dg, al = PH.wall_rate_law(p, wk, c, phi)
        dcs = du[wk['species'], 0] if wk['species'] >= 0 else 0.0
        dj = dj + np.asarray(wk['nu'], float) * wk['k'] * (dg * dcs + al * g * (dphiM - du[N, 0]))
    out['dwall_flux'] = dj
    out['admittance'] = 1j * omega * out['dsigma'] + (p.q * dj).sum()
    return out


def response(p, c, phi, omega=0.0, perturbation=PHIM, method='banded'):
    """One (operating point, frequency): dict of the header's outputs, complex (profiles 'dc' [N][nx], 'dphi' [nx])"""
    L, M, U = operator(p, c, phi, omega)
    du = METHODS[method](L, M, U, rhs(p, c, phi, perturbation))
    return outputs(p, c, phi, np.asarray(du, dtype=complex), omega, perturbation)


def rel_rows(a, b):
    """per-unknown max-norm relative difference: every row (last axis) scaled by its own maximum in b; rows that are zero in b must be
    zero in a (then 0)"""
    a, b = np.atleast_1d(np.asarray(a, complex)), np.atleast_1d(np.asarray(b, complex))
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    scale = np.abs(b).max(axis=1)
    diff = np.abs(a - b).max(axis=1)
    return float(np.max(np.where(scale > 0, diff / np.where(scale > 0, scale, 1.0), np.where(diff > 0, np.inf, 0.0))))


def disagreement(ra, rb):
    """Worst per-unknown relative difference of two results over profiles and scalars"""
    worst = 0.0
    for key in ('dc', 'dphi'):
        if key in ra and key in rb:
            worst = max(worst, rel_rows(ra[key], rb[key]))
    for key in SCALARS:
        a, b = np.atleast_1d(ra[key]).reshape(-1, 1), np.atleast_1d(rb[key]).reshape(-1, 1)
        worst = max(worst, rel_rows(a, b))
    return worst
