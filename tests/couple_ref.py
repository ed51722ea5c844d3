"""NumPy restatement of include/catint_couple.h (test infrastructure): the transport tangent T = W^-1 E of a stationary state of the
physical mode, built from the oracle's own Jacobian (oracle.pnp_physical.residual_and_jacobian with dt = inf, no wall table), in two
independent ways -- LAPACK's banded LU with partial pivoting on the point-major ordering with the N right-hand sides at once, and the
Schur recursion from the bulk row towards the wall -- and the Newton step of the self-consistency that follows from it.  The
disagreement of the two measures what rounding does to the case; tests/test_gpu_couple.py derives its tolerance from it."""
import numpy as np
from scipy.linalg import solve_banded

from oracle import pnp_physical as PH

SINGULAR, GROWTH = 1e-12, 1e8
FIELDS = ('T_c', 'T_phi', 'dflux', 'lambda', 'flux_new', 'dc_surface', 'dphi_surface')


def jacobian(p, c, phi):
    """(L, M, U) [nx, N+1, N+1] of the stationary residual at (c, phi); the problem must carry no wall table"""
    assert not p.wall_kinetics, 'the coupling is defined without a wall table'
    _, L, M, U = PH.residual_and_jacobian(p, c, phi, c, np.inf)
    return L, M, U


def wall_rhs(p):
    """E [(N+1), N]"""
    E = np.zeros((p.N + 1, p.N))
    for k in range(p.N):
        E[k, k] = p.dx / p.D[k]
    return E


def tangent_banded(p, c, phi):
    """T [(N+1), N]: banded LU (partial pivoting) of the whole operator against the N columns of E at the wall point"""
    L, M, U = jacobian(p, c, phi)
    nx, nb, _ = M.shape
    n = nx * nb
    kl = ku = 2 * nb - 1
    ab = np.zeros((kl + ku + 1, n))
    rr, ss = np.meshgrid(np.arange(nb), np.arange(nb), indexing='ij')
    for blk, joff in ((L, -1), (M, 0), (U, 1)):
        for i in range(max(0, -joff), min(nx, nx - joff)):
            ab[ku + (i * nb + rr) - ((i + joff) * nb + ss), (i + joff) * nb + ss] = blk[i]
    rhs = np.zeros((n, p.N))
    rhs[:nb] = wall_rhs(p)
    return solve_banded((kl, ku), ab, rhs)[:nb]


def schur_block(p, c, phi):
    """W = D'_0: D'_{nx-1} = M_{nx-1}, D'_{i-1} = M_{i-1} - U_{i-1} D'_i^-1 L_i"""
    L, M, U = jacobian(p, c, phi)
    D = M[-1].copy()
    for i in range(M.shape[0] - 1, 0, -1):
        D = M[i - 1] - U[i - 1] @ np.linalg.solve(D, L[i])
    return D


def tangent_schur(p, c, phi):
    return np.linalg.solve(schur_block(p, c, phi), wall_rhs(p))


METHODS = {'banded': tangent_banded, 'schur': tangent_schur}


def newton_matrix(T, Kc, Kphi, rf=1.0):
    """(A, scale): A = I - rf (Kc T_c + Kphi (x) T_phi); scale: the largest magnitude among the entries of A and the two terms each is
    the difference of (the header's scale of the singularity check)"""
    N = T.shape[1]
    X = rf * (np.asarray(Kc, float) @ T[:N] + np.outer(Kphi, T[N]))
    A = np.eye(N) - X
    return A, max(np.abs(A).max(), 1.0, np.abs(X).max())


def solve_pivoted(A, b, scale):
    """Gaussian elimination with partial row pivoting; (x, singular): a pivot that is zero, not finite or below SINGULAR * scale"""
    A, b = np.array(A, float), np.array(b, float)
    n = len(b)
    singular = False
    with np.errstate(all='ignore'):
        for p in range(n):
            col = np.where(np.isfinite(A[p:, p]), np.abs(A[p:, p]), np.inf)
            q = p + int(np.argmax(col))
            A[[p, q]], b[[p, q]] = A[[q, p]], b[[q, p]]
            piv = A[p, p]
            if piv == 0.0 or not np.isfinite(piv) or abs(piv) < SINGULAR * scale:
                singular = True
            for r in range(p + 1, n):
                f = A[r, p] / piv
                A[r, p:] -= f * A[p, p:]
                b[r] -= f * b[p]
        x = np.zeros(n)
        for p in range(n - 1, -1, -1):
            x[p] = (b[p] - A[p, p + 1:] @ x[p + 1:]) / A[p, p]
    return x, singular or not np.isfinite(x).all()


def damping(cs, dcs, dphi, dphi_max):
    """The largest lambda in (0, 1] that keeps every positive surface concentration above a tenth of its value and the step of the
    surface potential within dphi_max (<= 0: no limit)"""
    lam = 1.0
    for k in range(len(cs)):
        if cs[k] > 0.0 and dcs[k] < 0.0:
            lam = min(lam, 0.9 * cs[k] / (-dcs[k]))
    if dphi_max > 0.0 and abs(dphi) > dphi_max:
        lam = min(lam, dphi_max / abs(dphi))
    return lam


def step_from_tangent(T, cs, g, K, Kc, Kphi, rf=1.0, dphi_max=0.05):
    """The header's outputs from T [(N+1), N] and the surface concentrations cs [N]"""
    N = T.shape[1]
    g, K = np.asarray(g, float), np.asarray(K, float)
    A, scale = newton_matrix(T, Kc, Kphi, rf)
    dg, singular = solve_pivoted(A, -(g - rf * K), scale)
    with np.errstate(all='ignore'):
        dcs, dphi = T[:N] @ dg, float(T[N] @ dg)
    lam = damping(cs, dcs, dphi, dphi_max)
    return {'T_c': T[:N].copy(), 'T_phi': T[N].copy(), 'dflux': dg, 'lambda': lam, 'flux_new': g + lam * dg, 'dc_surface': dcs,
            'dphi_surface': dphi, 'status': 3 if singular else 0, 'A': A, 'cond': np.linalg.cond(A) if np.isfinite(A).all() else np.inf}


def step(p, c, phi, g, K, Kc, Kphi, rf=1.0, dphi_max=0.05, method='banded'):
    """One operating point: the Newton step about the state (c [N][nx], phi [nx]) that was solved with the wall fluxes g"""
    return step_from_tangent(METHODS[method](p, c, phi), np.asarray(c)[:, 0], g, K, Kc, Kphi, rf, dphi_max)


def rel(a, b):
    """max-norm relative difference of two arrays of the same shape, scaled by the maximum of b (zero b: a must be zero)"""
    a, b = np.atleast_1d(np.asarray(a, float)), np.atleast_1d(np.asarray(b, float))
    scale = np.abs(b).max()
    diff = np.abs(a - b).max()
    return float(diff / scale) if scale > 0 else (0.0 if diff == 0 else np.inf)


def rel_T(a, b):
    """the tangent: every row (one unknown's answers to the N fluxes) scaled by its own maximum"""
    return max(rel(np.asarray(a)[i], np.asarray(b)[i]) for i in range(np.asarray(b).shape[0]))


def disagreement(ra, rb):
    """per output: the relative difference of two results"""
    out = {}
    for k in FIELDS:
        out[k] = rel_T(ra[k], rb[k]) if k == 'T_c' else rel(ra[k], rb[k])
    return out
