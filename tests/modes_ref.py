"""NumPy restatement of include/catint_modes.h (test infrastructure): the subspace iteration on A = J^-1 S for the relaxation modes of a
stationary state of the physical mode.  Nothing of the physics is restated: the operator is the oracle's own Jacobian
(oracle.pnp_physical.residual_and_jacobian with dt = inf), and the storage matrix is what the oracle itself adds for a finite time
step, S = dt (J(dt) - J(inf)).  Two independent solution methods -- LAPACK's banded LU with partial pivoting on the point-major
ordering, and the Schur recursion from the bulk row towards the wall with a substitution back -- whose disagreement measures what
rounding does to the case (tests/test_gpu_modes.py derives its tolerance from it), and a dense reference: the eigenvalues of
solve(J, diag(S)) with left eigenvectors for their condition numbers.  Both can be refined with residuals in extended precision, for
the comparison of the two with each other below the rounding error of a plain solve."""
import numpy as np
import scipy.linalg

from oracle import pnp_physical as PH

BREAKDOWN = 1e-10
# S / DT dwarfs every entry of J (S is 1e-12 .. 1e-9 s, J is O(1)), so the difference J(DT) - J(inf) is S / DT to the last bit
DT = 1e-30


def pencil(p, c, phi):
    """(L, M, U) [nx][N+1][N+1] of the stationary Jacobian and S [N+1][nx], the diagonal of the storage matrix"""
    _, L, M, U = PH.residual_and_jacobian(p, c, phi, c, np.inf)
    _, Lt, Mt, Ut = PH.residual_and_jacobian(p, c, phi, c, DT)
    assert np.array_equal(L, Lt) and np.array_equal(U, Ut)
    dM = Mt - M
    S = DT * np.einsum('ikk->ki', dM)
    off = dM.copy()
    off[:, np.arange(p.N + 1), np.arange(p.N + 1)] = 0.0
    assert not off.any() and not S[p.N].any() and not S[:, -1].any() and (S[:p.N, :-1] > 0).all()
    return L, M, U, S


def solve_banded_lu(L, M, U, R):
    """LAPACK banded LU (partial pivoting), all columns at once.  R [m][N+1][nx]; returns W [m][N+1][nx]"""
    nx, nb, _ = M.shape
    n = nx * nb
    kl = ku = 2 * nb - 1
    ab = np.zeros((kl + ku + 1, n))
    rr, ss = np.meshgrid(np.arange(nb), np.arange(nb), indexing='ij')
    for blk, joff in ((L, -1), (M, 0), (U, 1)):
        for i in range(max(0, -joff), min(nx, nx - joff)):
            ab[ku + (i * nb + rr) - ((i + joff) * nb + ss), (i + joff) * nb + ss] = blk[i]
    b = np.stack([r.T.reshape(-1) for r in R], axis=1)
    x = scipy.linalg.solve_banded((kl, ku), ab, b)
    return np.stack([x[:, j].reshape(nx, nb).T for j in range(len(R))])


def solve_schur(L, M, U, R):
    """The Schur recursion from the bulk row: y_i = D'_i^-1 g'_i, T_i = D'_i^-1 L_i, D'_{i-1} = M_{i-1} - U_{i-1} T_i,
    g'_{i-1} = r_{i-1} - U_{i-1} y_i; w_0 = D'_0^-1 g'_0 and w_i = y_i - T_i w_{i-1}"""
    nx, nb, _ = M.shape
    G = np.stack([r.T for r in R], axis=2)        # [nx][nb][m]
    D, g = M[nx - 1].copy(), G[nx - 1].copy()
    T, Y = [None] * nx, [None] * nx
    for i in range(nx - 1, 0, -1):
        sol = np.linalg.solve(D, np.concatenate([L[i], g], axis=1))
        T[i], Y[i] = sol[:, :nb], sol[:, nb:]
        D = M[i - 1] - U[i - 1] @ T[i]
        g = G[i - 1] - U[i - 1] @ Y[i]
    w = [np.linalg.solve(D, g)]
    for i in range(1, nx):
        w.append(Y[i] - T[i] @ w[-1])
    return np.stack(w, axis=0).transpose(2, 1, 0).copy()


METHODS = {'banded': solve_banded_lu, 'schur': solve_schur}


def apply_jacobian(L, M, U, X):
    """J X in numpy.longdouble.  X [m][N+1][nx]"""
    LD = np.longdouble
    x = np.asarray(X).astype(LD).transpose(2, 1, 0)        # [nx][nb][m]
    y = np.einsum('irs,ism->irm', M.astype(LD), x)
    y[1:] += np.einsum('irs,ism->irm', L[1:].astype(LD), x[:-1])
    y[:-1] += np.einsum('irs,ism->irm', U[:-1].astype(LD), x[1:])
    return y.transpose(2, 1, 0)


def solve(L, M, U, R, method='banded', refine=0):
    """J W = R with `refine` steps of iterative refinement, the residual formed in extended precision: with refine = 2 the solution is
    accurate to about eps instead of eps cond(J), which the comparison with a dense eigensolver needs (tests/test_modes_abi.py)"""
    W = METHODS[method](L, M, U, R)
    if refine:
        W = W.astype(np.longdouble)
        for _ in range(refine):
            W = W + METHODS[method](L, M, U, (np.asarray(R).astype(np.longdouble) - apply_jacobian(L, M, U, W)).astype(float))
        W = W.astype(float)
    return W


def orth(V):
    """Modified Gram-Schmidt, columns in order, Euclidean inner product over all entries.  V [m][...]; returns (Q, breakdown)"""
    Q = np.array(V, dtype=float, order='C')          # (C order: the rows of `flat` below are views)
    flat = Q.reshape(len(Q), -1)
    broke = False
    for k in range(len(flat)):
        before = np.linalg.norm(V[k])
        after = np.linalg.norm(flat[k])
        if not after > BREAKDOWN * before:
            broke = True
            flat[k] = 0.0
            continue
        flat[k] /= after
        for j in range(k + 1, len(flat)):
            flat[j] -= (flat[k] @ flat[j]) * flat[k]
    return Q, broke


def iterate(p, c, phi, start, iterations, method='banded', refine=0):
    """One operating point: {'ritz' B [m][m], 'gram' G [m][m], 'basis' Q [m][N+1][nx], 'breakdown'} after `iterations` passes;
    'history': [(B, G)] of every pass; 'cond': the 2-norm condition number of the columns the last orth was given (one Gram-Schmidt
    sweep leaves an overlap of the order eps cond between its columns)"""
    L, M, U, S = pencil(p, c, phi)
    Q, broke = orth(np.asarray(start, float))
    m = len(Q)
    history, cond = [], np.linalg.cond(np.asarray(start, float).reshape(m, -1))
    for it in range(iterations):
        W = solve(L, M, U, S[None] * Q, method, refine)
        q, w = Q.reshape(m, -1), W.reshape(m, -1)
        B = q @ w.T
        r = w - B.T @ q
        G = r @ r.T
        history.append((B, G))
        if it < iterations - 1:
            Q, b = orth(W)
            cond = np.linalg.cond(w)
            broke = broke or b
    return {'ritz': B, 'gram': G, 'basis': Q, 'breakdown': broke, 'history': history, 'cond': cond}


def ritz_pairs(B, G):
    """theta [m], s [m][m] (columns) = eig(B) by descending |theta|, and the relative residuals sqrt(s^H G s) / (|theta| |s|)"""
    theta, s = np.linalg.eig(B)
    order = np.lexsort((-theta.imag, -np.abs(theta)))
    theta, s = theta[order].astype(complex), s[:, order].astype(complex)
    num = np.sqrt(np.maximum(np.real(np.einsum('aj,ab,bj->j', s.conj(), G, s)), 0.0))
    return theta, s, num / (np.abs(theta) * np.linalg.norm(s, axis=0))


def dense(p, c, phi, refine=2):
    """(theta [n] by descending |theta|, kappa [n]): the eigenvalues of A = solve(J, diag(S)), point-major ordering, and their condition
    numbers 1 / |y^H x| from unit left and right eigenvectors.  The columns of A are refined as in `solve`"""
    L, M, U, S = pencil(p, c, phi)
    nx, nb, _ = M.shape
    n = nx * nb
    R = np.zeros((n, nb, nx))
    for i in range(nx):
        for r in range(nb):
            R[i * nb + r, r, i] = S[r, i]
    A = solve(L, M, U, R, 'banded', refine).transpose(2, 1, 0).reshape(n, n)
    theta, vl, vr = scipy.linalg.eig(A, left=True, right=True)
    with np.errstate(divide='ignore'):
        kappa = 1.0 / np.abs(np.einsum('ij,ij->j', vl.conj(), vr))
    order = np.lexsort((-theta.imag, -np.abs(theta)))
    return theta[order], kappa[order]


def projector(Q):
    """Q Q^T [(N+1) nx][(N+1) nx] of a basis [m][N+1][nx]"""
    q = np.asarray(Q, float).reshape(len(Q), -1)
    return q.T @ q


def match(theta, dense_theta):
    """per Ritz value the index of the nearest dense eigenvalue"""
    return np.array([int(np.argmin(np.abs(dense_theta - t))) for t in theta])
