"""NumPy and mpmath restatements of include/catint_eis.h (test infrastructure, no tests of its own), composed from the references the
project already has:

  kinetic      K(omega) of one operating point from tests/kinetics_ref.py (rate_constants, rates, system, slopes): the scaled rows of the
               steady state with -i omega theta_s / D_s on the diagonal, one complex solve for the N + 2 parameters
  kinetic_mp   the same formulas at 60 digits (the rates by kinetics_ref._mp_state / _mp_rates)
  transfer     T_c, T_phi, t_c, t_phi of one (state, omega) from tests/response_ref.py: `operator` and its two solvers (LAPACK's banded LU
               and the block elimination), one right-hand side per wall flux and one for phi_M
  electrode    the closure with a complex restatement of tests/couple_ref.py: solve_pivoted (the same pivot rule and singularity scale)

The disagreement of the two transport solvers measures what rounding does to a case; tests/test_gpu_eis.py derives its tolerance from
it."""
import mpmath as mp
import numpy as np

from tests import couple_ref as CR
from tests import kinetics_ref as KR
from tests import response_ref as RR

ELECTRODE = ('admittance', 'faradaic', 'double_layer', 'dflux', 'dc_surface', 'dphi_surface', 'dsigma', 'Tc', 'Tphi', 'tc', 'tphi')


def _point(t, phiM, c, phi0, theta, w, CS, phi_pzc, sigma, off, gamma):
    N, R = t['N'], t['R']
    off = np.zeros((R, 2)) if off is None else np.asarray(off, float).reshape(R, 2)
    gamma = np.ones(N) if gamma is None else np.asarray(gamma, float)
    c = np.asarray(c, float).reshape(N)
    V, sg = KR.potential_and_charge(phiM, phi0, w, CS, phi_pzc, sigma)
    a = gamma * np.maximum(c, 0.0) / t['cref']
    lf, lb, br = KR.rate_constants(t, V, sg, off)
    y = np.array(KR.start(t, theta), float)
    return off, gamma, c, sg, a, lf, lb, br, y


def _dnet(t, c, gamma, a, sg, br, rf, rb, ef, eb, w, CS, sigma):
    """d rate_r / dp at fixed y, p = c_0 .. c_{N-1}, phi_M, phi_0: the text of kinetics_ref.solve_point"""
    N, R = t['N'], t['R']
    dnet = np.zeros((R, N + 2))
    for j in range(N):
        dadc = gamma[j] / t['cref'][j] if c[j] >= 0.0 else 0.0
        left_f = np.prod(np.power(a[None, :], np.maximum(t['ofs'] - (np.arange(N) == j), 0)), axis=1)
        left_b = np.prod(np.power(a[None, :], np.maximum(t['obs'] - (np.arange(N) == j), 0)), axis=1)
        dnet[:, j] = ef * (t['ofs'][:, j] * left_f * dadc) - eb * (t['obs'][:, j] * left_b * dadc)
    for q, (dV, ds) in enumerate(((1.0, CS if sigma is None else 0.0), (-1.0 if w else 0.0, -CS if sigma is None else 0.0))):
        dlf, dlb = KR.slopes(t, sg, br, dV, ds)
        dnet[:, N + q] = rf * dlf - rb * dlb
    return dnet


def kinetic(tab, phiM, c, phi0, theta, omega, w=1, CS=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None):
    """One (operating point, omega): {'Kc' [N][N], 'Kphi' [N][2], 'dy' [T][N+2] complex, 'residual', 'scale' [N][N+2]: the sum of the
    absolute terms of each entry of K (the dflux_scale convention of kinetics_ref), 'lam': max_s D_s / theta_s}"""
    t = KR._arrays(tab)
    N, T = t['N'], t['T']
    off, gamma, c, sg, a, lf, lb, br, y = _point(t, phiM, c, phi0, theta, w, CS, phi_pzc, sigma, off, gamma)
    rf, rb, ef, eb = KR.rates(t, y, a, lf, lb)
    J, F, D = KR.system(t, y, a, lf, lb)
    A = J.astype(complex)
    th = np.exp(y)
    for s in range(1, T):
        if D[s] != 0.0:
            A[s, s] -= 1j * omega * th[s] / D[s]
    Wy = rf[:, None] * t['ofc'] - rb[:, None] * t['obc']
    dnet = _dnet(t, c, gamma, a, sg, br, rf, rb, ef, eb, w, CS, sigma)
    rhs = t['m'].T @ dnet
    rhs[0] = 0.0
    for s in range(1, T):
        rhs[s] = 0.0 if D[s] == 0.0 else -rhs[s] / D[s]
    with np.errstate(all='ignore'):
        dy = np.linalg.solve(A, rhs.astype(complex))
        K = t['sd'] * (t['nu'].T @ (dnet + Wy @ dy))
        dy_terms = np.abs(np.linalg.inv(A)) @ (np.abs(A) @ np.abs(dy))
        scale = t['sd'] * (np.abs(t['nu']).T @ (np.abs(dnet) + np.abs(Wy) @ dy_terms))
        lam = max((D[s] / th[s] for s in range(1, T) if D[s] != 0.0 and th[s] > 0.0), default=0.0)
    return {'Kc': K[:, :N].copy(), 'Kphi': K[:, N:].copy(), 'dy': dy, 'residual': float(np.abs(F[1:]).max()), 'scale': scale, 'lam': lam}


def kinetic_batch(tab, phiM, csurf, phi_surface, theta, omegas, **kw):
    """Every point and frequency: stacked 'Kc' [n][F][N][N], 'Kphi' [n][F][N][2], 'dy' [n][F][T][N+2], 'scale' [n][F][N][N+2],
    'residual' [n]"""
    n = len(phiM)
    rows = [[kinetic(tab, phiM[i], csurf[i], phi_surface[i], theta[i], om, **kw) for om in omegas] for i in range(n)]
    out = {k: np.array([[r[k] for r in row] for row in rows]) for k in ('Kc', 'Kphi', 'dy', 'scale')}
    out['residual'] = np.array([row[0]['residual'] for row in rows])
    return out


def kinetic_mp(tab, phiM, c, phi0, theta, omega, w=1, CS=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None):
    """The formulas of `kinetic` at 60 digits from the same fp64 inputs: K [N][N+2] as nested lists of mpmath complex numbers.  The
    branch of Ga, the clamp of a negative concentration and the dead rows are taken as the fp64 evaluation takes them."""
    t = KR._arrays(tab)
    N, T, R = t['N'], t['T'], t['R']
    off, gamma, c, sg64, a64, lf64, lb64, br, y64 = _point(t, phiM, c, phi0, theta, w, CS, phi_pzc, sigma, off, gamma)
    _, _, D64 = KR.system(t, y64.copy(), a64, lf64, lb64)
    with mp.workdps(KR.DPS):
        f = mp.mpf
        a, lf, lb = KR._mp_state(t, phiM, c, phi0, w, CS, phi_pzc, sigma, off, gamma, True)
        y = [f(v) for v in y64]
        rf, rb = KR._mp_rates(t, y, a, lf, lb)
        sg = f(CS) * ((f(phiM) - f(phi_pzc)) - f(phi0)) if sigma is None else f(sigma)
        # the rows
        A = mp.zeros(T, T)
        D = [f(0)] * T
        for r in range(R):
            for s in range(1, T):
                m = int(t['m'][r, s])
                if not m:
                    continue
                D[s] += abs(m) * (rf[r] + rb[r])
                for k in range(T):
                    A[s, k] += m * (rf[r] * int(t['ofc'][r, k]) - rb[r] * int(t['obc'][r, k]))
        for s in range(1, T):
            if D64[s] == 0.0:
                for k in range(T):
                    A[s, k] = 1 if k == s else 0
            else:
                for k in range(T):
                    A[s, k] /= D[s]
                A[s, s] -= mp.mpc(0, 1) * f(omega) * mp.exp(y[s]) / D[s]
        for k in range(T):
            A[0, k] = f(t['ns'][k]) * mp.exp(y[k])
        # d rate / dp at fixed y
        dnet = [[f(0)] * (N + 2) for _ in range(R)]
        for r in range(R):
            ef, eb = rf[r], rb[r]
            for j in range(N):
                of, ob = int(t['ofs'][r, j]), int(t['obs'][r, j])
                dadc = f(gamma[j]) / f(t['cref'][j]) if c[j] >= 0.0 else f(0)
                # the product with one factor left out
                df = of * rf[r] / a[j] * dadc if (of and a[j] != 0) else f(0)
                db = ob * rb[r] / a[j] * dadc if (ob and a[j] != 0) else f(0)
                if a[j] == 0:
                    if of == 1:
                        rest = mp.exp(lf[r] + sum(int(t['ofc'][r, k]) * y[k] for k in range(T)))
                        for i in range(N):
                            if i != j:
                                rest *= a[i] ** int(t['ofs'][r, i])
                        df = rest * dadc
                    if ob == 1:
                        rest = mp.exp(lb[r] + sum(int(t['obc'][r, k]) * y[k] for k in range(T)))
                        for i in range(N):
                            if i != j:
                                rest *= a[i] ** int(t['obs'][r, i])
                        db = rest * dadc
                dnet[r][j] = df - db
            for q, (dV, ds) in enumerate(((1, CS if sigma is None else 0.0), (-1 if w else 0, -CS if sigma is None else 0.0))):
                ddG = f(t['dG'][r, 1]) * dV + (f(t['dG'][r, 2]) + 2 * f(t['dG'][r, 3]) * sg) * f(ds)
                if np.isneginf(t['Ea'][r, 0]):
                    dEa = f(0)
                else:
                    dEa = f(t['Ea'][r, 1]) * dV + (f(t['Ea'][r, 2]) + 2 * f(t['Ea'][r, 3]) * sg) * f(ds)
                dGa = dEa if br[r] == 0 else (ddG if br[r] == 1 else f(0))
                dnet[r][N + q] = ef * (-dGa) - eb * (-(dGa - ddG))
        K = [[None] * (N + 2) for _ in range(N)]
        Ainv = A ** -1
        for p in range(N + 2):
            rhs = mp.zeros(T, 1)
            for s in range(1, T):
                if D64[s] != 0.0:
                    rhs[s] = -sum(int(t['m'][r, s]) * dnet[r][p] for r in range(R)) / D[s]
            dy = Ainv * rhs
            for k in range(N):
                tot = mp.mpc(0)
                for r in range(R):
                    nu = f(t['nu'][r, k])
                    if nu == 0:
                        continue
                    ws = sum((rf[r] * int(t['ofc'][r, j]) - rb[r] * int(t['obc'][r, j])) * dy[j] for j in range(T))
                    tot += nu * (dnet[r][p] + ws)
                K[k][p] = f(t['sd']) * tot
    return K


def mp_err(K_mp, K, scale):
    """max |K - K_mp| / scale over the entries, the difference formed at 60 digits; an entry whose scale is 0 must be exact"""
    worst = 0.0
    with mp.workdps(KR.DPS):
        for k in range(len(K_mp)):
            for p in range(len(K_mp[k])):
                d = abs(mp.mpc(complex(K[k][p])) - K_mp[k][p])
                if scale[k][p] == 0.0:
                    worst = max(worst, 0.0 if d == 0 else np.inf)
                else:
                    worst = max(worst, float(d / mp.mpf(float(scale[k][p]))))
    return worst


# ---- transport and closure ---------------------------------------------------------------------------------------------------------
def transfer(p, c, phi, omega, method='banded'):
    """[(N+1), (N+1)] complex: column j < N the answer of the surface state (c_0 .. c_{N-1}, phi_0) to the wall flux of species j,
    column N its answer to phi_M at fixed fluxes.  p carries no wall table"""
    assert not p.wall_kinetics, 'the transfer functions are defined without a wall table'
    L, M, U = RR.operator(p, c, phi, omega)
    cols = []
    for pert in [('flux', j) for j in range(p.N)] + [RR.PHIM]:
        du = np.asarray(RR.METHODS[method](L, M, U, RR.rhs(p, c, phi, pert)), dtype=complex)
        cols.append(du[:, 0])
    return np.stack(cols, axis=1)


def solve_pivoted(A, b, scale):
    """couple_ref.solve_pivoted for complex numbers: the pivot by magnitude, (x, singular) by the same rule"""
    A, b = np.array(A, complex), np.array(b, complex)
    n = len(b)
    singular = False
    with np.errstate(all='ignore'):
        for p in range(n):
            col = np.where(np.isfinite(A[p:, p]), np.abs(A[p:, p]), np.inf)
            q = p + int(np.argmax(col))
            A[[p, q]], b[[p, q]] = A[[q, p]], b[[q, p]]
            piv = A[p, p]
            if piv == 0.0 or not np.isfinite(piv) or abs(piv) < CR.SINGULAR * scale:
                singular = True
            for r in range(p + 1, n):
                f = A[r, p] / piv
                A[r, p:] -= f * A[p, p:]
                b[r] -= f * b[p]
        x = np.zeros(n, complex)
        for p in range(n - 1, -1, -1):
            x[p] = (b[p] - A[p, p + 1:] @ x[p + 1:]) / A[p, p]
    return x, singular or not np.isfinite(x).all()


def closure(p, Tf, Kc, Kphi, omega, rf):
    """The header's outputs from the transfer functions Tf [(N+1), (N+1)] and the kinetic admittance"""
    N = p.N
    Tc, Tphi, tc, tphi = Tf[:N, :N], Tf[N, :N], Tf[:N, N], Tf[N, N]
    Kc, Kphi = np.asarray(Kc, complex), np.asarray(Kphi, complex)
    X = rf * (Kc @ Tc + np.outer(Kphi[:, 1], Tphi))
    A = np.eye(N) - X
    scale = max(np.abs(A).max(), 1.0, np.abs(X).max())
    b = rf * (Kphi[:, 0] + Kc @ tc + Kphi[:, 1] * tphi)
    df, singular = solve_pivoted(A, b, scale)
    with np.errstate(all='ignore'):
        dcs = Tc @ df + tc
        dphi = Tphi @ df + tphi
        dsig = p.CS * (1.0 - dphi)
        yf = (p.q * df).sum()
        ydl = 1j * omega * dsig
    return {'admittance': ydl + yf, 'faradaic': yf, 'double_layer': ydl, 'dflux': df, 'dc_surface': dcs, 'dphi_surface': dphi, 'dsigma': dsig,
            'Tc': Tc.copy(), 'Tphi': Tphi.copy(), 'tc': tc.copy(), 'tphi': tphi, 'status': 3 if singular else 0, 'A': A,
            'cond': np.linalg.cond(A) if np.isfinite(A).all() else np.inf}


def electrode(p, c, phi, omega, Kc, Kphi, rf=1.0, method='banded'):
    return closure(p, transfer(p, c, phi, omega, method), Kc, Kphi, omega, rf)


def disagreement(ra, rb):
    """per output: the relative difference of two results; matrices row by row (response_ref.rel_rows), scalars by themselves"""
    out = {}
    for k in ELECTRODE:
        a, b = np.atleast_1d(ra[k]), np.atleast_1d(rb[k])
        out[k] = RR.rel_rows(a, b) if a.ndim == 2 else RR.rel_rows(a.reshape(1, -1), b.reshape(1, -1))
    return out
