"""NumPy and mpmath restatements of include/catint_drc.h on the helpers of tests/kinetics_ref.py (test infrastructure, no tests of its
own).

control_fp64: the header operation for operation in fp64, one operating point after another, the linear systems by np.linalg.solve,
the refinement step included.
control_mp: the same formulas at 60 decimal digits AT THE SAME STATE (theta is an input of the library: the fp64 coverages are taken as
exact numbers), the linear systems by one LU factorisation per point.
Both return the names of catdrc_outputs.  control_fp64 also returns 'drc_scale': per raw field the sum of the absolute terms of every
entry, what its accuracy is stated relative to -- the part that comes out of the linear solve counted as |J^-1| |J| |dy| (Skeel's
componentwise bound of Gaussian elimination, as 'dflux_scale' of kinetics_ref has it) plus |J^-1| times the terms of the right-hand
side, where rf_r alpha_r and rb_r beta_r count each alone: the difference rf_r - rb_r of a quasi-equilibrated step cancels, and its
rounding is what limits the rate control of that step; for dy_drc that bound itself; for a normalised
field q = dflux / flux the first-order propagation  scale(dflux) / |flux| + |dflux| flux_scale / flux^2  (the header: the number of
digits of a normalised entry is what flux / flux_scale leaves of 16).

Columns: family kf (R), kb (R), drc (R), dG (S), in this order, P = 3 R + S."""
import mpmath as mp
import numpy as np

from tests import kinetics_ref as KR

RAW = ('dflux_dlnkf', 'dflux_dlnkb', 'dflux_drc', 'dflux_dG')
FIELDS = RAW + ('dy_drc', 'drc', 'tdrc', 'flux', 'flux_scale')


def clamp_log(theta):
    g = np.asarray(theta, float)
    with np.errstate(divide='ignore', invalid='ignore'):
        y = np.where(g >= 1.0, 0.0, np.where(g > 0.0, np.log(np.where(g > 0.0, g, 1.0)), KR.MIN_LOG))
    return np.maximum(y, KR.MIN_LOG)


def exponents(t, br):
    """alpha, beta [R][P]: d ln kf_r / dp and d ln kb_r / dp of every column; br [R] the branch of Ga (0: Ea, 1: dG, 2: zero)"""
    R, S = t['R'], t['S']
    P = 3 * R + S
    al, be = np.zeros((R, P)), np.zeros((R, P))
    for r in range(R):
        al[r, r] = 1.0
        be[r, R + r] = 1.0
        al[r, 2 * R + r] = be[r, 2 * R + r] = 1.0
    for s in range(1, S + 1):
        ddG = -t['m'][:, s]
        dEa = t['ofc'][:, s]
        dGa = np.where(br == 0, dEa, np.where(br == 1, ddG, 0.0))
        al[:, 3 * R + s - 1] = -dGa
        be[:, 3 * R + s - 1] = -(dGa - ddG)
    return al, be


def split(x, R):
    """[P][...] -> the four families"""
    return x[:R], x[R:2 * R], x[2 * R:3 * R], x[3 * R:]


def control_point(t, phiM, c, phi0, theta, w=1, CS=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None, residual_tol=1e-8):
    N, T, R, S = t['N'], t['T'], t['R'], t['S']
    off = np.zeros((R, 2)) if off is None else np.asarray(off, float).reshape(R, 2)
    gamma = np.ones(N) if gamma is None else np.asarray(gamma, float)
    c = np.asarray(c, float).reshape(N)
    theta = np.asarray(theta, float).reshape(T)
    V, sg = KR.potential_and_charge(phiM, phi0, w, CS, phi_pzc, sigma)
    shapes = {'dflux_dlnkf': (R, N), 'dflux_dlnkb': (R, N), 'dflux_drc': (R, N), 'dy_drc': (R, T), 'drc': (R, N), 'dflux_dG': (S, N),
              'tdrc': (S, N), 'flux': (N,), 'flux_scale': (N,)}
    fin = np.isfinite([phiM, phi0, sg]).all() and np.isfinite(c).all() and np.isfinite(gamma).all() and np.isfinite(off).all() and np.isfinite(theta).all()
    if not fin:
        out = {k: np.full(s, np.nan) for k, s in shapes.items()}
        out.update(status=2, residual=np.nan, drc_scale={k: np.full(shapes[k], np.nan) for k in RAW + ('dy_drc', 'drc', 'tdrc')})
        return out
    a = gamma * np.maximum(c, 0.0) / t['cref']
    lf, lb, br = KR.rate_constants(t, V, sg, off)
    y = clamp_log(theta)
    rf, rb, _, _ = KR.rates(t, y, a, lf, lb)
    J, F, D = KR.system(t, y, a, lf, lb)          # (sets y of a dead row to MIN_LOG; the rates stay those of the clamped input)
    residual = np.abs(F).max()
    al, be = exponents(t, br)
    dnet = rf[:, None] * al - rb[:, None] * be
    rhs = t['m'].T @ dnet
    rhs[0] = 0.0
    for s in range(1, T):
        rhs[s] = 0.0 if D[s] == 0.0 else -rhs[s] / D[s]
    # the terms of dnet_r are rf_r alpha_r and rb_r beta_r, each alone (rf - rb of a quasi-equilibrated step cancels); those of a
    # right-hand side follow from them, and they reach dy through |J^-1|
    abs_dnet = rf[:, None] * np.abs(al) + rb[:, None] * np.abs(be)
    rhs_terms = np.abs(t['m']).T @ abs_dnet
    rhs_terms[0] = 0.0
    for s in range(1, T):
        rhs_terms[s] = 0.0 if D[s] == 0.0 else rhs_terms[s] / D[s]
    status = 0 if residual <= residual_tol else 1
    Wy = rf[:, None] * t['ofc'] - rb[:, None] * t['obc']
    try:
        with np.errstate(all='ignore'):
            dy = np.linalg.solve(J, rhs)
            # the header's one step of refinement, the residual formed from the rates
            rho = t['m'].T @ (dnet + Wy @ dy)
            rho[0] = -((t['ns'] * np.exp(y)) @ dy)
            for s in range(1, T):
                rho[s] = -dy[s] if D[s] == 0.0 else -rho[s] / D[s]
            dy = dy + np.linalg.solve(J, rho)
            dy_terms = np.abs(np.linalg.inv(J)) @ (np.abs(J) @ np.abs(dy) + rhs_terms)
    except np.linalg.LinAlgError:
        dy = np.full(rhs.shape, np.nan)
        dy_terms = np.full(rhs.shape, np.nan)
        status = 3
    dflux = (t['sd'] * (t['nu'].T @ (dnet + Wy @ dy))).T                              # [P][N]
    scale = (t['sd'] * (np.abs(t['nu']).T @ (abs_dnet + np.abs(Wy) @ dy_terms))).T
    flux = t['sd'] * (t['nu'].T @ (rf - rb))
    flux_scale = t['sd'] * (np.abs(t['nu']).T @ (rf + rb))
    idle = ~(t['nu'] != 0.0).any(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        norm = np.where(idle[None, :], 0.0, dflux / flux[None, :])
        norm_scale = np.where(idle[None, :], 0.0, scale / np.abs(flux)[None, :] + np.abs(dflux) * flux_scale[None, :] / (flux * flux)[None, :])
    kf, kb, ts, dg = split(dflux, R)
    s_kf, s_kb, s_ts, s_dg = split(scale, R)
    return {'dflux_dlnkf': kf, 'dflux_dlnkb': kb, 'dflux_drc': ts, 'dflux_dG': dg, 'dy_drc': dy[:, 2 * R:3 * R].T.copy(), 'drc': split(norm, R)[2],
            'tdrc': split(norm, R)[3], 'flux': flux, 'flux_scale': flux_scale, 'residual': residual, 'status': status,
            'drc_scale': {'dflux_dlnkf': s_kf, 'dflux_dlnkb': s_kb, 'dflux_drc': s_ts, 'dflux_dG': s_dg, 'dy_drc': dy_terms[:, 2 * R:3 * R].T.copy(),
                          'drc': split(norm_scale, R)[2], 'tdrc': split(norm_scale, R)[3]}}


def control_fp64(tab, phiM, csurf, phi_surface, theta, w=1, CS=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None, residual_tol=1e-8):
    """Every operating point of the call; a dict of stacked arrays (the names of catdrc_outputs, and 'drc_scale': a dict of arrays)"""
    t = KR._arrays(tab)
    phiM = np.atleast_1d(np.asarray(phiM, float))
    n = len(phiM)
    csurf = np.asarray(csurf, float).reshape(n, t['N'])
    theta = np.asarray(theta, float).reshape(n, t['T'])
    outs = [control_point(t, phiM[i], csurf[i], np.asarray(phi_surface, float)[i], theta[i], w, CS, phi_pzc, KR._per_point(sigma, i),
                          KR._per_point(off, i), KR._per_point(gamma, i), residual_tol) for i in range(n)]
    res = {k: np.array([o[k] for o in outs]) for k in outs[0] if k != 'drc_scale'}
    res['status'] = res['status'].astype(np.int32)
    res['drc_scale'] = {k: np.array([o['drc_scale'][k] for o in outs]) for k in outs[0]['drc_scale']}
    return res


def control_mp(tab, phiM, csurf, phi_surface, theta, w=1, CS=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None):
    """The formulas of the header at 60 digits at the given (fp64) theta: nested lists of mpmath numbers under the names of FIELDS and
    'residual' [n]"""
    t = KR._arrays(tab)
    N, T, R, S = t['N'], t['T'], t['R'], t['S']
    P = 3 * R + S
    phiM = np.atleast_1d(np.asarray(phiM, float))
    n = len(phiM)
    csurf = np.asarray(csurf, float).reshape(n, N)
    theta = np.asarray(theta, float).reshape(n, T)
    res = {k: [] for k in FIELDS + ('residual',)}
    with mp.workdps(KR.DPS):
        f = mp.mpf
        for i in range(n):
            o = np.zeros((R, 2)) if off is None else np.asarray(off, float)[i].reshape(R, 2)
            g = np.ones(N) if gamma is None else np.asarray(gamma, float)[i]
            sgm = None if sigma is None else float(np.asarray(sigma)[i])
            a, lf, lb = KR._mp_state(t, phiM[i], csurf[i], phi_surface[i], w, CS, phi_pzc, sgm, o, g, True)
            # the branch of Ga, as _mp_state takes it
            V = f(phiM[i]) - (f(phi_surface[i]) if w else 0)
            sg = f(CS) * ((f(phiM[i]) - f(phi_pzc)) - f(phi_surface[i])) if sgm is None else f(sgm)
            br = []
            for r in range(R):
                dG = f(t['dG'][r, 0]) + f(t['dG'][r, 1]) * V + f(t['dG'][r, 2]) * sg + f(t['dG'][r, 3]) * sg * sg
                Ea = None if np.isneginf(t['Ea'][r, 0]) else f(t['Ea'][r, 0]) + f(t['Ea'][r, 1]) * V + f(t['Ea'][r, 2]) * sg + f(t['Ea'][r, 3]) * sg * sg
                br.append(0 if (Ea is not None and Ea >= dG and Ea >= 0) else (1 if dG >= 0 else 2))
            y = []
            for k in range(T):
                th = theta[i, k]
                y.append(f(0) if th >= 1.0 else (max(mp.log(f(th)), f(KR.MIN_LOG)) if th > 0.0 else f(KR.MIN_LOG)))
            rf, rb = KR._mp_rates(t, y, a, lf, lb)
            m = [[int(t['m'][r, s]) for s in range(T)] for r in range(R)]
            D = [sum(abs(m[r][s]) * (rf[r] + rb[r]) for r in range(R)) for s in range(T)]
            dead = {s for s in range(1, T) if D[s] == 0}
            for s in dead:
                y[s] = f(KR.MIN_LOG)
            J = mp.zeros(T, T)
            F = [f(0)] * T
            for k in range(T):
                J[0, k] = f(t['ns'][k]) * mp.exp(y[k])
            F[0] = sum(J[0, k] for k in range(T)) - 1
            W = [[rf[r] * int(t['ofc'][r, k]) - rb[r] * int(t['obc'][r, k]) for k in range(T)] for r in range(R)]
            for s in range(1, T):
                if s in dead:
                    J[s, s] = 1
                    continue
                for k in range(T):
                    J[s, k] = sum(m[r][s] * W[r][k] for r in range(R)) / D[s]
                F[s] = sum(m[r][s] * (rf[r] - rb[r]) for r in range(R)) / D[s]
            al, be = exponents(t, np.array(br))
            LU, piv = mp.mp.LU_decomp(J)
            sd = f(t['sd'])
            nu = [[f(t['nu'][r, k]) for k in range(N)] for r in range(R)]
            flux = [sd * sum(nu[r][k] * (rf[r] - rb[r]) for r in range(R)) for k in range(N)]
            idle = [all(t['nu'][r, k] == 0.0 for r in range(R)) for k in range(N)]
            cols, dys = [], []
            for p in range(P):
                dnet = [rf[r] * int(al[r, p]) - rb[r] * int(be[r, p]) for r in range(R)]
                rhs = mp.zeros(T, 1)
                for s in range(1, T):
                    if s not in dead:
                        rhs[s] = -sum(m[r][s] * dnet[r] for r in range(R)) / D[s]
                dy = mp.mp.U_solve(LU, mp.mp.L_solve(LU, rhs, piv))
                dys.append([dy[k] for k in range(T)])
                cols.append([sd * sum(nu[r][k] * (dnet[r] + sum(W[r][q] * dy[q] for q in range(T))) for r in range(R)) for k in range(N)])
            norm = [[f(0) if idle[k] else (col[k] / flux[k] if flux[k] != 0 else mp.nan) for k in range(N)] for col in cols]
            kf, kb, ts, dg = split(cols, R)
            res['dflux_dlnkf'].append(kf); res['dflux_dlnkb'].append(kb); res['dflux_drc'].append(ts); res['dflux_dG'].append(dg)
            res['dy_drc'].append(dys[2 * R:3 * R])
            res['drc'].append(norm[2 * R:3 * R]); res['tdrc'].append(norm[3 * R:])
            res['flux'].append(flux)
            res['flux_scale'].append([sd * sum(abs(nu[r][k]) * (rf[r] + rb[r]) for r in range(R)) for k in range(N)])
            res['residual'].append(max(abs(v) for v in F))
    return res


def errors(res, ref, fp):
    """Per field of `res` (device or fp64 result): the worst error against the 60-digit `ref` per point, in units of fp's 'drc_scale'
    (flux in units of flux_scale).  An entry whose scale is 0 must be exact."""
    out = {}
    for k in FIELDS:
        if k in res and k != 'flux_scale':
            out[k] = KR.mp_err(ref[k], res[k], fp['flux_scale'] if k == 'flux' else fp['drc_scale'][k])
    return out


def apparent(raw, Kc, Kphi, Tc, Tphi, rf=1.0):
    """numpy.linalg.solve form of the apparent derivative of one point: M^-1 (rf raw^T), M = I - rf (K_c T_c + K_phi (x) T_phi)"""
    M = np.eye(len(Kphi)) - rf * (Kc @ Tc + np.outer(Kphi, Tphi))
    return np.linalg.solve(M, rf * np.asarray(raw).T).T
