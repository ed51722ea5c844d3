"""NumPy and mpmath restatements of include/catint_iacontrol.h on the helpers of tests/interact_ref.py (test infrastructure, no tests of
its own), in the manner of tests/drc_ref.py, whose bookkeeping of 'drc_scale' it keeps.

control_fp64: the header operation for operation in fp64, one operating point after another, the linear systems by np.linalg.solve, the
refinement step included.  The four families of catint_drc.h are formed in one block of 3 R + S columns with the calls and shapes of
drc_ref.control_point, the strength column in a block of its own, so that with one site type and strength 0 the first block has the
bits of drc_ref.control_fp64.
control_mp: the same formulas at 60 decimal digits AT THE SAME STATE (theta is an input of the library: the fp64 coverages are taken as
exact numbers; y_mp: 60-digit log-coverages in their place), the contractions EG and EA formed exactly, one LU factorisation per point.

Columns: family kf (R), kb (R), drc (R), dG (S), strength (1), in this order."""
import mpmath as mp
import numpy as np

from tests import drc_ref as DR
from tests import interact_ref as IR
from tests import kinetics_ref as KR

RAW = DR.RAW + ('dflux_dstrength',)
DY = ('dy_drc', 'dy_dstrength')
NORM = ('drc', 'tdrc', 'strength_control')
FIELDS = RAW + DY + NORM + ('flux', 'flux_scale')
OLD = DR.FIELDS          # the fields catint_drc.h has as well


def shapes(t):
    N, T, R, S = t['N'], t['T'], t['R'], t['S']
    return {'dflux_dlnkf': (R, N), 'dflux_dlnkb': (R, N), 'dflux_drc': (R, N), 'dy_drc': (R, T), 'drc': (R, N), 'dflux_dG': (S, N), 'tdrc': (S, N),
            'dflux_dstrength': (N,), 'dy_dstrength': (T,), 'strength_control': (N,), 'flux': (N,), 'flux_scale': (N,)}


def exponents(t, br):
    """alpha, beta [R][3 R + S] of the four families of catint_drc.h, adsorbate a in column G + a"""
    R, S, G = t['R'], t['S'], t['G']
    P = 3 * R + S
    al, be = np.zeros((R, P)), np.zeros((R, P))
    for r in range(R):
        al[r, r] = 1.0
        be[r, R + r] = 1.0
        al[r, 2 * R + r] = be[r, 2 * R + r] = 1.0
    for a in range(S):
        ddG = -t['m'][:, G + a]
        dEa = t['ofc'][:, G + a]
        dGa = np.where(br == 0, dEa, np.where(br == 1, ddG, 0.0))
        al[:, 3 * R + a] = -dGa
        be[:, 3 * R + a] = -(dGa - ddG)
    return al, be


def strength_exponents(t, br, w):
    """alpha, beta [R][1] of the strength column at the surface state w [S] = f theta"""
    R, S = t['R'], t['S']
    sG, sA = np.zeros(R), np.zeros(R)
    for a in range(S):
        sG = sG + t['eg'][:, a] * w[a]
        sA = sA + t['ea'][:, a] * w[a]
    sA = np.where(t['ts'], sA, 0.0)
    dGa = np.where(br == 0, sA, np.where(br == 1, sG, 0.0))
    return (-dGa)[:, None], (-(dGa - sG))[:, None]


def _block(t, J, D, Wy, rf, rb, nth, al, be):
    """dy [T][P], its terms, dflux [P][N], its scale for the columns al, be [R][P]; None for dy where J is singular"""
    T, G = t['T'], t['G']
    dnet = rf[:, None] * al - rb[:, None] * be
    rhs = t['m'].T @ dnet
    rhs[:G] = 0.0
    for s in range(G, T):
        rhs[s] = 0.0 if D[s] == 0.0 else -rhs[s] / D[s]
    abs_dnet = rf[:, None] * np.abs(al) + rb[:, None] * np.abs(be)
    rhs_terms = np.abs(t['m']).T @ abs_dnet
    rhs_terms[:G] = 0.0
    for s in range(G, T):
        rhs_terms[s] = 0.0 if D[s] == 0.0 else rhs_terms[s] / D[s]
    ok = True
    try:
        with np.errstate(all='ignore'):
            dy = np.linalg.solve(J, rhs)
            rho = t['m'].T @ (dnet + Wy @ dy)
            for g in range(G):
                rho[g] = -(np.where(t['site_of'] == g, nth, 0.0) @ dy) / t['x'][g]
            for s in range(G, T):
                rho[s] = -dy[s] if D[s] == 0.0 else -rho[s] / D[s]
            dy = dy + np.linalg.solve(J, rho)
            dy_terms = np.abs(np.linalg.inv(J)) @ (np.abs(J) @ np.abs(dy) + rhs_terms)
    except np.linalg.LinAlgError:
        dy = np.full(rhs.shape, np.nan)
        dy_terms = np.full(rhs.shape, np.nan)
        ok = False
    with np.errstate(all='ignore'):
        dflux = (t['sd'] * (t['nu'].T @ (dnet + Wy @ dy))).T
        scale = (t['sd'] * (np.abs(t['nu']).T @ (abs_dnet + np.abs(Wy) @ dy_terms))).T
    return dy, dy_terms, dflux, scale, ok


def system(t, y, a, V, sg, off, lam):
    """interact_ref.system from the same helpers, the sums over the steps formed as kinetics_ref.system forms them (matrix products):
    with one site type and strength 0 every entry has the bits of that function.  Returns J, F, D, Wy, rf, rb, the branch, w [S]; a dead
    row sets its y to MIN_LOG (in place)"""
    G, T = t['G'], t['T']
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        th, wv, f, fp = IR.surface_state(t, y)
        lf, lb, br, es, qg, qs = IR.step_constants(t, V, sg, off, lam, th, wv)
        rf, rb, _, _ = IR.rates(t, y, a, lf, lb)
        ofe, obe = IR.effective_orders(t, lam, th, f, fp, es, qg, qs)
        Wy = rf[:, None] * ofe - rb[:, None] * obe
        m = t['m']
        B = m.T @ (rf - rb)
        D = np.abs(m).T @ (rf + rb)
        J = m.T @ Wy
        F = np.zeros(T)
        for s in range(G, T):
            if D[s] == 0.0:
                J[s] = 0.0
                J[s, s] = 1.0
                y[s] = IR.MIN_LOG
            else:
                J[s] /= D[s]
                F[s] = B[s] / D[s]
        nth = t['ns'] * np.exp(y)
        for g in range(G):
            on = t['site_of'] == g
            J[g] = np.where(on, nth / t['x'][g], 0.0)
            F[g] = np.where(on, nth, 0.0).sum() / t['x'][g] - 1.0
    return J, F, D, Wy, rf, rb, br, wv, nth


def control_point(t, phiM, c, phi0, theta, w=1, CS=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None, residual_tol=1e-8, strength=None):
    N, T, R = t['N'], t['T'], t['R']
    lam = t['strength'] if strength is None else float(strength)
    off = np.zeros((R, 2)) if off is None else np.asarray(off, float).reshape(R, 2)
    gamma = np.ones(N) if gamma is None else np.asarray(gamma, float)
    c = np.asarray(c, float).reshape(N)
    theta = np.asarray(theta, float).reshape(T)
    V, sg = KR.potential_and_charge(phiM, phi0, w, CS, phi_pzc, sigma)
    shp = shapes(t)
    fin = np.isfinite([phiM, phi0, sg]).all() and np.isfinite(c).all() and np.isfinite(gamma).all() and np.isfinite(off).all() and np.isfinite(theta).all()
    if not fin:
        out = {k: np.full(s, np.nan) for k, s in shp.items()}
        out.update(status=2, residual=np.nan, drc_scale={k: np.full(shp[k], np.nan) for k in RAW + DY + NORM})
        return out
    a = gamma * np.maximum(c, 0.0) / t['cref']
    y = DR.clamp_log(theta)
    J, F, D, Wy, rf, rb, br, wv, nth = system(t, y, a, V, sg, off, lam)   # (w at the clamped input, before a dead row moves its y)
    residual = np.abs(F).max()
    status = 0 if residual <= residual_tol else 1
    al, be = exponents(t, br)
    dy, dy_terms, dflux, scale, ok = _block(t, J, D, Wy, rf, rb, nth, al, be)
    al1, be1 = strength_exponents(t, br, wv)
    dy1, dy1_terms, dflux1, scale1, ok1 = _block(t, J, D, Wy, rf, rb, nth, al1, be1)
    if not (ok and ok1):
        status = 3
    flux = t['sd'] * (t['nu'].T @ (rf - rb))
    flux_scale = t['sd'] * (np.abs(t['nu']).T @ (rf + rb))
    idle = ~(t['nu'] != 0.0).any(axis=0)

    def normalise(d, s):
        with np.errstate(divide='ignore', invalid='ignore'):
            return (np.where(idle[None, :], 0.0, d / flux[None, :]),
                    np.where(idle[None, :], 0.0, s / np.abs(flux)[None, :] + np.abs(d) * flux_scale[None, :] / (flux * flux)[None, :]))
    norm, norm_scale = normalise(dflux, scale)
    norm1, norm1_scale = normalise(dflux1, scale1)
    with np.errstate(invalid='ignore'):
        norm1, norm1_scale = np.where(idle[None, :], 0.0, lam * norm1), abs(lam) * norm1_scale
    kf, kb, ts, dg = DR.split(dflux, R)
    s_kf, s_kb, s_ts, s_dg = DR.split(scale, R)
    return {'dflux_dlnkf': kf, 'dflux_dlnkb': kb, 'dflux_drc': ts, 'dflux_dG': dg, 'dy_drc': dy[:, 2 * R:3 * R].T.copy(), 'drc': DR.split(norm, R)[2],
            'tdrc': DR.split(norm, R)[3], 'dflux_dstrength': dflux1[0], 'dy_dstrength': dy1[:, 0].copy(), 'strength_control': norm1[0],
            'flux': flux, 'flux_scale': flux_scale, 'residual': residual, 'status': status,
            'drc_scale': {'dflux_dlnkf': s_kf, 'dflux_dlnkb': s_kb, 'dflux_drc': s_ts, 'dflux_dG': s_dg, 'dy_drc': dy_terms[:, 2 * R:3 * R].T.copy(),
                          'drc': DR.split(norm_scale, R)[2], 'tdrc': DR.split(norm_scale, R)[3], 'dflux_dstrength': scale1[0],
                          'dy_dstrength': dy1_terms[:, 0].copy(), 'strength_control': norm1_scale[0]}}


def control_fp64(tab, phiM, csurf, phi_surface, theta, w=1, CS=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None, residual_tol=1e-8,
                 strength=None):
    """Every operating point of the call; a dict of stacked arrays (the names of catic_outputs, and 'drc_scale': a dict of arrays)"""
    t = IR._arrays(tab)
    phiM = np.atleast_1d(np.asarray(phiM, float))
    n = len(phiM)
    csurf = np.asarray(csurf, float).reshape(n, t['N'])
    theta = np.asarray(theta, float).reshape(n, t['T'])
    pp = KR._per_point
    outs = [control_point(t, phiM[i], csurf[i], np.asarray(phi_surface, float)[i], theta[i], w, CS, phi_pzc, pp(sigma, i), pp(off, i), pp(gamma, i),
                          residual_tol, strength) for i in range(n)]
    res = {k: np.array([o[k] for o in outs]) for k in outs[0] if k != 'drc_scale'}
    res['status'] = res['status'].astype(np.int32)
    res['drc_scale'] = {k: np.array([o['drc_scale'][k] for o in outs]) for k in outs[0]['drc_scale']}
    return res


def _mp_point(t, V, sg, a, off, lam, y):
    """One point at 60 digits: y [T] mpmath log-coverages.  Returns the dict of one point's fields, 'dy' [P][T] of every column and
    'residual'."""
    f = mp.mpf
    N, G, S, R, T = t['N'], t['G'], t['S'], t['R'], t['T']
    site_of = [int(v) for v in t['site_of']]
    th = [mp.exp(v) for v in y]
    crowd = [f(0)] * G
    for k in range(G, T):
        crowd[site_of[k]] += f(t['ns'][k]) * th[k]
    fg, fpg = [], []
    for g in range(G):
        if not t['piecewise']:
            fg.append(f(1)); fpg.append(f(0))
            continue
        C, c, s = crowd[g] / f(t['x'][g]), f(t['cutoff'][g]), f(t['smooth'][g])
        below, inside = C <= c - s, C < c + s
        fg.append(f(0) if below else ((C - c + s) ** 2 / (4 * s) if inside else C - c))
        fpg.append(f(0) if below else ((C - c + s) / (2 * s) if inside else f(1)))
    gu = [site_of[G + u] for u in range(S)]
    wv = [fg[gu[u]] * th[G + u] for u in range(S)]
    m = [[int(t['m'][r, k]) for k in range(T)] for r in range(R)]
    ofc = [[int(t['ofc'][r, k]) for k in range(T)] for r in range(R)]
    obc = [[int(t['obc'][r, k]) for k in range(T)] for r in range(R)]
    eps = [[f(t['eps'][k, u]) for u in range(S)] for k in range(S)]
    EG = [[sum(m[r][G + k] * eps[k][u] for k in range(S)) for u in range(S)] for r in range(R)]
    EA = [[f(t['ets'][r, u]) - sum(ofc[r][G + k] * eps[k][u] for k in range(S)) for u in range(S)] for r in range(R)]
    rf, rb, br, sGs, sAs = [], [], [], [], []
    for r in range(R):
        sG = sum(EG[r][u] * wv[u] for u in range(S))
        sA = sum(EA[r][u] * wv[u] for u in range(S)) if t['ts'][r] else f(0)
        dG = f(t['dG'][r, 0]) + f(t['dG'][r, 1]) * V + f(t['dG'][r, 2]) * sg + f(t['dG'][r, 3]) * sg * sg + lam * sG
        Ea = None
        if t['ts'][r]:
            Ea = f(t['Ea'][r, 0]) + f(t['Ea'][r, 1]) * V + f(t['Ea'][r, 2]) * sg + f(t['Ea'][r, 3]) * sg * sg + lam * sA
        b = 0 if (Ea is not None and Ea >= dG and Ea >= 0) else (1 if dG >= 0 else 2)
        Ga = Ea if b == 0 else (dG if b == 1 else f(0))
        sf = f(t['lnA'][r]) - Ga + f(off[r, 0])
        sb = f(t['lnA'][r]) - (Ga - dG) + f(off[r, 1])
        pf = pb = f(1)
        for k in range(T):
            sf += ofc[r][k] * y[k]
            sb += obc[r][k] * y[k]
        for j in range(N):
            pf *= a[j] ** int(t['ofs'][r, j])
            pb *= a[j] ** int(t['obs'][r, j])
        rf.append(mp.exp(sf) * pf); rb.append(mp.exp(sb) * pb); br.append(b); sGs.append(sG); sAs.append(sA)
    # the effective orders
    W = [[None] * T for _ in range(R)]
    for r in range(R):
        ES = [EA[r][u] if br[r] == 0 else (EG[r][u] if br[r] == 1 else f(0)) for u in range(S)]
        qg, qs = [f(0)] * G, [f(0)] * G
        for u in range(S):
            qg[gu[u]] += EG[r][u] * th[G + u]
            qs[gu[u]] += ES[u] * th[G + u]
        for k in range(T):
            ofe, obe = f(ofc[r][k]), f(obc[r][k])
            if k >= G:
                u, g = k - G, gu[k - G]
                nx = f(t['ns'][k]) / f(t['x'][g])
                gG = lam * (EG[r][u] * fg[g] + nx * fpg[g] * qg[g])
                gS = lam * (ES[u] * fg[g] + nx * fpg[g] * qs[g])
                ofe -= th[k] * gS
                obe -= th[k] * (gS - gG)
            W[r][k] = rf[r] * ofe - rb[r] * obe
    D = [sum(abs(m[r][s]) * (rf[r] + rb[r]) for r in range(R)) for s in range(T)]
    dead = {s for s in range(G, T) if D[s] == 0}
    ys = list(y)
    for s in dead:
        ys[s] = f(KR.MIN_LOG)
    J = mp.zeros(T, T)
    F = [f(0)] * T
    for g in range(G):
        for k in range(T):
            if site_of[k] == g:
                J[g, k] = f(t['ns'][k]) * mp.exp(ys[k]) / f(t['x'][g])
        F[g] = sum(J[g, k] for k in range(T)) - 1
    for s in range(G, T):
        if s in dead:
            J[s, s] = 1
            continue
        for k in range(T):
            J[s, k] = sum(m[r][s] * W[r][k] for r in range(R)) / D[s]
        F[s] = sum(m[r][s] * (rf[r] - rb[r]) for r in range(R)) / D[s]
    al0, be0 = exponents(t, np.array(br))
    al = [[f(int(al0[r, p])) for p in range(al0.shape[1])] for r in range(R)]
    be = [[f(int(be0[r, p])) for p in range(be0.shape[1])] for r in range(R)]
    for r in range(R):
        dGa = sAs[r] if br[r] == 0 else (sGs[r] if br[r] == 1 else f(0))
        al[r].append(-dGa)
        be[r].append(-(dGa - sGs[r]))
    P = 3 * R + S + 1
    LU, piv = mp.mp.LU_decomp(J)
    sd = f(t['sd'])
    nu = [[f(t['nu'][r, k]) for k in range(N)] for r in range(R)]
    flux = [sd * sum(nu[r][k] * (rf[r] - rb[r]) for r in range(R)) for k in range(N)]
    idle = [all(t['nu'][r, k] == 0.0 for r in range(R)) for k in range(N)]
    cols, dys = [], []
    for p in range(P):
        dnet = [rf[r] * al[r][p] - rb[r] * be[r][p] for r in range(R)]
        rhs = mp.zeros(T, 1)
        for s in range(G, T):
            if s not in dead:
                rhs[s] = -sum(m[r][s] * dnet[r] for r in range(R)) / D[s]
        dy = mp.mp.U_solve(LU, mp.mp.L_solve(LU, rhs, piv))
        dys.append([dy[k] for k in range(T)])
        cols.append([sd * sum(nu[r][k] * (dnet[r] + sum(W[r][q] * dy[q] for q in range(T))) for r in range(R)) for k in range(N)])
    norm = [[f(0) if idle[k] else (col[k] / flux[k] if flux[k] != 0 else mp.nan) for k in range(N)] for col in cols]
    kf, kb, ts, dg = DR.split(cols[:-1], R)
    return {'dflux_dlnkf': kf, 'dflux_dlnkb': kb, 'dflux_drc': ts, 'dflux_dG': dg, 'dy_drc': dys[2 * R:3 * R], 'drc': norm[2 * R:3 * R],
            'tdrc': norm[3 * R:-1], 'dflux_dstrength': cols[-1], 'dy_dstrength': dys[-1], 'strength_control': [lam * v for v in norm[-1]],
            'flux': flux, 'flux_scale': [sd * sum(abs(nu[r][k]) * (rf[r] + rb[r]) for r in range(R)) for k in range(N)],
            'residual': max(abs(v) for v in F), 'dy': dys}


def control_mp(tab, phiM, csurf, phi_surface, theta, w=1, CS=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None, strength=None, y_mp=None):
    """The formulas of the header at 60 digits at the given (fp64) theta, or at the 60-digit log-coverages y_mp [n][T]: nested lists of
    mpmath numbers under the names of FIELDS, 'residual' [n] and 'dy' [n][P][T]"""
    t = IR._arrays(tab)
    N, T, R = t['N'], t['T'], t['R']
    phiM = np.atleast_1d(np.asarray(phiM, float))
    n = len(phiM)
    csurf = np.asarray(csurf, float).reshape(n, N)
    if y_mp is None:
        theta = np.asarray(theta, float).reshape(n, T)
    res = {k: [] for k in FIELDS + ('residual', 'dy')}
    with mp.workdps(KR.DPS):
        f = mp.mpf
        lam = f(t['strength'] if strength is None else strength)
        for i in range(n):
            o = np.zeros((R, 2)) if off is None else np.asarray(off, float)[i].reshape(R, 2)
            g = np.ones(N) if gamma is None else np.asarray(gamma, float)[i]
            sgm = None if sigma is None else float(np.asarray(sigma)[i])
            V, sg, a = IR._mp_inputs(t, phiM[i], csurf[i], phi_surface[i], w, CS, phi_pzc, sgm, g)
            if y_mp is not None:
                y = list(y_mp[i])
            else:
                y = []
                for k in range(T):
                    th = theta[i, k]
                    y.append(f(0) if th >= 1.0 else (max(mp.log(f(th)), f(KR.MIN_LOG)) if th > 0.0 else f(KR.MIN_LOG)))
            one = _mp_point(t, V, sg, a, o, lam, y)
            for k in res:
                res[k].append(one[k])
    return res


def errors(res, ref, fp):
    """Per field of `res` (device or fp64 result): the worst error against the 60-digit `ref` per point, in units of fp's 'drc_scale'
    (flux in units of flux_scale).  An entry whose scale is 0 must be exact."""
    out = {}
    for k in FIELDS:
        if k in res and k != 'flux_scale':
            out[k] = KR.mp_err(ref[k], res[k], fp['flux_scale'] if k == 'flux' else fp['drc_scale'][k])
    return out
