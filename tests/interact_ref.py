"""NumPy and mpmath restatements of include/catint_interact.h (test infrastructure, no tests of its own), in the manner of
tests/kinetics_ref.py, whose helpers it uses where the two headers agree.

solve_fp64: the ramped iteration of the header operation for operation in fp64, one operating point after another, the linear systems
by np.linalg.solve.  solve_mp: the root of the last stage at 60 decimal digits by Newton from the fp64 result, the Jacobian by
differences with a step of 1e-30 (so nothing of the analytic Jacobian under test enters it); sensitivities by central differences of
such solves as in kinetics_ref.solve_mp.

tables: the keys of MeanFieldModel.tables() with 'order_f', 'order_b' [R][N+T] and 'site_count' [T], plus 'site_of' [T] int,
'site_fraction' [G], 'eps' [S][S], 'eps_ts' [R][S], 'response' ('linear' | 'piecewise'), 'cutoff', 'smoothing' [G] and 'strength' --
what catint_amd.interactions.InteractingModel.tables() returns and catint_amd._interact.InteractingKinetics.solve takes."""
import mpmath as mp
import numpy as np

from tests import kinetics_ref as KR

MIN_LOG = KR.MIN_LOG
DPS = KR.DPS
mp_err = KR.mp_err


def shape(tab):
    """(N, G, S, R)"""
    R, M = np.asarray(tab['order_f']).shape
    T, G = len(tab['site_count']), len(tab['site_fraction'])
    return M - T, G, T - G, R


def _arrays(tab):
    N, G, S, R = shape(tab)
    T = G + S
    of, ob = np.asarray(tab['order_f'], int), np.asarray(tab['order_b'], int)
    eps = np.asarray(tab['eps'], float).reshape(S, S)
    ets = np.zeros((R, S)) if tab.get('eps_ts') is None else np.asarray(tab['eps_ts'], float).reshape(R, S)
    m = (ob[:, N:] - of[:, N:]).astype(float)
    ofc = of[:, N:].astype(float)
    # the contractions of the header, t ascending
    eg, ea = np.zeros((R, S)), np.zeros((R, S))
    for r in range(R):
        for u in range(S):
            g = f = 0.0
            for a in range(S):
                g = g + m[r, G + a] * eps[a, u]
                f = f + ofc[r, G + a] * eps[a, u]
            eg[r, u], ea[r, u] = g, ets[r, u] - f
    piecewise = tab.get('response', 'linear') == 'piecewise'
    site_of = np.asarray(tab['site_of'], int)
    x = np.asarray(tab['site_fraction'], float)
    ns = np.asarray(tab['site_count'], float)
    return dict(N=N, G=G, S=S, R=R, T=T, ofs=of[:, :N], obs=ob[:, :N], ofc=ofc, obc=ob[:, N:].astype(float), m=m,
                nu=np.asarray(tab['nu'], float).reshape(R, N), cref=np.asarray(tab['cref'], float), ns=ns, site_of=site_of, x=x,
                nx=ns / x[site_of], dG=np.asarray(tab['dG'], float), Ea=np.asarray(tab['Ea'], float), lnA=np.asarray(tab['lnA'], float),
                sd=float(tab['site_density']), eps=eps, ets=ets, eg=eg, ea=ea, piecewise=piecewise,
                cutoff=np.asarray(tab['cutoff'], float) if piecewise else np.zeros(G),
                smooth=np.asarray(tab['smoothing'], float) if piecewise else np.ones(G), strength=float(tab.get('strength', 1.0)),
                ts=~np.isneginf(np.asarray(tab['Ea'], float)[:, 0]))


def stage_strengths(strength, K):
    return [strength if k == K - 1 else (strength * k) / (K - 1) for k in range(K)]


def response(t, crowd):
    """f_g, f'_g"""
    if not t['piecewise']:
        return np.ones(t['G']), np.zeros(t['G'])
    c, s = t['cutoff'], t['smooth']
    d = crowd - c
    u = d + s
    f = np.where(d <= -s, 0.0, np.where(d < s, (u * u) / (4.0 * s), d))
    fp = np.where(d <= -s, 0.0, np.where(d < s, u / (2.0 * s), 1.0))
    return f, fp


def surface_state(t, y):
    """theta [T], w [S] = f theta of the adsorbates, f, f' [G]"""
    G, T = t['G'], t['T']
    with np.errstate(over='ignore'):
        th = np.exp(y)
    crowd = np.zeros(G)
    for k in range(G, T):
        crowd[t['site_of'][k]] = crowd[t['site_of'][k]] + t['ns'][k] * th[k]
    f, fp = response(t, crowd / t['x'])
    return th, f[t['site_of'][G:]] * th[G:], f, fp


def step_constants(t, V, sg, off, lam, th, w):
    """ln kf, ln kb, branch, and the per-type sums qg, qs [R][G] of the piecewise Jacobian"""
    R, S, G = t['R'], t['S'], t['G']
    with np.errstate(invalid='ignore', over='ignore'):
        s2 = sg * sg
        dG0 = ((t['dG'][:, 0] + t['dG'][:, 1] * V) + t['dG'][:, 2] * sg) + t['dG'][:, 3] * s2
        Ea0 = ((t['Ea'][:, 0] + t['Ea'][:, 1] * V) + t['Ea'][:, 2] * sg) + t['Ea'][:, 3] * s2
        sG, sA = np.zeros(R), np.zeros(R)
        for a in range(S):
            sG = sG + t['eg'][:, a] * w[a]
            sA = sA + t['ea'][:, a] * w[a]
        dG = dG0 + lam * sG
        Ea = np.where(t['ts'], Ea0 + lam * sA, Ea0)
    b0 = (Ea >= dG) & (Ea >= 0.0)
    b1 = ~b0 & (dG >= 0.0)
    br = np.where(b0, 0, np.where(b1, 1, 2))
    with np.errstate(invalid='ignore'):
        Ga = np.where(b0, Ea, np.where(b1, dG, 0.0))
        lf = (t['lnA'] - Ga) + off[:, 0]
        lb = (t['lnA'] - (Ga - dG)) + off[:, 1]
    es = np.where((br == 0)[:, None], t['ea'], np.where((br == 1)[:, None], t['eg'], 0.0))
    qg, qs = np.zeros((R, G)), np.zeros((R, G))
    if t['piecewise']:
        for a in range(S):
            g = t['site_of'][G + a]
            qg[:, g] = qg[:, g] + t['eg'][:, a] * th[G + a]
            qs[:, g] = qs[:, g] + es[:, a] * th[G + a]
    return lf, lb, br, es, qg, qs


def effective_orders(t, lam, th, f, fp, es, qg, qs):
    """d ln rf_r / dy_t, d ln rb_r / dy_t [R][T]"""
    G = t['G']
    ofe, obe = t['ofc'].copy(), t['obc'].copy()
    g = t['site_of'][G:]
    with np.errstate(invalid='ignore', over='ignore'):
        gG = lam * (t['eg'] * f[g][None, :] + (t['nx'][G:] * fp[g])[None, :] * qg[:, g])
        gS = lam * (es * f[g][None, :] + (t['nx'][G:] * fp[g])[None, :] * qs[:, g])
        ofe[:, G:] = ofe[:, G:] - th[None, G:] * gS
        obe[:, G:] = obe[:, G:] - th[None, G:] * (gS - gG)
    return ofe, obe


def rates(t, y, a, lf, lb):
    with np.errstate(over='ignore', invalid='ignore'):
        ef, eb = np.exp(lf + t['ofc'] @ y), np.exp(lb + t['obc'] @ y)
        pf = np.prod(np.power(a[None, :], t['ofs']), axis=1) if t['N'] else np.ones(t['R'])
        pb = np.prod(np.power(a[None, :], t['obs']), axis=1) if t['N'] else np.ones(t['R'])
        return ef * pf, eb * pb, ef, eb


def system(t, y, a, V, sg, off, lam):
    """scaled Jacobian, scaled residual, row scales, d rate / dy [R][T], rf, rb, ef, eb, branch; a dead row sets its y to MIN_LOG (in place)"""
    G, T, R = t['G'], t['T'], t['R']
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        th, w, f, fp = surface_state(t, y)
        lf, lb, br, es, qg, qs = step_constants(t, V, sg, off, lam, th, w)
        rf, rb, ef, eb = rates(t, y, a, lf, lb)
        ofe, obe = effective_orders(t, lam, th, f, fp, es, qg, qs)
        Wy = rf[:, None] * ofe - rb[:, None] * obe
        m = t['m']
        B, D, J = np.zeros(T), np.zeros(T), np.zeros((T, T))
        for r in range(R):
            B = B + m[r] * (rf[r] - rb[r])
            D = D + np.abs(m[r]) * (rf[r] + rb[r])
            J = J + m[r][:, None] * Wy[r][None, :]
        F = np.zeros(T)
        for s in range(G, T):
            if D[s] == 0.0:
                J[s] = 0.0
                J[s, s] = 1.0
                y[s] = MIN_LOG
            else:
                J[s] /= D[s]
                F[s] = B[s] / D[s]
        nth = t['ns'] * np.exp(y)
        for g in range(G):
            on = t['site_of'] == g
            J[g] = np.where(on, nth / t['x'][g], 0.0)
            F[g] = np.where(on, nth, 0.0).sum() / t['x'][g] - 1.0
    return J, F, D, Wy, rf, rb, ef, eb, br


def start(t, guess):
    if guess is None:
        per_type = np.array([t['ns'][t['site_of'] == g].sum() for g in range(t['G'])])
        return np.log(t['x'][t['site_of']] / per_type[t['site_of']])
    g = np.asarray(guess, float)
    with np.errstate(divide='ignore', invalid='ignore'):
        y = np.where(g >= 1.0, 0.0, np.where(g > 0.0, np.log(np.where(g > 0.0, g, 1.0)), MIN_LOG))
    return np.maximum(y, MIN_LOG)


def solve_point(t, phiM, c, phi0, w=1, CS=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None, guess=None, tol=1e-12, maxit=200, sens=True,
                ramp=1, strength=None):
    N, T, R, S = t['N'], t['T'], t['R'], t['S']
    strength = t['strength'] if strength is None else float(strength)
    off = np.zeros((R, 2)) if off is None else np.asarray(off, float).reshape(R, 2)
    gamma = np.ones(N) if gamma is None else np.asarray(gamma, float)
    c = np.asarray(c, float).reshape(N)
    V, sg = KR.potential_and_charge(phiM, phi0, w, CS, phi_pzc, sigma)
    nan = dict(theta=np.full(T, np.nan), y=np.full(T, np.nan), rate=np.full(R, np.nan), rate_gross=np.full(R, np.nan), flux=np.full(N, np.nan),
               flux_scale=np.full(N, np.nan), dflux_dc=np.full((N, N), np.nan), dflux_dphi=np.full((N, 2), np.nan), energy_shift=np.full(S, np.nan),
               status=2, iterations=0, ramp_reached=0, strength_reached=np.nan)
    fin = np.isfinite([phiM, phi0, sg]).all() and np.isfinite(c).all() and np.isfinite(gamma).all() and np.isfinite(off).all()
    if guess is not None:
        fin = fin and np.isfinite(guess).all()
    if not fin:
        return nan
    a = gamma * np.maximum(c, 0.0) / t['cref']
    y = np.array(start(t, guess), float)
    status, total, reached, lam = 1, 0, 0, strength
    for k, lam in enumerate(stage_strengths(strength, ramp)):
        status, reached = 1, k
        for _ in range(maxit):
            J, F = system(t, y, a, V, sg, off, lam)[:2]
            try:
                with np.errstate(all='ignore'):
                    dy = np.linalg.solve(J, -F)
            except np.linalg.LinAlgError:
                status = 3
                break
            mx = np.abs(dy).max() if np.isfinite(dy).all() else np.nan
            sc = 3.0 / mx if mx > 3.0 else 1.0
            y = np.maximum(y + sc * dy, MIN_LOG) if np.isfinite(mx) else y + dy
            total += 1
            if mx < tol:
                status = 0
                break
        if status != 0:
            break
    th, wv, f, fp = surface_state(t, y)
    lf, lb, br = step_constants(t, V, sg, off, lam, th, wv)[:3]
    rf, rb, ef, eb = rates(t, y, a, lf, lb)
    shift = np.zeros(S)
    for u in range(S):
        shift = shift + t['eps'][:, u] * wv[u]
    out = dict(theta=np.exp(y), y=y.copy(), rate=rf - rb, rate_gross=rf + rb, flux=t['sd'] * (t['nu'].T @ (rf - rb)),
               flux_scale=t['sd'] * (np.abs(t['nu']).T @ (rf + rb)), energy_shift=lam * shift, status=status, iterations=total, ramp_reached=reached,
               strength_reached=lam)
    if sens:
        J, F, D, Wy, rf, rb, ef, eb, br = system(t, y, a, V, sg, off, lam)
        dnet = np.zeros((R, N + 2))
        for j in range(N):
            dadc = gamma[j] / t['cref'][j] if c[j] >= 0.0 else 0.0
            left_f = np.prod(np.power(a[None, :], np.maximum(t['ofs'] - (np.arange(N) == j), 0)), axis=1)
            left_b = np.prod(np.power(a[None, :], np.maximum(t['obs'] - (np.arange(N) == j), 0)), axis=1)
            dnet[:, j] = ef * (t['ofs'][:, j] * left_f * dadc) - eb * (t['obs'][:, j] * left_b * dadc)
        for q, (dV, ds) in enumerate(((1.0, CS if sigma is None else 0.0), (-1.0 if w else 0.0, -CS if sigma is None else 0.0))):
            dlf, dlb = KR.slopes(t, sg, br, dV, ds)
            dnet[:, N + q] = rf * dlf - rb * dlb
        rhs = t['m'].T @ dnet
        rhs[:t['G']] = 0.0
        for s in range(t['G'], T):
            rhs[s] = 0.0 if D[s] == 0.0 else -rhs[s] / D[s]
        try:
            with np.errstate(all='ignore'):
                dy = np.linalg.solve(J, rhs)
                dy_terms = np.abs(np.linalg.inv(J)) @ (np.abs(J) @ np.abs(dy))
        except np.linalg.LinAlgError:
            dy = np.full((T, N + 2), np.nan)
            dy_terms = np.full((T, N + 2), np.nan)
            out['status'] = 3
        dflux = t['sd'] * (t['nu'].T @ (dnet + Wy @ dy))
        out['dflux_dc'], out['dflux_dphi'] = dflux[:, :N].copy(), dflux[:, N:].copy()
        # the scales of kinetics_ref.solve_point, with the full d rate / dy
        out['dflux_scale'] = t['sd'] * (np.abs(t['nu']).T @ (np.abs(dnet) + np.abs(Wy) @ dy_terms))
        out['dflux_terms'] = t['sd'] * (np.abs(t['nu']).T @ (np.abs(dnet) + np.abs(Wy) @ np.abs(dy)))
        out['jacobian'], out['residual'] = J, F
    return out


def solve_fp64(tab, phiM, csurf, phi_surface, w=1, CS=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None, theta_guess=None, tol=1e-12,
               maxit=200, sens=True, ramp=1, strength=None):
    """Every operating point of the call; a dict of stacked arrays (the names of catia_outputs, and 'y', 'dflux_scale', 'strength_reached')"""
    t = _arrays(tab)
    phiM = np.atleast_1d(np.asarray(phiM, float))
    n = len(phiM)
    csurf = np.asarray(csurf, float).reshape(n, t['N'])
    pp = KR._per_point
    outs = [solve_point(t, phiM[i], csurf[i], np.asarray(phi_surface, float)[i], w, CS, phi_pzc, pp(sigma, i), pp(off, i), pp(gamma, i),
                        pp(theta_guess, i), tol, maxit, sens, ramp, strength) for i in range(n)]
    keys = [k for k in outs[0] if all(k in o for o in outs)] if outs else []
    res = {k: np.array([o[k] for o in outs]) for k in keys}
    for k in ('status', 'iterations', 'ramp_reached'):
        if outs:
            res[k] = res[k].astype(np.int32)
    return res


# ---- 60 digits -----------------------------------------------------------------------------------------------------------------------
def _mp_inputs(t, phiM, c, phi0, w, CS, phi_pzc, sigma, gamma):
    f = mp.mpf
    V = f(phiM) - (f(phi0) if w else 0)
    sg = f(CS) * ((f(phiM) - f(phi_pzc)) - f(phi0)) if sigma is None else f(sigma)
    a = []
    for j in range(t['N']):
        cj = f(c[j])
        a.append(f(gamma[j]) * (cj if cj > 0 else f(0)) / f(t['cref'][j]))
    return V, sg, a


def _mp_rates(t, y, V, sg, a, off, lam):
    """rf, rb [R] and the shifts dE [S] from the definition of the header (not from the contracted rows)"""
    f = mp.mpf
    G, T, S, R, N = t['G'], t['T'], t['S'], t['R'], t['N']
    th = [mp.exp(v) for v in y]
    crowd = [f(0)] * G
    for k in range(G, T):
        crowd[t['site_of'][k]] += f(t['ns'][k]) * th[k]
    fg = []
    for g in range(G):
        if not t['piecewise']:
            fg.append(f(1))
            continue
        C, c, s = crowd[g] / f(t['x'][g]), f(t['cutoff'][g]), f(t['smooth'][g])
        fg.append(f(0) if C <= c - s else ((C - c + s) ** 2 / (4 * s) if C < c + s else C - c))
    wv = [fg[t['site_of'][G + u]] * th[G + u] for u in range(S)]
    dE = [lam * sum(f(t['eps'][k, u]) * wv[u] for u in range(S)) for k in range(S)]
    rf, rb = [], []
    for r in range(R):
        dG = f(t['dG'][r, 0]) + f(t['dG'][r, 1]) * V + f(t['dG'][r, 2]) * sg + f(t['dG'][r, 3]) * sg * sg
        dG += sum(int(t['m'][r, G + k]) * dE[k] for k in range(S))
        Ea = None
        if t['ts'][r]:
            Ea = f(t['Ea'][r, 0]) + f(t['Ea'][r, 1]) * V + f(t['Ea'][r, 2]) * sg + f(t['Ea'][r, 3]) * sg * sg
            Ea += lam * sum(f(t['ets'][r, u]) * wv[u] for u in range(S)) - sum(int(t['ofc'][r, G + k]) * dE[k] for k in range(S))
        Ga = Ea if (Ea is not None and Ea >= dG and Ea >= 0) else (dG if dG >= 0 else f(0))
        sf = f(t['lnA'][r]) - Ga + f(off[r, 0])
        sb = f(t['lnA'][r]) - (Ga - dG) + f(off[r, 1])
        pf = pb = f(1)
        for k in range(T):
            sf += int(t['ofc'][r, k]) * y[k]
            sb += int(t['obc'][r, k]) * y[k]
        for j in range(N):
            pf *= a[j] ** int(t['ofs'][r, j])
            pb *= a[j] ** int(t['obs'][r, j])
        rf.append(mp.exp(sf) * pf)
        rb.append(mp.exp(sb) * pb)
    return rf, rb, dE


def _mp_residual(t, y, V, sg, a, off, lam, dead, D):
    G, T, R = t['G'], t['T'], t['R']
    rf, rb, _ = _mp_rates(t, y, V, sg, a, off, lam)
    F = [mp.mpf(0)] * T
    for g in range(G):
        F[g] = sum(mp.mpf(t['ns'][k]) * mp.exp(y[k]) for k in range(T) if t['site_of'][k] == g) / mp.mpf(t['x'][g]) - 1
    for s in range(G, T):
        if s not in dead:
            F[s] = sum(int(t['m'][r, s]) * (rf[r] - rb[r]) for r in range(R)) / D[s]
    return F


def _mp_jacobian(t, y, V, sg, a, off, lam, dead, D, live):
    h = mp.mpf(10) ** -30
    J = mp.zeros(len(live), len(live))
    for jc, k in enumerate(live):
        yp, ym = list(y), list(y)
        yp[k] += h
        ym[k] -= h
        Fp, Fm = _mp_residual(t, yp, V, sg, a, off, lam, dead, D), _mp_residual(t, ym, V, sg, a, off, lam, dead, D)
        for ir, s in enumerate(live):
            J[ir, jc] = (Fp[s] - Fm[s]) / (2 * h)
    return J


def _mp_scales(t, y, V, sg, a, off, lam):
    G, T, R = t['G'], t['T'], t['R']
    rf, rb, _ = _mp_rates(t, y, V, sg, a, off, lam)
    return [sum(abs(int(t['m'][r, s])) * (abs(rf[r]) + abs(rb[r])) for r in range(R)) if s >= G else mp.mpf(1) for s in range(T)]


def _mp_newton(t, y, V, sg, a, off, lam, dead, frozen=None, iters=60):
    """Newton from y.  frozen: (row scales, Jacobian) of a neighbouring solution, kept for every iteration -- for a solve whose inputs
    differ from that solution's by 1e-20 the error then falls by that factor per iteration"""
    live = [s for s in range(t['T']) if s not in dead]
    for _ in range(iters):
        D, J = frozen if frozen is not None else (_mp_scales(t, y, V, sg, a, off, lam), None)
        if J is None:
            J = _mp_jacobian(t, y, V, sg, a, off, lam, dead, D, live)
        F0 = _mp_residual(t, y, V, sg, a, off, lam, dead, D)
        dy = mp.lu_solve(J, -mp.matrix([F0[s] for s in live]))
        mx = max(abs(v) for v in dy)
        sc = 3 / mx if mx > 3 else 1
        for jc, k in enumerate(live):
            y[k] += sc * dy[jc]
        if mx < mp.mpf(10) ** (-(DPS - 12)):
            break
    return y


def _mp_solve(t, y0, dead, phiM, c, phi0, w, CS, phi_pzc, sigma, off, gamma, lam, frozen=None, want_frozen=False):
    V, sg, a = _mp_inputs(t, phiM, c, phi0, w, CS, phi_pzc, sigma, gamma)
    y = _mp_newton(t, [mp.mpf(v) for v in y0], V, sg, a, off, lam, dead, frozen)
    rf, rb, dE = _mp_rates(t, y, V, sg, a, off, lam)
    sd = mp.mpf(t['sd'])
    flux = [sd * sum(mp.mpf(t['nu'][r, k]) * (rf[r] - rb[r]) for r in range(t['R'])) for k in range(t['N'])]
    if want_frozen:
        D = _mp_scales(t, y, V, sg, a, off, lam)
        frozen = (D, _mp_jacobian(t, y, V, sg, a, off, lam, dead, D, [s for s in range(t['T']) if s not in dead]))
    return y, rf, rb, flux, dE, frozen


def solve_mp(tab, phiM, csurf, phi_surface, fp64, w=1, CS=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None, sens=True, strength=None):
    """The points of solve_fp64's result `fp64` at 60 digits and the strength those points ended with.  Nested lists of mpmath numbers:
    'y' [n][T], 'rate', 'rate_gross' [n][R], 'flux', 'flux_scale' [n][N], 'energy_shift' [n][S], with sens 'dflux_dc', 'dflux_dphi'."""
    t = _arrays(tab)
    N, T, R, G = t['N'], t['T'], t['R'], t['G']
    phiM = np.atleast_1d(np.asarray(phiM, float))
    n = len(phiM)
    csurf = np.asarray(csurf, float).reshape(n, N)
    res = {k: [] for k in ('y', 'rate', 'rate_gross', 'flux', 'flux_scale', 'energy_shift', 'dflux_dc', 'dflux_dphi')}
    with mp.workdps(DPS):
        f = mp.mpf
        for i in range(n):
            o = np.zeros((R, 2)) if off is None else np.asarray(off, float)[i].reshape(R, 2)
            g = np.ones(N) if gamma is None else np.asarray(gamma, float)[i]
            sgm = None if sigma is None else float(np.asarray(sigma)[i])
            lam = f(float(fp64['strength_reached'][i]) if strength is None else strength)
            y0 = fp64['y'][i]
            V, sg, a = _mp_inputs(t, phiM[i], csurf[i], phi_surface[i], w, CS, phi_pzc, sgm, g)
            rf, rb, _ = _mp_rates(t, [f(v) for v in y0], V, sg, a, o, lam)
            dead = {s for s in range(G, T) if sum(abs(int(t['m'][r, s])) * (rf[r] + rb[r]) for r in range(R)) == 0}
            args = (w, CS, phi_pzc, sgm, o, g, lam)
            y, rf, rb, flux, dE, frozen = _mp_solve(t, y0, dead, f(phiM[i]), [f(v) for v in csurf[i]], f(phi_surface[i]), *args, want_frozen=sens)
            res['y'].append(y)
            res['rate'].append([rf[r] - rb[r] for r in range(R)])
            res['rate_gross'].append([rf[r] + rb[r] for r in range(R)])
            res['flux'].append(flux)
            res['flux_scale'].append([f(t['sd']) * sum(abs(f(t['nu'][r, k])) * (rf[r] + rb[r]) for r in range(R)) for k in range(N)])
            res['energy_shift'].append(dE)
            if not sens:
                continue
            dc = [[None] * N for _ in range(N)]
            dphi = [[None] * 2 for _ in range(N)]
            for p in range(N + 2):
                pm, cc, p0 = f(phiM[i]), [f(v) for v in csurf[i]], f(phi_surface[i])
                one_sided = p < N and cc[p] == 0
                fl = []
                for sign in ((1, 2) if one_sided else (1, -1)):
                    qm, qc, q0 = pm, list(cc), p0
                    if p < N:
                        h = f(10) ** -30 * f(t['cref'][p]) if one_sided else f(10) ** -20 * abs(cc[p])
                        qc[p] = cc[p] + sign * h
                    else:
                        h = f(10) ** -20
                        if p == N:
                            qm = pm + sign * h
                        else:
                            q0 = p0 + sign * h
                    # (from c = 0 the log-coverages move by more than the step: a full Newton iteration there)
                    fl.append(_mp_solve(t, y, dead, qm, qc, q0, *args, frozen=None if one_sided else frozen)[3])
                for k in range(N):
                    d = (-3 * flux[k] + 4 * fl[0][k] - fl[1][k]) / (2 * h) if one_sided else (fl[0][k] - fl[1][k]) / (2 * h)
                    if p < N:
                        dc[k][p] = d
                    else:
                        dphi[k][p - N] = d
            res['dflux_dc'].append(dc)
            res['dflux_dphi'].append(dphi)
    return res
