"""NumPy and mpmath restatements of include/catint_kinetics.h (test infrastructure, no tests of its own).

solve_fp64: the iteration of the header operation for operation in fp64, one operating point after another, the linear systems by
np.linalg.solve.  solve_mp: the same root at 60 decimal digits by plain Newton from the fp64 result; sensitivities by central
differences of such solves with a relative step of 1e-20 (truncation and rounding both near 1e-40; at a concentration of exactly 0,
where log-coverages admit no negative side, the one-sided second-order formula).

tables: {'order_f', 'order_b' [R][N+S+1] int, 'nu' [R][N], 'cref' [N], 'site_count' [S+1], 'dG', 'Ea' [R][4], 'lnA' [R],
'site_density'} -- what catint_amd.microkinetics.MeanFieldModel.tables() returns and catint_amd._kinetics.KineticsSolver.solve takes."""
import mpmath as mp
import numpy as np

MIN_LOG = -700.0
DPS = 60


def shape(tab):
    R, M = np.asarray(tab['order_f']).shape
    T = len(tab['site_count'])
    return M - T, T - 1, R


def _arrays(tab):
    N, S, R = shape(tab)
    of, ob = np.asarray(tab['order_f'], int), np.asarray(tab['order_b'], int)
    return dict(N=N, S=S, R=R, T=S + 1, ofs=of[:, :N], obs=ob[:, :N], ofc=of[:, N:].astype(float), obc=ob[:, N:].astype(float),
                m=(ob[:, N:] - of[:, N:]).astype(float), nu=np.asarray(tab['nu'], float).reshape(R, N), cref=np.asarray(tab['cref'], float),
                ns=np.asarray(tab['site_count'], float), dG=np.asarray(tab['dG'], float), Ea=np.asarray(tab['Ea'], float),
                lnA=np.asarray(tab['lnA'], float), sd=float(tab['site_density']))


def potential_and_charge(phiM, phi0, w, CS, phi_pzc, sigma):
    V = phiM - (phi0 if w else 0.0)
    sg = CS * ((phiM - phi_pzc) - phi0) if sigma is None else sigma
    return V, sg


def rate_constants(t, V, sg, off):
    with np.errstate(invalid='ignore'):
        s2 = sg * sg
        dG = ((t['dG'][:, 0] + t['dG'][:, 1] * V) + t['dG'][:, 2] * sg) + t['dG'][:, 3] * s2
        Ea = ((t['Ea'][:, 0] + t['Ea'][:, 1] * V) + t['Ea'][:, 2] * sg) + t['Ea'][:, 3] * s2
    b0 = (Ea >= dG) & (Ea >= 0.0)
    b1 = ~b0 & (dG >= 0.0)
    Ga = np.where(b0, Ea, np.where(b1, dG, 0.0))
    lf = (t['lnA'] - Ga) + off[:, 0]
    lb = (t['lnA'] - (Ga - dG)) + off[:, 1]
    return lf, lb, np.where(b0, 0, np.where(b1, 1, 2))


def slopes(t, sg, br, dV, ds):
    ddG = t['dG'][:, 1] * dV + (t['dG'][:, 2] + 2.0 * t['dG'][:, 3] * sg) * ds
    dEa = t['Ea'][:, 1] * dV + (t['Ea'][:, 2] + 2.0 * t['Ea'][:, 3] * sg) * ds
    dGa = np.where(br == 0, dEa, np.where(br == 1, ddG, 0.0))
    return -dGa, -(dGa - ddG)


def rates(t, y, a, lf, lb):
    with np.errstate(over='ignore', invalid='ignore'):
        ef, eb = np.exp(lf + t['ofc'] @ y), np.exp(lb + t['obc'] @ y)
        pf = np.prod(np.power(a[None, :], t['ofs']), axis=1) if t['N'] else np.ones(t['R'])
        pb = np.prod(np.power(a[None, :], t['obs']), axis=1) if t['N'] else np.ones(t['R'])
        return ef * pf, eb * pb, ef, eb


def system(t, y, a, lf, lb):
    """scaled Jacobian, scaled residual, row scales; an adsorbate that nothing produces or consumes is set to MIN_LOG in y (in place)"""
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        rf, rb, _, _ = rates(t, y, a, lf, lb)
        m, T = t['m'], t['T']
        G = m.T @ (rf - rb)
        D = np.abs(m).T @ (rf + rb)
        J = m.T @ (rf[:, None] * t['ofc'] - rb[:, None] * t['obc'])
        F = np.zeros(T)
        for s in range(1, T):
            if D[s] == 0.0:
                J[s] = 0.0
                J[s, s] = 1.0
                y[s] = MIN_LOG
            else:
                J[s] /= D[s]
                F[s] = G[s] / D[s]
        th = t['ns'] * np.exp(y)
        J[0] = th
        F[0] = th.sum() - 1.0
    return J, F, D


def start(t, guess):
    if guess is None:
        return np.full(t['T'], np.log(1.0 / t['ns'].sum()))
    g = np.asarray(guess, float)
    with np.errstate(divide='ignore', invalid='ignore'):
        y = np.where(g >= 1.0, 0.0, np.where(g > 0.0, np.log(np.where(g > 0.0, g, 1.0)), MIN_LOG))
    return np.maximum(y, MIN_LOG)


def solve_point(t, phiM, c, phi0, w=1, CS=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None, guess=None, tol=1e-12, maxit=200, sens=True):
    N, T, R = t['N'], t['T'], t['R']
    off = np.zeros((R, 2)) if off is None else np.asarray(off, float).reshape(R, 2)
    gamma = np.ones(N) if gamma is None else np.asarray(gamma, float)
    c = np.asarray(c, float).reshape(N)
    V, sg = potential_and_charge(phiM, phi0, w, CS, phi_pzc, sigma)
    nan = dict(theta=np.full(T, np.nan), y=np.full(T, np.nan), rate=np.full(R, np.nan), rate_gross=np.full(R, np.nan), flux=np.full(N, np.nan),
               flux_scale=np.full(N, np.nan), dflux_dc=np.full((N, N), np.nan), dflux_dphi=np.full((N, 2), np.nan), status=2, iterations=0)
    fin = np.isfinite([phiM, phi0, sg]).all() and np.isfinite(c).all() and np.isfinite(gamma).all() and np.isfinite(off).all()
    if guess is not None:
        fin = fin and np.isfinite(guess).all()
    if not fin:
        return nan
    a = gamma * np.maximum(c, 0.0) / t['cref']
    lf, lb, br = rate_constants(t, V, sg, off)
    y = np.array(start(t, guess), float)
    status, it = 1, 0
    for _ in range(maxit):
        J, F, D = system(t, y, a, lf, lb)
        try:
            with np.errstate(all='ignore'):
                dy = np.linalg.solve(J, -F)
        except np.linalg.LinAlgError:
            status = 3
            break
        mx = np.abs(dy).max() if np.isfinite(dy).all() else np.nan
        sc = 3.0 / mx if mx > 3.0 else 1.0
        y = np.maximum(y + sc * dy, MIN_LOG) if np.isfinite(mx) else y + dy
        it += 1
        if mx < tol:
            status = 0
            break
    rf, rb, ef, eb = rates(t, y, a, lf, lb)
    out = dict(theta=np.exp(y), y=y.copy(), rate=rf - rb, rate_gross=rf + rb, flux=t['sd'] * (t['nu'].T @ (rf - rb)),
               flux_scale=t['sd'] * (np.abs(t['nu']).T @ (rf + rb)), status=status, iterations=it)
    if sens:
        J, F, D = system(t, y, a, lf, lb)
        Wy = rf[:, None] * t['ofc'] - rb[:, None] * t['obc']          # d rate_r / d y_t
        dnet = np.zeros((R, N + 2))                                   # d rate_r / dp at fixed y
        for j in range(N):
            dadc = gamma[j] / t['cref'][j] if c[j] >= 0.0 else 0.0
            left_f = np.prod(np.power(a[None, :], np.maximum(t['ofs'] - (np.arange(N) == j), 0)), axis=1)
            left_b = np.prod(np.power(a[None, :], np.maximum(t['obs'] - (np.arange(N) == j), 0)), axis=1)
            dnet[:, j] = ef * (t['ofs'][:, j] * left_f * dadc) - eb * (t['obs'][:, j] * left_b * dadc)
        for q, (dV, ds) in enumerate(((1.0, CS if sigma is None else 0.0), (-1.0 if w else 0.0, -CS if sigma is None else 0.0))):
            dlf, dlb = slopes(t, sg, br, dV, ds)
            dnet[:, N + q] = rf * dlf - rb * dlb
        rhs = t['m'].T @ dnet
        rhs[0] = 0.0
        for s in range(1, T):
            rhs[s] = 0.0 if D[s] == 0.0 else -rhs[s] / D[s]
        try:
            with np.errstate(all='ignore'):
                dy = np.linalg.solve(J, rhs)
        except np.linalg.LinAlgError:
            dy = np.full((T, N + 2), np.nan)
            out['status'] = 3
        dflux = t['sd'] * (t['nu'].T @ (dnet + Wy @ dy))              # [N][N+2]
        out['dflux_dc'], out['dflux_dphi'] = dflux[:, :N].copy(), dflux[:, N:].copy()
        # the sum of the absolute terms of each entry: what the accuracy of a sensitivity is stated relative to.  dy comes out of a linear
        # solve, whose result is itself a sum that cancels: its terms are those of J^-1 (J dy), |J^-1| |J| |dy| -- the componentwise
        # bound of Gaussian elimination (Skeel), of which |dy| and |J^-1| |rhs| are lower estimates that miss the conditioning of J
        try:
            with np.errstate(all='ignore'):
                dy_terms = np.abs(np.linalg.inv(J)) @ (np.abs(J) @ np.abs(dy))
        except np.linalg.LinAlgError:
            dy_terms = np.full((T, N + 2), np.nan)
        terms = np.abs(t['nu']).T @ (np.abs(dnet) + np.abs(Wy) @ dy_terms)
        out['dflux_scale'] = t['sd'] * terms
        # (the plain term sum, |dy| in the place of the bound: what DESIGN quotes beside it)
        out['dflux_terms'] = t['sd'] * (np.abs(t['nu']).T @ (np.abs(dnet) + np.abs(Wy) @ np.abs(dy)))
    return out


def _per_point(x, i):
    return None if x is None else np.asarray(x)[i]


def solve_fp64(tab, phiM, csurf, phi_surface, w=1, CS=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None, theta_guess=None, tol=1e-12,
               maxit=200, sens=True):
    """Every operating point of the call; returns a dict of stacked arrays (the names of catkin_outputs, and 'y', 'dflux_scale')"""
    t = _arrays(tab)
    phiM = np.atleast_1d(np.asarray(phiM, float))
    n = len(phiM)
    csurf = np.asarray(csurf, float).reshape(n, t['N'])
    outs = [solve_point(t, phiM[i], csurf[i], np.asarray(phi_surface, float)[i], w, CS, phi_pzc, _per_point(sigma, i), _per_point(off, i),
                        _per_point(gamma, i), _per_point(theta_guess, i), tol, maxit, sens) for i in range(n)]
    keys = [k for k in outs[0] if all(k in o for o in outs)] if outs else []
    res = {k: np.array([o[k] for o in outs]) for k in keys}
    if outs:
        res['status'] = res['status'].astype(np.int32)
        res['iterations'] = res['iterations'].astype(np.int32)
    return res


# ---- 60 digits -----------------------------------------------------------------------------------------------------------------------
def _mp_state(t, phiM, c, phi0, w, CS, phi_pzc, sigma, off, gamma, clamp):
    f = mp.mpf
    N, R = t['N'], t['R']
    V = f(phiM) - (f(phi0) if w else 0)
    sg = f(CS) * ((f(phiM) - f(phi_pzc)) - f(phi0)) if sigma is None else f(sigma)
    a = []
    for j in range(N):
        cj = f(c[j])
        if clamp and cj < 0:
            cj = f(0)
        a.append(f(gamma[j]) * cj / f(t['cref'][j]))
    lf, lb = [], []
    for r in range(R):
        dG = f(t['dG'][r, 0]) + f(t['dG'][r, 1]) * V + f(t['dG'][r, 2]) * sg + f(t['dG'][r, 3]) * sg * sg
        if np.isneginf(t['Ea'][r, 0]):
            Ea = None
        else:
            Ea = f(t['Ea'][r, 0]) + f(t['Ea'][r, 1]) * V + f(t['Ea'][r, 2]) * sg + f(t['Ea'][r, 3]) * sg * sg
        if Ea is not None and Ea >= dG and Ea >= 0:
            Ga = Ea
        elif dG >= 0:
            Ga = dG
        else:
            Ga = f(0)
        lf.append(f(t['lnA'][r]) - Ga + f(off[r, 0]))
        lb.append(f(t['lnA'][r]) - (Ga - dG) + f(off[r, 1]))
    return a, lf, lb


def _mp_rates(t, y, a, lf, lb):
    rf, rb = [], []
    for r in range(t['R']):
        sf, sb = lf[r], lb[r]
        for k in range(t['T']):
            if t['ofc'][r, k]:
                sf += int(t['ofc'][r, k]) * y[k]
            if t['obc'][r, k]:
                sb += int(t['obc'][r, k]) * y[k]
        pf = pb = mp.mpf(1)
        for j in range(t['N']):
            pf *= a[j] ** int(t['ofs'][r, j])
            pb *= a[j] ** int(t['obs'][r, j])
        rf.append(mp.exp(sf) * pf)
        rb.append(mp.exp(sb) * pb)
    return rf, rb


def _mp_newton(t, y, a, lf, lb, dead, iters=300):
    T, R = t['T'], t['R']
    live = [s for s in range(T) if s not in dead]
    for _ in range(iters):
        rf, rb = _mp_rates(t, y, a, lf, lb)
        J = mp.zeros(T, T)
        F = mp.zeros(T, 1)
        D = [mp.mpf(0)] * T
        for r in range(R):
            net, gross = rf[r] - rb[r], abs(rf[r]) + abs(rb[r])      # (any positive row scale: a difference at c = 0 has a negative side)
            for s in range(1, T):
                m = int(t['m'][r, s])
                if not m:
                    continue
                F[s] += m * net
                D[s] += abs(m) * gross
                for k in range(T):
                    J[s, k] += m * (rf[r] * int(t['ofc'][r, k]) - rb[r] * int(t['obc'][r, k]))
        for k in range(T):
            J[0, k] = mp.mpf(t['ns'][k]) * mp.exp(y[k])
            F[0] += J[0, k]
        F[0] -= 1
        for s in range(1, T):
            if s in dead:
                for k in range(T):
                    J[s, k] = 1 if k == s else 0
                F[s] = 0
            else:
                for k in range(T):
                    J[s, k] /= D[s]
                F[s] /= D[s]
        dy = mp.lu_solve(J, -F)
        mx = max(abs(dy[k]) for k in live)
        sc = 3 / mx if mx > 3 else 1          # (a full step everywhere but on the far side of a difference at c = 0)
        for k in live:
            y[k] += sc * dy[k]
        if mx < mp.mpf(10) ** (-(DPS - 12)):
            break
    return y


def _mp_solve(t, y0, dead, phiM, c, phi0, w, CS, phi_pzc, sigma, off, gamma, clamp=True):
    a, lf, lb = _mp_state(t, phiM, c, phi0, w, CS, phi_pzc, sigma, off, gamma, clamp)
    y = _mp_newton(t, [mp.mpf(v) for v in y0], a, lf, lb, dead)
    rf, rb = _mp_rates(t, y, a, lf, lb)
    sd = mp.mpf(t['sd'])
    flux = [sd * sum(mp.mpf(t['nu'][r, k]) * (rf[r] - rb[r]) for r in range(t['R'])) for k in range(t['N'])]
    return y, rf, rb, flux


def solve_mp(tab, phiM, csurf, phi_surface, fp64, w=1, CS=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None, sens=True):
    """The points of solve_fp64's result `fp64` at 60 digits.  Returns a dict of mpmath numbers in nested lists: 'y' [n][T], 'rate', 'rate_gross'
    [n][R], 'flux', 'flux_scale' [n][N], and with sens 'dflux_dc' [n][N][N], 'dflux_dphi' [n][N][2]."""
    t = _arrays(tab)
    N, T, R = t['N'], t['T'], t['R']
    phiM = np.atleast_1d(np.asarray(phiM, float))
    n = len(phiM)
    csurf = np.asarray(csurf, float).reshape(n, N)
    res = {k: [] for k in ('y', 'rate', 'rate_gross', 'flux', 'flux_scale', 'dflux_dc', 'dflux_dphi')}
    with mp.workdps(DPS):
        f = mp.mpf
        for i in range(n):
            o = np.zeros((R, 2)) if off is None else np.asarray(off, float)[i].reshape(R, 2)
            g = np.ones(N) if gamma is None else np.asarray(gamma, float)[i]
            sgm = None if sigma is None else float(np.asarray(sigma)[i])
            y0 = fp64['y'][i]
            # a row that nothing produces or consumes keeps y = CATKIN_MIN_LOG
            a, lf, lb = _mp_state(t, phiM[i], csurf[i], phi_surface[i], w, CS, phi_pzc, sgm, o, g, True)
            rf, rb = _mp_rates(t, [f(v) for v in y0], a, lf, lb)
            dead = {s for s in range(1, T) if sum(abs(int(t['m'][r, s])) * (rf[r] + rb[r]) for r in range(R)) == 0}
            args = (w, CS, phi_pzc, sgm, o, g)
            y, rf, rb, flux = _mp_solve(t, y0, dead, f(phiM[i]), [f(v) for v in csurf[i]], f(phi_surface[i]), *args)
            res['y'].append(y)
            res['rate'].append([rf[r] - rb[r] for r in range(R)])
            res['rate_gross'].append([rf[r] + rb[r] for r in range(R)])
            res['flux'].append(flux)
            res['flux_scale'].append([f(t['sd']) * sum(abs(f(t['nu'][r, k])) * (rf[r] + rb[r]) for r in range(R)) for k in range(N)])
            if not sens:
                continue
            dc = [[None] * N for _ in range(N)]
            dphi = [[None] * 2 for _ in range(N)]
            for p in range(N + 2):
                pm, cc, p0 = f(phiM[i]), [f(v) for v in csurf[i]], f(phi_surface[i])
                # at c = 0 the log-coverages admit no negative side: the one-sided second-order formula (-3 f(0) + 4 f(h) - f(2h)) / (2h)
                one_sided = p < N and cc[p] == 0
                fl = []
                for sign in ((1, 2) if one_sided else (1, -1)):
                    qm, qc, q0 = pm, list(cc), p0
                    if p < N:
                        # (one-sided: a step of 1e-30 cref, so that the h^2 term of the formula stays below the 1e-40 of the central one)
                        h = f(10) ** -30 * f(t['cref'][p]) if one_sided else f(10) ** -20 * abs(cc[p])
                        qc[p] = cc[p] + sign * h
                    else:
                        h = f(10) ** -20
                        if p == N:
                            qm = pm + sign * h
                        else:
                            q0 = p0 + sign * h
                    fl.append(_mp_solve(t, y, dead, qm, qc, q0, *args)[3])
                for k in range(N):
                    d = (-3 * flux[k] + 4 * fl[0][k] - fl[1][k]) / (2 * h) if one_sided else (fl[0][k] - fl[1][k]) / (2 * h)
                    if p < N:
                        dc[k][p] = d
                    else:
                        dphi[k][p - N] = d
            res['dflux_dc'].append(dc)
            res['dflux_dphi'].append(dphi)
    return res


def mp_err(x_mp, x, scale=None):
    """max |x - x_mp| (/ scale) per point, the difference formed at 60 digits: x, scale float arrays [n][...]; returns [n]"""
    x = np.asarray(x, float)
    out = np.zeros(len(x))
    with mp.workdps(DPS):
        for i in range(len(x)):
            flat_mp = _flatten(x_mp[i])
            flat = x[i].reshape(-1)
            sc = None if scale is None else np.asarray(scale, float)[i].reshape(-1)
            worst = 0.0
            for k, v in enumerate(flat_mp):
                d = abs(mp.mpf(float(flat[k])) - v)
                if sc is not None:
                    if sc[k] == 0.0:
                        d = mp.mpf(0) if d == 0 else mp.inf
                    else:
                        d = d / mp.mpf(float(sc[k]))
                worst = max(worst, float(d))
            out[i] = worst
    return out


def _flatten(x):
    if isinstance(x, list):
        return [v for row in x for v in _flatten(row)]
    return [x]
