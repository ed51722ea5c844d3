"""NumPy restatement of include/catint_kintrans.h (test infrastructure, no tests of its own), on top of tests/kinetics_ref.py: implicit
Euler in the log-coverages with step doubling, one operating point after another, operation for operation as the header states them;
the linear systems by np.linalg.solve.  About 0.4 ms per inner Newton iteration: tests/kintrans_cases.py keeps the cases small and
caches every run.

solve_point also returns what tests/test_kintrans_ref.py guards the device comparison with: 'err_margin', the smallest |err - 1| over
the accept / reject decisions, and 'newton_margin', the smallest |max|dy| / newton_tol - 1| over the Newton iterations -- a decision
closer to its threshold than the device's exp and log differ from NumPy's could fall the other way there."""
import numpy as np

from tests import kinetics_ref as KR

MIN_LOG = KR.MIN_LOG
DONE, STEADY, INPUT, STEPS = 0, 1, 2, 3
MIN_STEP = 1e-300
DEFAULTS = dict(rtol=1e-4, atol=1e-12, steady_tol=0.0, h0=0.0, newton_tol=1e-10, newton_maxit=8, max_steps=20000)


class _Point(object):
    """The constants of one operating point and the sums at a y"""

    def __init__(self, t, lf, lb, a):
        self.t, self.lf, self.lb = t, lf, lb
        self.mT, self.amT = t['m'].T.copy(), np.abs(t['m']).T.copy()
        # the activity products do not change along the integration: KR.rates at y = 0 returns them as rf / ef
        with np.errstate(over='ignore', invalid='ignore'):
            self.pf = np.prod(np.power(a[None, :], t['ofs']), axis=1) if t['N'] else np.ones(t['R'])
            self.pb = np.prod(np.power(a[None, :], t['obs']), axis=1) if t['N'] else np.ones(t['R'])

    def rates(self, y):
        with np.errstate(over='ignore', invalid='ignore'):
            return np.exp(self.lf + self.t['ofc'] @ y) * self.pf, np.exp(self.lb + self.t['obc'] @ y) * self.pb

    def rows(self, y, jac=False):
        """G_s, D_s (entry 0 unused) and, with jac, Jraw"""
        rf, rb = self.rates(y)
        with np.errstate(over='ignore', invalid='ignore'):
            G, D = self.mT @ (rf - rb), self.amT @ (rf + rb)
            J = self.mT @ (rf[:, None] * self.t['ofc'] - rb[:, None] * self.t['obc']) if jac else None
        return G, D, J

    def drift(self, y):
        G, D, _ = self.rows(y)
        on = D[1:] > 0.0
        with np.errstate(invalid='ignore', divide='ignore'):
            d = np.abs(G[1:][on]) / D[1:][on]
        if not len(d):
            return 0.0
        return np.nan if np.isnan(d).any() else float(d.max())

    def fluxes(self, y):
        rf, rb = self.rates(y)
        return self.t['sd'] * (self.t['nu'].T @ (rf - rb)), self.t['sd'] * (np.abs(self.t['nu']).T @ (rf + rb))


def implicit_euler(P, y_old, h, newton_tol, newton_maxit, log):
    """BE(y_old, h): (y, converged, iterations applied)"""
    t = P.t
    y = np.array(y_old, float)
    th_old = np.exp(y_old)
    it = 0
    for _ in range(newton_maxit):
        G, D, J = P.rows(y, jac=True)
        with np.errstate(all='ignore'):
            th = np.exp(y)
            w = th + h * D
            A = (np.diag(th) - h * J) / w[:, None]
            F = ((th - th_old) - h * G) / w
            A[0] = t['ns'] * th
            F[0] = A[0].sum() - 1.0
            try:
                dy = np.linalg.solve(A, -F)
            except np.linalg.LinAlgError:
                return y, False, it
        if not np.isfinite(dy).all():
            return y, False, it
        mx = np.abs(dy).max()
        sc = 3.0 / mx if mx > 3.0 else 1.0
        y = np.maximum(y + sc * dy, MIN_LOG)
        it += 1
        log['newton_margin'] = min(log['newton_margin'], abs(mx / newton_tol - 1.0))
        if mx < newton_tol:
            return y, True, it
    return y, False, it


def solve_point(t, phiM, c, phi0, t_out, w=1, CS=0.0, phi_pzc=0.0, sigma=None, off=None, gamma=None, theta0=None, rtol=1e-4, atol=1e-12,
                steady_tol=0.0, h0=0.0, newton_tol=1e-10, newton_maxit=8, max_steps=20000, lnk_shift=0):
    """One operating point.  t: KR._arrays(tables).  lnk_shift: every ln kf and ln kb moved by that many ulp (the measure of what ulps in
    exp and log do to the result).  Returns the rows of catkt_outputs and 'y' [n_out][T], 'err_margin', 'newton_margin', 'h_first'."""
    N, T, R = t['N'], t['T'], t['R']
    t_out = np.atleast_1d(np.asarray(t_out, float))
    K = len(t_out)
    off = np.zeros((R, 2)) if off is None else np.asarray(off, float).reshape(R, 2)
    gamma = np.ones(N) if gamma is None else np.asarray(gamma, float)
    c = np.asarray(c, float).reshape(N)
    V, sg = KR.potential_and_charge(phiM, phi0, w, CS, phi_pzc, sigma)
    out = dict(theta=np.full((K, T), np.nan), y=np.full((K, T), np.nan), flux=np.full((K, N), np.nan), flux_scale=np.full((K, N), np.nan),
               drift=np.full(K, np.nan), t_reached=np.nan, status=INPUT, steps=np.zeros(3, np.int32), err_margin=np.inf, newton_margin=np.inf,
               h_first=np.nan)
    fin = np.isfinite([phiM, phi0, sg]).all() and np.isfinite(c).all() and np.isfinite(gamma).all() and np.isfinite(off).all()
    if theta0 is not None:
        fin = fin and np.isfinite(np.asarray(theta0, float)[1:]).all()
    if not fin:
        return out
    a = gamma * np.maximum(c, 0.0) / t['cref']
    lf, lb, _ = KR.rate_constants(t, V, sg, off)
    if lnk_shift:
        lf, lb = lf + lnk_shift * np.spacing(lf), lb + lnk_shift * np.spacing(lb)
    y = np.array(KR.start(t, theta0), float)
    if theta0 is not None:
        free = 1.0 - (t['ns'][1:] * np.exp(y[1:])).sum()
        if not free > 0.0:
            return out
        y[0] = max(np.log(free), MIN_LOG)
    P = _Point(t, lf, lb, a)
    G, D, _ = P.rows(y)
    on = D[1:] > 0.0
    fastest = float((D[1:][on] / np.exp(y[1:][on])).max()) if on.any() else 0.0
    h = h0 if h0 > 0.0 else (0.01 / fastest if fastest > 0.0 else t_out[0])
    out['h_first'] = h
    log = out
    tn, k, acc, rej, its, last_drift = 0.0, 0, 0, 0, 0, np.nan
    status = None
    while status is None:
        if acc + rej >= max_steps or not h >= MIN_STEP:
            status = STEPS
            break
        rem = t_out[k] - tn
        lands, shortened = rem <= h, rem < h
        hh = rem if shortened else h
        half = 0.5 * hh
        y1, ok, n1 = implicit_euler(P, y, hh, newton_tol, newton_maxit, log)
        its += n1
        if ok:
            ya, ok, n2 = implicit_euler(P, y, half, newton_tol, newton_maxit, log)
            its += n2
        if ok:
            yb, ok, n3 = implicit_euler(P, ya, half, newton_tol, newton_maxit, log)
            its += n3
        if not ok:
            rej += 1
            h = 0.25 * hh
            continue
        with np.errstate(all='ignore'):
            thb, th1 = np.exp(yb), np.exp(y1)
            d = np.abs(thb - th1) / (atol + rtol * np.maximum(thb, th1))
            err = np.nan if np.isnan(d).any() else float(d.max())
            f = 0.9 / np.sqrt(err) if err != 0.0 else np.inf
        fac = 5.0 if f > 5.0 else (f if f >= 0.2 else 0.2)
        if not np.isnan(err):
            log['err_margin'] = min(log['err_margin'], abs(err - 1.0))
        if not err <= 1.0:
            rej += 1
            h = fac * hh
            continue
        acc += 1
        y = yb
        tn = t_out[k] if lands else tn + hh
        hn = fac * hh
        h = h if shortened and h > hn else hn
        last_drift = P.drift(y)
        if steady_tol > 0.0 and last_drift < steady_tol:
            status = STEADY
            break
        if lands:
            out['y'][k], out['theta'][k], out['drift'][k] = y, np.exp(y), last_drift
            out['flux'][k], out['flux_scale'][k] = P.fluxes(y)
            k += 1
            if k == K:
                status = DONE
    if status == STEADY:
        out['y'][k:], out['theta'][k:], out['drift'][k:] = y, np.exp(y), last_drift
        out['flux'][k:], out['flux_scale'][k:] = P.fluxes(y)
    out['status'], out['t_reached'], out['steps'] = status, tn, np.array([acc, rej, its], np.int32)
    return out


def solve(tab, phiM, csurf, phi_surface, t_out, sigma=None, off=None, gamma=None, theta0=None, **kw):
    """Every operating point of the call; returns a dict of stacked arrays (the names of catkt_outputs, and 'y', the two margins)"""
    t = KR._arrays(tab)
    phiM = np.atleast_1d(np.asarray(phiM, float))
    n = len(phiM)
    csurf = np.asarray(csurf, float).reshape(n, t['N'])
    outs = [solve_point(t, phiM[i], csurf[i], np.asarray(phi_surface, float)[i], t_out, sigma=KR._per_point(sigma, i), off=KR._per_point(off, i),
                        gamma=KR._per_point(gamma, i), theta0=KR._per_point(theta0, i), **kw) for i in range(n)]
    res = {k: np.array([o[k] for o in outs]) for k in outs[0]} if outs else {}
    if outs:
        res['status'] = res['status'].astype(np.int32)
        res['steps'] = res['steps'].astype(np.int32)
    return res
