"""NumPy restatement of include/catint_iasweep.h (test infrastructure, no tests of its own): the model of tests/interact_ref.py
(_arrays, surface_state, step_constants, effective_orders, rates) under the step loop of tests/voltam_ref.py -- implicit Euler in the
log-coverages along the potential program or at a held potential, step doubling with the turnover in the error norm, the extrapolated
state accepted; one operating point after another, operation for operation as the header states them, the linear systems by
np.linalg.solve.  With G = 1 and strength 0 every expression is voltam_ref's, so the two return the same bits
(tests/test_iasweep_ref.py).  tests/iasweep_cases.py keeps the cases small and caches every run.

solve_point returns the rows of catis_outputs and the decision margins of voltam_ref.solve_point ('err_margin', 'newton_margin',
'extrap_margin', 'land_margin'); 'branch_margin' is here the distance of Ea - dG, Ea and dG from 0 WITH the coverage-dependent terms,
over the sum of the absolute terms, at every rate evaluation.  It also returns 'theta_start' [T], 'dq' [n_out] and the counters."""
import numpy as np

from tests import interact_ref as IR
from tests import kinetics_ref as KR
from tests import voltam_ref as VR

MIN_LOG = KR.MIN_LOG
DONE, INPUT, STEPS = VR.DONE, VR.INPUT, VR.STEPS
MIN_STEP = VR.MIN_STEP
START_MAXIT = VR.START_MAXIT
FARADAY = VR.FARADAY
DEFAULTS = VR.DEFAULTS
potential_at, output_time = VR.potential_at, VR.output_time


class _Point(object):
    """The constants of one operating point; the potential is set per solve, the rate constants follow the coverages"""

    def __init__(self, t, a, ne, off, w, phi0, CS, phi_pzc, sigma, lam, lnk_shift, log):
        self.t, self.a, self.ne, self.ane, self.off, self.lam = t, a, ne, np.abs(ne), off, lam
        self.w, self.phi0, self.CS, self.pzc, self.sigma, self.shift, self.log = w, phi0, CS, phi_pzc, sigma, lnk_shift, log
        self.mT, self.amT = t['m'].T.copy(), np.abs(t['m']).T.copy()
        with np.errstate(over='ignore', invalid='ignore'):
            self.pf = np.prod(np.power(a[None, :], t['ofs']), axis=1) if t['N'] else np.ones(t['R'])
            self.pb = np.prod(np.power(a[None, :], t['obs']), axis=1) if t['N'] else np.ones(t['R'])
        self.V = self.sg = None

    def at(self, E):
        self.V, self.sg = KR.potential_and_charge(E, self.phi0, self.w, self.CS, self.pzc, self.sigma)

    def _margin(self, wv):
        t, V, sg, lam = self.t, self.V, self.sg, self.lam
        ts = t['ts']
        base = np.array([1.0, V, sg, sg * sg])
        with np.errstate(all='ignore'):
            tg = np.concatenate([t['dG'] * base, lam * t['eg'] * wv[None, :]], axis=1)
            te = np.where(ts[:, None], np.concatenate([np.where(ts[:, None], t['Ea'], 0.0) * base, lam * t['ea'] * wv[None, :]], axis=1), 0.0)
            dG, Ea = tg.sum(axis=1), te.sum(axis=1)
            scale = np.abs(tg).sum(axis=1) + np.abs(te).sum(axis=1)
            top = (Ea >= dG) & (Ea >= 0.0)
            with_ts = np.where(top, np.minimum(Ea - dG, Ea), np.where(Ea >= 0.0, np.minimum(dG - Ea, np.abs(dG)), np.minimum(-Ea, np.abs(dG))))
            cand = np.where(ts, with_ts, np.abs(dG))
            m = np.where(scale > 0.0, cand / np.where(scale > 0.0, scale, 1.0), np.inf)
        return float(m.min())

    def state(self, y):
        """what a rate evaluation at y needs: theta, w, f, f', ln kf, ln kb, the rows of the branch, qg, qs, rf, rb"""
        t = self.t
        th, wv, f, fp = IR.surface_state(t, y)
        lf, lb, br, es, qg, qs = IR.step_constants(t, self.V, self.sg, self.off, self.lam, th, wv)
        if self.shift:
            lf, lb = lf + self.shift * np.spacing(lf), lb + self.shift * np.spacing(lb)
        self.log['branch_margin'] = min(self.log['branch_margin'], self._margin(wv))
        with np.errstate(over='ignore', invalid='ignore'):
            rf, rb = np.exp(lf + t['ofc'] @ y) * self.pf, np.exp(lb + t['obc'] @ y) * self.pb
        return th, wv, f, fp, es, qg, qs, rf, rb

    def rates(self, y):
        return self.state(y)[-2:]

    def rows(self, y, jac=False):
        """G_s, D_s (the free-site entries unused) and, with jac, dG_s/dy_v"""
        t = self.t
        th, wv, f, fp, es, qg, qs, rf, rb = self.state(y)
        with np.errstate(over='ignore', invalid='ignore'):
            G, D = self.mT @ (rf - rb), self.amT @ (rf + rb)
            J = None
            if jac:
                ofe, obe = IR.effective_orders(t, self.lam, th, f, fp, es, qg, qs)
                J = self.mT @ (rf[:, None] * ofe - rb[:, None] * obe)
        return G, D, J

    def turnover(self, y):
        rf, rb = self.rates(y)
        ti = tg = 0.0
        with np.errstate(over='ignore', invalid='ignore'):
            for r in range(len(rf)):
                ti = ti + self.ne[r] * (rf[r] - rb[r])
                tg = tg + self.ane[r] * (rf[r] + rb[r])
        return float(ti), float(tg)

    def fluxes(self, y):
        rf, rb = self.rates(y)
        return self.t['sd'] * (self.t['nu'].T @ (rf - rb)), self.t['sd'] * (np.abs(self.t['nu']).T @ (rf + rb))

    def energy_shift(self, y):
        t = self.t
        wv = IR.surface_state(t, y)[1]
        shift = np.zeros(t['S'])
        for u in range(t['S']):
            shift = shift + t['eps'][:, u] * wv[u]
        return self.lam * shift


def be_system(P, y, th_old, h):
    """the scaled Jacobian and residual of BE(y_old, h, E) at y, the rate constants at P's potential"""
    t = P.t
    G_, D, J = P.rows(y, jac=True)
    with np.errstate(all='ignore'):
        th = np.exp(y)
        w = th + h * D
        A = (np.diag(th) - h * J) / w[:, None]
        F = ((th - th_old) - h * G_) / w
        nth = t['ns'] * th
        for g in range(t['G']):
            on = t['site_of'] == g
            A[g] = np.where(on, nth / t['x'][g], 0.0)
            F[g] = np.where(on, nth, 0.0).sum() / t['x'][g] - 1.0
    return A, F


def implicit_euler(P, y_old, h, newton_tol, newton_maxit, log):
    """BE(y_old, h): (y, converged, iterations applied)"""
    y = np.array(y_old, float)
    th_old = np.exp(y_old)
    it = 0
    for _ in range(newton_maxit):
        A, F = be_system(P, y, th_old, h)
        with np.errstate(all='ignore'):
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


def steady_start(P, y, strength, ramp, tol, maxit):
    """the ramped steady solve of include/catint_interact.h at P's potential from y, with the sums of P.rows; (y, status)"""
    t = P.t
    G, T = t['G'], t['T']
    keep, status = (P.lam, P.log, P.mT, P.amT), 1
    P.log = dict(branch_margin=np.inf)          # the start's decisions are the steady library's
    P.mT, P.amT = t['m'].T, np.abs(t['m']).T    # the operands of kinetics_ref.system: the same products with the same bits
    for lam in IR.stage_strengths(strength, ramp):
        P.lam, status = lam, 1
        for _ in range(maxit):
            B, D, J = P.rows(y, jac=True)
            with np.errstate(all='ignore'):
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
                try:
                    dy = np.linalg.solve(J, -F)
                except np.linalg.LinAlgError:
                    status = 3
                    break
            mx = np.abs(dy).max() if np.isfinite(dy).all() else np.nan
            sc = 3.0 / mx if mx > 3.0 else 1.0
            y = np.maximum(y + sc * dy, MIN_LOG) if np.isfinite(mx) else y + dy
            if mx < tol:
                status = 0
                break
        if status != 0:
            break
    P.lam, P.log, P.mT, P.amT = keep
    return y, status


def free_sites(t, th):
    """x_g minus what the adsorbates of type g hold, summed from the last adsorbate down"""
    used = np.zeros(t['G'])
    for s in range(t['T'] - 1, t['G'] - 1, -1):
        used[t['site_of'][s]] = used[t['site_of'][s]] + t['ns'][s] * th[s]
    return t['x'] - used


def solve_point(t, electrons, E_start, E_vertex, scan_rate, c, phi0, n_segments=2, samples=8, rate_floor=0.0, w=1, CS=0.0, phi_pzc=0.0, sigma=None,
                off=None, gamma=None, theta0=None, rtol=1e-4, atol=1e-12, h0=0.0, newton_tol=1e-10, newton_maxit=8, max_steps=20000, lnk_shift=0,
                hold_time=None, start_ramp=1, strength=None):
    """One operating point.  t: IR._arrays(tables).  lnk_shift: every ln kf and ln kb of the step loop moved by that many ulp."""
    N, T, R, G, S, K = t['N'], t['T'], t['R'], t['G'], t['S'], int(samples)
    lam = t['strength'] if strength is None else float(strength)
    n_out = int(n_segments) * K
    ne = np.asarray(electrons, float).reshape(R)
    off = np.zeros((R, 2)) if off is None else np.asarray(off, float).reshape(R, 2)
    gamma = np.ones(N) if gamma is None else np.asarray(gamma, float)
    c = np.asarray(c, float).reshape(N)
    nan1 = np.full(n_out, np.nan)
    out = dict(theta=np.full((n_out, T), np.nan), y=np.full((n_out, T), np.nan), flux=np.full((n_out, N), np.nan),
               flux_scale=np.full((n_out, N), np.nan), energy_shift=np.full((n_out, S), np.nan), current=nan1.copy(), current_scale=nan1.copy(),
               charge=nan1.copy(), E_out=nan1.copy(), dq=nan1.copy(), t_reached=np.nan, status=INPUT, steps=np.zeros(4, np.int32),
               theta_start=np.full(T, np.nan), err_margin=np.inf, newton_margin=np.inf, extrap_margin=np.inf, land_margin=np.inf,
               branch_margin=np.inf, h_first=np.nan)
    with np.errstate(all='ignore'):
        V0, sg0 = KR.potential_and_charge(E_start, phi0, w, CS, phi_pzc, sigma)
        holds = bool(E_vertex == E_start and hold_time is not None and hold_time > 0.0 and np.isfinite(hold_time))
        tau = float(hold_time) if holds else VR.program(E_start, E_vertex, scan_rate)
    fin = np.isfinite([E_start, phi0, sg0, E_vertex]).all() and np.isfinite(c).all() and np.isfinite(gamma).all() and np.isfinite(off).all()
    fin = fin and tau > 0.0 and np.isfinite(float(n_segments) * tau)
    if theta0 is not None:
        fin = fin and np.isfinite(np.asarray(theta0, float)[G:]).all()
    if not fin:
        return out
    a = gamma * np.maximum(c, 0.0) / t['cref']
    log = out
    P = _Point(t, a, ne, off, w, phi0, CS, phi_pzc, sigma, lam, lnk_shift, log)
    P.at(E_start)
    if theta0 is not None:
        y = np.array(IR.start(t, theta0), float)
        used = np.zeros(G)
        for s in range(G, T):
            used[t['site_of'][s]] = used[t['site_of'][s]] + t['ns'][s] * np.exp(y[s])
        free = t['x'] - used
        if not (free > 0.0).all():
            return out
        y[:G] = np.maximum(np.log(free), MIN_LOG)
    else:
        P.shift = 0                              # the start is the steady library's: its constants are not moved
        y, s0 = steady_start(P, np.array(IR.start(t, None), float), lam, int(start_ramp), newton_tol, START_MAXIT)
        P.shift = lnk_shift
        if s0 != 0:
            return out
    out['theta_start'] = np.exp(y)
    G_, D, _ = P.rows(y)
    on = D[G:] > 0.0
    fastest = float((D[G:][on] / np.exp(y[G:][on])).max()) if on.any() else 0.0
    h = h0 if h0 > 0.0 else (0.01 / fastest if fastest > 0.0 else output_time(tau, K, 0))
    out['h_first'] = h
    i_floor = rate_floor * scan_rate
    Fsd = FARADAY * t['sd']
    tn, k, acc, rej, its, plain, q = 0.0, 0, 0, 0, 0, 0, 0.0
    status = None
    while status is None:
        if acc + rej >= max_steps or not h >= MIN_STEP:
            status = STEPS
            break
        seg = k // K
        t_next = output_time(tau, K, k)
        rem = t_next - tn
        lands, shortened = rem <= h, rem < h
        if rem != h:
            log['land_margin'] = min(log['land_margin'], abs(rem / h - 1.0))
        hh = rem if shortened else h
        half = 0.5 * hh
        E_end = potential_at(E_start, E_vertex, tau, seg, t_next if lands else tn + hh)
        E_mid = potential_at(E_start, E_vertex, tau, seg, tn + half)
        P.at(E_end)
        y1, ok, n1 = implicit_euler(P, y, hh, newton_tol, newton_maxit, log)
        its += n1
        if ok:
            i1, g1 = P.turnover(y1)
            P.at(E_mid)
            ya, ok, n2 = implicit_euler(P, y, half, newton_tol, newton_maxit, log)
            its += n2
        if ok:
            ia, _ = P.turnover(ya)
            P.at(E_end)
            yb, ok, n3 = implicit_euler(P, ya, half, newton_tol, newton_maxit, log)
            its += n3
        if not ok:
            rej += 1
            h = 0.25 * hh
            continue
        ib, gb = P.turnover(yb)
        with np.errstate(all='ignore'):
            thb, th1 = np.exp(yb), np.exp(y1)
            d = np.abs(thb - th1) / (atol + rtol * np.maximum(thb, th1))
            err = np.nan if np.isnan(d).any() else float(d.max())
            den = rtol * (max(abs(ib), abs(i1)) + i_floor) + newton_tol * max(gb, g1)
            di = 0.0 if ib == i1 else abs(ib - i1) / den
            err = di if (di > err or di != di) else err
            f = 0.9 / np.sqrt(err) if err != 0.0 else np.inf
        fac = 5.0 if f > 5.0 else (f if f >= 0.2 else 0.2)
        if not np.isnan(err):
            log['err_margin'] = min(log['err_margin'], abs(err - 1.0))
        if not err <= 1.0:
            rej += 1
            h = fac * hh
            continue
        the = 2.0 * thb - th1
        the[:G] = free_sites(t, the)
        positive = bool((the > 0.0).all())
        log['extrap_margin'] = min(log['extrap_margin'], float((np.abs(the) / np.maximum(thb, th1)).min()))
        acc += 1
        if positive:
            y = np.maximum(np.log(the), MIN_LOG)
        else:
            y = yb
            plain += 1
        dq1, dqb = hh * i1, half * (ia + ib)
        q = q + ((2.0 * dqb - dq1) if positive else dqb)
        tn = t_next if lands else tn + hh
        hn = fac * hh
        h = h if shortened and h > hn else hn
        if lands:
            # (the potential of P is E_end)
            io, go = P.turnover(y)
            out['y'][k], out['theta'][k] = y, np.exp(y)
            out['flux'][k], out['flux_scale'][k] = P.fluxes(y)
            out['energy_shift'][k] = P.energy_shift(y)
            out['current'][k], out['current_scale'][k], out['charge'][k], out['E_out'][k], out['dq'][k] = -(Fsd * io), Fsd * go, -(Fsd * q), E_end, q
            k += 1
            if k == n_out:
                status = DONE
    out['status'], out['t_reached'], out['steps'] = status, tn, np.array([acc, rej, its, plain], np.int32)
    return out


def solve(tab, electrons, E_start, E_vertex, scan_rate, csurf, phi_surface, sigma=None, off=None, gamma=None, theta0=None, hold_time=None, **kw):
    """Every operating point of the call; returns a dict of stacked arrays (the names of catis_outputs, and what solve_point adds)"""
    t = IR._arrays(tab)
    E_start = np.atleast_1d(np.asarray(E_start, float))
    n = len(E_start)
    csurf = np.asarray(csurf, float).reshape(n, t['N'])
    pp = KR._per_point
    outs = [solve_point(t, electrons, E_start[i], np.asarray(E_vertex, float)[i], np.asarray(scan_rate, float)[i], csurf[i],
                        np.asarray(phi_surface, float)[i], sigma=pp(sigma, i), off=pp(off, i), gamma=pp(gamma, i), theta0=pp(theta0, i),
                        hold_time=pp(hold_time, i), **kw) for i in range(n)]
    res = {k: np.array([o[k] for o in outs]) for k in outs[0]} if outs else {}
    if outs:
        res['status'] = res['status'].astype(np.int32)
        res['steps'] = res['steps'].astype(np.int32)
    return res


def mean_field_tables(tab):
    """the tables of a mean-field model with the keys of one site type without interactions"""
    T = len(tab['site_count'])
    return dict(tab, site_of=np.zeros(T, np.int32), site_fraction=np.ones(1), eps=np.zeros((T - 1, T - 1)), eps_ts=None, response='linear',
                strength=0.0)
