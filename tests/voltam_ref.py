"""NumPy restatement of include/catint_voltam.h (test infrastructure, no tests of its own), on top of tests/kinetics_ref.py and with
the method of tests/kintrans_ref.py: implicit Euler in the log-coverages along the potential program, step doubling with the turnover
in the error norm, the extrapolated state accepted; one operating point after another, operation for operation as the header states
them, the linear systems by np.linalg.solve.  About 0.4 ms per inner Newton iteration: tests/voltam_cases.py keeps the cases small
and caches every run.

solve_point also returns what tests/test_voltam_ref.py guards the device comparison with, each the smallest relative distance of a
decision from its threshold: 'err_margin' (|err - 1| over the accept / reject decisions), 'newton_margin' (|max|dy| / newton_tol - 1|
over the Newton iterations), 'extrap_margin' (|theta_e,t| / max(theta_b,t, theta_1,t) over the accepted steps), 'land_margin'
(|rem / h - 1| over the attempted steps, exact ties aside: they are decided by the same arithmetic everywhere) and 'branch_margin'
(the distance of Ea - dG, Ea and dG from 0 over the sum of the absolute terms of the two polynomials, at the potential of every
solve).  It also returns 'theta_start' [T], 'dq' [n_out] (the cumulative sum of the accepted dq, in 1/site) and the counters."""
import numpy as np

from tests import kinetics_ref as KR
from tests import kintrans_ref as KT

MIN_LOG = KR.MIN_LOG
DONE, INPUT, STEPS = 0, 2, 3
MIN_STEP = 1e-300
START_MAXIT = 100
FARADAY = 96485.33289
DEFAULTS = dict(rtol=1e-4, atol=1e-12, h0=0.0, newton_tol=1e-10, newton_maxit=8, max_steps=20000)


def program(E_start, E_vertex, scan_rate):
    return abs(E_vertex - E_start) / scan_rate


def potential_at(Es, Ev, tau, k, t):
    Ea, Ez = (Ev, Es) if k & 1 else (Es, Ev)
    return Ea + (Ez - Ea) * ((t - float(k) * tau) / tau)


def output_time(tau, K, j):
    k = j // K
    m = j - k * K + 1
    return (float(k) + float(m) / float(K)) * tau


def branch_margin(t, V, sg):
    """the smallest distance of a Ga decision from its threshold at (V, sigma), relative to the sum of the absolute terms"""
    s2 = sg * sg
    worst = np.inf
    for r in range(t['R']):
        g, e = t['dG'][r], t['Ea'][r]
        tg = np.array([g[0], g[1] * V, g[2] * sg, g[3] * s2])
        dG = ((tg[0] + tg[1]) + tg[2]) + tg[3]
        scale = np.abs(tg).sum()
        if np.isfinite(e[0]):
            te = np.array([e[0], e[1] * V, e[2] * sg, e[3] * s2])
            Ea = ((te[0] + te[1]) + te[2]) + te[3]
            scale = scale + np.abs(te).sum()
            if Ea >= dG and Ea >= 0.0:
                cand = (Ea - dG, Ea)
            elif Ea >= 0.0:
                cand = (dG - Ea, abs(dG))
            else:
                cand = (-Ea, abs(dG))
        else:
            cand = (abs(dG),)
        if scale > 0.0:
            worst = min(worst, min(cand) / scale)
    return worst


class _Point(KT._Point):
    """The constants of one operating point; the rate constants are set per solve"""

    def __init__(self, t, a, ne, off, w, phi0, CS, phi_pzc, sigma, lnk_shift, log):
        KT._Point.__init__(self, t, None, None, a)
        self.ne, self.ane, self.off, self.w, self.phi0, self.CS, self.pzc, self.sigma = ne, np.abs(ne), off, w, phi0, CS, phi_pzc, sigma
        self.shift, self.log = lnk_shift, log

    def at(self, E):
        """the rate constants at the electrode potential E"""
        V, sg = KR.potential_and_charge(E, self.phi0, self.w, self.CS, self.pzc, self.sigma)
        lf, lb, _ = KR.rate_constants(self.t, V, sg, self.off)
        if self.shift:
            lf, lb = lf + self.shift * np.spacing(lf), lb + self.shift * np.spacing(lb)
        self.lf, self.lb = lf, lb
        self.log['branch_margin'] = min(self.log['branch_margin'], branch_margin(self.t, V, sg))

    def turnover(self, y):
        rf, rb = self.rates(y)
        ti = tg = 0.0
        with np.errstate(over='ignore', invalid='ignore'):
            for r in range(len(rf)):
                ti = ti + self.ne[r] * (rf[r] - rb[r])
                tg = tg + self.ane[r] * (rf[r] + rb[r])
        return float(ti), float(tg)


def solve_point(t, electrons, E_start, E_vertex, scan_rate, c, phi0, n_segments=2, samples=8, rate_floor=0.0, w=1, CS=0.0, phi_pzc=0.0, sigma=None,
                off=None, gamma=None, theta0=None, rtol=1e-4, atol=1e-12, h0=0.0, newton_tol=1e-10, newton_maxit=8, max_steps=20000, lnk_shift=0,
                extrapolate=True, current_norm=True):
    """One operating point.  t: KR._arrays(tables).  lnk_shift: every ln kf and ln kb moved by that many ulp.  extrapolate=False,
    current_norm=False: the step rule of include/catint_kintrans.h, for the comparison DESIGN.md quotes (not a mode of the library).
    Returns the rows of catvm_outputs and what the module docstring lists."""
    N, T, R, K = t['N'], t['T'], t['R'], int(samples)
    n_out = int(n_segments) * K
    ne = np.asarray(electrons, float).reshape(R)
    off = np.zeros((R, 2)) if off is None else np.asarray(off, float).reshape(R, 2)
    gamma = np.ones(N) if gamma is None else np.asarray(gamma, float)
    c = np.asarray(c, float).reshape(N)
    nan1 = np.full(n_out, np.nan)
    out = dict(theta=np.full((n_out, T), np.nan), y=np.full((n_out, T), np.nan), flux=np.full((n_out, N), np.nan),
               flux_scale=np.full((n_out, N), np.nan), current=nan1.copy(), current_scale=nan1.copy(), charge=nan1.copy(), E_out=nan1.copy(),
               dq=nan1.copy(), t_reached=np.nan, status=INPUT, steps=np.zeros(4, np.int32), theta_start=np.full(T, np.nan), err_margin=np.inf,
               newton_margin=np.inf, extrap_margin=np.inf, land_margin=np.inf, branch_margin=np.inf, h_first=np.nan)
    with np.errstate(all='ignore'):
        V0, sg0 = KR.potential_and_charge(E_start, phi0, w, CS, phi_pzc, sigma)
        tau = program(E_start, E_vertex, scan_rate)
    fin = np.isfinite([E_start, phi0, sg0, E_vertex]).all() and np.isfinite(c).all() and np.isfinite(gamma).all() and np.isfinite(off).all()
    fin = fin and tau > 0.0 and np.isfinite(float(n_segments) * tau)
    if theta0 is not None:
        fin = fin and np.isfinite(np.asarray(theta0, float)[1:]).all()
    if not fin:
        return out
    a = gamma * np.maximum(c, 0.0) / t['cref']
    if theta0 is not None:
        y = np.array(KR.start(t, theta0), float)
        free = 1.0 - (t['ns'][1:] * np.exp(y[1:])).sum()
        if not free > 0.0:
            return out
        y[0] = max(np.log(free), MIN_LOG)
    else:
        s = KR.solve_point(t, E_start, c, phi0, w, CS, phi_pzc, sigma, off, gamma, None, newton_tol, START_MAXIT, sens=False)
        if s['status'] != 0:
            return out
        y = np.array(s['y'], float)
    out['theta_start'] = np.exp(y)
    log = out
    P = _Point(t, a, ne, off, w, phi0, CS, phi_pzc, sigma, lnk_shift, log)
    P.at(E_start)
    G, D, _ = P.rows(y)
    on = D[1:] > 0.0
    fastest = float((D[1:][on] / np.exp(y[1:][on])).max()) if on.any() else 0.0
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
        y1, ok, n1 = KT.implicit_euler(P, y, hh, newton_tol, newton_maxit, log)
        its += n1
        if ok:
            i1, g1 = P.turnover(y1)
            P.at(E_mid)
            ya, ok, n2 = KT.implicit_euler(P, y, half, newton_tol, newton_maxit, log)
            its += n2
        if ok:
            ia, _ = P.turnover(ya)
            P.at(E_end)
            yb, ok, n3 = KT.implicit_euler(P, ya, half, newton_tol, newton_maxit, log)
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
            if current_norm:
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
        # the extrapolated coverages, the free site from the balance (summed from the last adsorbate down)
        the = 2.0 * thb - th1
        used = 0.0
        for s_ in range(T - 1, 0, -1):
            used = used + t['ns'][s_] * the[s_]
        the[0] = 1.0 - used
        positive = bool((the > 0.0).all()) and extrapolate
        if extrapolate:
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
            # (the rate constants of P are those of E_end)
            io, go = P.turnover(y)
            out['y'][k], out['theta'][k] = y, np.exp(y)
            out['flux'][k], out['flux_scale'][k] = P.fluxes(y)
            out['current'][k], out['current_scale'][k], out['charge'][k], out['E_out'][k], out['dq'][k] = -(Fsd * io), Fsd * go, -(Fsd * q), E_end, q
            k += 1
            if k == n_out:
                status = DONE
    out['status'], out['t_reached'], out['steps'] = status, tn, np.array([acc, rej, its, plain], np.int32)
    return out


def solve(tab, electrons, E_start, E_vertex, scan_rate, csurf, phi_surface, sigma=None, off=None, gamma=None, theta0=None, **kw):
    """Every operating point of the call; returns a dict of stacked arrays (the names of catvm_outputs, and what solve_point adds)"""
    t = KR._arrays(tab)
    E_start = np.atleast_1d(np.asarray(E_start, float))
    n = len(E_start)
    csurf = np.asarray(csurf, float).reshape(n, t['N'])
    outs = [solve_point(t, electrons, E_start[i], np.asarray(E_vertex, float)[i], np.asarray(scan_rate, float)[i], csurf[i],
                        np.asarray(phi_surface, float)[i], sigma=KR._per_point(sigma, i), off=KR._per_point(off, i), gamma=KR._per_point(gamma, i),
                        theta0=KR._per_point(theta0, i), **kw) for i in range(n)]
    res = {k: np.array([o[k] for o in outs]) for k in outs[0]} if outs else {}
    if outs:
        res['status'] = res['status'].astype(np.int32)
        res['steps'] = res['steps'].astype(np.int32)
    return res


def mean_current(charge, tau, samples):
    """charge [n][n_out] differenced over the output times: [n][n_out] in A/m^2 (the first interval starts at charge 0, t = 0)"""
    charge = np.asarray(charge, float)
    dt = (np.asarray(tau, float) / samples)[:, None]
    return np.diff(np.concatenate([np.zeros((len(charge), 1)), charge], axis=1), axis=1) / dt
