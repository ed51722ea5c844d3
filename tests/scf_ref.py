"""Plain restatement (NumPy and the CPU oracle, no device) of the kinetics <-> transport self-consistency loop pnp_scf_cycle runs on the
device, written from the contract in include/catint_pnp.h (pnp_scf_params, pnp_scf_state) and the lines of the reference's
Calculator.run_scf_cycle / evaluate_accuracy it cites (catint/calculator.py:260-283, :294-406).  One lane at a time; scf_batch calls it
per lane.

Per iteration `it` (= istep + 1, ..., max_iter) of a lane that is still active:
 1. `it - step_to_check > 40`: mix *= 0.9, step_to_check = it                                                  (:319-323)
 2. it > 2: a surface concentration < 0 falls back to the previous iterate, every other one is mixed, mix * sc + (1 - mix) * sc_old
    (:328-338); it <= 2: a negative one becomes 1e-20                                                           (:341-344)
 3. sc_old <- sc                                                                                                 (:362-364)
 4. surface pH from H+, else from OH-, and only from a value > 0                                                 (:346-359)
 5. fluxes of the wall table, flux_k = sum_r (nu_rk K_r) g_r with g = max(c, 0) (1 for species -1) / (1 + K_sat c)
    * exp(alpha (phiM - surface potential of the PREVIOUS solve))                                                (:373, catint_pnp.h)
 6. the transport solve                                                                                          (:385)
 7. current densities flux * nel * F / nprod / 10, left to right                                                 (:398)
 8. err = max_k |cd - cd_old| / cd over cd != 0 -- the SIGNED quotient -- and -inf when there is none             (:271-277)
 9. it > 1: accuracy <- err                                                                                      (:401-402)
10. a non-finite surface value or a transport solve that ended in NaN: failed, and the lane leaves
11. otherwise the lane stays active while accuracy > tau or a surface concentration is negative                  (:316)

The transport is a callable flux [N] -> (surface concentrations [N], surface potential, surface field, status) with status 'ok',
'stuck' (the solve did not converge: it reports -1.0 for every surface concentration, COMSOL's unreachable-flux answer) or 'nan'.
OracleTransport is the warm stationary Newton solve of oracle/pnp_physical.py with the wall reactions as PRESCRIBED fluxes (the loop's
kinetics are explicit) and the per-lane snapshot of the contract: a converged solve becomes the snapshot, a solve that hit maxit puts
the lane back on it, surface potential and field are read after that.
"""
import numpy as np

from oracle import pnp_physical as PH

ROWS = ('surface_concentration', 'surface_concentration_old', 'flux', 'current_density_old')      # [N] per lane
SCALARS = ('mix', 'accuracy', 'surface_pH', 'surface_potential', 'surface_efield')
FLAGS = ('step_to_check', 'active', 'failed')


class OracleTransport(object):
    """problem: a PH.PhysicalProblem WITHOUT wall_kinetics; (c, phi): its converged state at the flux the loop is entered with."""

    def __init__(self, problem, c, phi, tol=1e-10, maxit=12, dphi_max=0.05):
        assert not problem.wall_kinetics
        self.p, self.kw = problem, dict(tol=tol, maxit=maxit, dphi_max=dphi_max)
        self.c, self.phi = np.array(c, float), np.array(phi, float)
        self.snap = (self.c.copy(), self.phi.copy())
        self.iterations = []               # Newton iterations of every solve (maxit + 1: not converged)

    def __call__(self, flux):
        self.p.flux = np.array(flux, float)
        with np.errstate(all='ignore'):
            c, phi, it, _ = PH.newton_step(self.p, self.c, self.phi, self.c, np.inf, **self.kw)
        self.iterations.append(it)
        if not (np.isfinite(c).all() and np.isfinite(phi).all()):
            status = 'nan'
            self.c, self.phi = c, phi
        elif it == self.kw['maxit'] + 1:
            status = 'stuck'
            self.c, self.phi = self.snap[0].copy(), self.snap[1].copy()
        else:
            status = 'ok'
            self.c, self.phi = c, phi
            self.snap = (c.copy(), phi.copy())
        x = self.p.x
        sc = np.full(self.p.N, -1.0) if status == 'stuck' else self.c[:, 0].copy()
        return sc, self.phi[0], -(self.phi[1] - self.phi[0]) / (x[1] - x[0]), status


def wall_fluxes(wall, K, sc, phiM, vsurf):
    """Step 5.  wall: {'species': [n], 'nu': [n][N], 'alpha': [n] or None, 'saturation': [n] or None}; K [n]."""
    n, N = len(wall['species']), len(sc)
    alpha = wall.get('alpha') if wall.get('alpha') is not None else np.zeros(n)
    sat = wall.get('saturation') if wall.get('saturation') is not None else np.zeros(n)
    flux = np.zeros(N)
    with np.errstate(all='ignore'):
        for r in range(n):
            s = wall['species'][r]
            c = 1.0 if s < 0 else (0.0 if sc[s] < 0.0 else sc[s])          # max(c, 0); a NaN stays a NaN
            g = c
            if sat[r] != 0.0:
                g = g * (1.0 / (1.0 + sat[r] * c))
            if alpha[r] != 0.0:
                g = g * np.exp(alpha[r] * (phiM - vsurf))
            for k in range(N):
                if wall['nu'][r][k] != 0.0:
                    flux[k] = flux[k] + (wall['nu'][r][k] * K[r]) * g
    return flux


def scf_lane(state, wall, K, phiM, transport, istep, max_iter, tau, faraday, nel=None, nprod=None, species_H=-1, species_OH=-1):
    """One lane.  state: its entries of the loop arrays (ROWS [N], SCALARS, FLAGS).  Returns (final state, last iteration number at which
    the lane was active (istep if it never was), trace).  trace: per iteration {'iteration', 'sc' (mixed), 'flux', 'sc_out', 'accuracy',
    'stuck', 'status', 'fired': set of 'decay', 'mix', 'fallback', 'clamp', 'pH_H', 'pH_OH', 'pH_kept', 'acc_none', 'acc_negative'}."""
    s = {k: np.array(state[k], float) for k in ROWS}
    s.update({k: float(state[k]) for k in SCALARS})
    s.update({k: int(state[k]) for k in FLAGS})
    N = len(s['surface_concentration'])
    nel = np.ones(N) if nel is None else np.asarray(nel, float)
    nprod = np.ones(N) if nprod is None else np.asarray(nprod, float)
    last, trace = istep, []
    for it in range(istep + 1, max_iter + 1):
        if not s['active']:
            break
        last, fired = it, set()
        if it - s['step_to_check'] > 40:
            s['mix'] = s['mix'] * 0.9
            s['step_to_check'] = it
            fired.add('decay')
        sc, old, mix = s['surface_concentration'], s['surface_concentration_old'], s['mix']
        for k in range(N):
            if it > 2:
                if sc[k] < 0.0:
                    sc[k] = old[k]
                    fired.add('fallback')
                else:
                    sc[k] = mix * sc[k] + (1.0 - mix) * old[k]
                    fired.add('mix')
            elif sc[k] < 0.0:
                sc[k] = 1e-20
                fired.add('clamp')
        old[:] = sc
        if species_H >= 0:
            if sc[species_H] > 0.0:
                s['surface_pH'] = -np.log10(sc[species_H] / 1000.0)
                fired.add('pH_H')
            else:
                fired.add('pH_kept')
        elif species_OH >= 0:
            if sc[species_OH] > 0.0:
                s['surface_pH'] = 14.0 + np.log10(sc[species_OH] / 1000.0)
                fired.add('pH_OH')
            else:
                fired.add('pH_kept')
        mixed = sc.copy()
        s['flux'] = wall_fluxes(wall, K, sc, phiM, s['surface_potential'])
        out, vsurf, esurf, status = transport(s['flux'])
        sc[:] = out
        s['surface_potential'], s['surface_efield'] = float(vsurf), float(esurf)
        err = -np.inf
        with np.errstate(all='ignore'):
            for k in range(N):
                cd = s['flux'][k] * nel[k] * faraday / nprod[k] / 10.0
                if cd != 0.0:
                    q = abs(cd - s['current_density_old'][k]) / cd
                    if q > err:
                        err = q
                s['current_density_old'][k] = cd
        if it > 1:
            s['accuracy'] = err
            if err == -np.inf:
                fired.add('acc_none')
            elif err < 0.0:
                fired.add('acc_negative')
        bad = status == 'nan' or not np.isfinite(sc).all()
        if bad:
            s['failed'] = 1
        s['active'] = int((not bad) and bool(s['accuracy'] > tau or (sc < 0.0).any()))
        trace.append({'iteration': it, 'sc': mixed, 'flux': s['flux'].copy(), 'sc_out': sc.copy(), 'accuracy': s['accuracy'],
                      'stuck': status == 'stuck', 'status': status, 'fired': fired, 'mix': s['mix'], 'surface_pH': s['surface_pH']})
    return s, last, trace


def scf_batch(state, wall, K, phiM, transports, istep, max_iter, tau, faraday, **kw):
    """The batch: state holds [B][...] arrays, K [B][n], phiM [B], transports one callable per lane.  Returns (final arrays, the last
    iteration number that had an active lane, traces per lane)."""
    B = len(phiM)
    lanes = [scf_lane({k: state[k][b] for k in ROWS + SCALARS + FLAGS}, wall, K[b], phiM[b], transports[b], istep, max_iter, tau, faraday, **kw)
             for b in range(B)]
    out = {k: np.array([l[0][k] for l in lanes]) for k in ROWS + SCALARS}
    out.update({k: np.array([l[0][k] for l in lanes], np.int32) for k in FLAGS})
    return out, max([istep] + [l[1] for l in lanes]), [l[2] for l in lanes]
