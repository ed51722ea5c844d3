"""Plain restatement (NumPy and the CPU oracle, no device) of pnp_scf_cycle_fn with the flux function of include/catint_scfkin.h: the loop
of tests/scf_ref.py with the mean-field microkinetic model of tests/kinetics_ref.py where the wall table stood.  One lane at a time.

Per iteration of a lane that is still active, steps 1-4 and 6-11 are those of tests/scf_ref.py (its module docstring); step 5 is
 5. the steady state of the model at the MIXED surface concentrations and the surface potential of the PREVIOUS transport solve
    (kinetics_ref.solve_fp64), started from the coverages the lane's last call found when all of them are finite, else from the uniform
    coverages 1 / sum_t n_t; status 0: flux = flux_last = the model's fluxes; any other status: flux = NaN -- the transport solve then
    ends non-finite and the lane fails -- and flux_last keeps its value.  theta, flux_scale, status and iterations_last are the call's,
    iterations_total and calls count.
"""
import numpy as np

from tests import kinetics_ref as KR
from tests.scf_ref import FLAGS, ROWS, SCALARS, OracleTransport  # noqa: F401  (OracleTransport: part of this module's interface)

KIN_ROWS = ('theta', 'flux_scale', 'flux_last')
KIN_FLAGS = ('status', 'iterations_last', 'iterations_total', 'calls')


class Kinetics(object):
    """The model and what catsk_begin is given besides the per-lane arrays"""

    def __init__(self, tables, potential_drop='stern', stern_capacitance=0.0, phi_pzc=0.0, tol=1e-12, maxit=200):
        self.tables, self.w, self.CS, self.phi_pzc, self.tol, self.maxit = tables, 1 if potential_drop == 'stern' else 0, stern_capacitance, phi_pzc, tol, maxit
        self.N, self.S, self.R = KR.shape(tables)
        self.start = 1.0 / float(np.sum(tables['site_count']))

    def begin(self, theta_guess=None):
        """the per-lane buffers of one lane after catsk_begin"""
        T = self.S + 1
        return {'theta': np.full(T, np.nan) if theta_guess is None else np.array(theta_guess, float), 'flux_scale': np.zeros(self.N),
                'flux_last': np.zeros(self.N), 'status': 0, 'iterations_last': 0, 'iterations_total': 0, 'calls': 0}

    def call(self, k, sc, phiM, vsurf, gamma=None):
        """One call of the flux function for one active lane: updates the lane's buffers k, returns the flux row"""
        guess = k['theta'] if np.isfinite(k['theta']).all() else np.full(self.S + 1, self.start)
        with np.errstate(all='ignore'):
            r = KR.solve_fp64(self.tables, [phiM], np.asarray(sc, float)[None], [vsurf], w=self.w, CS=self.CS, phi_pzc=self.phi_pzc,
                              gamma=None if gamma is None else np.asarray(gamma, float)[None], theta_guess=guess[None], tol=self.tol,
                              maxit=self.maxit, sens=False)
        status = int(r['status'][0])
        k['theta'], k['flux_scale'] = r['theta'][0].copy(), r['flux_scale'][0].copy()
        k['status'], k['iterations_last'] = status, int(r['iterations'][0])
        k['iterations_total'] += int(r['iterations'][0])
        k['calls'] += 1
        if status != 0:
            return np.full(self.N, np.nan)
        k['flux_last'] = r['flux'][0].copy()
        return r['flux'][0].copy()


def scfkin_lane(state, kin, kstate, phiM, transport, istep, max_iter, tau, faraday, gamma=None, nel=None, nprod=None, species_H=-1,
                species_OH=-1):
    """One lane.  state: its entries of the loop arrays (ROWS [N], SCALARS, FLAGS); kin: a Kinetics; kstate: the lane's buffers
    (Kinetics.begin), updated in place.  Returns (final state, last iteration number at which the lane was active (istep if it never
    was), trace).  trace: per iteration {'iteration', 'sc' (mixed), 'flux', 'sc_out', 'accuracy', 'status', 'kinetic_status',
    'kinetic_iterations', 'decay'}."""
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
        last, decay = it, False
        if it - s['step_to_check'] > 40:
            s['mix'] = s['mix'] * 0.9
            s['step_to_check'] = it
            decay = True
        sc, old, mix = s['surface_concentration'], s['surface_concentration_old'], s['mix']
        for k in range(N):
            if it > 2:
                sc[k] = old[k] if sc[k] < 0.0 else mix * sc[k] + (1.0 - mix) * old[k]
            elif sc[k] < 0.0:
                sc[k] = 1e-20
        old[:] = sc
        if species_H >= 0:
            if sc[species_H] > 0.0:
                s['surface_pH'] = -np.log10(sc[species_H] / 1000.0)
        elif species_OH >= 0:
            if sc[species_OH] > 0.0:
                s['surface_pH'] = 14.0 + np.log10(sc[species_OH] / 1000.0)
        mixed = sc.copy()
        s['flux'] = kin.call(kstate, sc, phiM, s['surface_potential'], gamma)
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
        bad = status == 'nan' or not np.isfinite(sc).all()
        if bad:
            s['failed'] = 1
        s['active'] = int((not bad) and bool(s['accuracy'] > tau or (sc < 0.0).any()))
        trace.append({'iteration': it, 'sc': mixed, 'flux': s['flux'].copy(), 'sc_out': sc.copy(), 'accuracy': s['accuracy'], 'status': status,
                      'kinetic_status': kstate['status'], 'kinetic_iterations': kstate['iterations_last'], 'decay': decay})
    return s, last, trace


def scfkin_batch(state, kin, kstates, phiM, transports, istep, max_iter, tau, faraday, gamma=None, **kw):
    """The batch: state holds [B][...] arrays, kstates one dict of buffers per lane, transports one callable per lane, gamma [B][N] or
    None.  Returns (final arrays, the per-lane buffers stacked, the last iteration number that had an active lane, traces per lane)."""
    B = len(phiM)
    lanes = [scfkin_lane({k: state[k][b] for k in ROWS + SCALARS + FLAGS}, kin, kstates[b], phiM[b], transports[b], istep, max_iter, tau, faraday,
                         gamma=None if gamma is None else gamma[b], **kw) for b in range(B)]
    out = {k: np.array([l[0][k] for l in lanes]) for k in ROWS + SCALARS}
    out.update({k: np.array([l[0][k] for l in lanes], np.int32) for k in FLAGS})
    kout = {k: np.array([ks[k] for ks in kstates]) for k in KIN_ROWS}
    kout.update({k: np.array([ks[k] for ks in kstates], np.int32) for k in KIN_FLAGS})
    return out, kout, max([istep] + [l[1] for l in lanes]), [l[2] for l in lanes]
