"""The cases of tests/test_eis_ref.py and tests/test_gpu_eis.py (test infrastructure, no tests of its own): the Langmuir adsorption step
with its known answer, and a three-step mechanism for any number of solution species that the electrolyte cases of
tests/response_cases.py can carry at their wall.  The energies are illustrative numbers chosen for this file."""
import numpy as np

from tests import kinetics_ref as KR

FB = 96485.33289 / (8.3144598 * 298.14)      # F beta, 1/V


def langmuir_tables(lnA=3.0, a0=-0.4, a1=0.5 * FB, site_density=2e-5, cref=40.0):
    """A + * <-> A*, N = 1, S = 1, no transition state: kf = exp(lnA - max(dG, 0)), kb = exp(lnA - max(dG, 0) + dG), dG = a0 + a1 V"""
    return {'order_f': np.array([[1, 1, 0]], np.int32), 'order_b': np.array([[0, 0, 1]], np.int32), 'nu': np.array([[-1.0]]),
            'cref': np.array([cref]), 'site_count': np.array([1.0, 1.0]), 'dG': np.array([[a0, a1, 0.02, 0.0]]),
            'Ea': np.array([[-np.inf, 0.0, 0.0, 0.0]]), 'lnA': np.array([lnA]), 'site_density': site_density}


def langmuir_points(n=7):
    """phiM, csurf [n][1], phi_surface: potentials on both sides of dG = 0, concentrations over eight decades (a concentration of exactly 0 empties the adsorbate, whose log-coverage then has no stationary value)"""
    phiM = np.linspace(-0.25, 0.2, n)
    csurf = np.array([30.0, 1e-2, 100.0, 1e-6, 3.0, 55.0, 0.4])[np.arange(n) % 7][:, None]
    return phiM, csurf, 0.15 * phiM


def langmuir_answer(tab, phiM, c, phi0, omega, CS=0.2, phi_pzc=0.05):
    """(theta [2], K [1][3] complex, lam, terms [1][3]) of one point in closed form.  theta_A = kf a / lam, lam = kf a + kb; at fixed theta
    the net rate r = kf a theta_* - kb theta_A has the slopes rho_p, and K_p = site_density nu rho_p i omega / (i omega + lam).
    terms: the two magnitudes each K_p is the difference of, site_density |rho_p| (1 + lam / |i omega + lam|)"""
    t = KR._arrays(tab)
    V, sg = KR.potential_and_charge(phiM, phi0, 1, CS, phi_pzc, None)
    lf, lb, br = KR.rate_constants(t, V, sg, np.zeros((1, 2)))
    kf, kb = np.exp(lf[0]), np.exp(lb[0])
    a = max(c, 0.0) / t['cref'][0]
    lam = kf * a + kb
    th_a = kf * a / lam
    th = np.array([1.0 - th_a, th_a])
    rho = np.zeros(3)
    rho[0] = kf * th[0] / t['cref'][0] if c >= 0.0 else 0.0
    for q, (dV, ds) in enumerate(((1.0, CS), (-1.0, -CS))):
        dlf, dlb = KR.slopes(t, sg, br, dV, ds)
        rho[1 + q] = kf * a * th[0] * dlf[0] - kb * th[1] * dlb[0]
    z = 1j * omega
    K = t['sd'] * t['nu'][0, 0] * rho * (z / (z + lam))
    terms = t['sd'] * np.abs(rho) * (1.0 + lam / abs(z + lam))
    return th, K[None, :], lam, terms[None, :]


def chain_tables(N, lnA=6.0, site_density=1e-6):
    """S = 2 adsorbates X1, X2 over N >= 1 solution species: species 0 adsorbs (potential dependent), X1 turns into X2 over a
    transition state that feels the potential and the charge (with species 1 as a second educt when N >= 3), X2 leaves as species N-1
    (N = 1: as something the electrolyte does not carry)"""
    T, M = 3, N + 3
    of, ob, nu = np.zeros((3, M), np.int32), np.zeros((3, M), np.int32), np.zeros((3, N))
    of[0, 0], of[0, N], ob[0, N + 1], nu[0, 0] = 1, 1, 1, -1.0
    of[1, N + 1], ob[1, N + 2] = 1, 1
    if N >= 3:
        of[1, 1], nu[1, 1] = 1, -1.0
    of[2, N + 2], ob[2, N] = 1, 1
    if N >= 2:
        ob[2, N - 1], nu[2, N - 1] = 1, 1.0
    dG = np.array([[0.5, 0.0, 0.0, 0.0], [-1.0, 0.5 * FB, 0.3, 0.0], [-0.5, 0.0, 0.0, 0.0]])
    Ea = np.array([[-np.inf, 0.0, 0.0, 0.0], [3.0, 0.25 * FB, 0.1, 2.0], [-np.inf, 0.0, 0.0, 0.0]])
    return {'order_f': of, 'order_b': ob, 'nu': nu, 'cref': np.full(N, 40.0), 'site_count': np.ones(T), 'dG': dG, 'Ea': Ea,
            'lnA': np.full(3, lnA), 'site_density': site_density}
