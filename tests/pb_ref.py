"""NumPy restatement of the definition in include/catint_equil.h (test infrastructure): the discrete size-modified Poisson-Boltzmann
problem the stationary zero-flux system of oracle/pnp_physical.py collapses to, solved by the damped Newton iteration of the header
with LAPACK's banded LU.  The device kernel is compared against this; this is compared against the oracle (tests/test_equil_abi.py)."""
import numpy as np
from scipy.linalg import solve_banded

N_AVOGADRO = 6.022140857e23
MAX_EXPONENT = 500.0


def grid_weights(x, dx):
    """w_e = dx / h_e [nx - 1] and v_i = V_i / dx [nx] (half cells at the ends): oracle/pnp_physical.py PhysicalProblem"""
    h = np.diff(np.asarray(x, float))
    v = np.empty(len(h) + 1)
    v[1:-1] = 0.5 * (h[1:] + h[:-1]) / dx
    v[0], v[-1] = 0.5 * h[0] / dx, 0.5 * h[-1] / dx
    return dx / h, v


def concentrations(phi, charges, beta, c_bulk, phi_bulk, vol):
    """c[N][nx] of the potential row, and d rho / d phi [nx]"""
    q, cb = np.asarray(charges, float), np.asarray(c_bulk, float)
    u = np.clip(-(q * beta)[:, None] * (phi - phi_bulk)[None, :], -MAX_EXPONENT, MAX_EXPONENT)
    a = (cb / (1.0 - (vol * cb).sum()))[:, None] * np.exp(u)
    c = a / (1.0 + (vol[:, None] * a).sum(axis=0))[None, :]
    rho = (q[:, None] * c).sum(axis=0)
    drho = -beta * ((q * q)[:, None] * c).sum(axis=0) + beta * rho * ((vol * q)[:, None] * c).sum(axis=0)
    return c, drho


def solve(x, dx, charges, beta, eps, c_bulk, phiM, phi_bulk=0.0, mpb_radius=None, stern_capacitance=None, phi_pzc=0.0, tol=1e-10,
          maxit=100):
    """One operating point.  Returns c [N][nx], phi [nx], status (0, or 1: not converged), iterations."""
    x, q = np.asarray(x, float), np.asarray(charges, float)
    nx = len(x)
    w, v = grid_weights(x, dx)
    pe = dx * dx / eps
    vol = N_AVOGADRO * (np.zeros(len(q)) if mpb_radius is None else np.asarray(mpb_radius, float)) ** 3
    qbmax = np.abs(q * beta).max()
    phi = np.full(nx, float(phi_bulk))
    status, it = 1, 0
    maxit = min(int(maxit), 1000)
    while it < maxit:
        c, drho = concentrations(phi, q, beta, c_bulk, phi_bulk, vol)
        rho = (q[:, None] * c).sum(axis=0)
        F = np.empty(nx)
        ab = np.zeros((3, nx))
        F[1:-1] = w[1:] * (phi[2:] - phi[1:-1]) - w[:-1] * (phi[1:-1] - phi[:-2]) + pe * v[1:-1] * rho[1:-1]
        ab[1, 1:-1] = -(w[1:] + w[:-1]) + pe * v[1:-1] * np.minimum(drho[1:-1], 0.0)
        ab[0, 2:] = w[1:]              # superdiagonal of rows 1 .. nx-2
        ab[2, :-2] = w[:-1]            # subdiagonal of rows 1 .. nx-2
        if stern_capacitance is None:
            F[0] = phi[0] - phiM
            ab[1, 0] = 1.0
        else:
            g = dx * stern_capacitance / eps
            F[0] = w[0] * (phi[1] - phi[0]) + g * (phiM - phi_pzc - phi[0])
            ab[1, 0] = -w[0] - g
            ab[0, 1] = w[0]
        F[-1] = phi[-1] - phi_bulk
        ab[1, -1] = 1.0
        d = solve_banded((1, 1), ab, -F)
        upd = qbmax * np.abs(d).max()
        phi = phi + min(1.0, 2.0 / upd if upd > 0.0 else 1.0) * d
        it += 1
        if upd < tol:
            status = 0
            break
    c, _ = concentrations(phi, q, beta, c_bulk, phi_bulk, vol)
    return c, phi, status, it
