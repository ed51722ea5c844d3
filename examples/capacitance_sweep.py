#!/usr/bin/env python3
"""Differential capacitance and impedance from the linear response of stationary states (PnpSolver.get_response,
include/catint_response.h), on one MI355X.

  1. A voltage sweep of a 0.1 M 1:1 electrolyte with steric ions (both radii 4 Angstrom) against a Dirichlet wall: every voltage is one
     lane, the zero-flux state is solved on the device, and one get_response call gives C_d(phiM) = d sigma / d phiM of all lanes.
     Printed next to Kornyshev's formula for the lattice-gas (Bikerman) double layer,
     C = (eps / lambda_D) cosh(u/2) / (1 + s) sqrt(s / ln(1 + s)), s = 2 gamma sinh^2(u/2), u = F beta |phiM|: the bell shape.
  2. The CO2R inputs (examples/co2r_inputs.py) at a few voltages through the Calculator with tp.newton['response']: the admittance
     and impedance spectrum of the electrode, from the double-layer plateau down to the diffusion tail."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from catint_amd import PnpSolver
from catint_amd.host import graded_mesh
from catint_amd.units import unit_F, unit_NA, unit_R, unit_eps0


def kornyshev(phiM, c_bulk, radius, beta, eps):
    lam = np.sqrt(eps / beta / (2.0 * unit_F ** 2 * c_bulk))
    gamma = 2.0 * c_bulk * radius ** 3 * unit_NA
    u = unit_F * beta * np.abs(phiM)
    s = 2.0 * gamma * np.sinh(0.5 * u) ** 2
    with np.errstate(invalid='ignore', divide='ignore'):
        shape = np.where(s > 0, np.sqrt(s / np.log1p(s)), 1.0)
    return eps / lam * np.cosh(0.5 * u) / (1.0 + s) * shape


def capacitance_sweep(lanes, nx):
    beta, eps = 1.0 / (unit_R * 298.14), 78.36 * unit_eps0
    c_bulk, radius = 100.0, 4e-10
    lam = np.sqrt(eps / beta / (2.0 * unit_F ** 2 * c_bulk))
    x = graded_mesh(30.0 * lam, 0.02e-9, nx)
    phiM = np.linspace(0.0, -0.8, lanes)
    with PnpSolver(2, nx, float(x[1] - x[0]), 1.0, beta, eps, [1.957e-9, 1.185e-9], [unit_F, -unit_F], method='Newton',
                   batch_capacity=lanes) as s:
        s.set_newton(wall_bc='dirichlet', mpb_radius=[radius, radius], tol=1e-10, maxit=80)
        s.set_grid(x)
        pb = np.zeros((lanes, 4))
        pb[:, 0] = phiM
        s.set_batch(np.full((lanes, 2, nx), c_bulk), pb, np.zeros(lanes), np.zeros((lanes, 2)))
        s.set_equilibrium()                      # zero flux: the Poisson-Boltzmann state is the stationary state
        status = s.solve_stationary()
        res = s.get_response()
        ms = s._responder.last_kernel_ms
    print('C_d(phiM) of a 0.1 M 1:1 electrolyte, ion radius 4 A, %d grid points (response kernel: %.3f ms for %d lanes)' % (nx, ms, lanes))
    print('%8s %14s %14s %10s %s' % ('phiM / V', 'C_d / F m^-2', 'Kornyshev', 'rel. diff', 'status'))
    want = kornyshev(phiM, c_bulk, radius, beta, eps)
    for b in range(lanes):
        cd = res['differential_capacitance'][b]
        print('%8.3f %14.6f %14.6f %+10.2e %d/%d' % (phiM[b], cd, want[b], cd / want[b] - 1.0, status[b], res['status'][b, 0]))


def co2r_impedance(lanes, nx):
    import co2r_physical_sweep as ex
    from catint_amd.calculator import Calculator
    tp, phis = ex.build(lanes, nx, phimin=-0.5, phimax=-0.9)
    calc = Calculator(transport=tp, calc='comsol')
    omega = np.logspace(0, 8, 9)
    tp.newton = {'tol': 1e-9, 'maxit': 80, 'response': {'omega': [0.0] + list(omega)}}
    # Tafel kinetics in the Butler-Volmer form: the response sees the potential dependence of a rate through alpha (a rate given as
    # a function of phiM is a constant per lane to the library)
    alpha = -0.5 * unit_F / (unit_R * tp.system['temperature'])
    k0 = float(ex.tafel_rate(tp)(np.array([0.0]))[0])
    calc.set_surface_kinetics([{'species': 'CO2', 'rate': lambda phiM: np.full(np.shape(phiM), k0), 'alpha': alpha,
                                'stoichiometry': {'CO2': -1.0, 'CO': 1.0, 'OH-': 2.0}}])
    calc.run()
    print('\nCO2R inputs, %d grid points: impedance per unit area of the electrode' % nx)
    for b in range(lanes):
        d = tp.alldata[b]['system']
        print('phiM = %.3f V (status %d): C_d = %.4f F m^-2, polarization resistance %.4g Ohm m^2'
              % (phis[b], calc.status[b], d['differential_capacitance'], d['impedance'][0].real))
        print('  %12s %14s %14s' % ('omega / s^-1', 'Re Z / Ohm m^2', '-Im Z / Ohm m^2'))
        for w, z in zip(d['response_omega'][1:], d['impedance'][1:]):
            print('  %12.3g %14.6g %14.6g' % (w, z.real, -z.imag))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lanes', type=int, default=17)
    ap.add_argument('--nx', type=int, default=258)
    ap.add_argument('--co2r-lanes', type=int, default=3)
    ap.add_argument('--co2r-nx', type=int, default=96)
    a = ap.parse_args()
    capacitance_sweep(a.lanes, a.nx)
    co2r_impedance(a.co2r_lanes, a.co2r_nx)


if __name__ == '__main__':
    main()
