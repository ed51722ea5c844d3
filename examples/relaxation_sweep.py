#!/usr/bin/env python3
"""The CO2R polarization sweep of examples/co2r_physical_sweep.py with the slowest relaxation modes of every operating point formed on
the device (tp.newton['relaxation'], include/catint_modes.h): at which rate the stationary state found would be approached, and whether
it is stable.  Per voltage the slowest rate is printed next to the two time scales one would guess it from -- diffusion across the cell,
D_min / L^2, and the charging of the double layer through the cell, D_max / (lambda_D L) -- and its time constant next to the step
catint_amd.synthetic.make_batch takes for a transient of such a system, 0.1 lambda_D L / D_max.

    python examples/relaxation_sweep.py --lanes 64
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from catint_amd.calculator import Calculator      # noqa: E402
import co2r_physical_sweep as sweep               # noqa: E402  (the system, its mesh and its Tafel kinetics)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lanes', type=int, default=64)
    ap.add_argument('--nx', type=int, default=384)
    ap.add_argument('--iterations', type=int, default=12)
    a = ap.parse_args()
    tp, phis = sweep.build(a.lanes, a.nx)
    calc = Calculator(transport=tp, calc='comsol')
    tp.newton = {'tol': 1e-8, 'maxit': 80, 'relaxation': {'nmodes': 3, 'iterations': a.iterations}}
    calc.set_surface_kinetics([{'species': 'CO2', 'rate': sweep.tafel_rate(tp), 'stoichiometry': {'CO2': -1.0, 'CO': 1.0, 'OH-': 2.0}}])
    calc.run()
    ok = calc.status == 0
    res = calc.relaxation
    print('%d lanes x %d species x %d points: %d converged; relaxation status %s, all three rates converged in %d lanes'
          % (a.lanes, tp.nspecies, tp.nx, ok.sum(), np.bincount(res['status'], minlength=4).tolist(), int(res['converged'].all(axis=1).sum())))
    D = np.asarray(tp.D, float)
    z = np.array([float(sp['charge']) for sp in tp.species.values()])
    cb = tp.c0.reshape(tp.nspecies, -1)[:, -1]
    L = float(tp.xmesh[-1] - tp.xmesh[0])
    debye = float(np.sqrt(tp.eps / tp.beta / ((z * 96485.33289) ** 2 * cb).sum()))
    dt_guess = 0.1 * debye * L / D.max()
    print('D_min / L^2 = %.3e 1/s, D_max / (lambda_D L) = %.3e 1/s, make_batch would step with dt = %.3e s' % (D.min() / L ** 2, D.max() / (debye * L), dt_guess))
    print('%10s %14s %14s %12s %8s %14s' % ('phiM [V]', 'slowest [1/s]', 'tau_1 [s]', 'residual', 'stable', 'tau_1 / dt'))
    for i in np.linspace(0, a.lanes - 1, min(a.lanes, 9)).astype(int):
        d = tp.alldata[i]['system']['relaxation']
        print('%10.3f %14.4e %14.4e %12.1e %8s %14.1f' % (phis[i], d['rates'][0].real, d['time_constants'][0], d['residual'][0], d['stable'],
                                                         d['time_constants'][0] / dt_guess))


if __name__ == '__main__':
    main()
