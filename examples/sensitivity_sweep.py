#!/usr/bin/env python3
"""The CO2R polarization sweep of examples/co2r_physical_sweep.py with the parameter sensitivities of every operating point formed on
the device (tp.newton['sensitivities'], include/catint_sens.h): how the current density answers the numbers the model takes from the
literature -- the rate constants of the buffer reactions, the diffusion coefficients -- and the salt concentration, printed as
elasticities d ln|j| / d ln p per voltage.  An elasticity of 1 means: 1 % more of the parameter, 1 % more current.  The bulk-salt
direction adds K+ and HCO3- in equal amounts (electroneutral): its elasticity is per relative change of that added amount, taken at
the size of the bicarbonate concentration.

    python examples/sensitivity_sweep.py --lanes 64
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
    a = ap.parse_args()
    tp, phis = sweep.build(a.lanes, a.nx)
    names = list(tp.species.keys())
    reactions = [key for key, rx in tp.reactions.items() if 'rates' in rx]          # the solver's reaction r is the r-th of these
    salt = np.zeros(len(names))
    salt[names.index('K+')] = salt[names.index('HCO3-')] = float(tp.c0.reshape(len(names), -1)[names.index('HCO3-'), -1])
    params = ([('kf', r) for r in range(len(reactions))] + [('kr', r) for r in range(len(reactions))]
              + [('D', sp) for sp in names] + [('c_bulk', salt)])
    labels = (['kf ' + key for key in reactions] + ['kr ' + key for key in reactions] + ['D ' + sp for sp in names] + ['KHCO3'])
    calc = Calculator(transport=tp, calc='comsol')
    tp.newton = {'tol': 1e-8, 'maxit': 80, 'sensitivities': params}
    calc.set_surface_kinetics([{'species': 'CO2', 'rate': sweep.tafel_rate(tp), 'stoichiometry': {'CO2': -1.0, 'CO': 1.0, 'OH-': 2.0}}])
    calc.run()
    ok = calc.status == 0
    print('%d lanes x %d species x %d points: %d converged; %d parameters per operating point, sensitivity status %s'
          % (a.lanes, tp.nspecies, tp.nx, ok.sum(), len(params), np.bincount(calc.sensitivities['status'], minlength=3).tolist()))
    shown = np.linspace(0, a.lanes - 1, min(a.lanes, 7)).astype(int)
    print('elasticities d ln|j| / d ln p of the current density')
    print('%-28s' % 'phiM [V]' + ''.join('%10.3f' % phis[i] for i in shown))
    for m, label in enumerate(labels):
        row = [tp.alldata[i]['system']['sensitivities']['elasticity']['dcurrent'][m] for i in shown]
        print('%-28s' % label[:28] + ''.join('%10.2e' % v for v in row))


if __name__ == '__main__':
    main()
