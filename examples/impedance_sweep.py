#!/usr/bin/env python3
"""Nyquist data of the CO2 reduction sweep with the microkinetic electrode (examples/co2r_microkinetic_sweep.py): after the Newton SCF
loop has found the fixed point of kinetics and transport at every voltage, the small-signal impedance of the working electrode at that
state -- the linearised surface kinetics with adsorbate storage, the transport transfer functions at the same frequency and the Stern
layer, closed at the wall on the device (include/catint_eis.h, Calculator.set_microkinetics(..., impedance=[omega ...])).

    python examples/impedance_sweep.py --lanes 8 --nfreq 25

Prints, per voltage, the polarisation resistance 1 / Re Y(0) (the slope of the polarisation curve of the coupled electrode, without a
finite difference), and for a few voltages the Nyquist points (Re Z, -Im Z) in Ohm cm^2 over the frequency list, with the faradaic and
the double-layer share of the admittance.  tp.newton['response'] on the same run gives the admittance of a BLOCKING electrode: the SCF
loop prescribes the wall fluxes, so the plain linear response knows nothing of the reaction."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from catint_amd.calculator import Calculator          # noqa: E402
import co2r_microkinetic_sweep as sweep                # noqa: E402
import co2r_physical_sweep                             # noqa: E402  (the transport of the sweep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lanes', type=int, default=8)
    ap.add_argument('--nx', type=int, default=192)
    ap.add_argument('--phimin', type=float, default=-0.6)
    ap.add_argument('--phimax', type=float, default=-1.2)
    ap.add_argument('--nfreq', type=int, default=25, help='frequencies: 0 and nfreq - 1 logarithmically spaced from fmin to fmax (Hz)')
    ap.add_argument('--fmin', type=float, default=1e-2)
    ap.add_argument('--fmax', type=float, default=1e6)
    ap.add_argument('--site-fraction', type=float, default=1e-3)
    a = ap.parse_args()
    omega = np.concatenate([[0.0], 2.0 * np.pi * np.logspace(np.log10(a.fmin), np.log10(a.fmax), a.nfreq - 1)])
    tp, phis = co2r_physical_sweep.build(a.lanes, a.nx, a.phimin, a.phimax)
    tp.newton = {'tol': 1e-8, 'maxit': 80}
    calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-6)
    calc.set_microkinetics(sweep.model(tp), site_density=a.site_fraction * float(tp.system['active site density']), scf='newton', impedance=omega)
    names = list(tp.species.keys())
    out = calc.run_scf_cycle(nel=[2.0 if sp == 'CO' else 1.0 for sp in names], max_iter=200)
    imp = out['impedance']
    print('%d lanes, %d converged; impedance status counts: %s' % (a.lanes, out['converged'].sum(), np.bincount(imp['status'].reshape(-1)).tolist()))
    print('phiM [V]   R_p = 1 / Re Y(0) [Ohm cm2]   |Z| at %.0e Hz [Ohm cm2]' % a.fmax)
    for i in range(a.lanes):
        print('%7.3f   %14.5e   %14.5e' % (phis[i], 1e4 / imp['admittance'][i, 0].real, 1e4 * abs(imp['impedance'][i, -1])))
    for i in sorted(set(np.linspace(0, a.lanes - 1, min(a.lanes, 3)).astype(int))):
        print('Nyquist data at phiM = %.3f V:   f [Hz]   Re Z   -Im Z [Ohm cm2]   |Y_F| / |Y|   |Y_dl| / |Y|' % phis[i])
        for f in range(1, len(omega)):
            z, y = imp['impedance'][i, f], imp['admittance'][i, f]
            print('   %10.3e   %12.5e   %12.5e   %6.3f   %6.3f' % (omega[f] / (2.0 * np.pi), 1e4 * z.real, -1e4 * z.imag, abs(imp['faradaic'][i, f]) / abs(y),
                                                                 abs(imp['double_layer'][i, f]) / abs(y)))


if __name__ == '__main__':
    main()
