#!/usr/bin/env python3
"""Cyclic voltammetry of an adsorbate couple on the device (libcatint_voltam): one model, a batch of scan rates over four decades, one
launch.  A + * + e- <-> A* behind a transition state (beta = 0.5, k0 = 10 /s at the formal potential E0 = 0.1 V): reversible at the slow
end of the batch, irreversible at the fast end.  Prints per scan rate the cathodic peak potential and current, the separation of the
two peaks and the charge under the cathodic one in units of a monolayer (F site_density).

    python examples/adsorbate_voltammetry.py [--rates 13] [--samples 400]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

E0, K0, PREFACTOR = 0.1, 10.0, 1e5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rates', type=int, default=13, help='scan rates between 1e-2 and 1e2 V/s')
    ap.add_argument('--samples', type=int, default=400, help='output times per segment')
    a = ap.parse_args()
    from catint_amd import Voltammetry
    from catint_amd.microkinetics import MeanFieldModel
    from catint_amd.voltammetry import DONE, FARADAY
    kT = MeanFieldModel(['A'], {'A': 1}, [], {}).kT
    barrier = kT * np.log(PREFACTOR / K0)          # eV at E0: kf = kb = k0 there
    # energies at V = 0: the couple is at equilibrium at E0, so A* lies E0 below A + * + e-
    model = MeanFieldModel(['A'], {'A': 1}, ['A_g + *_t + ele_g <-> A-ele_t <-> A*_t; beta=0.5; prefactor=%r' % PREFACTOR],
                           {'A': -E0, 'A-ele': barrier - 0.5 * E0}, cref=1.0, site_density=1e-5)
    v = np.geomspace(1e-2, 1e2, a.rates)
    n = len(v)
    with Voltammetry(0) as vm:
        out = vm.sweep(None, model, None, np.full(n, E0 + 0.35), np.full(n, E0 - 0.3), v, n_segments=2, samples=a.samples, csurf=np.ones((n, 1)),
                       phi_surface=np.zeros(n), potential_drop='full', rtol=1e-4)
        print('kernel %s: %.2f ms for %d sweeps' % (vm.last_kernel, vm.last_kernel_ms, n))
    K = a.samples
    monolayer = FARADAY * model.site_density
    print('%10s %12s %14s %12s %12s %8s' % ('v / V/s', 'E_pc / V', 'i_pc / A/m^2', 'dE_p / V', 'Q_c / ML', 'steps'))
    for i in range(n):
        if out['status'][i] != DONE:
            print('%10.3g status %d' % (v[i], out['status'][i]))
            continue
        cur, E = out['mean_current'][i], out['E_out'][i]
        pc, pa = int(cur[:K].argmin()), K + int(cur[K:].argmax())
        print('%10.3g %12.4f %14.4g %12.4f %12.4f %8d' % (v[i], E[pc], cur[pc], E[pa] - E[pc], -out['charge'][i, K - 1] / monolayer,
                                                           out['steps'][i, :2].sum()))


if __name__ == '__main__':
    main()
