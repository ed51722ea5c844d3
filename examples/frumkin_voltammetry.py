#!/usr/bin/env python3
"""Voltammetry of an adsorbate with lateral interactions on the device (libcatint_iasweep): one reversible couple, A + * + e- <-> A*
(k0 = 1e4 /s, formal potential E0 = 0.1 V), a batch of self-interaction energies from attractive to repulsive, one launch.  Prints per
eps the cathodic peak current against the Frumkin closed form v / ((4 + eps) kT) and the full width of the peak at half its height:
repulsion lowers and broadens the peak, attraction raises and sharpens it (a mean-field peak is 3.53 kT = 90.6 mV wide at 298 K).

    python examples/frumkin_voltammetry.py [--eps -2 -1 0 1 2 4] [--rate 0.05] [--samples 600]

Run on one MI355X with the defaults: peak heights within 1.1e-4 of the closed form for eps = -2 .. 4 kT, widths 38.0, 63.7, 90.6, 118.1,
145.8 and 201.7 mV, 2734 to 5559 attempted steps per sweep."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

E0, K0 = 0.1, 1e4


def tables(eps, kT):
    """columns: A | *, A*.  dG = (E - E0) / kT + eps theta, no transition state"""
    return {'order_f': np.array([[1, 1, 0]], np.int32), 'order_b': np.array([[0, 0, 1]], np.int32), 'nu': np.array([[-1.0]]), 'cref': np.ones(1),
            'site_count': np.ones(2), 'dG': np.array([[-E0 / kT, 1.0 / kT, 0.0, 0.0]]), 'Ea': np.array([[-np.inf, 0.0, 0.0, 0.0]]),
            'lnA': np.array([np.log(K0)]), 'site_density': 1e-5, 'site_of': np.zeros(2, np.int32), 'site_fraction': np.ones(1),
            'eps': np.array([[float(eps)]]), 'eps_ts': None, 'response': 'linear', 'strength': 1.0}


def width_at_half(E, i):
    j = int(i.argmax())
    half = 0.5 * i[j]

    def crossing(rng):
        for q in rng:
            if (i[q] - half) * (i[q + 1] - half) <= 0.0:
                return E[q] + (half - i[q]) * (E[q + 1] - E[q]) / (i[q + 1] - i[q])
        return np.nan
    return abs(crossing(range(j, len(i) - 1)) - crossing(range(j - 1, -1, -1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--eps', type=float, nargs='+', default=[-2.0, -1.0, 0.0, 1.0, 2.0, 4.0], help='self-interaction energies in kT (> -4)')
    ap.add_argument('--rate', type=float, default=0.05, help='scan rate, V/s')
    ap.add_argument('--samples', type=int, default=600, help='output times of the sweep')
    a = ap.parse_args()
    from catint_amd import InteractingVoltammetry
    from catint_amd.iasweep import DONE, FARADAY
    from catint_amd.units import unit_e, unit_kB
    kT = unit_kB * 298.15 / unit_e
    print('%8s %14s %14s %12s %10s' % ('eps / kT', 'i_p / A/m^2', 'closed form', 'width / mV', 'steps'))
    with InteractingVoltammetry(0) as iv:
        for eps in a.eps:          # eps is a table entry: one call per value, the context and its buffers kept
            # the sweep turns where the free site is still above 1e-5 (the limit of the implicit Euler solve in ln theta)
            E_vertex = E0 - kT * (np.log(1e5) - max(-eps, 0.0)) + 0.01
            out = iv.sweep(None, tables(eps, kT), [1.0], [E0 + 0.31], [E_vertex], [a.rate], n_segments=1, samples=a.samples, csurf=np.ones((1, 1)),
                           phi_surface=np.zeros(1), potential_drop='full', kT=kT, rtol=1e-4, atol=1e-8)
            if out['status'][0] != DONE:
                print('%8.2f  status %d' % (eps, out['status'][0]))
                continue
            i = -out['current'][0]
            print('%8.2f %14.6e %14.6e %12.2f %10d' % (eps, i.max(), FARADAY * 1e-5 * a.rate / ((4.0 + eps) * kT),
                                                     1e3 * width_at_half(out['E_out'][0], i), out['steps'][0, :2].sum()))


if __name__ == '__main__':
    main()
