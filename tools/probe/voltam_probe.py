#!/usr/bin/env python3
"""Voltammetry on the device (libcatint_voltam): what a sweep costs, what the divergence of the lanes costs and how often the
extrapolated state is not accepted.  One run on one MI355X writes profiles/voltam_probe.md (or the file given as the first argument);
no figure in it is fixed in advance.  A record, not a gate: nobody has measured this kernel before.

The model is the two-site CO2 reduction mechanism of tests/kinetics_cases.py at 30 mol/m^3 CO2.  n = 4096 points, E_start spread over
-0.55 .. -0.65 V so that no two lanes of a wave integrate the same program, E_vertex = -1.0 V, 2 segments of 50 output times, rtol
1e-4, at three scan rates.  Recorded per scan rate: catvm_last_kernel_ms (HIP events around the launch, median / min / max of 5 calls
after 1 warm-up), the mean attempted steps per lane, the ratio of the largest to the mean step count per wave of 64 lanes (a wave
runs as long as its slowest lane) averaged over the waves and at its worst, and the share of accepted steps that were not
extrapolated.  A second table does the same for a surface-confined couple (A + * + e- <-> A*, k0 = 10 /s), where the current, not
the coverages, sets the step."""
import os
import sys

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)

CALLS, WARMUPS = 5, 1
N_POINTS, SEGMENTS, SAMPLES, RTOL = 4096, 2, 50, 1e-4
RATES = (0.01, 1.0, 100.0)


def measure(vm, label, tables, electrons, E_start, E_vertex, csurf, phi_surface, lines, **kw):
    for rate in RATES:
        ms = []
        for r in range(CALLS + WARMUPS):
            out = vm.sweep(None, tables, electrons, E_start, E_vertex, np.full(len(E_start), rate), n_segments=SEGMENTS, samples=SAMPLES, csurf=csurf,
                           phi_surface=phi_surface, rtol=RTOL, fields=('theta', 'current', 'charge'), **kw)
            if r >= WARMUPS:
                ms.append(vm.last_kernel_ms)
        att = out['steps'][:, :2].sum(axis=1).astype(float)
        waves = att.reshape(-1, 64)
        ratio = waves.max(axis=1) / waves.mean(axis=1)
        acc = out['steps'][:, 0].sum()
        lines.append('| %s | %g | `%s` %.2f ms (min %.2f, max %.2f) | %.3f us | %.0f / %d | %.3f / %.3f | %.2e | %.0f | %s |'
                     % (label, rate, vm.last_kernel, float(np.median(ms)), min(ms), max(ms), 1e3 * float(np.median(ms)) / len(E_start), att.mean(),
                        att.max(), ratio.mean(), ratio.max(), out['steps'][:, 3].sum() / max(acc, 1), out['steps'][:, 2].mean(),
                        ', '.join('%d x %d' % (int((out['status'] == v).sum()), v) for v in np.unique(out['status']))))
        print(lines[-1], flush=True)


def main():
    from catint_amd import voltammetry
    from tests import kinetics_cases as KC
    from tests import voltam_cases as VC
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, 'profiles', 'voltam_probe.md')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    model = KC.co2r_model('two_site')
    n = N_POINTS
    lines = ['# Voltammetry on the device: kernel time, lane divergence and extrapolation (tools/probe/voltam_probe.py, one MI355X)', '',
             '%d points x %d segments x %d output times, rtol %g, the steady state at E_start as the start.  Kernel times are HIP events around '
             'the launch (median of %d calls after %d warm-up).  co2r: the two-site CO2 reduction mechanism (N = 3, S = 3, R = 4) at 30 mol/m^3 '
             'CO2, E_start spread over -0.55 .. -0.65 V, E_vertex -1.0 V.  couple: A + * + e- <-> A* with k0 = 10 /s (N = 1, S = 1, R = 1), E_start '
             'spread over E0 + 0.26 .. E0 + 0.31 V, E_vertex E0 - 0.29 V.' % (n, SEGMENTS, SAMPLES, RTOL, CALLS, WARMUPS), '',
             '| model | scan rate V/s | kernel | per point | attempted steps per lane (mean / largest) | largest / mean steps per wave (mean over '
             'waves / worst wave) | share of accepted steps not extrapolated | Newton iterations per lane (mean) | statuses |',
             '|---|---|---|---|---|---|---|---|---|']
    rng = np.random.RandomState(0)
    with voltammetry.Voltammetry(0) as vm:
        E_start = rng.uniform(-0.65, -0.55, n)
        measure(vm, 'co2r', model, None, E_start, np.full(n, -1.0), np.tile([30.0, 1e-3, 0.1], (n, 1)), np.full(n, -0.08), lines,
                potential_drop='stern', stern_capacitance=KC.STERN['CS'], phi_pzc=KC.STERN['phi_pzc'])
        c = VC.case('langmuir_quasi')
        E_start = VC.E0 + rng.uniform(0.26, 0.31, n)
        measure(vm, 'couple', c.tables, c.electrons, E_start, np.full(n, VC.E0 - 0.29), np.ones((n, 1)), np.zeros(n), lines, potential_drop='full',
                rate_floor=VC.RATE_FLOOR)
    with open(path, 'w') as out_file:
        out_file.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
