#!/usr/bin/env python3
"""Voltammetry of interacting adsorbates on the device (libcatint_iasweep): what a sweep costs, what the coverage-dependent rate
constants cost on top of the mean-field kernel, what the divergence of the lanes costs and how often the extrapolated state is not
accepted.  One run on one MI355X writes profiles/iasweep_probe.md (or the file given as the first argument); no figure in it is fixed
in advance.  A record, not a gate.

The shape is that of tools/probe/voltam_probe.py: n = 4096 points, 2 segments of 50 output times, rtol 1e-4, at three scan rates,
E_start spread so that no two lanes of a wave integrate the same program.  Three models:
  co2r_weak    the one-site CO2 reduction mechanism of tests/interact_cases.py with the weak interaction, -0.55 .. -0.65 V to -1.0 V,
               the start ramped in 10 stages
  frumkin      A + * + e- <-> A* with k0 = 10 /s and a self-interaction of +2 kT (tests/iasweep_cases.py: frumkin_quasi)
  mean field   the two-site CO2 reduction mechanism of tests/kinetics_cases.py WITHOUT interactions, once through
               catis::sweep_kernel at strength 0 (G = 1, start_ramp 1: the same bits) and once through catvm::sweep_kernel on the same
               inputs, in the same run -- the yardstick
Recorded per row: the kernel time (HIP events around the launch, median / min / max of 5 calls after 1 warm-up), the attempted steps
per lane, the ratio of the largest to the mean step count per wave of 64 lanes, the share of accepted steps that were not
extrapolated, the Newton iterations per lane and the statuses."""
import os
import sys

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)

CALLS, WARMUPS = 5, 1
N_POINTS, SEGMENTS, SAMPLES, RTOL = 4096, 2, 50, 1e-4
RATES = (0.01, 1.0, 100.0)


def measure(ctx, label, tables, electrons, E_start, E_vertex, csurf, phi_surface, lines, **kw):
    for rate in RATES:
        ms = []
        for r in range(CALLS + WARMUPS):
            out = ctx.sweep(None, tables, electrons, E_start, E_vertex, np.full(len(E_start), rate), n_segments=SEGMENTS, samples=SAMPLES, csurf=csurf,
                            phi_surface=phi_surface, rtol=RTOL, fields=('theta', 'current', 'charge'), **kw)
            if r >= WARMUPS:
                ms.append(ctx.last_kernel_ms)
        att = out['steps'][:, :2].sum(axis=1).astype(float)
        waves = att.reshape(-1, 64)
        ratio = waves.max(axis=1) / np.maximum(waves.mean(axis=1), 1.0)
        acc = out['steps'][:, 0].sum()
        lines.append('| %s | %g | `%s` %.2f ms (min %.2f, max %.2f) | %.3f us | %.0f / %d | %.3f / %.3f | %.2e | %.0f | %s |'
                     % (label, rate, ctx.last_kernel, float(np.median(ms)), min(ms), max(ms), 1e3 * float(np.median(ms)) / len(E_start), att.mean(),
                        att.max(), ratio.mean(), ratio.max(), out['steps'][:, 3].sum() / max(acc, 1), out['steps'][:, 2].mean(),
                        ', '.join('%d x %d' % (int((out['status'] == v).sum()), v) for v in np.unique(out['status']))))
        print(lines[-1], flush=True)
    return out


def main():
    from catint_amd import iasweep, voltammetry
    from tests import iasweep_cases as SC
    from tests import iasweep_ref as SR
    from tests import interact_cases as IC
    from tests import kinetics_cases as KC
    from tests import voltam_cases as VC
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, 'profiles', 'iasweep_probe.md')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    n = N_POINTS
    lines = ['# Voltammetry of interacting adsorbates on the device: kernel time, lane divergence and extrapolation '
             '(tools/probe/iasweep_probe.py, one MI355X)', '',
             '%d points x %d segments x %d output times, rtol %g, the steady state at E_start as the start.  Kernel times are HIP events around '
             'the launch (median of %d calls after %d warm-up).  co2r_weak: the one-site CO2 reduction mechanism with 0.3 / 0.15 eV interactions '
             '(N = 3, S = 4, R = 4; start ramped in 10 stages) at 30 mol/m^3 CO2, E_start spread over -0.55 .. -0.65 V, E_vertex -1.0 V.  frumkin: '
             'A + * + e- <-> A* with k0 = 10 /s and eps = +2 kT, E_start spread over E0 + 0.26 .. E0 + 0.31 V, E_vertex E0 - 0.29 V.  mean field: '
             'the two-site CO2 reduction mechanism without interactions (N = 3, S = 3, R = 4) through the new kernel at strength 0 and through '
             'the mean-field kernel, same inputs, same run; the two return the same bits.' % (n, SEGMENTS, SAMPLES, RTOL, CALLS, WARMUPS), '',
             '| model | scan rate V/s | kernel | per point | attempted steps per lane (mean / largest) | largest / mean steps per wave (mean over '
             'waves / worst wave) | share of accepted steps not extrapolated | Newton iterations per lane (mean) | statuses |',
             '|---|---|---|---|---|---|---|---|---|']
    rng = np.random.RandomState(0)
    stern = dict(potential_drop='stern', stern_capacitance=KC.STERN['CS'], phi_pzc=KC.STERN['phi_pzc'])
    E_co2r = rng.uniform(-0.65, -0.55, n)
    csurf, phis = np.tile([30.0, 1e-3, 0.1], (n, 1)), np.full(n, -0.08)
    with iasweep.InteractingVoltammetry(0) as iv:
        measure(iv, 'co2r_weak', IC.co2r_model('one_site', 0.3, 0.15), None, E_co2r, np.full(n, -1.0), csurf, phis, lines, **stern)
        c = SC.case('frumkin_quasi')
        E_start = VC.E0 + rng.uniform(0.26, 0.31, n)
        measure(iv, 'frumkin', c.tables, c.electrons, E_start, np.full(n, VC.E0 - 0.29), np.ones((n, 1)), np.zeros(n), lines, potential_drop='full',
                rate_floor=VC.RATE_FLOOR)
        model = KC.co2r_model('two_site')
        new = measure(iv, 'mean field, new kernel', SR.mean_field_tables(model.tables()), model.electrons(), E_co2r, np.full(n, -1.0), csurf, phis,
                      lines, kT=model.kT, start_ramp=1, **stern)
    with voltammetry.Voltammetry(0) as vm:
        old = measure(vm, 'mean field, parent kernel', model, None, E_co2r, np.full(n, -1.0), csurf, phis, lines, **stern)
    same = all(np.array_equal(new[k], old[k], equal_nan=True) for k in old)
    lines += ['', 'The two mean-field rows returned %s.' % ('the same bits in every output' if same else 'DIFFERENT bits')]
    with open(path, 'w') as out_file:
        out_file.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
