#!/usr/bin/env python3
"""Relaxation modes on the device (libcatint_modes): what a pass of the subspace iteration costs next to the 8-column sensitivity call,
which is one elimination with as many carried right-hand sides and nothing else.  One run on one MI355X writes profiles/modes_probe.md (or
the file given as the first argument); no figure in it is fixed in advance.

Two handles of point ions against a Dirichlet wall on the graded grid of tools/probe/response_probe.py, nx = 512, 4096 operating points
each, brought to their stationary state first: N = 3 (block size 4, 16 systems per wave) and N = 8 (block size 9, 7 systems per wave).
Per handle, for 64 lanes (every 64th) and for all 4096, in the same process, after one warm-up, five repeats in which the sides alternate:
  catmodes_last_kernel_ms (HIP events around the launch) of get_relaxation(subspace=8, iterations=12) and of the same call with one pass;
  (12 passes - 1 pass) / 11 is the cost of a pass: elimination with records, substitution, Rayleigh-Ritz matrices, orthonormalisation;
  catsens_last_kernel_ms of get_sensitivities with 8 parameters on the same handle and lanes;
  per pass / sensitivity call, and 1 - sensitivity call / per pass: the share of a pass that is not the elimination itself.  The kernel has
  no switch that would take the orthonormalisation out, so its share alone is not separated from the records, the substitution and the
  Rayleigh-Ritz sums: the figure is an upper bound for it.
Minimum, median and maximum of the five repeats are reported."""
import os
import sys

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import response_probe as RP          # noqa: E402  (constants and the grid)
from catint_amd import PnpSolver, _modes         # noqa: E402
from catint_amd.units import unit_F  # noqa: E402

REPEATS, WARMUPS = 5, 1
NX, BATCH = 512, 4096


def handle(N):
    """point ions, Dirichlet wall, electroneutral bulk"""
    z = np.array([1, -1, 2, -1, 0, 1, -2, -1][:N], float)
    cb = np.array([100.0, 50.0, 20.0, 60.0, 30.0, 10.0, 15.0, 10.0][:N])
    if N == 3:
        cb[1] = 140.0
    assert (z * cb).sum() == 0.0
    x = RP.graded_mesh(4e-8, 5e-11, NX)
    s = PnpSolver(N, NX, float(x[1] - x[0]), 1.0, RP.BETA, RP.EPS, 1e-9 * (1.0 + 0.3 * np.arange(N)), z * unit_F, method='Newton', batch_capacity=BATCH)
    s.set_grid(x)
    pb = np.zeros((BATCH, 4))
    pb[:, 0] = np.linspace(-0.25, 0.25, BATCH)
    s.set_batch(np.repeat(np.repeat(cb[None, :, None], NX, axis=2), BATCH, axis=0), pb, np.zeros(BATCH), np.zeros((BATCH, N)))
    s.set_equilibrium()
    return s, s.solve_stationary()


def spread(v):
    return '%.3f (min %.3f, max %.3f)' % (float(np.median(v)), min(v), max(v))


def measure(s, status, lines, ratios):
    N = s.N
    specs = (['phiM', 'velocity'] + [(kind, j) for kind in ('c_bulk', 'D', 'flux') for j in range(N)])[:8]
    for n in (64, BATCH):
        lanes = np.arange(0, BATCH, BATCH // n)
        full, one, sens = [], [], []
        for r in range(REPEATS + WARMUPS):
            res = s.get_relaxation(subspace=8, iterations=12, lanes=lanes)
            f_ms = s._mode_solver.last_kernel_ms
            s.get_relaxation(subspace=8, iterations=1, lanes=lanes)
            o_ms = s._mode_solver.last_kernel_ms
            s.get_sensitivities(specs, lanes=lanes, fields=['dcurrent'])
            s_ms = s._sensitizer.last_kernel_ms
            if r >= WARMUPS:
                full.append(f_ms), one.append(o_ms), sens.append(s_ms)
        per_pass = (float(np.median(full)) - float(np.median(one))) / 11.0
        sm = float(np.median(sens))
        good = status[lanes] == 0
        conv = res['converged'][good].sum(axis=1)
        lines.append('| N = %d, nx = %d, %d lanes | `%s`; %d of %d solved lanes status 0, 3 rates converged in %d, stable in %d | %s | %s | %.3f | %s | '
                     '%.2f | %.0f %% |'
                     % (N, NX, n, s._mode_solver.last_kernel, int((res['status'][good] == 0).sum()), int(good.sum()), int((conv == 3).sum()),
                        sum(1 for v in res['stable'][good] if v is True), spread(full), spread(one), per_pass, spread(sens), per_pass / sm,
                        100.0 * (1.0 - sm / per_pass)))
        ratios.append(('N = %d, %d lanes' % (N, n), per_pass / sm))
        print(lines[-1], flush=True)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, 'profiles', 'modes_probe.md')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    lines = ['# Relaxation modes on the device: a pass of the subspace iteration next to the 8-column sensitivity call '
             '(tools/probe/modes_probe.py, one MI355X)', '',
             'Median (minimum, maximum) of %d repeats after %d warm-up, the sides alternating in one process.  Kernel times are HIP events '
             'around the launch.  Per pass = (12 passes - 1 pass) / 11.  The last column is 1 - sensitivity call / per pass: everything a '
             'pass adds to the elimination (records, substitution, Rayleigh-Ritz sums, orthonormalisation), an upper bound for the share of '
             'the orthonormalisation, which the kernel cannot run without.' % (REPEATS, WARMUPS),
             '', '| handle | call | `get_relaxation(subspace=8, iterations=12)` kernel, ms | the same with 1 pass, ms | per pass, ms | '
             '`get_sensitivities`, 8 parameters, kernel, ms | per pass / sensitivity call | share of a pass beyond the elimination |',
             '|---|---|---|---|---|---|---|---|']
    ratios = []
    for N in (3, 8):
        s, status = handle(N)
        with s:
            measure(s, status, lines, ratios)
    ws = _modes.MAX_SUBSPACE
    lines += ['', 'Workspace per resident system: (N+1) nx (N + 17) doubles -- %.2f MiB at N = 3, %.2f MiB at N = 8 -- under the cap of 2 GiB.'
              % (4 * NX * (3 + 2 * ws + 1) * 8 / 2.0 ** 20, 9 * NX * (8 + 2 * ws + 1) * 8 / 2.0 ** 20)]
    over = ['%s: %.2f' % r for r in ratios if r[1] > 3.0]
    if over:
        lines += ['', 'A pass adds the round trip of the records and that of the basis to the sensitivity call, which should keep it near 3 x that '
                  'call while both stay in the L2.  Above 3 x (%s) they are leaving it: the slots of the systems resident at once are far larger '
                  'than the 4 MiB L2, so the substitution and the sweeps of the wave phase read from HBM or the Infinity Cache.' % '; '.join(over)]
    else:
        lines += ['', 'Every per-pass cost is within 3 x the sensitivity call: the records and the basis stay in the L2.']
    with open(path, 'w') as out:
        out.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
