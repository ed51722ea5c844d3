#!/usr/bin/env python3
"""Degree of rate control on the device (libcatint_drc): what the call costs next to the steady-state solve it follows, on the same
operating points.  One run on one MI355X writes profiles/drc_probe.md (or the file given as the first argument); no figure in it is
fixed in advance.

Two mechanisms of tests/kinetics_cases.py, their operating points tiled to 65536 (host-surface path, no handle):
  * the four-step CO2 reduction mechanism, two-site variant: N = 3, S = 3, R = 4 (3 R + S = 15 columns);
  * the random network of eight adsorbates: N = 8, S = 8, R = 16 (56 columns, 165 LDS slots per lane).
Per mechanism, in the same process, after one warm-up, five repeats in which the two sides alternate:
  catkin_last_kernel_ms of a cold solve (from the uniform surface) with its own sensitivities (dflux_dc, dflux_dphi), and of a solve
  warm-started from the converged coverages (what an SCF iteration pays);
  catdrc_last_kernel_ms with every field, with the two normalised fields alone (one family of R and one of S columns), and the wall
  time of the full call, copies included.
Minimum, median and maximum of the five repeats are reported."""
import os
import sys
import time

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)

from catint_amd import _drc, _kinetics          # noqa: E402
from tests import kinetics_cases as KC          # noqa: E402

REPEATS, WARMUPS, POINTS = 5, 1, 65536


def spread(v):
    return '%.3f (min %.3f, max %.3f)' % (float(np.median(v)), min(v), max(v))


def measure(name, lines):
    case = KC.case(name)
    idx = np.arange(POINTS) % len(case.phiM)
    pm, cs, ps = case.phiM[idx], case.csurf[idx], case.phi_surface[idx]
    kw = dict(potential_drop='stern' if case.kw['w'] else 'full', stern_capacitance=case.kw['CS'], phi_pzc=case.kw['phi_pzc'])
    of = np.asarray(case.tables['order_f'])
    T = len(case.tables['site_count'])
    Rn, N, S = of.shape[0], of.shape[1] - T, T - 1
    with _kinetics.KineticsSolver(0) as ks, _drc.RateControl(0) as rc:
        cold, warm, full, norm, wall = [], [], [], [], []
        for r in range(REPEATS + WARMUPS):
            kin = ks.solve(None, case.tables, pm, csurf=cs, phi_surface=ps, fields=('theta', 'flux', 'dflux_dc', 'dflux_dphi'), **kw)
            c_ms = ks.last_kernel_ms
            ks.solve(None, case.tables, pm, csurf=cs, phi_surface=ps, fields=('theta', 'flux'), theta_guess=kin['theta'], **kw)
            w_ms = ks.last_kernel_ms
            t0 = time.perf_counter()
            out = rc.solve(None, case.tables, pm, kin['theta'], csurf=cs, phi_surface=ps, fields=list(_drc.FIELDS), **kw)
            t_ms, f_ms = 1e3 * (time.perf_counter() - t0), rc.last_kernel_ms
            rc.solve(None, case.tables, pm, kin['theta'], csurf=cs, phi_surface=ps, fields=('drc', 'tdrc'), **kw)
            n_ms = rc.last_kernel_ms
            if r >= WARMUPS:
                cold.append(c_ms), warm.append(w_ms), full.append(f_ms), norm.append(n_ms), wall.append(t_ms)
        ok = int((out['status'] == 0).sum())
        lines.append('| %s: N = %d, S = %d, R = %d, %d points | %d of %d status 0, worst residual %.1e | %s | %s | %s | %s | %s | %.2f | %.2f |'
                     % (name, N, S, Rn, POINTS, ok, POINTS, float(out['residual'].max()), spread(cold), spread(warm), spread(full), spread(norm),
                        spread(wall), float(np.median(full)) / float(np.median(cold)), float(np.median(full)) / float(np.median(warm))))
        print(lines[-1], flush=True)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, 'profiles', 'drc_probe.md')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    lines = ['# Degree of rate control on the device next to the steady-state solve on the same points (tools/probe/drc_probe.py, one MI355X)', '',
             'Median (minimum, maximum) of %d repeats after %d warm-up, the sides alternating in one process.  Kernel times are HIP events '
             'around the launch; the call is wall time with the copies.  `catkin::steady_kernel` cold: from the uniform surface, with '
             'dflux_dc and dflux_dphi; warm: from the converged coverages, fluxes only.  `catdrc::control_kernel` full: all 3 R + S '
             'columns and every field; normalised: drc and tdrc alone (R + S columns).' % (REPEATS, WARMUPS),
             '', '| mechanism | status | `catkin` cold, ms | `catkin` warm, ms | `catdrc` full, ms | `catdrc` normalised only, ms | '
             '`catdrc_solve` wall (full), ms | full / cold | full / warm |', '|---|---|---|---|---|---|---|---|---|']
    for name in ('co2r_two_site', 'random_S8'):
        measure(name, lines)
    with open(path, 'w') as out:
        out.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
