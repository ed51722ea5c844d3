#!/usr/bin/env python3
"""Lateral interactions and several site types on the device (libcatint_interact): what the general rows cost next to the mean-field
kernel, what a stage of the ramp costs, and the two-site-type case.  One run on one MI355X writes profiles/interact_probe.md (or the
file given as the first argument) below the marker line, keeping what stands above it; no figure in it is fixed in advance.  A record,
not a gate: nobody has measured this kernel before.

The points are the 39 of the CO2 reduction lattice of tests/kinetics_cases.py (13 potentials x CO2 at 30, 1e-3 and 0 mol/m^3) repeated
to n = 4096.  Kernel times are <prefix>last_kernel_ms (HIP events around the launch, without the copies): the median, smallest and
largest of CALLS calls after WARMUPS warm-ups, the compared kernels alternating call by call in one process.
  1. eps = 0, G = 1, one stage, on the two-site mechanism: catia_solve against catkin_solve (libcatint_kinetics is unchanged by this
     library: its code object is the parent commit's, profiles/interact_probe.md lists the hashes) -- the price of the general rows.
  2. The same mechanism with the weak interaction of tests/interact_cases.py at ramp = 1, 2, 5 and 10: the cost per further stage, as
     (t(K) - t(2)) / (K - 2), beside the iterations the stages take.  The base is ramp = 2, not 1: in one stage some points of this
     case stop at maxit (200 iterations), and a wave runs as long as its slowest lane.
  3. The terrace-and-step case (two site types, S = 5), one stage."""
import os
import sys

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)

CALLS, WARMUPS, N_POINTS = 7, 2, 4096
MARKER = '<!-- below this line: written by tools/probe/interact_probe.py -->'


def spread(v):
    return '%.3f ms (min %.3f, max %.3f)' % (float(np.median(v)), min(v), max(v))


def main():
    from catint_amd import _interact, _kinetics
    from tests import interact_cases as IC
    from tests import kinetics_cases as KC
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, 'profiles', 'interact_probe.md')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    head = ''
    if os.path.exists(path):
        text = open(path).read()
        head = text[:text.index(MARKER)] if MARKER in text else text
    c = KC.co2r_case('two_site')
    idx = np.arange(N_POINTS) % len(c.phiM)
    pm, cs, ps = c.phiM[idx], c.csurf[idx], c.phi_surface[idx]
    kw = dict(potential_drop='stern', stern_capacitance=c.kw['CS'], phi_pzc=c.kw['phi_pzc'], csurf=cs, phi_surface=ps)
    T = len(c.tables['site_count'])
    zero = dict(c.tables, site_of=np.zeros(T, np.int32), site_fraction=np.ones(1), eps=np.zeros((T - 1, T - 1)))
    fields = ('theta', 'flux', 'flux_scale')
    lines = [MARKER, '', '## Kernel times (%d points, median of %d calls after %d warm-ups, the compared kernels alternating)' % (N_POINTS, CALLS, WARMUPS), '']
    with _kinetics.KineticsSolver(0) as ks, _interact.InteractingKinetics(0) as ia:
        t_kin, t_ia = [], []
        for r in range(CALLS + WARMUPS):
            a = ks.solve(None, c.tables, pm, fields=fields, **kw)
            b = ia.solve(None, zero, pm, fields=fields, **kw)
            if r >= WARMUPS:
                t_kin.append(ks.last_kernel_ms), t_ia.append(ia.last_kernel_ms)
        equal = all(np.array_equal(a[k], b[k]) for k in fields + ('status', 'iterations'))
        lines += ['1. Without interactions on one site type (two-site CO2 reduction mechanism, N = 3, S = 3, R = 4; %d .. %d iterations per '
                  'point): `%s` %s, `%s` %s: the general rows cost a factor %.2f.  Results bitwise equal: %s.'
                  % (a['iterations'].min(), a['iterations'].max(), ks.last_kernel, spread(t_kin), ia.last_kernel, spread(t_ia),
                     float(np.median(t_ia)) / float(np.median(t_kin)), 'yes' if equal else 'no'), '']
        print(lines[-2], flush=True)
        weak = IC.case('co2r_two_site_weak').tables
        ramps = (1, 2, 5, 10)
        times, its = {K: [] for K in ramps}, {}
        for r in range(CALLS + WARMUPS):
            for K in ramps:
                out = ia.solve(None, weak, pm, fields=fields, ramp=K, **kw)
                its[K] = out
                if r >= WARMUPS:
                    times[K].append(ia.last_kernel_ms)
        lines += ['2. The same mechanism with 0.3 / 0.15 eV between all adsorbates:', '', '| ramp | kernel | iterations per point (mean / largest) | '
                  'statuses | per further stage beyond two |', '|---|---|---|---|---|']
        t2 = float(np.median(times[2]))
        for K in ramps:
            o = its[K]
            lines.append('| %d | %s | %.0f / %d | %s | %s |' % (K, spread(times[K]), o['iterations'].mean(), o['iterations'].max(),
                                                                ', '.join('%d x %d' % (int((o['status'] == v).sum()), v) for v in np.unique(o['status'])),
                                                                '' if K <= 2 else '%.3f ms' % ((float(np.median(times[K])) - t2) / (K - 2))))
        lines.append('')
        print('\n'.join(lines[-7:]), flush=True)
        ts = IC.case('terrace_step')
        j = np.arange(N_POINTS) % len(ts.phiM)
        t_ts = []
        for r in range(CALLS + WARMUPS):
            out = ia.solve(None, ts.tables, ts.phiM[j], fields=fields, ramp=1, potential_drop='stern', stern_capacitance=ts.kw['CS'],
                           phi_pzc=ts.kw['phi_pzc'], csurf=ts.csurf[j], phi_surface=ts.phi_surface[j])
            if r >= WARMUPS:
                t_ts.append(ia.last_kernel_ms)
        lines += ['3. Terrace and step sites (two site types, N = 3, S = 5, R = 7, one stage; %d .. %d iterations per point, statuses %s): %s.'
                  % (out['iterations'].min(), out['iterations'].max(),
                     ', '.join('%d x %d' % (int((out['status'] == v).sum()), v) for v in np.unique(out['status'])), spread(t_ts)), '']
        print(lines[-2], flush=True)
    with open(path, 'w') as f:
        f.write(head + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
