#!/usr/bin/env python3
"""Transient microkinetics on the device (libcatint_kintrans): what an integration costs and what the divergence of the lanes costs.
One run on one MI355X writes profiles/kintrans_probe.md (or the file given as the first argument); no figure in it is fixed in
advance.  A record, not a gate: nobody has measured this kernel before.

The points are the 39 of the two-site CO2 reduction case of tests/kinetics_cases.py (13 potentials x CO2 at 30, 1e-3 and 0 mol/m^3),
repeated to n = 4096 and n = 32768.  Every point starts from the steady state 0.1 V more negative (catkin_solve on the device) and is
integrated to 1 s with four output times, rtol 1e-4: the potential step.  Recorded per n: catkt_last_kernel_ms (HIP events around the
launch, median / min / max of 5 calls after 1 warm-up), the largest and the mean number of attempted steps and of Newton iterations
per lane -- a wave runs as long as its slowest lane, so largest / mean is what the divergence costs -- and, for scale, the time per
point of the NumPy restatement (tests/kintrans_ref.py) on the host's CPU."""
import os
import sys
import time

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)

CALLS, WARMUPS = 5, 1
T_OUT = (1e-9, 1e-6, 1e-3, 1.0)
RTOL = 1e-4


def main():
    from catint_amd import _kinetics, _kintrans
    from tests import kinetics_cases as KC
    from tests import kintrans_ref as KT
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, 'profiles', 'kintrans_probe.md')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    c = KC.co2r_case('two_site')
    kw = dict(potential_drop='stern', stern_capacitance=c.kw['CS'], phi_pzc=c.kw['phi_pzc'])
    with _kinetics.KineticsSolver(0) as ks:
        before = ks.solve(None, c.tables, c.phiM - 0.1, csurf=c.csurf, phi_surface=c.phi_surface, fields=('theta',), **kw)
    assert (before['status'] == 0).all()
    t0 = time.perf_counter()
    ref = KT.solve(c.tables, c.phiM, c.csurf, c.phi_surface, T_OUT, theta0=before['theta'], rtol=RTOL, **c.kw)
    ref_ms = 1e3 * (time.perf_counter() - t0) / len(c.phiM)
    lines = ['# Transient microkinetics on the device: kernel time and lane divergence (tools/probe/kintrans_probe.py, one MI355X)', '',
             'The %d points of the two-site CO2 reduction case (N = 3 species, S = 3 adsorbates, R = 4 steps) repeated to n, each started from '
             'the steady state 0.1 V more negative and integrated to %g s (%d output times, rtol %g).  Kernel times are HIP events around the '
             'launch (median of %d calls after %d warm-up).  The NumPy restatement takes %.1f ms per point on this host\'s CPU '
             '(%d .. %d accepted steps, %d Newton iterations at most).'
             % (len(c.phiM), T_OUT[-1], len(T_OUT), RTOL, CALLS, WARMUPS, ref_ms, ref['steps'][:, 0].min(), ref['steps'][:, 0].max(), ref['steps'][:, 2].max()),
             '', '| n | kernel | per point | attempted steps per lane (mean / largest) | Newton iterations per lane (mean / largest) | statuses |',
             '|---|---|---|---|---|---|']
    with _kintrans.TransientKinetics(0) as ts:
        for n in (4096, 32768):
            idx = np.arange(n) % len(c.phiM)
            ms = []
            for r in range(CALLS + WARMUPS):
                out = ts.solve(None, c.tables, c.phiM[idx], T_OUT, csurf=c.csurf[idx], phi_surface=c.phi_surface[idx], theta0=before['theta'][idx],
                               rtol=RTOL, fields=('theta', 'flux', 'flux_scale'), **kw)
                if r >= WARMUPS:
                    ms.append(ts.last_kernel_ms)
            att, it = out['steps'][:, :2].sum(axis=1), out['steps'][:, 2]
            same = np.array_equal(out['steps'][:len(c.phiM)], ref['steps'])
            lines.append('| %d | `%s` %.2f ms (min %.2f, max %.2f) | %.3f us | %.0f / %d | %.0f / %d | %s; step counts %s the restatement\'s |'
                         % (n, ts.last_kernel, float(np.median(ms)), min(ms), max(ms), 1e3 * float(np.median(ms)) / n, att.mean(), att.max(), it.mean(),
                            it.max(), ', '.join('%d x %d' % (int((out['status'] == v).sum()), v) for v in np.unique(out['status'])),
                            'equal' if same else 'differ from'))
            print(lines[-1], flush=True)
    with open(path, 'w') as out_file:
        out_file.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
