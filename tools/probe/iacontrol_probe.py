#!/usr/bin/env python3
"""Degree of rate control of interacting adsorbates on the device (libcatint_iacontrol): what one call with all families costs, next to
the mean-field kernel on the same mechanism without interactions and next to what finite differences would cost.  One run on one MI355X
writes profiles/iacontrol_probe.md (or the file given as the first argument) below the marker line, keeping what stands above it; no
figure in it is fixed in advance.  A record, not a gate: nobody has measured this kernel before.

The points are the 39 of the CO2 reduction lattice of tests/kinetics_cases.py (13 potentials x CO2 at 30, 1e-3 and 0 mol/m^3) repeated
to n = 4096, the mechanism the two-site one (N = 3, S = 3, R = 4) with the weak interaction of tests/interact_cases.py (0.3 eV self,
0.15 eV cross).  Kernel times are <prefix>last_kernel_ms (HIP events around the launch, without the copies): the median, smallest and
largest of CALLS rounds after WARMUPS warm-up rounds, the three measurements alternating round by round in one process.
  1. catic_solve, every field, at the coverages catia_solve returned with the case's ramp.
  2. catdrc_solve, every field, on the same mechanism without interactions at the coverages of catkin_solve (libcatint_drc is unchanged by
     this library: its code object is the parent commit's, profiles/iacontrol_probe.md lists the hashes).
  3. 3 R + S + 1 calls of catia_solve with the case's ramp from the uniform start, their kernel times summed: one ramped re-solve per
     energy, what central differences would cost with ONE-sided differences (CatMAP's method; central ones cost twice that).  The calls
     are the unperturbed solve repeated: a shift of one energy by a difference step does not change the iteration count."""
import os
import sys

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)

CALLS, WARMUPS, N_POINTS = 7, 2, 4096
MARKER = '<!-- below this line: written by tools/probe/iacontrol_probe.py -->'


def spread(v):
    return '%.3f ms (min %.3f, max %.3f)' % (float(np.median(v)), min(v), max(v))


def main():
    from catint_amd import _drc, _interact, _kinetics, iacontrol
    from tests import interact_cases as IC
    from tests import kinetics_cases as KC
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, 'profiles', 'iacontrol_probe.md')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    head = ''
    if os.path.exists(path):
        text = open(path).read()
        head = text[:text.index(MARKER)] if MARKER in text else text
    c = IC.case('co2r_two_site_weak')
    mf = KC.co2r_case('two_site')
    idx = np.arange(N_POINTS) % len(c.phiM)
    pm, cs, ps = c.phiM[idx], c.csurf[idx], c.phi_surface[idx]
    kw = dict(potential_drop='stern', stern_capacitance=c.kw['CS'], phi_pzc=c.kw['phi_pzc'], csurf=cs, phi_surface=ps)
    n_rates, T = np.asarray(c.tables['order_f']).shape[0], len(c.tables['site_count'])
    columns = 3 * n_rates + (T - 1) + 1
    with _kinetics.KineticsSolver(0) as ks, _interact.InteractingKinetics(0) as ia, _drc.RateControl(0) as old, \
            iacontrol.InteractingRateControl(0) as new:
        state = ia.solve(None, c.tables, pm, fields=('theta',), ramp=c.ramp, **kw)
        state_mf = ks.solve(None, mf.tables, pm, fields=('theta',), **kw)
        assert (state['status'] == 0).all() and (state_mf['status'] == 0).all()
        t_new, t_old, t_fd = [], [], []
        for r in range(CALLS + WARMUPS):
            a = new.solve(None, c.tables, pm, state['theta'], fields=list(iacontrol.FIELDS), **kw)
            t_a = new.last_kernel_ms
            b = old.solve(None, mf.tables, pm, state_mf['theta'], fields=list(_drc.FIELDS), **kw)
            t_b = old.last_kernel_ms
            t_c = 0.0
            for _ in range(columns):
                ia.solve(None, c.tables, pm, fields=('flux',), ramp=c.ramp, **kw)
                t_c += ia.last_kernel_ms
            if r >= WARMUPS:
                t_new.append(t_a), t_old.append(t_b), t_fd.append(t_c)
        assert (a['status'] == 0).all() and (b['status'] == 0).all()
        m_new, m_old, m_fd = (float(np.median(v)) for v in (t_new, t_old, t_fd))
        lines = [MARKER, '', '## Kernel times (%d points, median of %d rounds after %d warm-up rounds, the three alternating)' % (N_POINTS, CALLS, WARMUPS),
                 '', 'Two-site CO2 reduction mechanism, N = 3, S = 3, R = 4; %d columns (3 R + S + 1) with the weak interaction, %d without.' %
                 (columns, columns - 1), '',
                 '| what | kernel | time |', '|---|---|---|',
                 '| all families with interactions | `%s` | %s |' % (new.last_kernel, spread(t_new)),
                 '| all families, mean field, no interactions | `%s` | %s |' % (old.last_kernel, spread(t_old)),
                 '| %d ramped solves (ramp %d), summed | `%s` | %s |' % (columns, c.ramp, ia.last_kernel, spread(t_fd)), '',
                 'The general rows and the strength column cost a factor %.2f over the mean-field kernel; one launch replaces one-sided finite '
                 'differences that cost %.1f times as much kernel time (central differences: %.1f times).' % (m_new / m_old, m_fd / m_new, 2.0 * m_fd / m_new),
                 'Largest residual of the states: %.1e (with interactions), %.1e (mean field).' % (a['residual'].max(), b['residual'].max()), '']
        print('\n'.join(lines), flush=True)
    with open(path, 'w') as f:
        f.write(head + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
