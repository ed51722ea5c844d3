#!/usr/bin/env python3
"""How the surface gets to its steady state after a potential step: the coverages of the microkinetic model of
examples/co2r_microkinetic_sweep.py integrated in time on the device (include/catint_kintrans.h, PnpSolver.get_kinetics_transient),
every target potential of the sweep at once, each with its own step size.

The electrode rests at --from, where the coverages are the steady state (PnpSolver.get_kinetics).  At t = 0 the potential steps to each
of the --lanes potentials between --phimin and --phimax.  The double layer follows within nanoseconds, so the surface state the
kinetics see is the stationary, flux-free one of the new potential (one transport solve per lane, held fixed: depletion of CO2 by the
reaction is the business of the SCF loop, not of this example); the coverages start from those of the old potential and relax.  Printed
per potential: t against the coverages and the CO current density, the scaled steady residual (drift) and the number of steps the
lane took.  The energies are illustrative numbers, as in the sweep.

    python examples/coverage_relaxation.py --lanes 4
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from catint_amd.calculator import Calculator          # noqa: E402
from catint_amd.units import unit_F                   # noqa: E402
import co2r_microkinetic_sweep as mk                   # noqa: E402  (the mechanism)
import co2r_physical_sweep                             # noqa: E402  (the transport of the sweep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lanes', type=int, default=4)
    ap.add_argument('--nx', type=int, default=192)
    ap.add_argument('--from', dest='start', type=float, default=-0.5, help='the potential the electrode rests at before the step [V]')
    ap.add_argument('--phimin', type=float, default=-0.6)
    ap.add_argument('--phimax', type=float, default=-1.2)
    ap.add_argument('--site-fraction', type=float, default=1e-3, help='fraction of the active site density that takes part')
    ap.add_argument('--rtol', type=float, default=1e-4)
    ap.add_argument('--decades', type=int, nargs=2, default=(-12, 0), help='first and last output time as powers of ten [s]')
    a = ap.parse_args()
    tp, phis = co2r_physical_sweep.build(a.lanes, a.nx, a.phimin, a.phimax)
    tp.newton = {'tol': 1e-8, 'maxit': 80}
    calc = Calculator(transport=tp, calc='comsol')
    B, names = a.lanes, list(tp.species.keys())
    model = mk.model(tp)
    sd = a.site_fraction * float(tp.system['active site density'])
    t_out = 10.0 ** np.arange(a.decades[0], a.decades[1] + 1)
    s = calc._physical_solver(B)
    with s:
        c0 = np.repeat(np.asarray(tp.c0, float)[None, :], B, axis=0)
        status = calc.solve_physical(s, c0, np.asarray(phis, float), np.zeros((B, tp.nspecies)))
        if (status != 0).any():
            sys.exit('the transport solve failed in lanes %s' % np.flatnonzero(status != 0).tolist())
        before = s.get_kinetics(model, phiM=np.full(B, a.start), site_density=sd, fields=('theta',))
        if (before['status'] != 0).any():
            sys.exit('no steady state at %.3f V (status %s)' % (a.start, before['status'].tolist()))
        out = s.get_kinetics_transient(model, t_out, theta0=before['theta'], rtol=a.rtol, steady_tol=1e-10, site_density=sd)
        kernel, ms = s._transient.last_kernel, s._transient.last_kernel_ms
    iCO = names.index('CO')
    tried = out['steps'][:, :2].sum(axis=1)
    print('%d potentials, step from %.3f V: %s %.3f ms; steps per lane %d .. %d' % (B, a.start, kernel, ms, tried.min(), tried.max()))
    what = {0: 'reached the last output time', 1: 'stationary at t = %.3e s', 2: 'bad input', 3: 'out of steps at t = %.3e s'}
    for i in range(B):
        st = int(out['status'][i])
        print('\nphiM = %.3f V: %s (%d accepted, %d rejected steps, %d Newton iterations)'
              % (phis[i], what[st] % out['t_reached'][i] if '%' in what[st] else what[st], *out['steps'][i]))
        print('    t [s]      theta_*     theta_CO2   theta_COOH  theta_CO    j_CO [mA/cm2]   drift')
        for k, t in enumerate(t_out):
            print('  %9.1e   %s   %12.5e   %8.1e' % (t, '   '.join('%9.3e' % v for v in out['theta'][i, k]),
                                                     out['flux'][i, k, iCO] * 2 * unit_F / 10.0, out['drift'][i, k]))


if __name__ == '__main__':
    main()
