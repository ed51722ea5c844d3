#!/usr/bin/env python3
"""The CO2 reduction system of examples/co2r_inputs.py with a mean-field microkinetic model of the electrode in the place of the
analytic rate law: the self-consistency loop of the reference (kinetics <-> transport), the kinetic half solved on the device for every
voltage of the sweep at once (include/catint_kinetics.h, Calculator.set_microkinetics).

Mechanism (one site type, adsorbed intermediates compete for the sites):
    CO2 + *            <-> CO2*
    CO2* + H2O + e-    <-> COOH* + OH-
    COOH* + e-         <-> [COOH-e]  <-> CO* + OH-          (transition state, beta = 0.5)
    CO*                <-> CO + *
The free energies (eV, with a linear and a quadratic dependence on the surface charge in micro C/cm^2) are ILLUSTRATIVE numbers; they
are not fitted to any surface.  With every site of tp.system['active site density'] active they ask for 400 - 1200 mA/cm^2 between
-0.6 and -1.2 V, far beyond the 16 mA/cm^2 that diffusion of CO2 delivers here, and the SCF loop then finds no fixed point with
positive concentrations (--site-fraction 1: 0 of 16 lanes converged in 2000 iterations on an MI355X).  The default takes one site in a
thousand as active: 16 of 16 lanes converge in 47 SCF iterations, j_CO rises from 0.33 to 0.84 mA/cm^2 and falls again beyond -1.12 V
as the surface CO2 concentration drops from 5.7 to 0.14 mol/m^3 and CO* gives way to free sites (same machine, --lanes 16).

    python examples/co2r_microkinetic_sweep.py --lanes 16
    python examples/co2r_microkinetic_sweep.py --lanes 16 --newton
    python examples/co2r_microkinetic_sweep.py --lanes 16 --device-loop

--newton: the same fixed point by a Newton iteration on the wall fluxes (Calculator.set_microkinetics(..., scf='newton'),
include/catint_couple.h) in the place of the mixing loop: a handful of transport solves instead of one per mixing iteration.  The
figures of both are in profiles/couple_probe.md.

--device-loop: the mixing loop itself on the device (Calculator.set_microkinetics(..., device_loop=True), include/catint_scfkin.h):
after the first host iterations the kinetics run between the loop's bookkeeping and its transport solve with no host round trip per
iteration; the same iterates as the default.  The figures of both are in profiles/scfkin_probe.md.

--rate-control: after the loop, the degree of rate control of the CO flux at the final surface state of every voltage
(include/catint_drc.h, Calculator.set_microkinetics(..., rate_control=True)): per potential the step whose transition state and the
intermediate whose free energy control the flux most, with Campbell's coefficient -- intrinsic (fixed surface state) and, with --newton,
apparent (the coupled electrode: mass transport of CO2 takes its share of the control, so the apparent coefficients lie below the
intrinsic ones; on an MI355X with --lanes 16 --newton: step 2 0.50 intrinsic, 0.43 apparent, CO2* 1.00 and 0.86).

--interactions EV: the same mechanism with a CO self-interaction of EV eV per unit coverage (catint_amd.interactions.InteractingModel,
include/catint_interact.h): the binding energy of CO rises with its own coverage, the first SCF iteration ramps the interaction in ten
stages inside one launch (the reference's n_inter), later iterations warm-start at full strength.  Works with the default loop and
with --newton; the device-loop library is mean-field and refuses such a model, and so does the calculator's own rate_control option.

--interactions EV --rate-control: after the loop, one call of catint_amd.iacontrol.InteractingRateControl.solve
(include/catint_iacontrol.h) at the final surface concentrations, surface potentials and coverages of every voltage: the intrinsic
degree of rate control with the coverage dependence of the CO binding energy in the Jacobian, and the share of the CO flux that is owed
to the interaction (strength_control; on an MI355X with --lanes 16 --newton --interactions 0.3: step 2 0.50, CO2* 0.99 to 1.00, and
+0.020 of the CO flux at -0.6 V falling to +0.002 at -1.2 V as the CO coverage falls from 0.054 to 0.014).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from catint_amd.calculator import Calculator          # noqa: E402
from catint_amd.microkinetics import MeanFieldModel   # noqa: E402
from catint_amd.units import unit_F                   # noqa: E402
import co2r_physical_sweep                             # noqa: E402  (the transport of the sweep)

ADSORBATES = {'CO2': 1, 'COOH': 1, 'CO': 1}
STEPS = ['CO2_g + *_t <-> CO2*_t',
         'CO2*_t + H2O_g + ele_g <-> COOH*_t + OH_g',
         'COOH*_t + ele_g <-> COOH-ele_t <-> CO*_t + OH_g; beta=0.5',
         'CO*_t <-> CO_g + *_t']
ENERGIES = {'CO2': (0.42, 0.015, 1.0e-4), 'COOH': (0.55, 0.010, 0.0), 'CO': (0.15, 0.002, 0.0), 'COOH-ele': (1.05, 0.010, 0.0)}


def model(tp, co_self_interaction=None):
    if co_self_interaction is not None:
        from catint_amd.interactions import InteractingModel
        return InteractingModel(list(tp.species.keys()), {a: ('t', n) for a, n in ADSORBATES.items()}, STEPS, ENERGIES,
                                interactions={('CO', 'CO'): co_self_interaction},
                                solution={'CO2_g': 'CO2', 'CO_g': 'CO', 'OH_g': 'OH-', 'H2O_g': None}, solution_energies={'CO': 0.30},
                                temperature=tp.system['temperature'])
    return MeanFieldModel(list(tp.species.keys()), ADSORBATES, STEPS, ENERGIES, solution={'CO2_g': 'CO2', 'CO_g': 'CO', 'OH_g': 'OH-', 'H2O_g': None},
                          solution_energies={'CO': 0.30}, temperature=tp.system['temperature'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lanes', type=int, default=16)
    ap.add_argument('--nx', type=int, default=192)
    ap.add_argument('--phimin', type=float, default=-0.6)
    ap.add_argument('--phimax', type=float, default=-1.2)
    ap.add_argument('--site-fraction', type=float, default=1e-3, help='fraction of the active site density that takes part')
    ap.add_argument('--max-iter', type=int, default=2000)
    ap.add_argument('--newton', action='store_true', help='Newton iteration on the wall fluxes instead of the mixing loop')
    ap.add_argument('--device-loop', action='store_true', help='the mixing loop on the device, no host round trip per iteration')
    ap.add_argument('--rate-control', action='store_true', help='degree of rate control of the CO flux at the final state of every lane')
    ap.add_argument('--interactions', type=float, default=None, metavar='EV', help='CO self-interaction in eV per unit coverage')
    a = ap.parse_args()
    if a.interactions is not None and a.device_loop:
        ap.error('--device-loop works on the mean-field model: it excludes --interactions')
    if a.newton and a.device_loop:
        ap.error('--device-loop is the mixing loop on the device: it excludes --newton')
    tp, phis = co2r_physical_sweep.build(a.lanes, a.nx, a.phimin, a.phimax)
    tp.newton = {'tol': 1e-8, 'maxit': 80}
    calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-4, mix_scf=0.1)
    site_density = a.site_fraction * float(tp.system['active site density'])
    interacting = a.interactions is not None
    calc.set_microkinetics(model(tp, a.interactions), site_density=site_density, potential_drop='stern',
                          scf='newton' if a.newton else 'mixing', rate_control=a.rate_control and not interacting, device_loop=a.device_loop)
    names = list(tp.species.keys())
    t0 = time.time()
    out = calc.run_scf_cycle(nel=[2.0 if sp == 'CO' else 1.0 for sp in names], max_iter=a.max_iter)
    # (the mixing loop makes one transport solve per iteration)
    print('%d lanes: %d %s, %d transport solves, %d converged, %d failed, %.2f s'
          % (a.lanes, out['iterations'], 'Newton steps' if a.newton else 'SCF iterations', out.get('transport_solves', out['iterations']),
             out['converged'].sum(), out['failed'].sum(), time.time() - t0))
    iCO, iCO2 = names.index('CO'), names.index('CO2')
    print('phiM [V]   j_CO [mA/cm2]   digits   c_CO2(0)   theta_*    theta_CO2   theta_COOH   theta_CO')
    for i in range(a.lanes):
        # the number of digits of a flux is what flux / flux_scale leaves of 16
        with np.errstate(divide='ignore'):
            digits = 16.0 + np.log10(abs(out['flux'][i, iCO]) / out['flux_scale'][i, iCO])
        print('%7.3f   %12.5e   %6.1f   %8.4f   %s' % (phis[i], out['flux'][i, iCO] * 2 * unit_F / 10.0, digits, out['surface_concentration'][i, iCO2],
                                                     '   '.join('%9.3e' % v for v in out['coverage'][i])))
    if a.rate_control and interacting:
        # the calculator's rate_control option is mean-field: one call on the host-surface path at the state the loop ended with
        from catint_amd.iacontrol import InteractingRateControl
        ads = list(ADSORBATES)
        vs = np.array([tp.alldata[i]['system']['surface_potential'] for i in range(a.lanes)])
        tables = dict(model(tp, a.interactions).tables(), site_density=site_density)
        with InteractingRateControl() as irc:
            rc = irc.solve(None, tables, phis, out['coverage'], csurf=out['surface_concentration'], phi_surface=vs, potential_drop='stern',
                           stern_capacitance=float(tp.system.get('Stern capacitance', 0.0)) * 1e-2, phi_pzc=float(tp.system.get('phiPZC', 0.0)),
                           fields=('drc', 'tdrc', 'strength_control'), residual_tol=1e-3)
        print('degree of rate control of the CO flux with the CO self-interaction in the Jacobian: controlling step (X_rc), intermediate '
              '(X_trc) and the share of the flux owed to the interaction')
        for i in range(a.lanes):
            r, s = int(np.argmax(np.nan_to_num(np.abs(rc['drc'][i][:, iCO])))), int(np.argmax(np.nan_to_num(np.abs(rc['tdrc'][i][:, iCO]))))
            print('%7.3f   status %d   step %d %+.3f, %s* %+.3f, interaction %+.3f' % (phis[i], rc['status'][i], r + 1, rc['drc'][i][r, iCO], ads[s],
                                                                                      rc['tdrc'][i][s, iCO], rc['strength_control'][i, iCO]))
    elif a.rate_control:
        rc = out['rate_control']
        ads = list(ADSORBATES)
        kinds = [('intrinsic', 'drc', 'tdrc')] + ([('apparent', 'drc_apparent', 'tdrc_apparent')] if a.newton else [])
        print('degree of rate control of the CO flux: controlling step (X_rc) and intermediate (X_trc)')
        for i in range(a.lanes):
            parts = []
            for label, x, xt in kinds:
                r, s = int(np.argmax(np.nan_to_num(np.abs(rc[x][i][:, iCO])))), int(np.argmax(np.nan_to_num(np.abs(rc[xt][i][:, iCO]))))
                parts.append('%s: step %d %+.3f, %s* %+.3f' % (label, r + 1, rc[x][i][r, iCO], ads[s], rc[xt][i][s, iCO]))
            print('%7.3f   status %d   %s' % (phis[i], rc['status'][i], '   '.join(parts)))


if __name__ == '__main__':
    main()
