#!/usr/bin/env python3
"""Mean-field microkinetics on the device (libcatint_kinetics): what the kinetic half of an SCF iteration costs next to the transport
half.  One run on one MI355X writes profiles/kinetics_probe.md (or the file given as the first argument); no figure in it is fixed in
advance.  A record, not a gate: there is no earlier implementation to compare a time against.

One handle of 4096 operating points: the CO2R sweep's species (steric K+), buffer reactions, graded grid and Stern wall at nx = 384,
-0.5 .. -1.4 V, brought to its stationary state first.  On it, with the four-step mechanism of examples/co2r_microkinetic_sweep.py
reading the surface state through the view:
  * catkin::steady_kernel by HIP events around its launch (last_kernel_ms), median / min / max of 5 calls after 1 warm-up, from the
    uniform surface (cold) and from the coverages of the previous call (warm), with and without the sensitivities;
  * the wall time of one warm-started solve_surface on the same batch (the transport half of an SCF iteration).  The energies of
    the example are illustrative and at these potentials ask for more CO2 than diffusion delivers, so the fluxes handed to the
    transport are the model's scaled down to a tenth of the diffusion-limited CO2 flux at most: the solve is timed, not the physics."""
import os
import sys
import time

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, 'examples'))

CALLS, WARMUPS = 5, 1


def main():
    import co2r_microkinetic_sweep as mk
    import co2r_physical_sweep as ex
    from catint_amd.calculator import Calculator
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, 'profiles', 'kinetics_probe.md')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    B, nx = 4096, 384
    tp, phis = ex.build(B, nx, -0.5, -1.4)
    calc = Calculator(transport=tp, calc='comsol')
    tp.newton = {'tol': 1e-8, 'maxit': 80}
    s = calc._physical_solver(B)
    c0 = np.repeat(np.asarray(tp.c0, float)[None, :], B, axis=0)
    status = calc.solve_physical(s, c0, np.asarray(phis, float), np.zeros((B, tp.nspecies)))
    model = mk.model(tp)
    sd = float(tp.system['active site density'])
    lines = ['# Microkinetics on the device: kernel time next to the transport solve (tools/probe/kinetics_probe.py, one MI355X)', '',
             'B = %d operating points (%d with solver status 0), N = %d species, S = 3 adsorbates, R = 4 steps.  Kernel times are HIP events around the '
             'launch (median of %d calls after %d warm-up); the solve is wall time of one call.' % (B, int((status == 0).sum()), tp.nspecies, CALLS, WARMUPS),
             '', '| call | kernel | call wall | Newton iterations (min / median / max) | status 0 |', '|---|---|---|---|---|']
    with s:
        theta = None
        for name, fields, warm in (('cold start, fluxes', None, False), ('warm start, fluxes', None, True),
                                   ('cold start, fluxes and sensitivities', ['theta', 'flux', 'flux_scale', 'dflux_dc', 'dflux_dphi'], False),
                                   ('warm start, fluxes and sensitivities', ['theta', 'flux', 'flux_scale', 'dflux_dc', 'dflux_dphi'], True)):
            ms = []
            for r in range(CALLS + WARMUPS):
                t0 = time.perf_counter()
                out = s.get_kinetics(model, site_density=sd, fields=fields, theta_guess=theta if warm else None)
                wall = 1e3 * (time.perf_counter() - t0)
                if r >= WARMUPS:
                    ms.append(s._kinetics.last_kernel_ms)
            ok = out['status'] == 0
            theta = np.where(ok[:, None], out['theta'], 0.25)
            it = out['iterations'][ok]
            lines.append('| %s: `%s` | %.3f ms (min %.3f, max %.3f) | %.2f ms | %d / %d / %d | %d of %d |'
                         % (name, s._kinetics.last_kernel, float(np.median(ms)), min(ms), max(ms), wall, it.min(), int(np.median(it)), it.max(), int(ok.sum()), B))
            print(lines[-1], flush=True)
        flux = np.where(np.isfinite(out['flux']), out['flux'], 0.0)
        names = list(tp.species.keys())
        limit = 0.1 * tp.D[names.index('CO2')] * float(tp.species['CO2']['bulk_concentration']) / tp.xmesh[-1]
        flux = flux * min(1.0, limit / max(np.abs(flux[:, names.index('CO2')]).max(), 1e-300))
        s.solve_surface(flux)
        s.synchronize()
        t0 = time.perf_counter()
        _, _, _, st = s.solve_surface(flux)
        solve_ms = 1e3 * (time.perf_counter() - t0)
        lines.append('| one warm-started `solve_surface` with these fluxes scaled to 0.1 of the CO2 diffusion limit (%d lanes converged, %d Newton iterations at most) | | %.2f ms | | |'
                     % (int((st == 0).sum()), int(s.newton_iterations().max()), solve_ms))
    with open(path, 'w') as out_file:
        out_file.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
