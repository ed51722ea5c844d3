#!/usr/bin/env python3
"""Mesh continuation and grid transfer on the device, on the CO2R polarization sweep of examples/co2r_physical_sweep.py.

  1. the sweep is solved twice: the default path, and with tp.newton['coarse_nx'] -- the usual path on a coarse graded grid, the
     solution resampled onto the full grid on the device (libcatint_regrid: the Scharfetter-Gummel interpolant, nothing crosses PCIe),
     one direct Newton solve there.  Status, currents, Newton iterations and the time of the transport solves are printed side by side;
  2. the plain interface: PnpSolver.resample (to the host), PnpSolver.resample_to (handle to handle on the device).

    python examples/mesh_continuation.py --lanes 256 --nx 384 --coarse-nx 130
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from catint_amd.calculator import Calculator      # noqa: E402
from catint_amd.host import graded_mesh           # noqa: E402
from catint_amd.units import unit_F               # noqa: E402
import co2r_physical_sweep as ex                  # noqa: E402


def sweep(lanes, nx, **newton):
    tp, phis = ex.build(lanes, nx)
    calc = Calculator(transport=tp, calc='comsol')
    tp.newton = dict({'tol': 1e-8, 'maxit': 80}, **newton)
    calc.set_surface_kinetics([{'species': 'CO2', 'rate': ex.tafel_rate(tp), 'stoichiometry': {'CO2': -1.0, 'CO': 1.0, 'OH-': 2.0}}])
    calc.run()
    names = list(tp.species.keys())
    return tp, calc, phis, calc.kinetic_flux[:, names.index('CO')] * 2 * unit_F / 10.0       # mA/cm^2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lanes', type=int, default=256)
    ap.add_argument('--nx', type=int, default=384)
    ap.add_argument('--coarse-nx', type=int, default=130)
    a = ap.parse_args()
    sweep(min(a.lanes, 8), a.nx, coarse_nx=a.coarse_nx)          # (loads the code objects: the times below are of warm runs)
    _, ref, phis, j_ref = sweep(a.lanes, a.nx)
    tp, calc, _, j = sweep(a.lanes, a.nx, coarse_nx=a.coarse_nx)
    print('%d lanes x %d species x %d points' % (a.lanes, tp.nspecies, tp.nx))
    print('  default path:       %d converged, %6d Newton iterations, %.3f s in the transport solves'
          % ((ref.status == 0).sum(), ref.newton_iterations_total, ref.solve_seconds))
    print('  coarse_nx = %-6d   %d converged, %6d Newton iterations on both grids, %.3f s   %s'
          % (a.coarse_nx, (calc.status == 0).sum(), calc.newton_iterations_total, calc.solve_seconds, calc.mesh_continuation))
    print('  max |j_CO - j_CO(default)| / |j_CO| = %.2e' % (np.abs(j - j_ref) / np.abs(j_ref)).max())

    # the interface underneath: a solved handle resampled onto a finer grid, to the host and into another handle
    with calc._physical_solver(4) as coarse, calc._physical_solver(4, xmesh=graded_mesh(tp.xmesh[-1], tp.xmesh[1] / 2.0, 2 * tp.nx)) as fine:
        c0 = np.repeat(tp.c0[None, :], 4, axis=0)
        st = calc.solve_physical(coarse, c0, phis[:4], np.zeros((4, tp.nspecies)))
        c, phi = coarse.resample(fine.grid)                       # [4][N][2 nx], [4][2 nx] on the host
        pb = np.zeros((4, 4))
        pb[:, 0] = phis[:4]
        fine.set_batch(np.ones((4, tp.nspecies, 2 * tp.nx)), pb, np.zeros(4), np.zeros((4, tp.nspecies)))
        calc._apply_surface_kinetics(fine, phis[:4])
        coarse.resample_to(fine)                                  # the same values, from device to device
        cf, pf = fine.get_state(derived=False)
        print('resample: status %s; resample_to == resample to the bit: %s; kernel %s, %.3f ms'
              % (st.tolist(), bool(np.array_equal(cf, c) and np.array_equal(pf, phi)), coarse._regridder.last_kernel,
                 coarse._regridder.last_kernel_ms))
        st = fine.solve_stationary()
        print('the fine grid from the resampled solution: status %s, Newton iterations %s' % (st.tolist(), fine.newton_iterations().tolist()))


if __name__ == '__main__':
    main()
