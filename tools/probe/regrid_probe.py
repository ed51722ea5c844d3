#!/usr/bin/env python3
"""Grid transfer on the device (libcatint_regrid): what it costs and what it buys.  One run writes profiles/regrid_probe.jsonl (or the
file given as the first argument); no figure in it is fixed in advance.

  * kernel: time of catgrid::regrid_kernel by HIP events around its launch, median / min / max of 11 launches after 2 warm-ups, at
    4096 x 7 x 384 -> 768 (the CO2R sweep's species, steric K+, graded grids) and at 8192 x 8 x 512 -> 4096 (point ions).  Bytes:
    every source row once (species rows twice with steric ions), every result row written at its pitch.  Yardstick: the same bytes at
    the device-to-device copy rate README.md quotes for this pool (0.53 - 0.61 of 8 TB/s);
  * host path: wall time of get_state + the np.interp loop + set_lanes -- the mesh rung of the rerun ladder without
    tp.newton['regrid_on_device'] -- on the same arrays, measured on the first lanes of the batch and scaled (the part is recorded);
  * warm start: Newton iterations of a 130-point solve from the bulk state and from the resampled 66-point solution
    (tests/test_gpu_regrid.py: warm_start_counts);
  * mesh continuation: Newton iterations and wall time of the transport solves of the CO2R sweep (examples/co2r_physical_sweep.py)
    with tp.newton['coarse_nx'] against the default path, second run of each (the first loads the code objects)."""
import json
import os
import sys
import time

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, 'examples'))

from catint_amd import PnpSolver, _regrid
from catint_amd.host import graded_mesh
from catint_amd.units import unit_F, unit_R, unit_eps0

HBM_PEAK = 8.0e12
D2D_SHARE = (0.53, 0.61)          # README.md: a plain device-to-device copy on this pool, as a share of 8 TB/s
BETA = 1.0 / (unit_R * 298.15)
EPS = 78.36 * unit_eps0
LAUNCHES, WARMUPS = 11, 2


def state(B, N, nx, tile=512):
    rng = np.random.RandomState(7)
    b = min(B, tile)
    s = np.linspace(0.0, 1.0, nx)
    c = 10.0 * (1.0 + np.arange(N))[None, :, None] * np.exp(0.5 * np.sin(2 * np.pi * rng.uniform(0.5, 3.0, (b, N, 1)) * s + rng.uniform(0, 6.28, (b, N, 1))))
    phi = np.cumsum(rng.uniform(0.005, 0.015, (b, nx)) * rng.choice([-1.0, 1.0], (b, nx)), axis=1)
    reps = (B + b - 1) // b
    return np.ascontiguousarray(np.tile(c, (reps, 1, 1))[:B]), np.ascontiguousarray(np.tile(phi, (reps, 1))[:B])


def kernel_record(B, N, nx, nxt, out, co2r):
    if co2r:
        import co2r_physical_sweep as ex
        tp, _ = ex.build(4, nx)
        names = list(tp.species.keys())
        D, q, x, beta = np.asarray(tp.D, float), np.asarray(tp.charges, float), np.asarray(tp.xmesh, float), float(tp.beta)
        radii = np.array([float(tp.species[sp].get('MPB_radius', 0.0)) for sp in names])
        N = len(D)
    else:
        z = np.array([1, -1, 2, -1, 0, 1, -2, -1][:N], float)
        D, q, radii, beta = 1e-9 * (1.0 + 0.3 * np.arange(N)), z * unit_F, None, BETA
        x = graded_mesh(8e-5, 5e-11, nx)
    # the target: the source grid refined evenly in its index (a graded mesh of nxt points with the same first spacing and ends)
    xt = np.interp(np.linspace(0.0, nx - 1.0, nxt), np.arange(nx), x) if not co2r else graded_mesh(x[-1], x[1] - x[0], nxt)
    xt[-1] = x[-1]
    steric = radii is not None and bool(np.any(radii))
    c, phi = state(B, N, nx)
    pitch = _regrid.row_pitch(nxt)
    with PnpSolver(N, nx, float(x[1] - x[0]), 1.0, beta, EPS, D, q, method='Newton', batch_capacity=B) as s, _regrid.Regridder(0) as rg:
        s.set_newton(wall_bc='stern', stern_capacitance=0.2, mpb_radius=radii if steric else None)
        s.set_grid(x)
        s.set_batch(c, np.zeros((B, 4)), np.zeros(B), np.zeros((B, N)))
        s.set_potential(phi)
        view = s.device_view()
        kms = []
        for r in range(LAUNCHES + WARMUPS):
            rg.resample(view, D, q, x, beta, xt, mpb_radius=radii, to_host=False, device=True)
            if r >= WARMUPS:
                kms.append(rg.last_kernel_ms)
        kernel = rg.last_kernel
        # the host path on the first nb lanes: get_state, the np.interp loop, set_lanes into a handle of the target grid
        nb = min(B, 256)
        with PnpSolver(N, nx, float(x[1] - x[0]), 1.0, beta, EPS, D, q, method='Newton', batch_capacity=nb) as a, \
                PnpSolver(N, nxt, float(xt[1] - xt[0]), 1.0, beta, EPS, D, q, method='Newton', batch_capacity=nb) as t:
            for h, g, n in ((a, x, nx), (t, xt, nxt)):
                h.set_newton(wall_bc='stern', stern_capacitance=0.2, mpb_radius=radii if steric else None)
                h.set_grid(g)
                h.set_batch(np.ones((nb, N, n)), np.zeros((nb, 4)), np.zeros(nb), np.zeros((nb, N)))
            a.set_lanes(np.arange(nb), c[:nb], phi[:nb])
            host_s, dev_s = [], []
            for r in range(3):
                t0 = time.perf_counter()
                cs, ps = a.get_state()[:2]
                cs = np.stack([[np.interp(xt, x, row) for row in lane] for lane in cs])
                ps = np.stack([np.interp(xt, x, row) for row in ps])
                t.set_lanes(np.arange(nb), cs, ps)
                host_s.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                a.resample_to(t)
                dev_s.append(time.perf_counter() - t0)
    read = B * (N * (2 if steric else 1) + 1) * nx * 8
    written = B * (N + 1) * pitch * 8
    k = float(np.median(kms)) * 1e-3
    rec = {'probe': 'catgrid_resample', 'B': B, 'N': N, 'nx': nx, 'nx_target': nxt, 'steric': steric, 'kernel': kernel, 'launches': len(kms),
           'kernel_ms': round(float(np.median(kms)), 4), 'kernel_ms_min': round(float(np.min(kms)), 4), 'kernel_ms_max': round(float(np.max(kms)), 4),
           'bytes_read': read, 'bytes_written': written, 'kernel_bytes_per_s': round((read + written) / k, 0),
           'fraction_of_8TBps': round((read + written) / k / HBM_PEAK, 4),
           'yardstick_d2d_copy_ms': [round((read + written) / (f * HBM_PEAK) * 1e3, 4) for f in D2D_SHARE[::-1]],
           'host_path_lanes': nb, 'host_path_seconds': round(float(np.median(host_s)), 4),
           'host_path_seconds_scaled_to_B': round(float(np.median(host_s)) * B / nb, 3),
           'resample_to_seconds_same_lanes': round(float(np.median(dev_s)), 5)}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + '\n')
    out.flush()


def warm_start_record(out):
    from tests import test_gpu_regrid as T
    x = graded_mesh(T.LENGTH, T.DEBYE / 10.0, 66)
    with T.binary(x) as src:
        st = src.solve_stationary()
        it_coarse = src.newton_iterations()
        (st_cold, it_cold, c_cold, _), (st_warm, it_warm, c_warm, _) = T.warm_start_counts(src, x)
    rec = {'probe': 'warm_start', 'lanes': len(T.PHIM), 'phiM_minus_phiPZC': T.PHIM.tolist(), 'nx_coarse': 66, 'nx_fine': 130,
           'converged': bool((st == 0).all() and (st_cold == 0).all() and (st_warm == 0).all()),
           'newton_iterations_coarse_66': int(it_coarse.sum()), 'newton_iterations_fine_from_bulk': int(it_cold.sum()),
           'newton_iterations_fine_from_resampled': int(it_warm.sum()),
           'end_states_max_relative_difference': float((np.abs(c_warm - c_cold) / np.abs(c_cold)).max())}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + '\n')


def continuation_record(out, lanes, nx, coarse_nx):
    import co2r_physical_sweep as ex
    from catint_amd.calculator import Calculator
    res = {}
    for name, extra in (('default', {}), ('coarse', {'coarse_nx': coarse_nx})):
        for rep in range(2):
            tp, phis = ex.build(lanes, nx)
            calc = Calculator(transport=tp, calc='comsol')
            tp.newton = dict({'tol': 1e-8, 'maxit': 80}, **extra)
            calc.set_surface_kinetics([{'species': 'CO2', 'rate': ex.tafel_rate(tp), 'stoichiometry': {'CO2': -1.0, 'CO': 1.0, 'OH-': 2.0}}])
            calc.run()
            names = list(tp.species.keys())
            res[name] = (calc.solve_seconds, calc.newton_iterations_total, calc.newton_iterations_slowest, int((calc.status == 0).sum()),
                         np.array(calc.kinetic_flux)[:, names.index('CO')])
    j0, j1 = res['default'][4], res['coarse'][4]
    rec = {'probe': 'mesh_continuation', 'workload': 'examples/co2r_physical_sweep.py', 'lanes': lanes, 'nx': nx, 'coarse_nx': coarse_nx,
           'default_solve_seconds': round(res['default'][0], 4), 'coarse_solve_seconds': round(res['coarse'][0], 4),
           'default_newton_iterations': res['default'][1], 'coarse_newton_iterations_both_grids': res['coarse'][1],
           'default_newton_iterations_slowest_lane': res['default'][2], 'coarse_newton_iterations_slowest_lane_both_grids': res['coarse'][2],
           'default_converged': res['default'][3], 'coarse_converged': res['coarse'][3],
           'max_relative_difference_of_j_CO': float((np.abs(j1 - j0) / np.abs(j0)).max())}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + '\n')


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, 'profiles', 'regrid_probe.jsonl')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as out:
        kernel_record(4096, 7, 384, 768, out, co2r=True)
        kernel_record(8192, 8, 512, 4096, out, co2r=False)
        warm_start_record(out)
        continuation_record(out, 4096, 384, 130)
        continuation_record(out, 256, 1000, 258)


if __name__ == '__main__':
    main()
