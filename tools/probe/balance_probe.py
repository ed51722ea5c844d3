#!/usr/bin/env python3
"""Species fluxes, reaction rates and the mass balance on the device (libcatint_balance): time of catbal::species_kernel by HIP events
around its launch, after warm-up, median / min / max of 11 launches, at 4096 x 7 x 384 with the CO2R reaction table and one wall
reaction (the sweep of examples/co2r_physical_sweep.py) and at 32 768 x 8 x 512 without reactions, each with all rows and with the
scalars and wall rates only.  The same record carries two yardsticks: catobs::electrolyte_kernel's time on the same state with the
same choice of outputs (a kernel that reads the same rows), and the wall time of the NumPy restatement of tests/test_gpu_balance.py
on the same arrays (the host alternative; at 32 768 operating points on the first 2048 of them, scaled -- its temporaries would not
fit otherwise -- with the measured part recorded next to the scaled figure).

One run writes profiles/balance_probe.jsonl (or the file given as the first argument).  The states are arbitrary (smooth
concentrations, a random-walk potential): the kernel's work does not depend on the values.
Bytes: every species row once for the fluxes (twice with steric ions: pass 0), the potential row once, every participant row of
every reaction once (from L2), the rate rows written and read back once per participating species, plus every row written."""
import json
import os
import sys
import time

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, 'examples'))

from catint_amd import PnpSolver, _balance
from catint_amd.units import unit_F, unit_R, unit_eps0

HBM_PEAK = 8.0e12
BETA = 1.0 / (unit_R * 298.15)
EPS = 78.36 * unit_eps0
LAUNCHES = 11


def state(B, N, nx, tile=512):
    rng = np.random.RandomState(7)
    b = min(B, tile)
    s = np.linspace(0.0, 1.0, nx)
    c = 10.0 * (1.0 + np.arange(N))[None, :, None] * np.exp(0.5 * np.sin(2 * np.pi * rng.uniform(0.5, 3.0, (b, N, 1)) * s + rng.uniform(0, 6.28, (b, N, 1))))
    phi = np.cumsum(rng.uniform(0.005, 0.015, (b, nx)) * rng.choice([-1.0, 1.0], (b, nx)), axis=1)
    reps = (B + b - 1) // b
    return np.ascontiguousarray(np.tile(c, (reps, 1, 1))[:B]), np.ascontiguousarray(np.tile(phi, (reps, 1))[:B])


def co2r_problem(nx):
    """D, charges, radii, grid, reaction table and wall table of the CO2R sweep (examples/co2r_physical_sweep.py)."""
    import co2r_physical_sweep as ex
    tp, _ = ex.build(4, nx)
    names = list(tp.species.keys())
    radii = np.array([float(tp.species[sp].get('MPB_radius', 0.0)) for sp in names])
    table = [([names.index(x) for x in rx['reactants'][0] if x in names], [names.index(x) for x in rx['reactants'][1] if x in names],
              float(rx['rates'][0]), float(rx['rates'][1])) for rx in tp.reactions.values() if 'rates' in rx]
    nu = np.zeros((1, len(names)))
    nu[0, names.index('CO2')], nu[0, names.index('CO')], nu[0, names.index('OH-')] = -1.0, 1.0, 2.0
    return np.asarray(tp.D, float), np.asarray(tp.charges, float), radii, np.asarray(tp.xmesh, float), float(tp.beta), table, \
        {'species': [names.index('CO2')], 'nu': nu, 'alpha': None, 'saturation': None}


def records(B, N, nx, out, co2r):
    from tests.test_gpu_balance import reference
    if co2r:
        D, q, radii, x, beta, table, wall = co2r_problem(nx)
        N = len(D)
    else:
        z = np.array([1, -1, 2, -1, 0, 1, -2, -1][:N], float)
        D, q, radii, x, beta, table, wall = 1e-9 * (1.0 + 0.3 * np.arange(N)), z * unit_F, None, np.arange(nx) * 2e-10, BETA, [], None
    c, phi = state(B, N, nx)
    rng = np.random.RandomState(3)
    flux, phiM = rng.uniform(-2e-4, 2e-4, (B, N)), rng.uniform(-1.0, 0.0, B)
    if wall:
        wall = dict(wall, k=rng.uniform(1e-6, 1e-5, (B, 1)))
    steric = radii is not None and bool(np.any(radii))
    # the host alternative, once: the tests' NumPy restatement on the same arrays
    nb = min(B, 2048)
    t0 = time.perf_counter()
    reference(c[:nb], phi[:nb], x, D, q, flux[:nb], phiM[:nb], radii, 0.0, table, None if not wall else dict(wall, k=wall['k'][:nb]), beta=beta)
    numpy_s = time.perf_counter() - t0
    with PnpSolver(N, nx, float(x[1] - x[0]), 1.0, beta, EPS, D, q, method='Newton', batch_capacity=B) as s, _balance.Balancer(0) as bal:
        s.set_newton(wall_bc='stern', stern_capacitance=0.2, mpb_radius=radii if steric else None)
        s.set_grid(x)
        s.set_batch(c, np.zeros((B, 4)), np.zeros(B), np.zeros((B, N)))
        s.set_potential(phi)
        view = s.device_view()
        for what, fields, obs_fields in (('all rows', None, None), ('scalars and wall rates', ['wall_rate'], [])):
            kms, wms, oms = [], [], []
            for r in range(LAUNCHES + 2):                     # the first calls allocate and load the code object
                t0 = time.perf_counter()
                bal.species(view, D, q, x, beta, flux, phiM, mpb_radius=radii, reactions=table, wall=wall, fields=fields, scalars=True)
                if r >= 2:
                    wms.append((time.perf_counter() - t0) * 1e3)
                    kms.append(bal.last_kernel_ms)
            for r in range(LAUNCHES + 2):
                s.get_electrolyte(fields=obs_fields, scalars=True, species_H=0)
                if r >= 2:
                    oms.append(s._observer.last_kernel_ms)
            Rn, W = len(table), (0 if not wall else 1)
            parts = sum(len(l) + len(rr) for (l, rr, _, _) in table)                      # participant rows read in pass A
            uses = sum(len(set(l) | set(rr)) for (l, rr, _, _) in table)                  # (species, reaction) pairs: rate rows read in pass B
            absrows = 2                                                                   # scalars wanted: the |forward| + |backward| rows too
            read = B * ((N * (2 if steric else 1) + 1) * nx + parts * nx + uses * nx * absrows) * 8
            rows = (Rn * nx * absrows if fields else 0)                                   # workspace rows are written either way
            if fields is None:
                written = B * (N * (nx - 1) + Rn * nx * absrows + 2 * N * nx + W + N + N * _balance.NSCALARS) * 8
                to_host = B * (N * (nx - 1) + Rn * nx + 2 * N * nx + W + N + N * _balance.NSCALARS) * 8
            else:
                written = B * (rows + W + N * _balance.NSCALARS) * 8
                to_host = B * (W + N * _balance.NSCALARS) * 8
            k = float(np.median(kms)) * 1e-3
            rec = {'probe': 'catbal_species', 'B': B, 'N': N, 'nx': nx, 'steric': steric, 'reactions': Rn, 'wall_reactions': W, 'outputs': what,
                   'kernel': bal.last_kernel, 'launches': len(kms), 'kernel_ms': round(float(np.median(kms)), 4),
                   'kernel_ms_min': round(float(np.min(kms)), 4), 'kernel_ms_max': round(float(np.max(kms)), 4),
                   'wall_ms': round(float(np.median(wms)), 3), 'bytes_read': read, 'bytes_written': written, 'bytes_to_host': to_host,
                   'kernel_bytes_per_s': round((read + written) / k, 0), 'fraction_of_8TBps': round((read + written) / k / HBM_PEAK, 4),
                   'yardstick_electrolyte_kernel': s._observer.last_kernel, 'yardstick_electrolyte_kernel_ms': round(float(np.median(oms)), 4),
                   'yardstick_electrolyte_kernel_ms_min': round(float(np.min(oms)), 4), 'yardstick_electrolyte_kernel_ms_max': round(float(np.max(oms)), 4),
                   'yardstick_numpy_points': nb, 'yardstick_numpy_seconds': round(numpy_s, 4),
                   'yardstick_numpy_seconds_scaled_to_B': round(numpy_s * B / nb, 4)}
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + '\n')
            out.flush()


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, 'profiles', 'balance_probe.jsonl')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as out:
        records(4096, 7, 384, out, co2r=True)
        records(32768, 8, 512, out, co2r=False)


if __name__ == '__main__':
    main()
