#!/usr/bin/env python3
"""Electrolyte observables on the device (libcatint_observe): time of catobs_electrolyte by HIP events, bytes moved and the fraction
of the 8 TB/s HBM peak, at 4096 x 7 x 384 (the CO2R sweep) and 32 768 x 8 x 512, all rows and scalars only, point and steric ions; and
the wall time of Calculator.run()'s read-out (everything after the transport solves) on the CO2R sweep of 4096 voltages with the
quantities derived on the host (the default path) and on the device (derive_on_device=True), same process, same device.

One run writes profiles/observe_probe.jsonl (or the file given as the first argument).  The states of the first part are arbitrary
(smooth concentrations, a random-walk potential): the kernel's work does not depend on the values.
Bytes: every input row once ((N + 1) nx doubles per operating point, the species rows twice with steric ions) plus every row written.
'kernel_ms' is the kernel alone (events around its launch), 'call_ms' the whole call on the handle's stream (grid upload, kernel,
copies of the requested rows to the host), 'wall_ms' the host's clock around it."""
import json
import os
import sys
import time

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, 'examples'))

from catint_amd import PnpSolver, _observe
from catint_amd.units import unit_F, unit_R, unit_eps0

HBM_PEAK = 8.0e12
BETA = 1.0 / (unit_R * 298.15)
EPS = 78.36 * unit_eps0


def state(B, N, nx, tile=512):
    rng = np.random.RandomState(7)
    b = min(B, tile)
    s = np.linspace(0.0, 1.0, nx)
    c = 10.0 * (1.0 + np.arange(N))[None, :, None] * np.exp(0.5 * np.sin(2 * np.pi * rng.uniform(0.5, 3.0, (b, N, 1)) * s + rng.uniform(0, 6.28, (b, N, 1))))
    phi = np.cumsum(rng.uniform(0.005, 0.015, (b, nx)) * rng.choice([-1.0, 1.0], (b, nx)), axis=1)
    reps = (B + b - 1) // b
    return np.ascontiguousarray(np.tile(c, (reps, 1, 1))[:B]), np.ascontiguousarray(np.tile(phi, (reps, 1))[:B])


def kernel_records(B, N, nx, out, reps=5):
    z = np.array([1, -1, 2, -1, 0, 1, -2, -1][:N], float)
    D = 1e-9 * (1.0 + 0.3 * np.arange(N))
    c, phi = state(B, N, nx)
    for steric in (False, True):
        with PnpSolver(N, nx, 2e-10, 1.0, BETA, EPS, D, z * unit_F, method='Newton', batch_capacity=B) as s:
            s.set_newton(wall_bc='stern', stern_capacitance=0.2, mpb_radius=3e-10 * (1.0 + 0.1 * np.arange(N)) if steric else None)
            s.set_batch(c, np.zeros((B, 4)), np.zeros(B), np.zeros((B, N)))
            s.set_potential(phi)
            for what, fields in (('all rows', None), ('scalars only', [])):
                kms, cms, wms = [], [], []
                for r in range(reps + 1):                     # the first call allocates and loads the code object
                    t0 = time.perf_counter()
                    s.timer_start()
                    s.get_electrolyte(fields=fields, scalars=True, species_H=0)
                    ms = s.timer_stop()
                    if r:
                        wms.append((time.perf_counter() - t0) * 1e3)
                        cms.append(ms)
                        kms.append(s._observer.last_kernel_ms)
                rows_p = 0 if fields == [] else 6
                rows_e = 0 if fields == [] else 2
                read = B * (N * (2 if steric else 1) + 1) * nx * 8
                written = B * (rows_p * nx + rows_e * (nx - 1) + _observe.NSCALARS) * 8
                k = float(np.median(kms)) * 1e-3
                rec = {'probe': 'catobs_electrolyte', 'B': B, 'N': N, 'nx': nx, 'steric': steric, 'outputs': what,
                       'kernel': s._observer.last_kernel, 'kernel_ms': round(float(np.median(kms)), 4), 'kernel_ms_min': round(float(np.min(kms)), 4),
                       'call_ms': round(float(np.median(cms)), 3), 'wall_ms': round(float(np.median(wms)), 3),
                       'bytes_read': read, 'bytes_written': written, 'bytes_to_host': written,
                       'kernel_bytes_per_s': round((read + written) / k, 0), 'fraction_of_8TBps': round((read + written) / k / HBM_PEAK, 4)}
                print(json.dumps(rec), flush=True)
                out.write(json.dumps(rec) + '\n')
                out.flush()


def readout_records(lanes, nx, out, reps=3):
    import co2r_physical_sweep as ex
    from catint_amd.calculator import Calculator
    for derive in (False, True, False, True):              # alternating: the two paths see the same machine
        tp, _ = ex.build(lanes, nx)
        calc = Calculator(transport=tp, calc='comsol', derive_on_device=derive)
        tp.newton = {'tol': 1e-8, 'maxit': 80}
        calc.set_surface_kinetics([{'species': 'CO2', 'rate': ex.tafel_rate(tp), 'stoichiometry': {'CO2': -1.0, 'CO': 1.0, 'OH-': 2.0}}])
        total, solve = [], []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            calc.run()
            if r:
                total.append(time.perf_counter() - t0)
                solve.append(calc.solve_seconds)
        readout = np.array(total) - np.array(solve)
        rec = {'probe': 'Calculator.run read-out', 'lanes': lanes, 'N': tp.nspecies, 'nx': tp.nx, 'derive_on_device': derive,
               'converged': int((calc.status == 0).sum()), 'run_seconds': round(float(np.median(total)), 4),
               'transport_solve_seconds': round(float(np.median(solve)), 4), 'readout_seconds': round(float(np.median(readout)), 4),
               'readout_seconds_min': round(float(readout.min()), 4)}
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + '\n')
        out.flush()


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, 'profiles', 'observe_probe.jsonl')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as out:
        kernel_records(4096, 7, 384, out)
        kernel_records(32768, 8, 512, out)
        readout_records(4096, 384, out)


if __name__ == '__main__':
    main()
