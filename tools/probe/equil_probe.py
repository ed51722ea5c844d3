#!/usr/bin/env python3
"""Equilibrium start states on the device (libcatint_equil): what the kernel costs and what the start buys.  One run on one MI355X
writes profiles/equil_probe.jsonl (or the file given as the first argument); no figure in it is fixed in advance.

  * kernel: time of cateq::pb_kernel by HIP events around its launch, median / min / max of 11 launches after 2 warm-ups, at
    4096 x 7 x 384 (the CO2R sweep's species, steric K+, its graded grid and Stern wall, the sweep's voltages) and at 8192 x 8 x 512
    (point ions, Dirichlet wall, +-0.25 V).  Beside it: a device-to-device copy of the bytes the kernel writes (every result row at
    its pitch), timed the same way -- the kernel iterates on chip, so the copy is the floor of its memory traffic, not of its time;
  * CO2R sweep (examples/co2r_physical_sweep.py) at 4096 lanes, tol = 1e-8, with and without tp.newton['equilibrium_start'], second
    run of each path (the first loads the code objects): time of the transport solves, Newton iterations of all lanes and of the
    slowest lane per solve, lanes converged, and the largest relative difference of the CO current between the two paths on the lanes
    that converge in both (must be <= 1e-9: the probe fails otherwise)."""
import json
import os
import sys

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, 'examples'))

from catint_amd import PnpSolver
from catint_amd.host import graded_mesh
from catint_amd.units import unit_F, unit_R, unit_eps0

BETA = 1.0 / (unit_R * 298.15)
EPS = 78.36 * unit_eps0
LAUNCHES, WARMUPS = 11, 2


def stats(ms):
    return {'ms': round(float(np.median(ms)), 4), 'ms_min': round(float(np.min(ms)), 4), 'ms_max': round(float(np.max(ms)), 4)}


def copy_ms(nbytes):
    """A device-to-device copy of nbytes (hipMemcpyAsync), HIP events around it: median / min / max of LAUNCHES after WARMUPS"""
    import ctypes as C
    hip = C.CDLL('libamdhip64.so')

    def ok(rc):
        if rc != 0:
            raise RuntimeError('HIP error %d' % rc)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    src, dst, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipMalloc(C.byref(src), C.c_size_t(nbytes)))
    ok(hip.hipMalloc(C.byref(dst), C.c_size_t(nbytes)))
    ok(hip.hipEventCreate(C.byref(e0)))
    ok(hip.hipEventCreate(C.byref(e1)))
    ms = []
    try:
        for r in range(LAUNCHES + WARMUPS):
            ok(hip.hipEventRecord(e0, None))
            ok(hip.hipMemcpyAsync(dst, src, nbytes, 3, None))        # hipMemcpyDeviceToDevice
            ok(hip.hipEventRecord(e1, None))
            ok(hip.hipEventSynchronize(e1))
            t = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(t), e0, e1))
            if r >= WARMUPS:
                ms.append(t.value)
    finally:
        hip.hipFree(src)
        hip.hipFree(dst)
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
    return stats(ms)


def kernel_record(B, nx, out, co2r, N=8):
    if co2r:
        import co2r_physical_sweep as ex
        from catint_amd.calculator import Calculator
        tp, phis = ex.build(B, nx)
        calc = Calculator(transport=tp, calc='comsol')
        s = calc._physical_solver(B)
        N = tp.nspecies
        c0 = np.repeat(np.asarray(tp.c0, float)[None, :], B, axis=0)
        phiM = np.asarray(phis, float)
    else:
        z = np.array([1, -1, 2, -1, 0, 1, -2, -1][:N], float)
        cb = np.array([100.0, 50.0, 20.0, 60.0, 30.0, 10.0, 15.0, 10.0][:N])        # electroneutral
        x = graded_mesh(4e-8, 5e-11, nx)
        s = PnpSolver(N, nx, float(x[1] - x[0]), 1.0, BETA, EPS, 1e-9 * (1.0 + 0.3 * np.arange(N)), z * unit_F, method='Newton', batch_capacity=B)
        s.set_grid(x)
        c0 = np.repeat(np.repeat(cb[None, :, None], nx, axis=2), B, axis=0)
        phiM = np.linspace(-0.25, 0.25, B)
    with s:
        pb = np.zeros((B, 4))
        pb[:, 0] = phiM
        s.set_batch(c0, pb, np.zeros(B), np.zeros((B, N)))
        kms = []
        for r in range(LAUNCHES + WARMUPS):
            o = s.equilibrium(to_host=False)
            if r >= WARMUPS:
                kms.append(s._equilibrator.last_kernel_ms)
        written = B * (N + 1) * s.row_pitch * 8
        rec = {'probe': 'cateq_solve', 'B': B, 'N': N, 'nx': nx, 'steric': s._obs['mpb_radius'] is not None, 'wall': s._obs['wall_bc'],
               'phiM_range': [float(phiM.min()), float(phiM.max())], 'launches': len(kms),
               'kernel': dict(stats(kms), name=s._equilibrator.last_kernel), 'iterations_max': int(o['iterations'].max()),
               'iterations_mean': round(float(o['iterations'].mean()), 2), 'not_converged': int((o['status'] != 0).sum()),
               'bytes_written': written}
    rec['device_copy_of_bytes_written'] = copy_ms(written)
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + '\n')
    out.flush()


def sweep_record(out, lanes, nx):
    import co2r_physical_sweep as ex
    from catint_amd.calculator import Calculator
    res = {}
    for name, extra in (('continuation', {}), ('equilibrium_start', {'equilibrium_start': True})):
        for rep in range(2):
            tp, phis = ex.build(lanes, nx)
            calc = Calculator(transport=tp, calc='comsol')
            tp.newton = dict({'tol': 1e-8, 'maxit': 80}, **extra)
            calc.set_surface_kinetics([{'species': 'CO2', 'rate': ex.tafel_rate(tp), 'stoichiometry': {'CO2': -1.0, 'CO': 1.0, 'OH-': 2.0}}])
            calc.run()
            names = list(tp.species.keys())
            res[name] = {'solve_seconds': round(calc.solve_seconds, 4), 'newton_iterations': int(calc.newton_iterations_total),
                         'newton_iterations_slowest_lane': int(calc.newton_iterations_slowest), 'converged': int((calc.status == 0).sum()),
                         'stages': int(calc.continuation_stages), 'ladder': [(r['rung'], r['stages'], len(r['lanes']), len(r['recovered']))
                                                                             for r in getattr(calc, 'retry_log', [])],
                         'equilibrium_start': getattr(calc, 'equilibrium_start', None)}
            res[name + '_j'] = (np.array(calc.status), np.array(calc.kinetic_flux)[:, names.index('CO')])
    (s0, j0), (s1, j1) = res.pop('continuation_j'), res.pop('equilibrium_start_j')
    both = (s0 == 0) & (s1 == 0)
    diff = float((np.abs(j1[both] - j0[both]) / np.abs(j0[both])).max()) if both.any() else None
    rec = {'probe': 'co2r_sweep', 'workload': 'examples/co2r_physical_sweep.py', 'lanes': lanes, 'nx': nx, 'tol': 1e-8, 'run': 'second of each path',
           'continuation': res['continuation'], 'equilibrium_start': res['equilibrium_start'], 'converged_in_both': int(both.sum()),
           'max_relative_difference_of_j_CO': diff}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + '\n')
    out.flush()
    assert diff is not None and diff <= 1e-9, 'the currents of the two paths differ by %r relative' % diff


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, 'profiles', 'equil_probe.jsonl')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as out:
        kernel_record(4096, 384, out, co2r=True)
        kernel_record(8192, 512, out, co2r=False)
        sweep_record(out, 4096, 384)


if __name__ == '__main__':
    main()
