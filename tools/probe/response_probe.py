#!/usr/bin/env python3
"""Linear response on the device (libcatint_response): what a call costs next to the solve it follows.  One run on one MI355X writes
profiles/response_probe.md (or the file given as the first argument); no figure in it is fixed in advance.

Two handles of 4096 operating points, each brought to its stationary state first:
  * N = 7, nx = 384: the CO2R sweep's species (steric K+), buffer reactions, graded grid and Stern wall, -0.5 .. -2.0 V;
  * N = 8, nx = 512: point ions, Dirichlet wall, +-0.25 V, no reactions.
Per handle: catresp::response_kernel by HIP events around its launch (last_kernel_ms), median / min / max of 5 calls after 1 warm-up,
for a scalars-only call at omega = 0 (F = 1, the real instance), a scalars-only call at 16 frequencies (complex) and a profiles call at
omega = 0; and, in the same run on the same handle, the wall time of one warm-started solve_stationary (from the converged state: the
least a finite difference pays twice).  The fp64 rate counts the multiply-adds of the algorithm as written in DESIGN.md section 7g:
per block row NB (1.5 NB^2 - 0.5 NB) for the Gauss-Jordan step and NB^3 (steric) or 2 NB^2 (point ions) for U T, 2 flops each in
real and 8 in complex arithmetic."""
import os
import sys
import time

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, 'examples'))

from catint_amd import PnpSolver
from catint_amd.host import graded_mesh
from catint_amd.units import unit_F, unit_R, unit_eps0

BETA = 1.0 / (unit_R * 298.15)
EPS = 78.36 * unit_eps0
CALLS, WARMUPS = 5, 1


def flops(nsys, nx, NB, steric, cx):
    per_row = NB * (1.5 * NB * NB - 0.5 * NB) + (NB ** 3 if steric else 2 * NB * NB)
    return nsys * (nx - 1) * per_row * (8 if cx else 2)


def co2r_handle(B, nx):
    import co2r_physical_sweep as ex
    from catint_amd.calculator import Calculator
    tp, phis = ex.build(B, nx)
    calc = Calculator(transport=tp, calc='comsol')
    tp.newton = {'tol': 1e-8, 'maxit': 80}
    s = calc._physical_solver(B)
    c0 = np.repeat(np.asarray(tp.c0, float)[None, :], B, axis=0)
    status = calc.solve_physical(s, c0, np.asarray(phis, float), np.zeros((B, tp.nspecies)))
    return s, status, 'CO2R sweep, steric K+, reactions, Stern wall'


def plain_handle(B, nx, N=8):
    z = np.array([1, -1, 2, -1, 0, 1, -2, -1][:N], float)
    cb = np.array([100.0, 50.0, 20.0, 60.0, 30.0, 10.0, 15.0, 10.0][:N])        # electroneutral
    x = graded_mesh(4e-8, 5e-11, nx)
    s = PnpSolver(N, nx, float(x[1] - x[0]), 1.0, BETA, EPS, 1e-9 * (1.0 + 0.3 * np.arange(N)), z * unit_F, method='Newton', batch_capacity=B)
    s.set_grid(x)
    pb = np.zeros((B, 4))
    pb[:, 0] = np.linspace(-0.25, 0.25, B)
    s.set_batch(np.repeat(np.repeat(cb[None, :, None], nx, axis=2), B, axis=0), pb, np.zeros(B), np.zeros((B, N)))
    s.set_equilibrium()
    return s, s.solve_stationary(), 'point ions, Dirichlet wall'


def measure(s, lines, label):
    B, N, nx = s.B, s.N, s.nx
    steric = s._obs['mpb_radius'] is not None and np.any(np.asarray(s._obs['mpb_radius']) != 0)
    s.synchronize()
    t0 = time.perf_counter()
    st = s.solve_stationary()
    solve_ms = 1e3 * (time.perf_counter() - t0)
    its = s.newton_iterations()
    lines.append('| %s: B = %d, N = %d, nx = %d | warm-started `solve_stationary` (%d lanes converged, %d iterations at most) | %.2f ms wall | | |'
                 % (label, B, N, nx, int((st == 0).sum()), int(its.max()), solve_ms))
    lanes = np.flatnonzero(st == 0)
    out = {}
    for name, omega, profiles in (('scalars, F = 1 (omega = 0)', [0.0], False), ('scalars, F = 16', np.logspace(0, 7, 16), False),
                                  ('profiles, F = 1 (omega = 0)', [0.0], True)):
        ms = []
        for r in range(CALLS + WARMUPS):
            t0 = time.perf_counter()
            res = s.get_response(omega=omega, profiles=profiles)
            wall = 1e3 * (time.perf_counter() - t0)
            if r >= WARMUPS:
                ms.append(s._responder.last_kernel_ms)
        ok = int((res['status'][lanes] == 0).all(axis=1).sum())
        med = float(np.median(ms))
        fl = flops(B * len(omega), nx, N + 1, steric, np.any(np.asarray(omega) != 0))
        lines.append('| | %s: `%s` (%d of %d converged lanes status 0) | %.3f ms (min %.3f, max %.3f) | %.2f TFLOP/s | call %.1f ms wall |'
                     % (name, s._responder.last_kernel, ok, len(lanes), med, min(ms), max(ms), fl / med / 1e9, wall))
        out[name] = med
        print(lines[-1], flush=True)
    lines.append('| | omega = 0 scalars call / two warm-started solves | %.3f | | |' % (out['scalars, F = 1 (omega = 0)'] / (2.0 * solve_ms)))
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, 'profiles', 'response_probe.md')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    lines = ['# Linear response on the device: kernel time next to the solve (tools/probe/response_probe.py, one MI355X)', '',
             'Kernel times are HIP events around the launch (median of %d calls after %d warm-up); the solve is wall time of one call.' % (CALLS, WARMUPS),
             '', '| handle | call | time | fp64 rate of the algorithm\'s multiply-adds | |', '|---|---|---|---|---|']
    for make, args, label in ((co2r_handle, (4096, 384), 'CO2R'), (plain_handle, (4096, 512), 'point ions')):
        s, status, what = make(*args)
        with s:
            measure(s, lines, '%s (%s)' % (label, what))
    with open(path, 'w') as out:
        out.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
