#!/usr/bin/env python3
"""The Newton step of the self-consistency on the device (libcatint_couple): what a call costs next to what it replaces.  One run on
one MI355X writes profiles/couple_probe.md (or the file given as the first argument); no figure in it is fixed in advance.

The two handles of tools/probe/response_probe.py, 4096 operating points each, brought to their stationary state first (without a wall
table: the coupling is defined for prescribed fluxes):
  * CO2R: N = 7, nx = 384, steric K+, buffer reactions, graded grid, Stern wall;
  * point ions: N = 8, nx = 512, Dirichlet wall.
Per handle, in the same process, medians of 11 calls after 1 warm-up, HIP events around the launch (last_kernel_ms):
  catcpl::couple_kernel with seeded random kinetic inputs, against
  (a) one catresp scalars call at omega = 0 (one column of the transport tangent),
  (b) the N such calls the coupling replaces (their sum),
  (c) the wall time of one warm-started solve_stationary.
And for examples/co2r_microkinetic_sweep.py (16 lanes, nx = 192): wall time and number of transport solves with and without --newton."""
import os
import subprocess
import sys
import time

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, 'examples'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import response_probe as RP          # noqa: E402  (the two handles)

CALLS, WARMUPS = 11, 1


def measure(s, lines, label):
    B, N, nx = s.B, s.N, s.nx
    s.synchronize()
    t0 = time.perf_counter()
    st = s.solve_stationary()
    solve_ms = 1e3 * (time.perf_counter() - t0)
    lanes = np.flatnonzero(st == 0)
    flux = np.asarray(s._obs['flux'], float)
    rng = np.random.RandomState(1)
    zero = {'flux': np.zeros((B, N)), 'dflux_dc': np.zeros((B, N, N)), 'dflux_dphi': np.zeros((B, N, 2))}
    first = s.get_coupling(flux, zero, fields=['T_c', 'T_phi'])
    rowmax = np.nanmax(np.abs(first['T_c']), axis=2)
    pmax = np.nanmax(np.abs(first['T_phi']), axis=1)
    kin = {'flux': flux + 1e-9 * rng.uniform(-1, 1, (B, N)),
           'dflux_dc': 0.7 * rng.uniform(-1, 1, (B, N, N)) / (N * N * np.where(rowmax > 0, rowmax, 1.0)[:, None, :]),
           'dflux_dphi': np.stack([np.zeros((B, N)), 0.2 * rng.uniform(-1, 1, (B, N)) / (N * np.where(pmax > 0, pmax, 1.0)[:, None])], axis=2)}
    cpl, wall = [], 0.0
    for r in range(CALLS + WARMUPS):
        t0 = time.perf_counter()
        out = s.get_coupling(flux, kin)
        wall = 1e3 * (time.perf_counter() - t0)
        if r >= WARMUPS:
            cpl.append(s._coupler.last_kernel_ms)
    ok = int((out['status'][lanes] == 0).sum())
    one, allcols = [], []
    for r in range(CALLS + WARMUPS):
        total = 0.0
        for j in range(N):
            s.get_response(omega=[0.0], perturbation=('flux', j))
            total += s._responder.last_kernel_ms
            if j == 0 and r >= WARMUPS:
                one.append(s._responder.last_kernel_ms)
        if r >= WARMUPS:
            allcols.append(total)
    a, b, c = float(np.median(one)), float(np.median(allcols)), float(np.median(cpl))
    lines.append('| %s: B = %d, N = %d, nx = %d | `%s` (%d of %d converged lanes status 0) | %.3f ms (min %.3f, max %.3f); call %.1f ms wall |'
                 % (label, B, N, nx, s._coupler.last_kernel, ok, len(lanes), c, min(cpl), max(cpl), wall))
    lines.append('| | (a) one `%s` call, omega = 0 | %.3f ms; coupling / (a) = %.2f |' % (s._responder.last_kernel, a, c / a))
    lines.append('| | (b) the %d such calls the coupling replaces | %.3f ms; coupling / (b) = %.3f |' % (N, b, c / b))
    lines.append('| | (c) one warm-started `solve_stationary`, wall | %.2f ms; coupling / (c) = %.3f |' % (solve_ms, c / solve_ms))
    for line in lines[-4:]:
        print(line, flush=True)


def sweep(newton):
    cmd = [sys.executable, os.path.join(R, 'examples', 'co2r_microkinetic_sweep.py'), '--lanes', '16'] + (['--newton'] if newton else [])
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    head = [ln for ln in r.stdout.splitlines() if 'lanes:' in ln]
    return '| `%s` | %s | process %.1f s |' % (' '.join(cmd[1:]).replace(R + os.sep, ''), head[0] if head else 'rc %d: %s' % (r.returncode, r.stderr[-300:]), wall)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, 'profiles', 'couple_probe.md')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    lines = ['# The Newton step of the self-consistency on the device: kernel time next to what it replaces '
             '(tools/probe/couple_probe.py, one MI355X)', '',
             'Kernel times are HIP events around the launch (median of %d calls after %d warm-up); the solve is wall time of one call.' % (CALLS, WARMUPS),
             '', '| handle | call | time |', '|---|---|---|']
    for make, args, label in ((RP.co2r_handle, (4096, 384), 'CO2R'), (RP.plain_handle, (4096, 512), 'point ions')):
        s, status, what = make(*args)
        with s:
            measure(s, lines, '%s (%s)' % (label, what))
    lines += ['', '## examples/co2r_microkinetic_sweep.py, 16 lanes, nx = 192', '', '| command | result | |', '|---|---|---|']
    for newton in (False, True):
        lines.append(sweep(newton))
        print(lines[-1], flush=True)
    with open(path, 'w') as out:
        out.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
