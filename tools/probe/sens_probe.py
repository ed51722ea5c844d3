#!/usr/bin/env python3
"""Parameter sensitivities on the device (libcatint_sens): what the carried right-hand sides cost next to one elimination without them,
and next to the finite differences they replace.  One run on one MI355X writes profiles/sens_probe.md (or the file given as the first
argument); no figure in it is fixed in advance.

The two handles of tools/probe/response_probe.py, 4096 operating points each, brought to their stationary state first:
  * CO2R: N = 7, nx = 384, steric K+, buffer reactions, graded grid, Stern wall;
  * point ions: N = 8, nx = 512, Dirichlet wall.
Per handle and P = 8, 16, 32 parameters (every kind the handle supports, the list repeated cyclically), in the same process, after one
warm-up, five repeats in which the two sides alternate:
  catsens_last_kernel_ms (HIP events around the launch) and the wall time of the call, copies included;
  catcpl_last_kernel_ms on the same handle: one elimination with no carried columns.  sens / (chunks x coupling) is the price of the
  carried columns per chunk;
  what a user pays today: 2 P warm-started solve_stationary calls on the same handle, each after a move of every lane's electrode
  potential by a relative 1e-3 (up, then down), timed with the handle's timer.  Only the potential and the wall fluxes can be moved on a
  handle at all: for a diffusion coefficient or a rate constant the finite difference also pays for setting the medium up again, so
  this side is a lower bound.
Minimum, median and maximum of the five repeats are reported."""
import os
import sys
import time

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, 'examples'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import response_probe as RP          # noqa: E402  (the two handles)
from catint_amd import _sens         # noqa: E402

REPEATS, WARMUPS = 5, 1


def every_kind(s):
    o = s._obs
    specs = ['phiM', 'velocity'] + [(kind, j) for kind in ('c_bulk', 'D', 'flux') for j in range(s.N)]
    if o['wall_bc'] == 'stern':
        specs.append('stern_capacitance')
    for r in range(len(o['reactions'])):
        specs += [('kf', r), ('kr', r)]
    return specs


def sens_call(s, specs, flux):
    o = s._obs
    if getattr(s, '_sensitizer', None) is None:
        s._sensitizer = _sens.Sensitizer(o['device'])
    t0 = time.perf_counter()
    out = s._sensitizer.solve(s.device_view(), o['D'], o['charges'], o['x'], o['beta'], o['eps'], o['dx'], o['phiM'], flux, specs,
                              lanes=np.arange(s.B), mpb_radius=o['mpb_radius'], wall_bc=o['wall_bc'], stern_capacitance=o['stern_capacitance'],
                              phi_pzc=o['phi_pzc'], velocity=o['velocity'], reactions=o['reactions'], wall=None)
    return out, s._sensitizer.last_kernel_ms, 1e3 * (time.perf_counter() - t0)


def spread(v):
    return '%.3f (min %.3f, max %.3f)' % (float(np.median(v)), min(v), max(v))


def measure(s, lines, label):
    B, N = s.B, s.N
    st = s.solve_stationary()
    lanes = np.flatnonzero(st == 0)
    flux = np.asarray(s._obs['flux'], float)
    zero = {'flux': np.zeros((B, N)), 'dflux_dc': np.zeros((B, N, N)), 'dflux_dphi': np.zeros((B, N, 2))}
    kinds = every_kind(s)
    pb = np.zeros((B, 4))
    pb[:, 0], pb[:, 1] = s._obs['phiM'], s._obs['phi_bulk']
    for P in (8, 16, 32):
        specs = [kinds[m % len(kinds)] for m in range(P)]
        chunks = (P + _sens.CHUNK - 1) // _sens.CHUNK
        ker, wall, cpl, fd = [], [], [], []
        for r in range(REPEATS + WARMUPS):
            out, k_ms, w_ms = sens_call(s, specs, flux)
            s.get_coupling(flux, zero, fields=['T_c', 'T_phi'])
            c_ms = s._coupler.last_kernel_ms
            s.timer_start()
            for m in range(P):
                for sgn in (1.0, -1.0):
                    moved = pb.copy()
                    moved[:, 0] *= 1.0 + sgn * 1e-3
                    s.set_pb(moved, np.zeros(B))
                    s.solve_stationary()
            f_ms = s.timer_stop()
            s.set_pb(pb, np.zeros(B))
            assert (s.solve_stationary() == st).all()
            if r >= WARMUPS:
                ker.append(k_ms), wall.append(w_ms), cpl.append(c_ms), fd.append(f_ms)
        ok = int((out['status'][lanes] == 0).sum())
        a, c, f = float(np.median(ker)), float(np.median(cpl)), float(np.median(fd))
        lines.append('| %s: B = %d, N = %d, nx = %d | P = %d (%d chunks), `%s`, %d of %d converged lanes status 0 | %s | %s | %s; sens / (chunks x '
                     'coupling) = %.2f | %s; finite differences / sens kernel = %.1f |'
                     % (label, B, N, s.nx, P, chunks, s._sensitizer.last_kernel, ok, len(lanes), spread(ker), spread(wall), spread(cpl),
                        a / (chunks * c), spread(fd), f / a))
        print(lines[-1], flush=True)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, 'profiles', 'sens_probe.md')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    lines = ['# Parameter sensitivities on the device: the carried right-hand sides next to one elimination without them and next to '
             'finite differences (tools/probe/sens_probe.py, one MI355X)', '',
             'Median (minimum, maximum) of %d repeats after %d warm-up, the sides alternating in one process.  Kernel times are HIP events '
             'around the launch; the call is wall time with the copies; the finite differences are 2 P warm-started `solve_stationary` '
             'calls after a relative move of 1e-3 of every electrode potential, timed with the handle\'s timer (a lower bound: see the '
             'probe\'s docstring).' % (REPEATS, WARMUPS),
             '', '| handle | call | `catsens` kernel, ms | `catsens_solve` wall, ms | `catcpl::couple_kernel` (no carried columns), ms | '
             '2 P `solve_stationary`, ms |', '|---|---|---|---|---|---|']
    for make, args, label in ((RP.co2r_handle, (4096, 384), 'CO2R'), (RP.plain_handle, (4096, 512), 'point ions')):
        s, status, what = make(*args)
        with s:
            measure(s, lines, '%s (%s)' % (label, what))
    with open(path, 'w') as out:
        out.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
