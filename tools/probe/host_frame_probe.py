#!/usr/bin/env python3
"""Host cost of a small call of the satellite libraries, two builds side by side (profiles/host_frame.md).

The host frame of an entry point -- staging, reserve, launch, copy back -- shows only where the kernel is short: N = 2 species on
nx = 33 points, n = 64 operating points, the context warm and the outputs fixed.  For libcatint_response, libcatint_couple,
libcatint_kinetics and libcatint_eis (cateis_solve) one series is REPEATS calls after WARMUPS in a process of its own; it reports the
median wall time of a call (host clock around the call, which ends in a stream synchronise) and the median of last_kernel_ms.

    python tools/probe/host_frame_probe.py --old DIR [--series 6] [--out FILE]
    python tools/probe/host_frame_probe.py --old-tree DIR [--series 6] [--out FILE]

DIR holds the libraries of the build to compare with (libcatint_*.so); the tree's own build is the other.  With --old-tree the two sides
differ in their Python instead: DIR holds the catint_amd package of another checkout (its *.py; no lib/ is needed), both sides load this
tree's libraries, and the calls go through the PnpSolver entry points (get_response, get_coupling, get_kinetics, get_impedance), where
the Python share of a call sits.  The series run in the order
old new new old old new ..., so that neither build always follows the other, and each build has --series independent series.  The
noise of the comparison is the spread between the medians of the old build's own series; the table puts the difference of the two
builds' medians beside it.  No figure is fixed in advance."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)

REPEATS, WARMUPS = 300, 20
N_POINTS, NX = 64, 33
LIBS = ('response', 'couple', 'kinetics', 'eis')
ENTRIES = {'response': ('get_response', '_responder'), 'couple': ('get_coupling', '_coupler'), 'kinetics': ('get_kinetics', '_kinetics'),
           'eis': ('get_impedance', '_impedance')}


def series(solver=False):
    """one series of every library on the libraries the environment names; a JSON line.  solver: through the PnpSolver entry points"""
    if os.environ.get('CATINT_PROBE_TREE'):
        sys.path.insert(0, os.environ['CATINT_PROBE_TREE'])
    from catint_amd import _couple, _eis, _kinetics, _response
    from tests import eis_cases as EC
    from tests import response_cases as RC
    from tests.test_gpu_couple import load, open_solver
    case = RC.small(2, NX, stern=True)
    phis = case.phiM * np.linspace(1.0, 0.05, N_POINTS)
    s = open_solver(case, N_POINTS)
    load(s, case, phis, [case.bulk_state()] * N_POINTS)
    assert (s.solve_stationary() == 0).all()
    view, o = s.device_view(), s._obs
    lanes = np.arange(N_POINTS, dtype=np.int64)
    medium = [o[k] for k in ('D', 'charges', 'x', 'beta', 'eps', 'dx')]
    wall = dict(mpb_radius=o['mpb_radius'], wall_bc=o['wall_bc'], stern_capacitance=o['stern_capacitance'])
    surface = dict(stern_capacitance=o['stern_capacitance'], phi_pzc=o['phi_pzc'])
    tables = EC.chain_tables(case.N)
    flux = np.zeros((N_POINTS, case.N))
    omega = case.omegas()[:3]
    handles = {'response': _response.Responder(0), 'couple': _couple.Coupler(0), 'kinetics': _kinetics.KineticsSolver(0), 'eis': _eis.Impedance(0)}
    kin = handles['kinetics'].solve(view, tables, phis, lanes=lanes, fields=('theta', 'flux', 'dflux_dc', 'dflux_dphi'), **surface)
    kphi = np.ascontiguousarray(kin['dflux_dphi'][:, :, 1])
    out = {k: {} for k in LIBS}          # the outputs are allocated once: the calls write into the same arrays
    calls = {
        'response': lambda: handles['response'].solve(view, *medium, phis, omega=omega, lanes=lanes, out=out['response'], **wall),
        'couple': lambda: handles['couple'].solve(view, *medium, flux, kin['flux'], kin['dflux_dc'], kphi, lanes=lanes, out=out['couple'], **wall),
        'kinetics': lambda: handles['kinetics'].solve(view, tables, phis, lanes=lanes, out=out['kinetics'], **surface),
        'eis': lambda: handles['eis'].solve(view, tables, phis, kin['theta'], omega, *medium, rf=1.0, lanes=lanes, out=out['eis'], **wall,
                                            phi_pzc=o['phi_pzc']),
    }
    if solver:
        kin = s.get_kinetics(tables, fields=('theta', 'flux', 'dflux_dc', 'dflux_dphi'))
        calls = {'response': lambda: s.get_response(omega=omega), 'couple': lambda: s.get_coupling(None, kin),
                 'kinetics': lambda: s.get_kinetics(tables), 'eis': lambda: s.get_impedance(tables, omega, theta=kin['theta'])}
        for name in LIBS:
            calls[name]()
            handles[name].close()
            handles[name] = getattr(s, ENTRIES[name][1])
    res = {}
    for name in LIBS:
        f, h = calls[name], handles[name]
        wall_ms, kern_ms = [], []
        for r in range(REPEATS + WARMUPS):
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            if r >= WARMUPS:
                wall_ms.append(1e3 * (t1 - t0)), kern_ms.append(h.last_kernel_ms)
        res[name] = {'wall_ms': float(np.median(wall_ms)), 'kernel_ms': float(np.median(kern_ms)), 'kernel': h.last_kernel}
    for h in handles.values():
        h.close()          # (a solver's own library objects are closed a second time by s.close(): nothing happens)
    s.close()
    print('SERIES ' + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--old', help='directory with the libraries of the build to compare with')
    ap.add_argument('--old-tree', help='directory with the catint_amd package (Python) of the checkout to compare with')
    ap.add_argument('--solver', action='store_true', help='(internal, with --one) call through the PnpSolver entry points')
    ap.add_argument('--series', type=int, default=6)
    ap.add_argument('--out', default=None, help='also write the table to this file')
    ap.add_argument('--one', action='store_true', help='(internal) run one series in this process')
    a = ap.parse_args()
    if a.one:
        return series(a.solver)
    runs = {'old': [], 'new': []}
    for k in range(a.series):
        for build in (('old', 'new') if k % 2 == 0 else ('new', 'old')):
            env = dict(os.environ)
            if build == 'old' and a.old_tree:
                env['CATINT_PROBE_TREE'] = os.path.abspath(a.old_tree)
                for lib in LIBS + ('pnp',):
                    env['CATINT_%s_LIB' % lib.upper()] = os.path.join(os.path.abspath(R), 'catint_amd', 'lib', 'libcatint_%s.so' % lib)
            elif build == 'old':
                for lib in LIBS:
                    env['CATINT_%s_LIB' % lib.upper()] = os.path.join(os.path.abspath(a.old), 'libcatint_%s.so' % lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--one'] + (['--solver'] if a.old_tree else []), env=env,
                               capture_output=True, text=True, timeout=280)
            if r.returncode != 0:          # a series that failed ends the probe: nothing more is started on the device
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(r.returncode or 1)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith('SERIES ')][-1]
            runs[build].append(json.loads(line[7:]))
    lines = ['| library | kernel | figure | old build, median of each series (ms) | new build, median of each series (ms) | new - old, medians of the series (ms) | '
             'spread of the old build\'s series (ms) | within the spread |', '|---|---|---|---|---|---|---|---|']
    for lib in LIBS:
        for fig in ('wall_ms', 'kernel_ms'):
            old = [s[lib][fig] for s in runs['old']]
            new = [s[lib][fig] for s in runs['new']]
            diff, spread = float(np.median(new) - np.median(old)), max(old) - min(old)
            lines.append('| %s | `%s` | %s | %s | %s | %+.4f | %.4f | %s |' % (
                lib, runs['new'][0][lib]['kernel'], fig[:-3], ', '.join('%.4f' % v for v in old), ', '.join('%.4f' % v for v in new), diff, spread,
                'yes' if diff <= spread else 'NO'))
    text = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
