#!/usr/bin/env python3
"""The impedance of the microkinetic electrode on the device (libcatint_eis) next to what the tree could do before it: the same transfer
functions by N + 1 calls of get_response per frequency list.  One run on one MI355X writes profiles/eis_probe.md (or the file given with
--out); no figure in it is fixed in advance.

Workload: the CO2 reduction sweep of examples/co2r_microkinetic_sweep.py (N = 7 species, the four-step mechanism, one site in a
thousand active), nx = 201, 4096 voltages between -0.6 and -1.2 V, brought to its fixed point by the Newton SCF loop
(Calculator.set_microkinetics(scf='newton')); 32 angular frequencies, 0 and 31 logarithmically spaced from 1e-2 to 1e7 rad/s.  The
measurements run at the loop's final state, before the transport solver is closed.
Timing: HIP events around the kernels (cateis_last_kernel_ms / catresp_last_kernel_ms), one warm-up, then five repeats; median, minimum
and maximum.  `both kernels`: get_impedance with the admittance and the transfer functions asked for; `kinetic kernel`: the same pairs
through get_kinetic_admittance; `electrode kernel`: the difference of the two medians.  `get_response`: the sum of the kernel times of
its N + 1 calls (one per wall flux, one for phiM), the calls alternating with the get_impedance calls in one process.
Compiler figures: taken from the log of a build with -Rpass-analysis=kernel-resource-usage given with --resources, or compiled from the
tree by this script."""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, 'examples'))

from catint_amd.calculator import Calculator             # noqa: E402
import co2r_microkinetic_sweep as sweep                  # noqa: E402
import co2r_physical_sweep                               # noqa: E402

REPEATS, WARMUPS = 5, 1
TRANSFER = ('admittance', 'Tc', 'Tphi', 'tc', 'tphi')


def spread(v):
    return '%.2f (min %.2f, max %.2f)' % (float(np.median(v)), min(v), max(v))


def resources(log):
    """[(kernel, VGPRs, AGPRs, SGPRs, scratch bytes per lane, static LDS bytes, waves per SIMD)] of every instance"""
    if log:
        text = open(log).read()
    else:
        hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
        cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only', '-c', os.path.join(R, 'catint_amd', 'csrc', 'eis', 'cateis.hip'),
               '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage']
        r = subprocess.run(cmd, capture_output=True, text=True)
        text = r.stdout + r.stderr
    rows = []
    for block in text.split('Function Name: ')[1:]:
        name = block.split()[0]
        m = re.match(r'_ZN6cateis16electrode_kernelILi(\d)EEE', name)
        kernel = 'cateis::electrode_kernel<%s>' % m.group(1) if m else ('cateis::kinetic_kernel' if 'kinetic_kernel' in name else name)

        def num(label):
            mm = re.search(r'%s: (\d+)' % re.escape(label), block)
            return mm.group(1) if mm else '?'
        rows.append((kernel, num(' VGPRs'), num('AGPRs'), num('TotalSGPRs'), num('ScratchSize [bytes/lane]'), num('LDS Size [bytes/block]'),
                     num('Occupancy [waves/SIMD]')))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lanes', type=int, default=4096)
    ap.add_argument('--nx', type=int, default=201)
    ap.add_argument('--nfreq', type=int, default=32)
    ap.add_argument('--out', default=os.path.join(R, 'profiles', 'eis_probe.md'))
    ap.add_argument('--resources', default=None, help='log of a build of cateis.hip with -Rpass-analysis=kernel-resource-usage')
    a = ap.parse_args()
    omega = np.concatenate([[0.0], np.logspace(-2, 7, a.nfreq - 1)])
    tp, phis = co2r_physical_sweep.build(a.lanes, a.nx, -0.6, -1.2)
    tp.newton = {'tol': 1e-8, 'maxit': 80}
    calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-4, mix_scf=0.1)
    calc.set_microkinetics(sweep.model(tp), site_density=1e-3 * float(tp.system['active site density']), scf='newton', impedance=[0.0])
    found = {}
    final = calc._final_impedance

    def measure(solver, theta=None):
        tables = calc.microkinetics['tables']
        N = solver.N
        both, kinetic, resp, wall_eis, wall_resp = [], [], [], [], []
        for r in range(REPEATS + WARMUPS):
            t0 = time.perf_counter()
            out = solver.get_impedance(tables, omega, theta=theta, rf=float(calc.RF), fields=TRANSFER)
            t1 = time.perf_counter()
            ms_both = solver._impedance.last_kernel_ms
            kernel = solver._impedance.last_kernel
            th = theta if theta is not None else solver.get_kinetics(tables, fields=('theta',))['theta']
            solver.get_kinetic_admittance(tables, omega, theta=th, fields=('Kc', 'Kphi'))
            ms_kin = solver._impedance.last_kernel_ms
            t2 = time.perf_counter()
            ms_resp, names = 0.0, set()
            for pert in [('flux', j) for j in range(N)] + ['phiM']:
                rr = solver.get_response(omega=omega, perturbation=pert)
                ms_resp += solver._responder.last_kernel_ms
                names.add(solver._responder.last_kernel)
            t3 = time.perf_counter()
            if r >= WARMUPS:
                both.append(ms_both), kinetic.append(ms_kin), resp.append(ms_resp), wall_eis.append(1e3 * (t1 - t0)), wall_resp.append(1e3 * (t3 - t2))
        same = np.array_equal(out['tphi'], rr['dphi_surface']) and np.array_equal(out['tc'], rr['dc_surface'])
        found.update(both=both, kinetic=kinetic, resp=resp, wall_eis=wall_eis, wall_resp=wall_resp, kernel=kernel, resp_kernels=sorted(names),
                     status=np.bincount(out['status'].reshape(-1), minlength=5), same=same, N=N, T=len(tables['site_count']), pairs=out['status'].size,
                     y0=out['admittance'][:, 0].real.copy(), y_hi=out['admittance'][:, -1].copy())
        return final(solver, theta)
    calc._final_impedance = measure
    names = list(tp.species.keys())
    t0 = time.time()
    res = calc.run_scf_cycle(nel=[2.0 if sp == 'CO' else 1.0 for sp in names], max_iter=200)
    f = found
    med = {k: float(np.median(f[k])) for k in ('both', 'kinetic', 'resp', 'wall_eis', 'wall_resp')}
    lines = ['# Impedance of the microkinetic electrode (tools/probe/eis_probe.py, one MI355X)', '',
             'CO2 reduction sweep of `examples/co2r_microkinetic_sweep.py`: %d lanes x %d frequencies = %d (point, omega) pairs, N = %d, nx = %d; '
             'the Newton SCF loop converged %d of %d lanes in %d steps (%.1f s with the measurements).  Kernel times in ms by HIP events, '
             'median (minimum, maximum) of %d repeats after %d warm-up; the status of the pairs: %s.'
             % (a.lanes, len(omega), f['pairs'], f['N'], tp.nx, int(res['converged'].sum()), a.lanes, res['iterations'], time.time() - t0, REPEATS, WARMUPS,
                ', '.join('%d x status %d' % (c, s) for s, c in enumerate(f['status']) if c)), '',
             '| what | kernel(s) | ms |', '|---|---|---|',
             '| both kernels (`get_impedance`, admittance and transfer functions) | `cateis::kinetic_kernel`, `%s` | %s |' % (f['kernel'], spread(f['both'])),
             '| kinetic kernel alone (`get_kinetic_admittance`) | `cateis::kinetic_kernel` | %s |' % spread(f['kinetic']),
             '| electrode kernel (difference of the two medians) | `%s` | %.2f |' % (f['kernel'], med['both'] - med['kinetic']),
             '| the same transfer functions by %d calls of `get_response` | %s | %s |' % (f['N'] + 1, ', '.join('`%s`' % k for k in f['resp_kernels']),
                                                                                       spread(f['resp'])),
             '', 'Kernel time of the %d `get_response` calls over both kernels of `get_impedance`: %.2f.  Wall time of the calls with their copies: '
             '`get_impedance` %s ms, the %d `get_response` calls %s ms (ratio of the medians %.2f).  `tc`, `tphi` bit-identical to '
             '`get_response(\'phiM\')`: %s.' % (f['N'] + 1, med['resp'] / med['both'], spread(f['wall_eis']), f['N'] + 1, spread(f['wall_resp']),
                                              med['wall_resp'] / med['wall_eis'], 'yes' if f['same'] else 'no'),
             '', 'Re Y(0) over the sweep: %.3e .. %.3e A m^-2 V^-1; |Y| at the highest frequency: %.3e .. %.3e.'
             % (np.nanmin(f['y0']), np.nanmax(f['y0']), np.nanmin(np.abs(f['y_hi'])), np.nanmax(np.abs(f['y_hi']))),
             '', 'Compiler figures (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage; the LDS of the kinetic kernel is '
             'dynamic, (2 T^2 + 4 T + 3 N) x 512 B per wave: %d B here, T = %d):' % ((2 * f['T'] ** 2 + 4 * f['T'] + 3 * f['N']) * 512, f['T']), '',
             '| kernel | VGPRs | AGPRs | SGPRs | scratch, bytes per lane | static LDS, bytes | waves per SIMD |', '|---|---|---|---|---|---|---|']
    lines += ['| `%s` | %s | %s | %s | %s | %s | %s |' % row for row in resources(a.resources)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as out:
        out.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
