#!/usr/bin/env python3
"""The microkinetic SCF loop on the device (libcatint_scfkin, pnp_scf_cycle_fn) next to the host loop it replaces.  One run on one MI355X
writes profiles/scfkin_probe.md (or the file given as the first argument); no figure in it is fixed in advance.

Workload: the chemistry of the end-to-end case of tests/test_gpu_kinetics.py (K+, HCO3-, CO2, CO at a Stern wall, CO2 + * <-> CO2*,
CO2* + 2 e- <-> CO + *), 64 cells, B = 8, 512 and 4096 potentials between -0.30 and -0.38 V, tau_scf = 1e-8, mix_scf = 0.5; and once, at
B = 512, with mix_scf = 0.02 and max_iter = 400 (a long loop: both paths run all 400 iterations).
Timing: the wall time of Calculator.run_scf_cycle() with set_microkinetics(device_loop=False) and (device_loop=True), the two alternating
in one process; one warm-up each, then five repeats; median, minimum and maximum.  In the device path the call of PnpSolver.scf_cycle
is wrapped in pnp_timer_start / pnp_timer_stop (HIP events on the handle's stream): its share of the wall time is the share of the run
in which the device had the loop.
Compiler figures: both kernels compiled from the tree by this script with -Rpass-analysis=kernel-resource-usage."""
import collections
import os
import re
import subprocess
import sys
import time

import numpy as np

R = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, R)

from catint_amd import _capi                             # noqa: E402
from catint_amd.calculator import Calculator             # noqa: E402
from catint_amd.microkinetics import MeanFieldModel      # noqa: E402
from catint_amd.transport import Transport               # noqa: E402

REPEATS, WARMUPS = 5, 1
DEVICE_MS = []


def transport(B):
    phis = list(np.linspace(-0.30, -0.38, B))
    species = collections.OrderedDict([('K+', {'bulk_concentration': 100.0}), ('HCO3-', {'bulk_concentration': 100.0}),
                                       ('CO2', {'bulk_concentration': 34.0}), ('CO', {'bulk_concentration': 0.0})])
    sysd = {'phiM': phis[0], 'boundary thickness': 4e-8, 'Stern capacitance': 20.0, 'phiPZC': 0.1}
    return Transport(species=species, system=sysd, nx=64, descriptors={'phiM': phis})


def model(tp):
    return MeanFieldModel(list(tp.species.keys()), {'CO2': 1}, ['CO2_g + *_t <-> CO2*_t', 'CO2*_t + 2ele_g <-> TS_t <-> CO_g + *_t; beta=0.5'],
                          {'CO2': (0.10, 0.004, 0.0), 'TS': (0.62, 0.004, 0.0)}, solution_energies={'CO': -0.2}, site_density=2e-6)


def one_run(B, device_loop, mix, max_iter):
    tp = transport(B)
    calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-8, mix_scf=mix)
    calc.set_microkinetics(model(tp), site_density=2e-6, device_loop=device_loop)
    del DEVICE_MS[:]
    t0 = time.perf_counter()
    out = calc.run_scf_cycle(max_iter=max_iter)
    return time.perf_counter() - t0, out, (DEVICE_MS[0] if DEVICE_MS else None)


def timed_scf_cycle(self, *args, **kw):
    self.timer_start()
    try:
        return ORIGINAL(self, *args, **kw)
    finally:
        DEVICE_MS.append(self.timer_stop())


ORIGINAL = _capi.PnpSolver.scf_cycle
_capi.PnpSolver.scf_cycle = timed_scf_cycle


def spread(v):
    return '%.1f (min %.1f, max %.1f)' % (1e3 * float(np.median(v)), 1e3 * min(v), 1e3 * max(v))


def measure(B, mix, max_iter, lines, verdicts):
    wall = {False: [], True: []}
    dev_ms, outs = [], {}
    for r in range(REPEATS + WARMUPS):
        for device_loop in (False, True):
            t, out, ms = one_run(B, device_loop, mix, max_iter)
            if r >= WARMUPS:
                wall[device_loop].append(t)
                if device_loop:
                    dev_ms.append(ms)
            outs[device_loop] = out
    host, dev = outs[False], outs[True]
    same = all(np.array_equal(host[k], dev[k], equal_nan=True) for k in ('surface_concentration', 'flux', 'coverage', 'accuracy', 'mix'))
    it = host['iterations']
    hm, dm = float(np.median(wall[False])), float(np.median(wall[True]))
    host_its = len(dev['history'])
    lines.append('| %d | %g | %d (device path: %d; %d on the host, then the device) | %d / %d | %s | %s | %.2f | %.2f | %.2f | %.0f %% | %s |'
                 % (B, mix, it, dev['iterations'], host_its, int(host['converged'].sum()), int(dev['converged'].sum()), spread(wall[False]), spread(wall[True]),
                    1e3 * hm / it, 1e3 * dm / dev['iterations'], hm / dm, 100.0 * float(np.median(dev_ms)) * 1e-3 / dm, 'yes' if same else 'no'))
    verdicts.append((B, mix, hm, dm, max(wall[False]) - min(wall[False])))
    print(lines[-1], flush=True)


def resources():
    """(kernel, VGPRs, SGPRs, scratch bytes per lane, static LDS bytes) of the two kernels, compiled from the tree"""
    rows = []
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    for src, kernel in (('kinetics/catkin.hip', 'catkin::steady_kernel'), ('scfkin/catscfkin.hip', 'catsk::flux_kernel')):
        cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only', '-c', os.path.join(R, 'catint_amd', 'csrc', src), '-o', os.devnull,
               '-Rpass-analysis=kernel-resource-usage']
        r = subprocess.run(cmd, capture_output=True, text=True)
        text = r.stdout + r.stderr

        def num(label):
            m = re.search(r'%s: (\d+)' % re.escape(label), text)
            return m.group(1) if m else '?'
        rows.append((kernel, num(' VGPRs'), num('TotalSGPRs'), num('ScratchSize [bytes/lane]'), num('LDS Size [bytes/block]')))
    return rows


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(R, 'profiles', 'scfkin_probe.md')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    lines = ['# The microkinetic SCF loop: host loop against device loop (tools/probe/scfkin_probe.py, one MI355X)', '',
             'Wall time of `Calculator.run_scf_cycle()` in ms, median (minimum, maximum) of %d repeats after %d warm-up, the two paths alternating '
             'in one process.  Host path: `set_microkinetics(device_loop=False)`, per iteration one `catkin_solve` and one `pnp_solve_surface` with '
             'their copies.  Device path: `device_loop=True`, the host iterations until the hand-over, then `pnp_scf_cycle_fn` with '
             '`catsk_flux_fn`.  Device share: `pnp_timer_start` / `pnp_timer_stop` around that call over the wall time of the run.  The '
             'end-to-end case of the tests (N = 4, 64 cells, S = 1), tau_scf = 1e-8; the row with mix_scf = 0.02 runs max_iter = 400 iterations '
             'in both paths.' % (REPEATS, WARMUPS), '',
             '| B | mix_scf | SCF iterations | converged lanes, host / device | host path, ms | device path, ms | host path per iteration, ms | '
             'device path per iteration, ms | host / device | device share of the device path | results bit-identical |',
             '|---|---|---|---|---|---|---|---|---|---|---|']
    verdicts = []
    for B in (8, 512, 4096):
        measure(B, 0.5, 1000, lines, verdicts)
    measure(512, 0.02, 400, lines, verdicts)
    lines += ['', 'Acceptance: at B = 4096 the median of the device path is not above the median of the host path plus the host path\'s own '
              'spread (maximum - minimum of its five runs).']
    for B, mix, hm, dm, sp in verdicts:
        lines.append('- B = %d, mix_scf = %g: device %.1f ms, host %.1f ms + spread %.1f ms: %s' % (B, mix, 1e3 * dm, 1e3 * hm, 1e3 * sp,
                                                                                                   'met' if dm <= hm + sp else 'NOT met'))
    lines += ['', 'Compiler figures (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage, the tree this run was made from; LDS is '
              'dynamic, (max(T^2, N) + 3 T + 2 N) x 512 B per wave for both kernels):', '',
              '| kernel | VGPRs | SGPRs | scratch, bytes per lane | static LDS, bytes |', '|---|---|---|---|---|']
    lines += ['| `%s` | %s | %s | %s | %s |' % row for row in resources()]
    with open(path, 'w') as out:
        out.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
