"""Census of the compiled solver kernel instances (test infrastructure, no tests of its own).

The library compiles a few hundred template instances of its solver kernels; options, physics and batch size pick one at run time.
CENSUS maps every instance of the twelve solver families to ONE case that forces it through existing options, and
tests/test_gpu_kernel_census.py runs each case against the oracles.  Every other kernel of the library is listed in COVERED_ELSEWHERE
with the test that runs it.  tests/test_kernel_census.py checks, without a GPU, that the two maps together are exactly the kernels of
the built library (read from its gfx950 code objects), that every census instance appears in the committed record of a traced run of
the census module (profiles/kernel_census_dispatched.txt), and that every covering test dispatched its kernels when it was traced on
its own (profiles/kernel_census_covered.txt); tools/kernel_census_dispatched.py writes both records.

Names are in the census's own form: the demangled kernel name without return type, namespace, parameter list and clone suffix,
template arguments kept -- `newton_lane_kernel<3, 0, true, false>`, `bdf2_accumulate_kernel`.
"""
import os
import shutil
import struct
import subprocess
import tempfile
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'catint_amd', 'lib', 'libcatint_pnp.so')
DISPATCHED = os.path.join(ROOT, 'profiles', 'kernel_census_dispatched.txt')
COVERED = os.path.join(ROOT, 'profiles', 'kernel_census_covered.txt')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'

# the twelve solver families whose every instance has a census case
FAMILIES = ('newton_lane_kernel', 'newton_lane2_kernel', 'newton_lane4_kernel', 'newton_pair_kernel', 'newton_kernel', 'newton_team_kernel',
            'newton_sweep_kernel', 'newton_sweep2_kernel', 'step_kernel', 'step_kernel_rr', 'step_kernel_st', 'step_kernel_mw',
            'poisson_kernel_mw')


def census_name(name):
    """Census form of a kernel name: demangled (`void pnp::f<3, true>(pnp::Args) [clone .kd]`), a bare symbol (`f.kd`) or a trace's
    kernel name -> `f<3, true>`."""
    s = name.strip()
    for suffix in (' [clone .kd]', '.kd'):
        if s.endswith(suffix):
            s = s[:-len(suffix)]
    depth = 0
    for i, ch in enumerate(s):          # the parameter list starts at the first '(' outside the template argument list
        if ch == '<':
            depth += 1
        elif ch == '>':
            depth -= 1
        elif ch == '(' and depth == 0:
            s = s[:i]
            break
    if s.startswith('void '):
        s = s[5:]
    if s.startswith('pnp::'):
        s = s[5:]
    return s.strip()


def family(name):
    return name.split('<', 1)[0]


Case = namedtuple('Case', 'path kernel N nx B physics stepper method pb launch rates env')


def newton(kernel, N, nx, B, physics, stepper, **env):
    """Physical mode: CATINT_NEWTON_KERNEL=kernel (+ the options env), N species, nx points, B operating points.
    physics: '+'-joined of point (Dirichlet wall, point ions), stern (Stern wall), steric (size-modified ions, Stern wall), rx (homogeneous
    reactions), conv (convection), wk (wall kinetics, Stern wall).  stepper: stat (stationary), be (backward Euler), bdf2, pred
    (predictor), bdf2+pred; transient cases take three steps from the bulk state."""
    return Case('newton', kernel, N, nx, B, physics, stepper, None, None, None, False, tuple(sorted(env.items())))


def compat(N, nx, B, method, pb, launch, rates=False, **env):
    """Compat mode: method CN / FTCS, Poisson branch pb (dd, vwall_gbulk, gwall_vbulk, vwall_gwall, vbulk_gbulk, or all: every branch in
    turn), launch: step (one launch per timestep) or fused (all four steps of the case in one launch); rates: homogeneous reactions
    (FTCS rate terms); env: the CATINT_* options that force the instance."""
    return Case('compat', None, N, nx, B, None, None, method, pb, launch, rates, tuple(sorted(env.items())))


CENSUS = {
    # ---- newton_lane_kernel<NB, MODE, FUSED, R32> (pnp_lane.hip, 32 points per group): N = NB - 1
    'newton_lane_kernel<2, 0, false, false>': newton('lane', 1, 40, 45, 'point', 'stat', LANE_FUSED=0, NEWTON_LANE_GROUPS=1),
    'newton_lane_kernel<2, 0, true, false>': newton('lane', 1, 33, 45, 'stern', 'be'),
    'newton_lane_kernel<2, 1, false, false>': newton('lane', 1, 64, 45, 'steric', 'bdf2', LANE_FUSED=0),
    'newton_lane_kernel<2, 1, true, false>': newton('lane', 1, 47, 45, 'steric', 'pred'),
    'newton_lane_kernel<2, 2, false, false>': newton('lane', 1, 96, 45, 'conv', 'be', LANE_FUSED=0),
    'newton_lane_kernel<2, 2, true, false>': newton('lane', 1, 25, 45, 'conv+steric', 'stat'),
    'newton_lane_kernel<3, 0, false, false>': newton('lane', 2, 40, 45, 'point', 'be', LANE_FUSED=0, NEWTON_LANE_GROUPS=1),
    'newton_lane_kernel<3, 0, true, false>': newton('lane', 2, 33, 45, 'stern', 'bdf2'),
    'newton_lane_kernel<3, 0, true, true>': newton('lane', 2, 64, 37, 'point', 'pred', LANE_RECORDS='f32'),
    'newton_lane_kernel<3, 1, false, false>': newton('lane', 2, 47, 45, 'steric', 'bdf2+pred', LANE_FUSED=0),
    'newton_lane_kernel<3, 1, true, false>': newton('lane', 2, 96, 45, 'steric', 'stat'),
    'newton_lane_kernel<3, 1, true, true>': newton('lane', 2, 25, 37, 'steric', 'be', LANE_RECORDS='f32'),
    'newton_lane_kernel<3, 2, false, false>': newton('lane', 2, 40, 45, 'rx+steric', 'bdf2', LANE_FUSED=0),
    'newton_lane_kernel<3, 2, true, false>': newton('lane', 2, 33, 45, 'conv', 'pred'),
    'newton_lane_kernel<3, 2, true, true>': newton('lane', 2, 64, 37, 'rx+steric', 'bdf2+pred', LANE_RECORDS='f32'),
    'newton_lane_kernel<4, 0, false, false>': newton('lane', 3, 47, 45, 'point', 'stat', LANE_FUSED=0, NEWTON_LANE_GROUPS=1),
    'newton_lane_kernel<4, 0, true, false>': newton('lane', 3, 96, 45, 'stern', 'be'),
    'newton_lane_kernel<4, 0, true, true>': newton('lane', 3, 25, 37, 'wk', 'stat', LANE_RECORDS='f32'),
    'newton_lane_kernel<4, 1, false, false>': newton('lane', 3, 40, 45, 'steric', 'pred', LANE_FUSED=0),
    'newton_lane_kernel<4, 1, true, false>': newton('lane', 3, 33, 45, 'steric', 'bdf2+pred'),
    'newton_lane_kernel<4, 1, true, true>': newton('lane', 3, 64, 37, 'steric', 'stat', LANE_RECORDS='f32'),
    'newton_lane_kernel<4, 2, false, false>': newton('lane', 3, 47, 45, 'conv', 'be', LANE_FUSED=0),
    'newton_lane_kernel<4, 2, true, false>': newton('lane', 3, 96, 45, 'rx+steric', 'bdf2'),
    'newton_lane_kernel<4, 2, true, true>': newton('lane', 3, 25, 37, 'conv+steric', 'pred', LANE_RECORDS='f32'),
    'newton_lane_kernel<5, 0, false, false>': newton('lane', 4, 40, 45, 'point', 'bdf2+pred', LANE_FUSED=0, NEWTON_LANE_GROUPS=1),
    'newton_lane_kernel<5, 0, true, false>': newton('lane', 4, 33, 45, 'stern', 'stat'),
    'newton_lane_kernel<5, 0, true, true>': newton('lane', 4, 64, 37, 'wk', 'stat', LANE_RECORDS='f32'),
    'newton_lane_kernel<5, 1, false, false>': newton('lane', 4, 47, 45, 'steric', 'bdf2', LANE_FUSED=0),
    'newton_lane_kernel<5, 1, true, false>': newton('lane', 4, 96, 45, 'steric', 'pred'),
    'newton_lane_kernel<5, 1, true, true>': newton('lane', 4, 25, 37, 'steric', 'bdf2+pred', LANE_RECORDS='f32'),
    'newton_lane_kernel<5, 2, false, false>': newton('lane', 4, 40, 45, 'rx+steric', 'stat', LANE_FUSED=0),
    'newton_lane_kernel<5, 2, true, false>': newton('lane', 4, 33, 45, 'conv+steric', 'be'),
    'newton_lane_kernel<5, 2, true, true>': newton('lane', 4, 64, 37, 'rx+steric', 'bdf2', LANE_RECORDS='f32'),
    'newton_lane_kernel<6, 0, false, false>': newton('lane', 5, 47, 45, 'point', 'pred', LANE_FUSED=0, NEWTON_LANE_GROUPS=1),
    'newton_lane_kernel<6, 0, true, false>': newton('lane', 5, 96, 45, 'stern', 'bdf2+pred'),
    'newton_lane_kernel<6, 0, true, true>': newton('lane', 5, 25, 37, 'wk', 'stat', LANE_RECORDS='f32'),
    'newton_lane_kernel<6, 1, false, false>': newton('lane', 5, 40, 45, 'steric', 'be', LANE_FUSED=0),
    'newton_lane_kernel<6, 1, true, false>': newton('lane', 5, 33, 45, 'steric', 'bdf2'),
    'newton_lane_kernel<6, 1, true, true>': newton('lane', 5, 64, 37, 'steric', 'pred', LANE_RECORDS='f32'),
    'newton_lane_kernel<6, 2, false, false>': newton('lane', 5, 47, 45, 'conv+steric', 'be', LANE_FUSED=0),
    'newton_lane_kernel<6, 2, true, false>': newton('lane', 5, 96, 45, 'rx', 'stat'),
    'newton_lane_kernel<6, 2, true, true>': newton('lane', 5, 25, 37, 'conv', 'be', LANE_RECORDS='f32'),
    'newton_lane_kernel<7, 0, false, false>': newton('lane', 6, 40, 45, 'point', 'bdf2', LANE_FUSED=0, NEWTON_LANE_GROUPS=1),
    'newton_lane_kernel<7, 0, true, false>': newton('lane', 6, 33, 45, 'stern', 'pred'),
    'newton_lane_kernel<7, 0, true, true>': newton('lane', 6, 64, 37, 'wk', 'stat', LANE_RECORDS='f32'),
    'newton_lane_kernel<7, 1, false, false>': newton('lane', 6, 47, 45, 'steric', 'stat', LANE_FUSED=0),
    'newton_lane_kernel<7, 1, true, false>': newton('lane', 6, 96, 45, 'steric', 'be'),
    'newton_lane_kernel<7, 1, true, true>': newton('lane', 6, 25, 37, 'steric', 'bdf2', LANE_RECORDS='f32'),
    'newton_lane_kernel<7, 2, false, false>': newton('lane', 6, 40, 45, 'rx', 'pred', LANE_FUSED=0),
    'newton_lane_kernel<7, 2, true, false>': newton('lane', 6, 33, 45, 'conv', 'be'),
    'newton_lane_kernel<7, 2, true, true>': newton('lane', 6, 64, 37, 'rx+steric', 'stat', LANE_RECORDS='f32'),
    'newton_lane_kernel<8, 0, false, false>': newton('lane', 7, 47, 45, 'point', 'be', LANE_FUSED=0, NEWTON_LANE_GROUPS=1),
    'newton_lane_kernel<8, 0, true, false>': newton('lane', 7, 96, 45, 'stern', 'bdf2'),
    'newton_lane_kernel<8, 0, true, true>': newton('lane', 7, 25, 37, 'wk', 'stat', LANE_RECORDS='f32'),
    'newton_lane_kernel<8, 1, false, false>': newton('lane', 7, 40, 45, 'steric', 'bdf2+pred', LANE_FUSED=0),
    'newton_lane_kernel<8, 1, true, false>': newton('lane', 7, 33, 45, 'steric', 'stat'),
    'newton_lane_kernel<8, 1, true, true>': newton('lane', 7, 64, 37, 'steric', 'be', LANE_RECORDS='f32'),
    'newton_lane_kernel<8, 2, false, false>': newton('lane', 7, 47, 45, 'conv', 'be', LANE_FUSED=0),
    'newton_lane_kernel<8, 2, true, false>': newton('lane', 7, 96, 45, 'rx+steric', 'pred'),
    'newton_lane_kernel<8, 2, true, true>': newton('lane', 7, 25, 37, 'conv+steric', 'be', LANE_RECORDS='f32'),
    'newton_lane_kernel<9, 0, false, false>': newton('lane', 8, 40, 45, 'point', 'stat', LANE_FUSED=0, NEWTON_LANE_GROUPS=1),
    'newton_lane_kernel<9, 0, true, false>': newton('lane', 8, 33, 45, 'stern', 'be'),
    'newton_lane_kernel<9, 0, true, true>': newton('lane', 8, 64, 37, 'wk', 'stat', LANE_RECORDS='f32'),
    'newton_lane_kernel<9, 1, false, false>': newton('lane', 8, 47, 45, 'steric', 'pred', LANE_FUSED=0),
    'newton_lane_kernel<9, 1, true, false>': newton('lane', 8, 96, 45, 'steric', 'bdf2+pred'),
    'newton_lane_kernel<9, 1, true, true>': newton('lane', 8, 25, 37, 'steric', 'stat', LANE_RECORDS='f32'),
    'newton_lane_kernel<9, 2, false, false>': newton('lane', 8, 40, 45, 'rx+steric', 'be', LANE_FUSED=0),
    'newton_lane_kernel<9, 2, true, false>': newton('lane', 8, 33, 45, 'conv+steric', 'be'),
    'newton_lane_kernel<9, 2, true, true>': newton('lane', 8, 64, 37, 'rx', 'pred', LANE_RECORDS='f32'),
    # ---- newton_lane2_kernel<NB, MODE, BDF> (pnp_lane2.hip, 16 points per group)
    'newton_lane2_kernel<6, 0, false>': newton('lane2', 5, 48, 37, 'point', 'stat'),
    'newton_lane2_kernel<6, 0, true>': newton('lane2', 5, 41, 37, 'stern', 'bdf2'),
    'newton_lane2_kernel<6, 1, false>': newton('lane2', 5, 64, 37, 'steric', 'be', NEWTON_LANE_GROUPS=1),
    'newton_lane2_kernel<6, 1, true>': newton('lane2', 5, 35, 37, 'steric', 'bdf2'),
    'newton_lane2_kernel<6, 2, false>': newton('lane2', 5, 9, 37, 'rx', 'pred'),
    'newton_lane2_kernel<6, 2, true>': newton('lane2', 5, 48, 37, 'rx+steric', 'bdf2'),
    'newton_lane2_kernel<7, 0, false>': newton('lane2', 6, 41, 37, 'point', 'bdf2+pred'),
    'newton_lane2_kernel<7, 0, true>': newton('lane2', 6, 64, 37, 'stern', 'bdf2'),
    'newton_lane2_kernel<7, 1, false>': newton('lane2', 6, 35, 37, 'steric', 'stat', NEWTON_LANE_GROUPS=1),
    'newton_lane2_kernel<7, 1, true>': newton('lane2', 6, 9, 37, 'steric', 'bdf2'),
    'newton_lane2_kernel<7, 2, false>': newton('lane2', 6, 48, 37, 'rx+steric', 'be'),
    'newton_lane2_kernel<7, 2, true>': newton('lane2', 6, 41, 37, 'rx+steric', 'bdf2'),
    'newton_lane2_kernel<8, 0, false>': newton('lane2', 7, 64, 37, 'point', 'pred'),
    'newton_lane2_kernel<8, 0, true>': newton('lane2', 7, 35, 37, 'stern', 'bdf2'),
    'newton_lane2_kernel<8, 1, false>': newton('lane2', 7, 9, 37, 'steric', 'bdf2+pred', NEWTON_LANE_GROUPS=1),
    'newton_lane2_kernel<8, 1, true>': newton('lane2', 7, 48, 37, 'steric', 'bdf2'),
    'newton_lane2_kernel<8, 2, false>': newton('lane2', 7, 41, 37, 'rx', 'stat'),
    'newton_lane2_kernel<8, 2, true>': newton('lane2', 7, 64, 37, 'rx+steric', 'bdf2'),
    'newton_lane2_kernel<9, 0, false>': newton('lane2', 8, 35, 37, 'point', 'be'),
    'newton_lane2_kernel<9, 0, true>': newton('lane2', 8, 9, 37, 'stern', 'bdf2'),
    'newton_lane2_kernel<9, 1, false>': newton('lane2', 8, 48, 37, 'steric', 'pred', NEWTON_LANE_GROUPS=1),
    'newton_lane2_kernel<9, 1, true>': newton('lane2', 8, 41, 37, 'steric', 'bdf2'),
    'newton_lane2_kernel<9, 2, false>': newton('lane2', 8, 64, 37, 'rx+steric', 'bdf2+pred'),
    'newton_lane2_kernel<9, 2, true>': newton('lane2', 8, 35, 37, 'rx+steric', 'bdf2'),
    # ---- newton_lane4_kernel<NB, MODE, BDF> (pnp_lane4.hip, 8 points per group)
    'newton_lane4_kernel<6, 0, false>': newton('lane4', 5, 48, 21, 'point', 'stat'),
    'newton_lane4_kernel<6, 0, true>': newton('lane4', 5, 41, 21, 'stern', 'bdf2'),
    'newton_lane4_kernel<6, 1, false>': newton('lane4', 5, 64, 21, 'steric', 'be', NEWTON_LANE_GROUPS=1),
    'newton_lane4_kernel<6, 1, true>': newton('lane4', 5, 35, 21, 'steric', 'bdf2'),
    'newton_lane4_kernel<6, 2, false>': newton('lane4', 5, 9, 21, 'rx', 'pred'),
    'newton_lane4_kernel<6, 2, true>': newton('lane4', 5, 48, 21, 'rx+steric', 'bdf2'),
    'newton_lane4_kernel<7, 0, false>': newton('lane4', 6, 41, 21, 'point', 'bdf2+pred'),
    'newton_lane4_kernel<7, 0, true>': newton('lane4', 6, 64, 21, 'stern', 'bdf2'),
    'newton_lane4_kernel<7, 1, false>': newton('lane4', 6, 35, 21, 'steric', 'stat', NEWTON_LANE_GROUPS=1),
    'newton_lane4_kernel<7, 1, true>': newton('lane4', 6, 9, 21, 'steric', 'bdf2'),
    'newton_lane4_kernel<7, 2, false>': newton('lane4', 6, 48, 21, 'rx+steric', 'be'),
    'newton_lane4_kernel<7, 2, true>': newton('lane4', 6, 41, 21, 'rx+steric', 'bdf2'),
    'newton_lane4_kernel<8, 0, false>': newton('lane4', 7, 64, 21, 'point', 'pred'),
    'newton_lane4_kernel<8, 0, true>': newton('lane4', 7, 35, 21, 'stern', 'bdf2'),
    'newton_lane4_kernel<8, 1, false>': newton('lane4', 7, 9, 21, 'steric', 'bdf2+pred', NEWTON_LANE_GROUPS=1),
    'newton_lane4_kernel<8, 1, true>': newton('lane4', 7, 48, 21, 'steric', 'bdf2'),
    'newton_lane4_kernel<8, 2, false>': newton('lane4', 7, 41, 21, 'rx', 'stat'),
    'newton_lane4_kernel<8, 2, true>': newton('lane4', 7, 64, 21, 'rx+steric', 'bdf2'),
    'newton_lane4_kernel<9, 0, false>': newton('lane4', 8, 35, 21, 'point', 'be'),
    'newton_lane4_kernel<9, 0, true>': newton('lane4', 8, 9, 21, 'stern', 'bdf2'),
    'newton_lane4_kernel<9, 1, false>': newton('lane4', 8, 48, 21, 'steric', 'pred', NEWTON_LANE_GROUPS=1),
    'newton_lane4_kernel<9, 1, true>': newton('lane4', 8, 41, 21, 'steric', 'bdf2'),
    'newton_lane4_kernel<9, 2, false>': newton('lane4', 8, 64, 21, 'rx+steric', 'bdf2+pred'),
    'newton_lane4_kernel<9, 2, true>': newton('lane4', 8, 35, 21, 'rx+steric', 'bdf2'),
    # ---- newton_pair_kernel<NB, TS, MODE> (pnp_newton.hip; TS: threads rounded up to 64 / 128 / 256 / 512, nx <= 2 TS)
    'newton_pair_kernel<2, 128, 0>': newton('workgroup', 1, 129, 5, 'point', 'stat'),
    'newton_pair_kernel<2, 128, 1>': newton('workgroup', 1, 256, 5, 'steric+conv', 'be'),
    'newton_pair_kernel<2, 128, 2>': newton('workgroup', 1, 201, 5, 'rx', 'bdf2'),
    'newton_pair_kernel<2, 256, 0>': newton('workgroup', 1, 257, 5, 'stern', 'pred'),
    'newton_pair_kernel<2, 256, 1>': newton('workgroup', 1, 512, 5, 'steric', 'stat'),
    'newton_pair_kernel<2, 256, 2>': newton('workgroup', 1, 383, 5, 'rx', 'be'),
    'newton_pair_kernel<2, 512, 0>': newton('workgroup', 1, 513, 5, 'point', 'bdf2'),
    'newton_pair_kernel<2, 512, 1>': newton('workgroup', 1, 1024, 5, 'steric+conv', 'pred'),
    'newton_pair_kernel<2, 512, 2>': newton('workgroup', 1, 777, 5, 'rx', 'stat'),
    'newton_pair_kernel<2, 64, 0>': newton('workgroup', 1, 128, 5, 'stern', 'be'),
    'newton_pair_kernel<2, 64, 1>': newton('workgroup', 1, 63, 5, 'steric', 'bdf2'),
    'newton_pair_kernel<2, 64, 2>': newton('workgroup', 1, 100, 5, 'rx', 'pred'),
    'newton_pair_kernel<3, 128, 0>': newton('workgroup', 2, 129, 5, 'point', 'stat'),
    'newton_pair_kernel<3, 128, 1>': newton('workgroup', 2, 256, 5, 'steric+conv', 'be'),
    'newton_pair_kernel<3, 128, 2>': newton('workgroup', 2, 201, 5, 'rx+conv', 'be'),
    'newton_pair_kernel<3, 256, 0>': newton('workgroup', 2, 257, 5, 'stern', 'pred'),
    'newton_pair_kernel<3, 256, 1>': newton('workgroup', 2, 512, 5, 'steric', 'stat'),
    'newton_pair_kernel<3, 256, 2>': newton('workgroup', 2, 383, 5, 'rx+conv', 'be'),
    'newton_pair_kernel<3, 512, 0>': newton('workgroup', 2, 513, 5, 'point', 'bdf2'),
    'newton_pair_kernel<3, 512, 1>': newton('workgroup', 2, 1024, 5, 'steric+conv', 'pred'),
    'newton_pair_kernel<3, 512, 2>': newton('workgroup', 2, 777, 5, 'rx+conv', 'stat'),
    'newton_pair_kernel<3, 64, 0>': newton('workgroup', 2, 128, 5, 'stern', 'be'),
    'newton_pair_kernel<3, 64, 1>': newton('workgroup', 2, 63, 5, 'steric', 'bdf2'),
    'newton_pair_kernel<3, 64, 2>': newton('workgroup', 2, 100, 5, 'rx+conv', 'pred'),
    'newton_pair_kernel<4, 128, 0>': newton('workgroup', 3, 129, 5, 'point', 'stat'),
    'newton_pair_kernel<4, 128, 1>': newton('workgroup', 3, 256, 5, 'steric+conv', 'be'),
    'newton_pair_kernel<4, 128, 2>': newton('workgroup', 3, 201, 5, 'rx+conv', 'be'),
    'newton_pair_kernel<4, 256, 0>': newton('workgroup', 3, 257, 5, 'point', 'pred'),
    'newton_pair_kernel<4, 256, 1>': newton('workgroup', 3, 512, 5, 'steric', 'stat'),
    'newton_pair_kernel<4, 256, 2>': newton('workgroup', 3, 383, 5, 'rx+conv', 'be'),
    'newton_pair_kernel<4, 512, 0>': newton('workgroup', 3, 513, 5, 'point', 'bdf2'),
    'newton_pair_kernel<4, 512, 1>': newton('workgroup', 3, 1024, 5, 'steric+conv', 'pred'),
    'newton_pair_kernel<4, 512, 2>': newton('workgroup', 3, 777, 5, 'rx+conv', 'stat'),
    'newton_pair_kernel<4, 64, 0>': newton('workgroup', 3, 128, 5, 'point', 'be'),
    'newton_pair_kernel<4, 64, 1>': newton('workgroup', 3, 63, 5, 'steric', 'bdf2'),
    'newton_pair_kernel<4, 64, 2>': newton('workgroup', 3, 100, 5, 'rx+conv', 'pred'),
    'newton_pair_kernel<5, 128, 0>': newton('workgroup', 4, 129, 5, 'point', 'stat'),
    'newton_pair_kernel<5, 128, 1>': newton('workgroup', 4, 256, 5, 'steric+conv', 'be'),
    'newton_pair_kernel<5, 128, 2>': newton('workgroup', 4, 201, 5, 'rx+conv', 'be'),
    'newton_pair_kernel<5, 256, 0>': newton('workgroup', 4, 257, 5, 'point', 'pred'),
    'newton_pair_kernel<5, 256, 1>': newton('workgroup', 4, 512, 5, 'steric', 'stat'),
    'newton_pair_kernel<5, 256, 2>': newton('workgroup', 4, 383, 5, 'rx+conv', 'be'),
    'newton_pair_kernel<5, 64, 0>': newton('workgroup', 4, 128, 5, 'point', 'bdf2'),
    'newton_pair_kernel<5, 64, 1>': newton('workgroup', 4, 63, 5, 'steric+conv', 'pred'),
    'newton_pair_kernel<5, 64, 2>': newton('workgroup', 4, 100, 5, 'rx+conv', 'stat'),
    # ---- newton_kernel<NB, TMAX, MODE> (pnp_newton.hip, one row per thread; TMAX 256: the 512-register build of NB = 6, 7)
    'newton_kernel<2, 512, 0>': newton('generic', 1, 50, 4, 'point', 'stat'),
    'newton_kernel<2, 512, 1>': newton('generic', 1, 64, 4, 'steric+conv', 'be', NEWTON_EXCHANGE='global'),
    'newton_kernel<2, 512, 2>': newton('generic', 1, 77, 4, 'rx+conv', 'be'),
    'newton_kernel<3, 512, 0>': newton('generic', 2, 130, 4, 'stern', 'pred'),
    'newton_kernel<3, 512, 1>': newton('generic', 2, 9, 4, 'steric', 'stat', NEWTON_EXCHANGE='global'),
    'newton_kernel<3, 512, 2>': newton('generic', 2, 50, 4, 'rx+conv', 'be'),
    'newton_kernel<4, 512, 0>': newton('generic', 3, 64, 4, 'point', 'bdf2'),
    'newton_kernel<4, 512, 1>': newton('generic', 3, 77, 4, 'steric+conv', 'pred', NEWTON_EXCHANGE='global'),
    'newton_kernel<4, 512, 2>': newton('generic', 3, 130, 4, 'rx+conv', 'stat'),
    'newton_kernel<5, 512, 0>': newton('generic', 4, 9, 4, 'point', 'be'),
    'newton_kernel<5, 512, 1>': newton('generic', 4, 50, 4, 'steric', 'bdf2'),
    'newton_kernel<5, 512, 2>': newton('generic', 4, 64, 4, 'rx+conv', 'pred'),
    'newton_kernel<6, 512, 0>': newton('generic', 5, 77, 4, 'point', 'stat'),
    'newton_kernel<6, 512, 1>': newton('generic', 5, 130, 4, 'steric+conv', 'be'),
    'newton_kernel<6, 512, 2>': newton('generic', 5, 9, 4, 'rx+conv', 'be'),
    'newton_kernel<6, 256, 0>': newton('generic', 5, 50, 4, 'point', 'pred', NEWTON_REGS=512),
    'newton_kernel<6, 256, 1>': newton('generic', 5, 64, 4, 'steric', 'stat', NEWTON_REGS=512),
    'newton_kernel<6, 256, 2>': newton('generic', 5, 77, 4, 'rx+conv', 'be', NEWTON_REGS=512),
    'newton_kernel<7, 512, 0>': newton('generic', 6, 130, 4, 'point', 'bdf2'),
    'newton_kernel<7, 512, 1>': newton('generic', 6, 9, 4, 'steric+conv', 'pred'),
    'newton_kernel<7, 512, 2>': newton('generic', 6, 50, 4, 'rx+conv', 'stat'),
    'newton_kernel<7, 256, 0>': newton('generic', 6, 64, 4, 'point', 'be', NEWTON_REGS=512),
    'newton_kernel<7, 256, 1>': newton('generic', 6, 77, 4, 'steric', 'bdf2', NEWTON_REGS=512),
    'newton_kernel<7, 256, 2>': newton('generic', 6, 130, 4, 'rx+conv', 'pred', NEWTON_REGS=512),
    # ---- newton_team_kernel<NB, MODE> (pnp_newton.hip)
    'newton_team_kernel<3, 0>': newton('team', 2, 40, 7, 'stern', 'bdf2', NEWTON_EXCHANGE='global'),
    'newton_team_kernel<3, 1>': newton('team', 2, 33, 7, 'steric', 'pred', NEWTON_EXCHANGE='global'),
    'newton_team_kernel<3, 2>': newton('team', 2, 64, 7, 'rx', 'stat', NEWTON_EXCHANGE='global'),
    'newton_team_kernel<4, 0>': newton('team', 3, 51, 7, 'stern', 'be', NEWTON_EXCHANGE='global'),
    'newton_team_kernel<4, 1>': newton('team', 3, 8, 7, 'steric+conv', 'be', NEWTON_EXCHANGE='global'),
    'newton_team_kernel<4, 2>': newton('team', 3, 40, 7, 'rx', 'pred', NEWTON_EXCHANGE='global'),
    'newton_team_kernel<5, 0>': newton('team', 4, 33, 7, 'stern', 'stat'),
    'newton_team_kernel<5, 1>': newton('team', 4, 64, 7, 'steric', 'be'),
    'newton_team_kernel<5, 2>': newton('team', 4, 51, 7, 'rx+steric', 'bdf2'),
    'newton_team_kernel<6, 0>': newton('team', 5, 8, 7, 'stern', 'pred'),
    'newton_team_kernel<6, 1>': newton('team', 5, 40, 7, 'steric+conv', 'stat'),
    'newton_team_kernel<6, 2>': newton('team', 5, 33, 7, 'rx', 'be'),
    'newton_team_kernel<7, 0>': newton('team', 6, 64, 7, 'stern', 'bdf2'),
    'newton_team_kernel<7, 1>': newton('team', 6, 51, 7, 'steric', 'pred'),
    'newton_team_kernel<7, 2>': newton('team', 6, 8, 7, 'rx', 'stat'),
    'newton_team_kernel<8, 0>': newton('team', 7, 40, 7, 'stern', 'be'),
    'newton_team_kernel<8, 1>': newton('team', 7, 33, 7, 'steric+conv', 'be'),
    'newton_team_kernel<8, 2>': newton('team', 7, 64, 7, 'rx', 'pred'),
    'newton_team_kernel<9, 0>': newton('team', 8, 51, 7, 'stern', 'stat'),
    'newton_team_kernel<9, 1>': newton('team', 8, 8, 7, 'steric', 'be'),
    'newton_team_kernel<9, 2>': newton('team', 8, 40, 7, 'rx+steric', 'bdf2'),
    # ---- newton_sweep_kernel<NB, MODE> (pnp_newton.hip)
    'newton_sweep_kernel<3, 0>': newton('sweep', 2, 40, 23, 'stern', 'bdf2', NEWTON_SWEEP_BLOCKS=1),
    'newton_sweep_kernel<3, 1>': newton('sweep', 2, 33, 23, 'steric', 'pred'),
    'newton_sweep_kernel<3, 2>': newton('sweep', 2, 64, 23, 'rx', 'stat', NEWTON_SWEEP_BLOCKS=1),
    'newton_sweep_kernel<4, 0>': newton('sweep', 3, 51, 23, 'stern', 'be', NEWTON_SWEEP_BLOCKS=2),
    'newton_sweep_kernel<4, 1>': newton('sweep', 3, 8, 23, 'steric+conv', 'be'),
    'newton_sweep_kernel<4, 2>': newton('sweep', 3, 40, 23, 'rx', 'pred', NEWTON_SWEEP_BLOCKS=2),
    'newton_sweep_kernel<5, 0>': newton('sweep', 4, 33, 23, 'stern', 'stat', NEWTON_SWEEP_BLOCKS=1),
    'newton_sweep_kernel<5, 1>': newton('sweep', 4, 64, 23, 'steric', 'be'),
    'newton_sweep_kernel<5, 2>': newton('sweep', 4, 51, 23, 'rx+steric', 'bdf2', NEWTON_SWEEP_BLOCKS=1),
    'newton_sweep_kernel<6, 0>': newton('sweep', 5, 8, 23, 'stern', 'pred', NEWTON_SWEEP_BLOCKS=2),
    'newton_sweep_kernel<6, 1>': newton('sweep', 5, 40, 23, 'steric+conv', 'stat'),
    'newton_sweep_kernel<6, 2>': newton('sweep', 5, 33, 23, 'rx', 'be', NEWTON_SWEEP_BLOCKS=2),
    'newton_sweep_kernel<7, 0>': newton('sweep', 6, 64, 23, 'stern', 'bdf2', NEWTON_SWEEP_BLOCKS=1),
    'newton_sweep_kernel<7, 1>': newton('sweep', 6, 51, 23, 'steric', 'pred'),
    'newton_sweep_kernel<7, 2>': newton('sweep', 6, 8, 23, 'rx', 'stat', NEWTON_SWEEP_BLOCKS=1),
    'newton_sweep_kernel<8, 0>': newton('sweep', 7, 40, 23, 'stern', 'be', NEWTON_SWEEP_BLOCKS=2),
    'newton_sweep_kernel<8, 1>': newton('sweep', 7, 33, 23, 'steric+conv', 'be'),
    'newton_sweep_kernel<8, 2>': newton('sweep', 7, 64, 23, 'rx', 'pred', NEWTON_SWEEP_BLOCKS=2),
    'newton_sweep_kernel<9, 0>': newton('sweep', 8, 51, 23, 'stern', 'stat', NEWTON_SWEEP_BLOCKS=1),
    'newton_sweep_kernel<9, 1>': newton('sweep', 8, 8, 23, 'steric', 'be'),
    'newton_sweep_kernel<9, 2>': newton('sweep', 8, 40, 23, 'rx+steric', 'bdf2', NEWTON_SWEEP_BLOCKS=1),
    # ---- newton_sweep2_kernel<NB, MODE> (pnp_newton.hip)
    'newton_sweep2_kernel<6, 0>': newton('both', 5, 40, 23, 'stern', 'bdf2', NEWTON_SWEEP_BLOCKS=1),
    'newton_sweep2_kernel<6, 1>': newton('both', 5, 33, 23, 'steric', 'pred'),
    'newton_sweep2_kernel<6, 2>': newton('both', 5, 64, 23, 'rx', 'stat', NEWTON_SWEEP_BLOCKS=1),
    'newton_sweep2_kernel<7, 0>': newton('both', 6, 51, 23, 'stern', 'be', NEWTON_SWEEP_BLOCKS=2),
    'newton_sweep2_kernel<7, 1>': newton('both', 6, 8, 23, 'steric+conv', 'be'),
    'newton_sweep2_kernel<7, 2>': newton('both', 6, 40, 23, 'rx', 'pred', NEWTON_SWEEP_BLOCKS=2),
    'newton_sweep2_kernel<8, 0>': newton('both', 7, 33, 23, 'stern', 'stat', NEWTON_SWEEP_BLOCKS=1),
    'newton_sweep2_kernel<8, 1>': newton('both', 7, 64, 23, 'steric', 'be'),
    'newton_sweep2_kernel<8, 2>': newton('both', 7, 51, 23, 'rx+steric', 'bdf2', NEWTON_SWEEP_BLOCKS=1),
    'newton_sweep2_kernel<9, 0>': newton('both', 8, 8, 23, 'stern', 'pred', NEWTON_SWEEP_BLOCKS=2),
    'newton_sweep2_kernel<9, 1>': newton('both', 8, 40, 23, 'steric+conv', 'stat'),
    'newton_sweep2_kernel<9, 2>': newton('both', 8, 33, 23, 'rx', 'be', NEWTON_SWEEP_BLOCKS=2),
    # ---- step_kernel<P, W, G> (pnp_kernels.hip, LDS-staged: W waves per operating point, G species interleaved per wave, slots beyond
    # N - 1 clamped): P from nx (64 P + 2 points at most), forced with PNP_KERNEL = 2 and the W / G options
    'step_kernel<1, 1, 1>': compat(5, 66, 3, 'CN', 'dd', 'step', PNP_KERNEL=2, PNP_WAVES_PER_GRID=1, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<1, 1, 2>': compat(5, 5, 3, 'FTCS', 'vwall_gbulk', 'step', rates=True, PNP_KERNEL=2, PNP_WAVES_PER_GRID=1, PNP_SPECIES_PER_WAVE=2),
    'step_kernel<1, 1, 3>': compat(4, 33, 3, 'CN', 'gwall_vbulk', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=1, PNP_SPECIES_PER_WAVE=3),
    'step_kernel<1, 2, 1>': compat(2, 65, 3, 'FTCS', 'vwall_gwall', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=2, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<1, 2, 2>': compat(5, 66, 3, 'CN', 'all', 'step', PNP_KERNEL=2, PNP_WAVES_PER_GRID=2, PNP_SPECIES_PER_WAVE=2),
    'step_kernel<1, 3, 1>': compat(4, 5, 3, 'FTCS', 'dd', 'step', rates=True, PNP_KERNEL=2, PNP_WAVES_PER_GRID=3, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<1, 4, 1>': compat(2, 33, 3, 'CN', 'vwall_gbulk', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=4, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<2, 1, 1>': compat(2, 130, 3, 'FTCS', 'gwall_vbulk', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=1, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<2, 1, 2>': compat(3, 99, 3, 'CN', 'vwall_gwall', 'step', PNP_KERNEL=2, PNP_WAVES_PER_GRID=1, PNP_SPECIES_PER_WAVE=2),
    'step_kernel<2, 1, 3>': compat(2, 67, 3, 'FTCS', 'vbulk_gbulk', 'step', rates=True, PNP_KERNEL=2, PNP_WAVES_PER_GRID=1, PNP_SPECIES_PER_WAVE=3),
    'step_kernel<2, 2, 1>': compat(3, 130, 3, 'CN', 'dd', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=2, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<2, 2, 2>': compat(3, 99, 3, 'FTCS', 'vwall_gbulk', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=2, PNP_SPECIES_PER_WAVE=2),
    'step_kernel<2, 3, 1>': compat(2, 67, 3, 'CN', 'gwall_vbulk', 'step', PNP_KERNEL=2, PNP_WAVES_PER_GRID=3, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<2, 4, 1>': compat(3, 130, 3, 'FTCS', 'vwall_gwall', 'step', rates=True, PNP_KERNEL=2, PNP_WAVES_PER_GRID=4, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<4, 1, 1>': compat(5, 201, 3, 'CN', 'all', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=1, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<4, 1, 2>': compat(5, 131, 3, 'FTCS', 'dd', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=1, PNP_SPECIES_PER_WAVE=2),
    'step_kernel<4, 1, 3>': compat(4, 258, 3, 'CN', 'vwall_gbulk', 'step', PNP_KERNEL=2, PNP_WAVES_PER_GRID=1, PNP_SPECIES_PER_WAVE=3),
    'step_kernel<4, 2, 1>': compat(2, 201, 3, 'FTCS', 'gwall_vbulk', 'step', rates=True, PNP_KERNEL=2, PNP_WAVES_PER_GRID=2, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<4, 2, 2>': compat(5, 131, 3, 'CN', 'vwall_gwall', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=2, PNP_SPECIES_PER_WAVE=2),
    'step_kernel<4, 3, 1>': compat(4, 258, 3, 'FTCS', 'vbulk_gbulk', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=3, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<4, 4, 1>': compat(2, 201, 3, 'CN', 'dd', 'step', PNP_KERNEL=2, PNP_WAVES_PER_GRID=4, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<8, 1, 1>': compat(2, 259, 3, 'FTCS', 'vwall_gbulk', 'step', rates=True, PNP_KERNEL=2, PNP_WAVES_PER_GRID=1, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<8, 1, 2>': compat(3, 514, 3, 'CN', 'vwall_gwall', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=1, PNP_SPECIES_PER_WAVE=2),
    'step_kernel<8, 1, 3>': compat(2, 333, 3, 'FTCS', 'vwall_gwall', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=1, PNP_SPECIES_PER_WAVE=3),
    'step_kernel<8, 2, 1>': compat(3, 259, 3, 'CN', 'vbulk_gbulk', 'step', PNP_KERNEL=2, PNP_WAVES_PER_GRID=2, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<8, 2, 2>': compat(3, 514, 3, 'FTCS', 'dd', 'step', rates=True, PNP_KERNEL=2, PNP_WAVES_PER_GRID=2, PNP_SPECIES_PER_WAVE=2),
    'step_kernel<8, 3, 1>': compat(2, 333, 3, 'CN', 'vwall_gbulk', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=3, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<8, 4, 1>': compat(3, 259, 3, 'FTCS', 'gwall_vbulk', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=4, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<16, 1, 1>': compat(5, 1026, 3, 'CN', 'vwall_gwall', 'step', PNP_KERNEL=2, PNP_WAVES_PER_GRID=1, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<16, 1, 2>': compat(5, 777, 3, 'FTCS', 'vbulk_gbulk', 'step', rates=True, PNP_KERNEL=2, PNP_WAVES_PER_GRID=1, PNP_SPECIES_PER_WAVE=2),
    'step_kernel<16, 1, 3>': compat(4, 515, 3, 'CN', 'dd', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=1, PNP_SPECIES_PER_WAVE=3),
    'step_kernel<16, 2, 1>': compat(2, 1026, 3, 'FTCS', 'vwall_gbulk', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=2, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<16, 2, 2>': compat(5, 777, 3, 'CN', 'gwall_vbulk', 'step', PNP_KERNEL=2, PNP_WAVES_PER_GRID=2, PNP_SPECIES_PER_WAVE=2),
    'step_kernel<16, 3, 1>': compat(4, 515, 3, 'FTCS', 'vwall_gwall', 'step', rates=True, PNP_KERNEL=2, PNP_WAVES_PER_GRID=3, PNP_SPECIES_PER_WAVE=1),
    'step_kernel<16, 4, 1>': compat(2, 1026, 3, 'CN', 'vbulk_gbulk', 'fused', PNP_KERNEL=2, PNP_WAVES_PER_GRID=4, PNP_SPECIES_PER_WAVE=1),
    # ---- step_kernel_rr<P, W, CN> (register-resident, Dirichlet / Dirichlet only): PNP_KERNEL = 4, W = PNP_WAVES_PER_GRID
    'step_kernel_rr<2, 1, false>': compat(2, 67, 3, 'FTCS', 'dd', 'step', PNP_KERNEL=4, PNP_WAVES_PER_GRID=1),
    'step_kernel_rr<2, 1, true>': compat(3, 130, 3, 'CN', 'dd', 'step', PNP_KERNEL=4, PNP_WAVES_PER_GRID=1),
    'step_kernel_rr<2, 2, false>': compat(4, 99, 3, 'FTCS', 'dd', 'fused', PNP_KERNEL=4, PNP_WAVES_PER_GRID=2),
    'step_kernel_rr<2, 2, true>': compat(5, 67, 3, 'CN', 'dd', 'fused', PNP_KERNEL=4, PNP_WAVES_PER_GRID=2),
    'step_kernel_rr<2, 3, false>': compat(6, 130, 3, 'FTCS', 'dd', 'step', PNP_KERNEL=4, PNP_WAVES_PER_GRID=3),
    'step_kernel_rr<2, 3, true>': compat(2, 99, 3, 'CN', 'dd', 'step', PNP_KERNEL=4, PNP_WAVES_PER_GRID=3),
    'step_kernel_rr<2, 4, false>': compat(3, 67, 3, 'FTCS', 'dd', 'fused', PNP_KERNEL=4, PNP_WAVES_PER_GRID=4),
    'step_kernel_rr<2, 4, true>': compat(4, 130, 3, 'CN', 'dd', 'fused', PNP_KERNEL=4, PNP_WAVES_PER_GRID=4),
    'step_kernel_rr<4, 1, false>': compat(5, 201, 3, 'FTCS', 'dd', 'step', PNP_KERNEL=4, PNP_WAVES_PER_GRID=1),
    'step_kernel_rr<4, 1, true>': compat(6, 131, 3, 'CN', 'dd', 'step', PNP_KERNEL=4, PNP_WAVES_PER_GRID=1),
    'step_kernel_rr<4, 2, false>': compat(2, 258, 3, 'FTCS', 'dd', 'fused', PNP_KERNEL=4, PNP_WAVES_PER_GRID=2),
    'step_kernel_rr<4, 2, true>': compat(3, 201, 3, 'CN', 'dd', 'fused', PNP_KERNEL=4, PNP_WAVES_PER_GRID=2),
    'step_kernel_rr<4, 3, false>': compat(4, 131, 3, 'FTCS', 'dd', 'step', PNP_KERNEL=4, PNP_WAVES_PER_GRID=3),
    'step_kernel_rr<4, 3, true>': compat(5, 258, 3, 'CN', 'dd', 'step', PNP_KERNEL=4, PNP_WAVES_PER_GRID=3),
    'step_kernel_rr<4, 4, false>': compat(6, 201, 3, 'FTCS', 'dd', 'fused', PNP_KERNEL=4, PNP_WAVES_PER_GRID=4),
    'step_kernel_rr<4, 4, true>': compat(2, 131, 3, 'CN', 'dd', 'fused', PNP_KERNEL=4, PNP_WAVES_PER_GRID=4),
    'step_kernel_rr<8, 1, false>': compat(3, 514, 3, 'FTCS', 'dd', 'step', PNP_KERNEL=4, PNP_WAVES_PER_GRID=1),
    'step_kernel_rr<8, 1, true>': compat(4, 333, 3, 'CN', 'dd', 'step', PNP_KERNEL=4, PNP_WAVES_PER_GRID=1),
    'step_kernel_rr<8, 2, false>': compat(5, 259, 3, 'FTCS', 'dd', 'fused', PNP_KERNEL=4, PNP_WAVES_PER_GRID=2),
    'step_kernel_rr<8, 2, true>': compat(6, 514, 3, 'CN', 'dd', 'fused', PNP_KERNEL=4, PNP_WAVES_PER_GRID=2),
    'step_kernel_rr<8, 3, false>': compat(2, 333, 3, 'FTCS', 'dd', 'step', PNP_KERNEL=4, PNP_WAVES_PER_GRID=3),
    'step_kernel_rr<8, 3, true>': compat(3, 259, 3, 'CN', 'dd', 'step', PNP_KERNEL=4, PNP_WAVES_PER_GRID=3),
    'step_kernel_rr<8, 4, false>': compat(4, 514, 3, 'FTCS', 'dd', 'fused', PNP_KERNEL=4, PNP_WAVES_PER_GRID=4),
    'step_kernel_rr<8, 4, true>': compat(5, 333, 3, 'CN', 'dd', 'fused', PNP_KERNEL=4, PNP_WAVES_PER_GRID=4),
    'step_kernel_rr<16, 1, false>': compat(6, 515, 3, 'FTCS', 'dd', 'step', PNP_KERNEL=4, PNP_WAVES_PER_GRID=1),
    'step_kernel_rr<16, 1, true>': compat(2, 1026, 3, 'CN', 'dd', 'step', PNP_KERNEL=4, PNP_WAVES_PER_GRID=1),
    'step_kernel_rr<16, 2, false>': compat(3, 777, 3, 'FTCS', 'dd', 'fused', PNP_KERNEL=4, PNP_WAVES_PER_GRID=2),
    'step_kernel_rr<16, 2, true>': compat(4, 515, 3, 'CN', 'dd', 'fused', PNP_KERNEL=4, PNP_WAVES_PER_GRID=2),
    'step_kernel_rr<16, 3, false>': compat(5, 1026, 3, 'FTCS', 'dd', 'step', PNP_KERNEL=4, PNP_WAVES_PER_GRID=3),
    'step_kernel_rr<16, 3, true>': compat(6, 777, 3, 'CN', 'dd', 'step', PNP_KERNEL=4, PNP_WAVES_PER_GRID=3),
    'step_kernel_rr<16, 4, false>': compat(2, 515, 3, 'FTCS', 'dd', 'fused', PNP_KERNEL=4, PNP_WAVES_PER_GRID=4),
    'step_kernel_rr<16, 4, true>': compat(3, 1026, 3, 'CN', 'dd', 'fused', PNP_KERNEL=4, PNP_WAVES_PER_GRID=4),
    # ---- step_kernel_st<P, CN, GL> (pnp_stream.hip, persistent waves): PNP_KERNEL = 5 + GL; PNP_ST_WAVES_PER_CU = 1 leaves 256 waves
    # for 300 operating points (every wave walks more than one, the last ones ragged)
    'step_kernel_st<2, false, 0>': compat(2, 67, 300, 'FTCS', 'dd', 'step', PNP_KERNEL=5, PNP_ST_WAVES_PER_CU=1),
    'step_kernel_st<2, false, 1>': compat(3, 130, 300, 'FTCS', 'dd', 'step', PNP_KERNEL=6),
    'step_kernel_st<2, false, 2>': compat(5, 99, 300, 'FTCS', 'dd', 'fused', PNP_KERNEL=7, PNP_ST_WAVES_PER_CU=1),
    'step_kernel_st<2, true, 0>': compat(4, 67, 300, 'CN', 'dd', 'fused', PNP_KERNEL=5),
    'step_kernel_st<2, true, 1>': compat(6, 130, 300, 'CN', 'dd', 'step', PNP_KERNEL=6, PNP_ST_WAVES_PER_CU=1),
    'step_kernel_st<2, true, 2>': compat(2, 99, 300, 'CN', 'dd', 'step', PNP_KERNEL=7),
    'step_kernel_st<4, false, 0>': compat(3, 131, 300, 'FTCS', 'dd', 'fused', PNP_KERNEL=5, PNP_ST_WAVES_PER_CU=1),
    'step_kernel_st<4, false, 1>': compat(5, 258, 300, 'FTCS', 'dd', 'fused', PNP_KERNEL=6),
    'step_kernel_st<4, false, 2>': compat(4, 201, 300, 'FTCS', 'dd', 'step', PNP_KERNEL=7, PNP_ST_WAVES_PER_CU=1),
    'step_kernel_st<4, true, 0>': compat(6, 131, 300, 'CN', 'dd', 'step', PNP_KERNEL=5),
    'step_kernel_st<4, true, 1>': compat(2, 258, 300, 'CN', 'dd', 'fused', PNP_KERNEL=6, PNP_ST_WAVES_PER_CU=1),
    'step_kernel_st<4, true, 2>': compat(3, 201, 300, 'CN', 'dd', 'fused', PNP_KERNEL=7),
    'step_kernel_st<8, false, 0>': compat(5, 259, 300, 'FTCS', 'dd', 'step', PNP_KERNEL=5, PNP_ST_WAVES_PER_CU=1),
    'step_kernel_st<8, false, 1>': compat(4, 514, 300, 'FTCS', 'dd', 'step', PNP_KERNEL=6),
    'step_kernel_st<8, false, 2>': compat(6, 333, 300, 'FTCS', 'dd', 'fused', PNP_KERNEL=7, PNP_ST_WAVES_PER_CU=1),
    'step_kernel_st<8, true, 0>': compat(2, 259, 300, 'CN', 'dd', 'fused', PNP_KERNEL=5),
    'step_kernel_st<8, true, 1>': compat(3, 514, 300, 'CN', 'dd', 'step', PNP_KERNEL=6, PNP_ST_WAVES_PER_CU=1),
    'step_kernel_st<8, true, 2>': compat(5, 333, 300, 'CN', 'dd', 'step', PNP_KERNEL=7),
    'step_kernel_st<16, false, 0>': compat(4, 515, 300, 'FTCS', 'dd', 'fused', PNP_KERNEL=5, PNP_ST_WAVES_PER_CU=1),
    'step_kernel_st<16, false, 1>': compat(6, 1026, 300, 'FTCS', 'dd', 'fused', PNP_KERNEL=6),
    'step_kernel_st<16, false, 2>': compat(2, 777, 300, 'FTCS', 'dd', 'step', PNP_KERNEL=7, PNP_ST_WAVES_PER_CU=1),
    'step_kernel_st<16, true, 0>': compat(3, 515, 300, 'CN', 'dd', 'step', PNP_KERNEL=5),
    'step_kernel_st<16, true, 1>': compat(5, 1026, 300, 'CN', 'dd', 'fused', PNP_KERNEL=6, PNP_ST_WAVES_PER_CU=1),
    'step_kernel_st<16, true, 2>': compat(4, 777, 300, 'CN', 'dd', 'fused', PNP_KERNEL=7),
    # ---- step_kernel_mw<16, WY> / poisson_kernel_mw<16, WY> (WY waves per system: nx > 1026)
    'step_kernel_mw<16, 2>': compat(3, 1027, 2, 'CN', 'all', 'fused'),
    'step_kernel_mw<16, 4>': compat(2, 2051, 2, 'FTCS', 'dd', 'step'),
    'poisson_kernel_mw<16, 2>': compat(4, 2050, 2, 'FTCS', 'all', 'step'),
    'poisson_kernel_mw<16, 4>': compat(2, 4098, 2, 'CN', 'vwall_gbulk', 'fused'),
}

# every other kernel of the library: the test that runs it (checked against traced runs of each test: COVERED)
COVERED_ELSEWHERE = {
    'lane_transpose_kernel<false>': 'tests/test_gpu_lane.py::test_bitwise_reproducible',
    'lane_transpose_kernel<true>': 'tests/test_gpu_lane.py::test_bitwise_reproducible',
    'charge_row_kernel': 'tests/test_gpu_fullsize.py::test_ragged_grid_sizes',
    'poisson_kernel<1>': 'tests/test_gpu_fullsize.py::test_ragged_grid_sizes',
    'poisson_kernel<2>': 'tests/test_gpu_fullsize.py::test_ragged_grid_sizes',
    'poisson_kernel<4>': 'tests/test_gpu_fullsize.py::test_ragged_grid_sizes',
    'poisson_kernel<8>': 'tests/test_gpu_fullsize.py::test_ragged_grid_sizes',
    'poisson_kernel<16>': 'tests/test_gpu_fullsize.py::test_ragged_grid_sizes',
    'mol_rhs_kernel<1>': 'tests/test_gpu_kernel_census.py::test_method_of_lines_rhs_matches_the_oracle',
    'mol_rhs_kernel<2>': 'tests/test_gpu_kernel_census.py::test_method_of_lines_rhs_matches_the_oracle',
    'mol_rhs_kernel<4>': 'tests/test_gpu_kernel_census.py::test_method_of_lines_rhs_matches_the_oracle',
    'mol_rhs_kernel<8>': 'tests/test_gpu_kernel_census.py::test_method_of_lines_rhs_matches_the_oracle',
    'mol_rhs_kernel<16>': 'tests/test_gpu_kernel_census.py::test_method_of_lines_rhs_matches_the_oracle',
    'mol_rhs_pointwise_kernel': 'tests/test_gpu_fullsize.py::test_method_of_lines_rhs_on_grids_beyond_one_wave',
    'ode_begin_kernel': 'tests/test_gpu_ode.py::test_same_step_sequence_as_the_pinned_oracle',
    'ode_hinit_a_kernel': 'tests/test_gpu_ode.py::test_same_step_sequence_as_the_pinned_oracle',
    'ode_hinit_b_kernel': 'tests/test_gpu_ode.py::test_same_step_sequence_as_the_pinned_oracle',
    'ode_open_kernel': 'tests/test_gpu_ode.py::test_same_step_sequence_as_the_pinned_oracle',
    'ode_control_kernel': 'tests/test_gpu_ode.py::test_same_step_sequence_as_the_pinned_oracle',
    'ode_stage_kernel<2>': 'tests/test_gpu_ode.py::test_same_step_sequence_as_the_pinned_oracle',
    'ode_stage_kernel<3>': 'tests/test_gpu_ode.py::test_same_step_sequence_as_the_pinned_oracle',
    'ode_stage_kernel<4>': 'tests/test_gpu_ode.py::test_same_step_sequence_as_the_pinned_oracle',
    'ode_stage_kernel<5>': 'tests/test_gpu_ode.py::test_same_step_sequence_as_the_pinned_oracle',
    'ode_stage_kernel<6>': 'tests/test_gpu_ode.py::test_same_step_sequence_as_the_pinned_oracle',
    'ode_stage_kernel<7>': 'tests/test_gpu_ode.py::test_same_step_sequence_as_the_pinned_oracle',
    'ode853_stage_kernel': 'tests/test_gpu_ode.py::test_dop853_same_step_sequence_as_the_pinned_oracle',
    'ode853_control_a_kernel': 'tests/test_gpu_ode.py::test_dop853_same_step_sequence_as_the_pinned_oracle',
    'ode853_control_b_kernel': 'tests/test_gpu_ode.py::test_dop853_same_step_sequence_as_the_pinned_oracle',
    'rkc_begin_kernel': 'tests/test_gpu_ode.py::test_rkc_same_steps_and_stage_counts_as_the_oracle',
    'rkc_advance_kernel': 'tests/test_gpu_ode.py::test_rkc_same_steps_and_stage_counts_as_the_oracle',
    'scf_pre_kernel': 'tests/test_gpu_calculator.py::test_device_scf_loop_walks_the_same_iterates_as_the_host_loop',
    'scf_keep_kernel': 'tests/test_gpu_calculator.py::test_device_scf_loop_walks_the_same_iterates_as_the_host_loop',
    'scf_post_kernel': 'tests/test_gpu_calculator.py::test_device_scf_loop_walks_the_same_iterates_as_the_host_loop',
    'surface_kernel': 'tests/test_gpu_baseline_batch.py::test_config5_share_physical_mode_lane4_kernel_8192_lanes',
    'rates_kernel': 'tests/test_gpu_parity_golden.py::test_integrate_matches_reference_golden',
    'step_prepare_kernel': 'tests/test_gpu_lane_mask.py::test_masked_middle_call_matches_the_oracle',
    'bdf2_accumulate_kernel': 'tests/test_gpu_lane_mask.py::test_masked_middle_call_matches_the_oracle',
    'history_start_kernel': 'tests/test_gpu_lane_mask.py::test_stationary_solve_under_a_mask_restarts_only_the_lanes_it_solves',
    'unpack_state_kernel': 'tests/test_gpu_newton.py::test_stationary_matches_oracle',
}


class CensusUnavailable(Exception):
    """The built library or an LLVM tool is missing: the census cannot be taken (the test skips and says why)."""


def _tool(name):
    for d in (os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin'),):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    raise CensusUnavailable('%s not found under $ROCM_PATH/llvm/bin' % name)


def _demangler():
    p = shutil.which('c++filt')
    if p:
        return p
    try:
        return _tool('llvm-cxxfilt')
    except CensusUnavailable:
        raise CensusUnavailable('no c++filt on PATH and no llvm-cxxfilt under $ROCM_PATH/llvm/bin')


def split_bundles(blob):
    """The offload bundles of a linked .hip_fatbin section: one per translation unit, each starting with the
    __CLANG_OFFLOAD_BUNDLE__ magic (its header gives its size) or with the CCOB magic of a compressed bundle (versions >= 2 give
    their total size; a version-1 bundle runs to the next magic)."""
    plain, packed = b'__CLANG_OFFLOAD_BUNDLE__', b'CCOB'
    out, pos = [], 0
    while True:
        hits = [i for i in (blob.find(plain, pos), blob.find(packed, pos)) if i >= 0]
        if not hits:
            return out
        i = min(hits)
        if blob.startswith(plain, i):
            (n,) = struct.unpack_from('<Q', blob, i + len(plain))
            off, end = i + len(plain) + 8, i + len(plain) + 8
            for _ in range(n):
                o, size, tlen = struct.unpack_from('<QQQ', blob, off)
                off += 24 + tlen
                end = max(end, i + o + size)
        else:
            (version,) = struct.unpack_from('<H', blob, i + 4)
            if version == 2:
                end = i + struct.unpack_from('<I', blob, i + 8)[0]
            elif version >= 3:
                end = i + struct.unpack_from('<Q', blob, i + 8)[0]
            else:
                nxt = [j for j in (blob.find(plain, i + 4), blob.find(packed, i + 4)) if j >= 0]
                end = min(nxt) if nxt else len(blob)
        out.append(blob[i:end])
        pos = max(end, i + 4)


def compiled_kernels(lib=LIB):
    """Census names of every kernel in the gfx950 code objects of the built library (.kd symbols of each unbundled object)."""
    if not os.path.exists(lib):
        raise CensusUnavailable('the library is not built (%s missing): run __graft_entry__.build()' % os.path.relpath(lib, ROOT))
    objcopy, bundler, readelf, cxxfilt = _tool('llvm-objcopy'), _tool('clang-offload-bundler'), _tool('llvm-readelf'), _demangler()
    symbols = set()
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, 'fatbin')
        subprocess.run([objcopy, '--dump-section', '.hip_fatbin=' + fat, lib, os.path.join(tmp, 'copy.so')], check=True, capture_output=True)
        with open(fat, 'rb') as f:
            bundles = split_bundles(f.read())
        if not bundles:
            raise RuntimeError('no offload bundle in the .hip_fatbin section of %s' % lib)
        for k, blob in enumerate(bundles):
            src, obj = os.path.join(tmp, 'b%d' % k), os.path.join(tmp, 'o%d' % k)
            with open(src, 'wb') as f:
                f.write(blob)
            subprocess.run([bundler, '--unbundle', '--type=o', '--targets=' + TARGET, '--input=' + src, '--output=' + obj,
                            '--allow-missing-bundles'], check=True, capture_output=True)
            if not os.path.exists(obj) or os.path.getsize(obj) == 0:
                continue
            r = subprocess.run([readelf, '-s', '--wide', obj], check=True, capture_output=True, text=True)
            for line in r.stdout.splitlines():
                f = line.split()
                if len(f) >= 8 and f[-1].endswith('.kd'):
                    symbols.add(f[-1])
    r = subprocess.run([cxxfilt], input='\n'.join(sorted(symbols)) + '\n', check=True, capture_output=True, text=True)
    return {census_name(s) for s in r.stdout.splitlines() if s.strip()}


def read_dispatched(path=DISPATCHED):
    with open(path) as f:
        return {line.strip() for line in f if line.strip()}


def read_covered(path=COVERED):
    """(kernel, test) pairs of profiles/kernel_census_covered.txt: the kernels of COVERED_ELSEWHERE that a traced run of the test
    alone dispatched."""
    with open(path) as f:
        return {tuple(line.rstrip('\n').split('\t')) for line in f if line.strip()}
