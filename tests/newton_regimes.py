"""Driven inputs for the physical mode's damped Newton update (test infrastructure, no tests of its own).

The update has four data-dependent branches -- the dphi_max scaling, the floor at a tenth of the previous iterate, the free-volume
backtrack of steric ions and three exits -- in one definition (pnp_math.h: newton_damping, newton_floor_step, newton_free_volume,
newton_backtrack, newton_accept) with seven call sites for the eight kernel families (pnp_newton.hip: pair, row-per-thread, team, the
one-sided sweep's row update and the bookkeeping both sweep kernels share; pnp_lane.hip: separate passes and the fused update;
pnp_lane_cols.h for the lane pair and quad).  The two-sided sweep writes floor and backtrack out in its row update (measured:
profiles/newton_rule.md section 5).  The census's inputs (|phiM| <= 0.15 V,
cref = 10, radius 3.5e-10 m, Stern capacitance 0.25 F/m^2) never reach the backtrack; the cases of REGIMES do.

Recipes (RECIPES).  'crowded': radius 5.0e-10 m on every species, Stern capacitance 1.0 F/m^2, cref = 200, phiM in -0.8 .. 0.8 V: the
strong capacitance leaves the potential drop to the diffuse layer, the large ions fill it, and the window mixes mild and crowded lanes
in one wave.  'window06' / 'window045': the same with phiM within 0.6 / 0.45 V, for the batches of 21 - 37 operating points of which
one or two do not converge at 0.8 V (every lane of a batch must end with status 0): BDF2 of seven steric species (lane pair and quad)
and the reaction tables of five and more species (sweep, two-sided sweep).  Transient cases take three steps from the bulk state at
`factor` times the census timestep: 100 where that meets the conditions, 1000 for a few small batches, 10 for none.

What was tried and is not in the table:
  * the 1e-12 floor of the free volume ('free_min').  'harsh' (radius 5.5e-10 m, Stern capacitance 2.0, cref = 300, |phiM| <= 1 V) and
    'crowded' with the reaction tables reach it in lanes that converge with the banded LU of the oracle (team <6, 1>, <7, 2>, <9, 1>:
    150 seeds each; lane quad <7, 1, false>, <8, 2, false>: 8 seeds each), but in every such lane the oracle's cyclic reduction
    (solve_block_pcr, the device's solver) runs to maxit: the two solvers do not agree there, so no case can demand parity.
  * the lane pair and quad with BDF = true in MODE 2 (<6, 2, true>, <9, 2, true>): with convection or the reaction tables, BDF2 from
    the bulk state at 10 to 1000 times the census timestep leaves lanes of every batch tried at maxit, in all three windows.  BDF = true
    is driven in MODE 1 (<8, 1, true>), MODE 2 with BDF = false (<8, 2, false>).
  * one species with its reaction (pair <2, 64, 2>, row-per-thread <2, 512, 2>): the source pins the concentration near kf / kr = 10,
    the ions never crowd.  Block size 2 is driven in MODE 1.
  * reactions of five and more species in batches of 37 - 45 (lane <8, 2, true, false>, lane pair / quad MODE 2): lanes at maxit in
    every batch tried; those instances use convection, MODE 2 as well in the lane families.  The workgroup families compile only
    reactions into MODE 2 and keep the census's reaction tables.
Keys with a suffix are the extra cases: '/estimate' (error_estimate = True, the oracle leaves through the estimate in a compared lane),
'/predictor' (both clips of the predictor -- the floor at a tenth and "keep u_n where the extrapolated ions fill 90 %" -- fire in a
compared lane).  The single-precision record cases (lanes = None) compare the whole batch: their bar is a fraction of the batch.

Branch counts of the oracle, summed over the compared lanes of each family's cases (lanes in which the branch fired / iterations in
which it fired; tests/test_newton_regimes.py asserts the per-case conditions):
  family                cases  lanes  iterations  backtrack   floor      dphi_max   estimate exits  predictor points floored / kept
  newton_lane_kernel       14    146        1979   90 / 168   133 / 694  124 / 421              10  337 / 82
  newton_lane2_kernel       5     30         447   20 / 34     30 / 174   27 / 71                0  138 / 46
  newton_lane4_kernel       6     36         474   24 / 33     36 / 177   32 / 75                4  76 / 28
  newton_pair_kernel        6     30         494   19 / 20     27 / 161   26 / 135              13  817 / 42
  newton_kernel             8     32         537   24 / 30     29 / 210   31 / 153               0  1226 / 28
  newton_team_kernel       10     55         845   36 / 61     53 / 316   52 / 178               1  321 / 84
  newton_sweep_kernel       7     42         623   28 / 36     41 / 213   38 / 129               0  98 / 19
  newton_sweep2_kernel      7     41         600   27 / 38     41 / 231   38 / 99                0  137 / 48

A case names a census instance (tests/kernel_census.py) and takes from that instance's census case everything that selects the
instance -- the forced kernel, N, nx, B, the option environment, the physics class and the stepper kind -- and replaces only the inputs:
the recipe (ion radius, Stern capacitance, concentration scale, potential window), for transient cases a factor on the census
timestep, the seed and the list of compared lanes.  tests/test_newton_regimes.py checks on the CPU, with the oracle alone, that every
case reaches the branches; tests/test_gpu_newton_regimes.py runs every case on the device.
"""
import os
import zlib
from collections import namedtuple

import numpy as np

from oracle import pnp_physical as PH
from tests.kernel_census import CENSUS, ROOT, family
from tests.test_gpu_kernel_census import RX, RX6
from tests.test_gpu_newton import make_lanes, run_oracle

DISPATCHED = os.path.join(ROOT, 'profiles', 'newton_regimes_dispatched.txt')

# radius [m] of every species, Stern capacitance [F/m^2], cref and the window of the metal potential [V] of make_lanes
Recipe = namedtuple('Recipe', 'radius stern cref phi_lo phi_hi')
RECIPES = {
    'crowded': Recipe(5.0e-10, 1.0, 200.0, -0.8, 0.8),
    'window06': Recipe(5.0e-10, 1.0, 200.0, -0.6, 0.6),
    'window045': Recipe(5.0e-10, 1.0, 200.0, -0.45, 0.45),
    'harsh': Recipe(5.5e-10, 2.0, 300.0, -1.0, 1.0),
}

# the eight families and the position of MODE in their template argument lists
MODE_ARG = {'newton_lane_kernel': 1, 'newton_lane2_kernel': 1, 'newton_lane4_kernel': 1, 'newton_pair_kernel': 2, 'newton_kernel': 2,
            'newton_team_kernel': 1, 'newton_sweep_kernel': 1, 'newton_sweep2_kernel': 1}
LANE_FAMILIES = ('newton_lane_kernel', 'newton_lane2_kernel', 'newton_lane4_kernel')
WORKGROUP_FAMILIES = ('newton_pair_kernel', 'newton_kernel', 'newton_team_kernel', 'newton_sweep_kernel', 'newton_sweep2_kernel')

# instance: the census instance; physics: the physics class ('+'-joined, see kernel_census.newton; always steric); recipe: a key of RECIPES;
# factor: on the census timestep (None: stationary); lanes: the compared operating points (None: the whole batch, single-precision record
# columns); salt: added to the seed; extra: further set_newton options (error_estimate, maxit)
Regime = namedtuple('Regime', 'instance physics recipe factor lanes salt extra')


def regime(instance, physics, lanes, salt=0, factor=None, recipe='crowded', **extra):
    return Regime(instance, physics, recipe, factor, None if lanes is None else tuple(lanes), salt, tuple(sorted(extra.items())))


REGIMES = {
    # ---- newton_lane_kernel
    'newton_lane_kernel<2, 2, true, false>': regime('newton_lane_kernel<2, 2, true, false>', 'conv+steric', (0, 12, 14, 31, 34, 44)),
    'newton_lane_kernel<3, 1, true, false>': regime('newton_lane_kernel<3, 1, true, false>', 'steric', (0, 1, 3, 42, 43, 44)),
    'newton_lane_kernel<3, 1, true, true>': regime('newton_lane_kernel<3, 1, true, true>', 'steric', None, factor=100),
    'newton_lane_kernel<3, 2, false, false>': regime('newton_lane_kernel<3, 2, false, false>', 'rx+steric', (0, 1, 2, 42, 43, 44), salt=2, factor=100),
    'newton_lane_kernel<4, 1, false, false>': regime('newton_lane_kernel<4, 1, false, false>', 'steric', (0, 1, 4, 40, 43, 44), factor=100),
    'newton_lane_kernel<4, 1, false, false>/predictor': regime('newton_lane_kernel<4, 1, false, false>', 'steric', (0, 1, 2, 41, 42, 44), factor=100),
    'newton_lane_kernel<5, 1, true, false>': regime('newton_lane_kernel<5, 1, true, false>', 'steric', (0, 1, 2, 4, 43, 44), factor=100),
    'newton_lane_kernel<5, 1, true, false>/estimate': regime('newton_lane_kernel<5, 1, true, false>', 'steric', (0, 1, 3, 39, 42, 44), factor=100, error_estimate=True),
    'newton_lane_kernel<5, 2, false, false>': regime('newton_lane_kernel<5, 2, false, false>', 'rx+steric', (0, 1, 2, 3, 41, 44)),
    'newton_lane_kernel<6, 2, false, false>': regime('newton_lane_kernel<6, 2, false, false>', 'conv+steric', (0, 3, 8, 41, 43, 44), factor=100),
    'newton_lane_kernel<7, 1, false, false>': regime('newton_lane_kernel<7, 1, false, false>', 'steric', (0, 1, 2, 3, 43, 44)),
    'newton_lane_kernel<8, 1, true, false>': regime('newton_lane_kernel<8, 1, true, false>', 'steric', (0, 1, 2, 3, 43, 44)),
    'newton_lane_kernel<9, 1, true, true>': regime('newton_lane_kernel<9, 1, true, true>', 'steric', None),
    'newton_lane_kernel<9, 2, true, false>': regime('newton_lane_kernel<9, 2, true, false>', 'conv+steric', (0, 4, 19, 23, 36, 44), factor=100),
    # ---- newton_lane2_kernel
    'newton_lane2_kernel<6, 1, false>': regime('newton_lane2_kernel<6, 1, false>', 'steric', (0, 1, 3, 34, 35, 36), factor=100),
    'newton_lane2_kernel<7, 1, false>': regime('newton_lane2_kernel<7, 1, false>', 'steric', (0, 1, 2, 3, 35, 36)),
    'newton_lane2_kernel<8, 1, true>': regime('newton_lane2_kernel<8, 1, true>', 'steric', (0, 9, 14, 16, 30, 36), salt=2, factor=1000, recipe='window045'),
    'newton_lane2_kernel<8, 2, false>': regime('newton_lane2_kernel<8, 2, false>', 'conv+steric', (0, 8, 26, 29, 30, 36)),
    'newton_lane2_kernel<9, 1, false>': regime('newton_lane2_kernel<9, 1, false>', 'steric', (0, 1, 2, 3, 35, 36), factor=100),
    # ---- newton_lane4_kernel
    'newton_lane4_kernel<6, 1, false>': regime('newton_lane4_kernel<6, 1, false>', 'steric', (0, 1, 3, 18, 19, 20), factor=100),
    'newton_lane4_kernel<7, 1, false>': regime('newton_lane4_kernel<7, 1, false>', 'steric', (0, 1, 3, 17, 19, 20)),
    'newton_lane4_kernel<7, 1, false>/estimate': regime('newton_lane4_kernel<7, 1, false>', 'steric', (2, 3, 4, 5, 16, 20), error_estimate=True),
    'newton_lane4_kernel<8, 1, true>': regime('newton_lane4_kernel<8, 1, true>', 'steric', (0, 1, 2, 18, 19, 20), salt=2, factor=1000, recipe='window045'),
    'newton_lane4_kernel<8, 2, false>': regime('newton_lane4_kernel<8, 2, false>', 'conv+steric', (0, 7, 13, 14, 17, 20)),
    'newton_lane4_kernel<9, 1, false>': regime('newton_lane4_kernel<9, 1, false>', 'steric', (0, 1, 2, 3, 19, 20), factor=100),
    # ---- newton_pair_kernel
    'newton_pair_kernel<2, 64, 1>': regime('newton_pair_kernel<2, 64, 1>', 'steric', (0, 1, 2, 3, 4), salt=3, factor=1000),
    'newton_pair_kernel<3, 64, 2>': regime('newton_pair_kernel<3, 64, 2>', 'rx+conv+steric', (0, 1, 2, 3, 4), salt=13, factor=100),
    'newton_pair_kernel<4, 64, 1>': regime('newton_pair_kernel<4, 64, 1>', 'steric', (0, 1, 2, 3, 4), salt=7, factor=100),
    'newton_pair_kernel<4, 64, 1>/estimate': regime('newton_pair_kernel<4, 64, 1>', 'steric', (0, 1, 2, 3, 4), salt=48, factor=100, error_estimate=True),
    'newton_pair_kernel<5, 64, 1>': regime('newton_pair_kernel<5, 64, 1>', 'steric+conv', (0, 1, 2, 3, 4), salt=3, factor=100),
    'newton_pair_kernel<5, 64, 2>': regime('newton_pair_kernel<5, 64, 2>', 'rx+conv+steric', (0, 1, 2, 3, 4), salt=13),
    # ---- newton_kernel
    'newton_kernel<2, 512, 1>': regime('newton_kernel<2, 512, 1>', 'steric+conv', (0, 1, 2, 3), salt=18, factor=100),
    'newton_kernel<3, 512, 1>': regime('newton_kernel<3, 512, 1>', 'steric', (0, 1, 2, 3), salt=1),
    'newton_kernel<3, 512, 2>': regime('newton_kernel<3, 512, 2>', 'rx+conv+steric', (0, 1, 2, 3), salt=14, factor=100),
    'newton_kernel<4, 512, 1>': regime('newton_kernel<4, 512, 1>', 'steric+conv', (0, 1, 2, 3), salt=5, factor=1000),
    'newton_kernel<5, 512, 1>': regime('newton_kernel<5, 512, 1>', 'steric', (0, 1, 2, 3), salt=8, factor=100),
    'newton_kernel<5, 512, 2>': regime('newton_kernel<5, 512, 2>', 'rx+conv+steric', (0, 1, 2, 3), salt=4, factor=100),
    'newton_kernel<6, 256, 1>': regime('newton_kernel<6, 256, 1>', 'steric', (0, 1, 2, 3), salt=1),
    'newton_kernel<7, 256, 2>': regime('newton_kernel<7, 256, 2>', 'rx+conv+steric', (0, 1, 2, 3), salt=118, factor=1000),
    # ---- newton_team_kernel
    'newton_team_kernel<3, 1>': regime('newton_team_kernel<3, 1>', 'steric', (0, 1, 2, 4, 5, 6), salt=1, factor=100),
    'newton_team_kernel<4, 1>': regime('newton_team_kernel<4, 1>', 'steric+conv', (0, 1, 2, 3, 6), factor=100),
    'newton_team_kernel<5, 2>': regime('newton_team_kernel<5, 2>', 'rx+steric', (0, 1, 3, 5, 6), factor=100),
    'newton_team_kernel<6, 1>': regime('newton_team_kernel<6, 1>', 'steric+conv', (0, 1, 4, 5, 6), salt=1),
    'newton_team_kernel<6, 1>/estimate': regime('newton_team_kernel<6, 1>', 'steric+conv', (0, 1, 2, 4, 5, 6), salt=2, error_estimate=True),
    'newton_team_kernel<7, 1>': regime('newton_team_kernel<7, 1>', 'steric', (0, 1, 2, 4, 5, 6), factor=100),
    'newton_team_kernel<7, 1>/predictor': regime('newton_team_kernel<7, 1>', 'steric', (0, 1, 2, 5, 6), factor=100),
    'newton_team_kernel<7, 2>': regime('newton_team_kernel<7, 2>', 'rx+steric', (0, 1, 2, 3, 5, 6), salt=3),
    'newton_team_kernel<8, 1>': regime('newton_team_kernel<8, 1>', 'steric+conv', (0, 1, 4, 5, 6), salt=35, factor=100),
    'newton_team_kernel<9, 1>': regime('newton_team_kernel<9, 1>', 'steric', (0, 1, 2, 3, 5, 6), factor=100),
    # ---- newton_sweep_kernel
    'newton_sweep_kernel<3, 1>': regime('newton_sweep_kernel<3, 1>', 'steric', (0, 1, 2, 3, 21, 22), factor=100),
    'newton_sweep_kernel<4, 1>': regime('newton_sweep_kernel<4, 1>', 'steric+conv', (0, 1, 11, 12, 18, 22), factor=100),
    'newton_sweep_kernel<5, 2>': regime('newton_sweep_kernel<5, 2>', 'rx+steric', (0, 1, 2, 19, 21, 22), factor=100),
    'newton_sweep_kernel<6, 1>': regime('newton_sweep_kernel<6, 1>', 'steric+conv', (0, 1, 4, 18, 19, 22)),
    'newton_sweep_kernel<7, 2>': regime('newton_sweep_kernel<7, 2>', 'rx+steric', (0, 1, 3, 18, 21, 22), recipe='window045'),
    'newton_sweep_kernel<8, 1>': regime('newton_sweep_kernel<8, 1>', 'steric+conv', (0, 3, 18, 19, 21, 22), factor=100),
    'newton_sweep_kernel<9, 1>': regime('newton_sweep_kernel<9, 1>', 'steric', (0, 1, 4, 20, 21, 22), factor=100),
    # ---- newton_sweep2_kernel
    'newton_sweep2_kernel<6, 1>': regime('newton_sweep2_kernel<6, 1>', 'steric', (0, 1, 2, 18, 20, 22), factor=100),
    'newton_sweep2_kernel<6, 2>': regime('newton_sweep2_kernel<6, 2>', 'rx+steric', (0, 1, 3, 4, 5, 22), salt=2, recipe='window06'),
    'newton_sweep2_kernel<7, 1>': regime('newton_sweep2_kernel<7, 1>', 'steric+conv', (0, 4, 7, 11, 22), salt=3, factor=100),
    'newton_sweep2_kernel<7, 2>': regime('newton_sweep2_kernel<7, 2>', 'rx+steric', (0, 1, 2, 4, 21, 22), factor=100, recipe='window045'),
    'newton_sweep2_kernel<8, 2>': regime('newton_sweep2_kernel<8, 2>', 'rx+steric', (0, 1, 2, 8, 19, 22), salt=2, factor=100, recipe='window06'),
    'newton_sweep2_kernel<9, 1>': regime('newton_sweep2_kernel<9, 1>', 'steric+conv', (0, 3, 14, 18, 20, 22)),
    'newton_sweep2_kernel<9, 2>': regime('newton_sweep2_kernel<9, 2>', 'rx+steric', (0, 1, 2, 20, 21, 22), factor=100, recipe='window045'),
}


def template_args(instance):
    return [a.strip() for a in instance[instance.index('<') + 1:-1].split(',')]


def mode_of(instance, physics):
    """The MODE the host chooses for a physics class: the lane families compile reactions and convection into MODE 2, the workgroup
    families reactions only (newton_mode_lane, newton_mode_workgroup in catint_amd/csrc/pnp_internal.h)."""
    phys = set(physics.split('+'))
    assert 'steric' in phys, physics
    second = phys & ({'rx', 'conv'} if family(instance) in LANE_FAMILIES else {'rx'})
    return 2 if second else 1


def seed_of(key):
    return zlib.crc32(key.encode()) + REGIMES[key].salt


def regime_args(key, r=None):
    """run_both's / run_oracle's arguments (all but lanes) of a case: tests/test_gpu_kernel_census.py: newton_args with the recipe's
    inputs in place of the census's."""
    r = r or REGIMES[key]
    case = CENSUS[r.instance]
    rec = RECIPES[r.recipe]
    seed = zlib.crc32(key.encode()) + r.salt
    N, nx, B = case.N, case.nx, case.B
    phys = set(r.physics.split('+'))
    lane_kw = dict(phi_lo=rec.phi_lo, phi_hi=rec.phi_hi, cref=rec.cref)
    if N == 1:                                  # (one species is not neutral: its grid stays a few Debye lengths long)
        lane_kw['points_per_debye'] = max(6.0, nx / 12.0)
    D, q, cb, dx, phiM = make_lanes(N, nx, B, seed, **lane_kw)
    kw = dict(wall_bc='stern', stern_capacitance=rec.stern, mpb_radius=[rec.radius] * N)
    kw.update(dict(r.extra))
    args = dict(N=N, nx=nx, B=B, seed=seed, **lane_kw)
    if 'rx' in phys:
        args['reactions'] = RX.get(N, RX6)
    if 'conv' in phys:
        args['velocity'] = 3.0 * D.max() / ((nx - 1) * dx)
    assert (case.stepper == 'stat') == (r.factor is None), key
    if case.stepper != 'stat':
        kw['time_order'] = 2 if 'bdf2' in case.stepper else 1
        kw['predictor'] = 'pred' in case.stepper
        census_dt = 1e-7 if 'rx' in set(case.physics.split('+')) else 0.3 * (6 * dx) * (nx * dx) / D.max()
        args.update(dt=r.factor * census_dt, nsteps=3, stationary=False)
    args['newton_kw'] = kw
    return args


def compared_lanes(key, r=None):
    r = r or REGIMES[key]
    return list(range(CENSUS[r.instance].B)) if r.lanes is None else list(r.lanes)


def is_f32(r):
    return dict(CENSUS[r.instance].env).get('LANE_RECORDS') == 'f32'


def conditions(key, branches, iterations, r=None):
    """What the oracle's branch counters of the compared lanes must show for a case (lists in the lanes' order); raises AssertionError."""
    r = r or REGIMES[key]
    maxit = dict(r.extra).get('maxit', 50)
    steps = 1 if r.factor is None else 3
    assert all(b['maxit'] == 0 for b in branches) and np.all(np.asarray(iterations) <= steps * maxit), (key, 'not converged', iterations)
    fired = lambda name: sum(1 for b in branches if b[name] > 0)
    assert fired('free_volume') >= 3, (key, 'free-volume backtrack in %d compared lanes' % fired('free_volume'))
    assert fired('floor') >= 1 and fired('damped') >= 1, (key, 'floor %d, dphi_max %d' % (fired('floor'), fired('damped')))
    assert fired('free_volume') < len(branches), (key, 'no mild lane')
    if dict(r.extra).get('error_estimate'):
        assert fired('estimate') >= 1, (key, 'no lane left through the error estimate')
    if 'predictor' in key.split('/')[1:]:
        assert any(sum(b['pred_floor']) > 0 for b in branches) and any(sum(b['pred_keep']) > 0 for b in branches), (key, 'predictor clips')
    if 'free_min' in key.split('/')[1:]:
        assert fired('free_min') >= 1, (key, 'the 1e-12 floor of the free volume was not reached')


def oracle(key, solver=None, branches=None, r=None, lanes=None):
    return run_oracle(lanes=compared_lanes(key, r) if lanes is None else lanes, solver=solver, branches=branches, **regime_args(key, r))


def thomas_f32(L, M, U, rhs):
    """Block Thomas whose back-substitution sees the records T in single precision: the arithmetic of tools/probe/f32_records_oracle.py
    for the lane kernels' LANE_RECORDS = f32 columns."""
    nx, nb, _ = M.shape
    T = np.zeros((nx, nb, nb)); t = np.zeros((nx, nb))
    for i in range(nx):
        D = M[i] - (L[i] @ T[i - 1] if i > 0 else 0.0)
        r = rhs[:, i] - (L[i] @ t[i - 1] if i > 0 else 0.0)
        T[i] = np.linalg.solve(D, U[i]) if i < nx - 1 else 0.0
        t[i] = np.linalg.solve(D, r)
    Tb = T.astype(np.float32).astype(np.float64)
    x = np.zeros((nx, nb))
    x[nx - 1] = t[nx - 1]
    for i in range(nx - 2, -1, -1):
        x[i] = t[i] - Tb[i] @ x[i + 1]
    return x.T
