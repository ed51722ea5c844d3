"""GPU: every solver kernel instance the library compiles, each forced through existing options by its census case
(tests/kernel_census.py), against the oracles at the suite's bars.

Physical mode: oracle/pnp_physical.py on three lanes of the batch -- the first, one in the middle and the last, which for the lane
families sits in a ragged last group -- with assert_close of tests/test_gpu_newton.py (2e-9 of the profile scale, 1e-6 per species
relative, identical Newton iteration counts); every lane of the batch must end with status 0.  Single-precision record columns
(LANE_RECORDS = f32) are held to the bar of tests/test_gpu_lane.py::test_record_columns_in_single_precision_give_the_same_iteration:
the same state bound, iteration counts at most one apart in at most a tenth of the operating points -- a fraction of the batch, so
those cases run the oracle on every lane.

Compat mode: the C oracle (oracle/pnp_oracle.c) on three lanes, state, potential, gradient and Laplacian to rtol 1e-9.

The method-of-lines right-hand side (pnp_mol_rhs: mol_rhs_kernel<P> on grids of one wave, the kernel behind the device ODE integrators)
against oracle/pnp_ref.py's mol_rhs to rtol 1e-9, on both sides of every points-per-lane boundary.
"""
import zlib

import numpy as np
import pytest

from catint_amd.host import solver_from_problem
from catint_amd.synthetic import make_batch
from oracle import pnp_ref as R
from oracle import c_oracle as CO
from tests.kernel_census import CENSUS
from tests.test_gpu_newton import assert_close, make_lanes, run_both

pytestmark = pytest.mark.gpu

OPTIONS = ('NEWTON_KERNEL', 'NEWTON_EXCHANGE', 'NEWTON_TEAM_THREADS', 'NEWTON_REGS', 'NEWTON_BLOCKS', 'NEWTON_LANE_GROUPS',
           'NEWTON_SWEEP_BLOCKS', 'LANE_PIVOT_LIMIT', 'LANE_ORDER', 'LANE_STAGGER', 'LANE_FUSED', 'LANE_RECORDS', 'PNP_KERNEL',
           'PNP_WAVES_PER_GRID', 'PNP_SPECIES_PER_WAVE', 'PNP_STEP_STREAMS', 'PNP_ALTERNATE_ROWS', 'PNP_ST_WAVES_PER_CU',
           'PNP_NO_POST_UPLOAD_DISPATCH')

# homogeneous reactions per species count (species of tests/test_gpu_newton.py: SPECIES)
RX = {
    1: [{'lhs': [], 'rhs': [0], 'kf': 1e9, 'kr': 1e8}],
    2: [{'lhs': [], 'rhs': [0, 1], 'kf': 2e3, 'kr': 1.5e2}],
    3: [{'lhs': [1], 'rhs': [2], 'kf': 4e5, 'kr': 9e5}, {'lhs': [], 'rhs': [0, 1], 'kf': 2e3, 'kr': 1.5e2}],
    4: [{'lhs': [1], 'rhs': [2], 'kf': 4e5, 'kr': 9e5}, {'lhs': [], 'rhs': [0, 1], 'kf': 2e3, 'kr': 1.5e2},
        {'lhs': [0], 'rhs': [3], 'kf': 1e3, 'kr': 2e3}],
    5: [{'lhs': [1], 'rhs': [2], 'kf': 4e5, 'kr': 9e5}, {'lhs': [0, 2], 'rhs': [4], 'kf': 2e3, 'kr': 1e4},
        {'lhs': [], 'rhs': [0, 1], 'kf': 2e3, 'kr': 1.5e2}],
}
RX6 = [{'lhs': [1], 'rhs': [2], 'kf': 4e5, 'kr': 9e5}, {'lhs': [0, 2, 2], 'rhs': [4, 5], 'kf': 5.0, 'kr': 1e2}]


def newton_args(case, seed):
    """run_both's arguments for a physical-mode case."""
    N, nx, B = case.N, case.nx, case.B
    phys = set(case.physics.split('+'))
    # (one species is not neutral: its grid stays a few Debye lengths long)
    lane_kw = {'points_per_debye': max(6.0, nx / 12.0)} if N == 1 else {}
    D, q, cb, dx, phiM = make_lanes(N, nx, B, seed, **lane_kw)
    kw, args = {}, dict(N=N, nx=nx, B=B, seed=seed, **lane_kw)
    if phys & {'stern', 'steric'}:
        kw.update(wall_bc='stern', stern_capacitance=0.25)
    if 'steric' in phys:
        kw['mpb_radius'] = [3.5e-10] * N
    if 'wk' in phys:
        kw.update(wall_bc='stern', stern_capacitance=0.2, phi_pzc=0.05)
        rng = np.random.default_rng(seed)
        args['wall_kinetics'] = [
            {'species': 2, 'k': rng.uniform(0.05, 1.0, B), 'nu': [0.0, 0.0, -1.0] + [1.0] * (N > 3) + [0.0] * max(N - 4, 0), 'alpha': -6.0,
             'saturation': 0.05},
            {'species': -1, 'k': rng.uniform(1e-6, 1e-5, B), 'nu': [0.0, 1.0, 0.0] + [0.0] * (N - 3), 'alpha': -4.0}]
    if 'rx' in phys:
        args['reactions'] = RX.get(N, RX6)
    if 'conv' in phys:
        args['velocity'] = 3.0 * D.max() / ((nx - 1) * dx)
    if case.stepper != 'stat':
        kw['time_order'] = 2 if 'bdf2' in case.stepper else 1
        kw['predictor'] = 'pred' in case.stepper
        # (steps from the bulk state: damped first iterations; with reactions the step of the suite's reaction tests)
        args.update(dt=1e-7 if 'rx' in phys else 0.3 * (6 * dx) * (nx * dx) / D.max(), nsteps=3, stationary=False)
    args['newton_kw'] = kw
    return args


def assert_close_f32_records(got, ref):
    # the bar of tests/test_gpu_lane.py::test_record_columns_in_single_precision_give_the_same_iteration
    c, phi, its, st = got
    rc, rphi, rit = ref
    assert np.all(st == 0), st
    cscale = np.abs(rc).max(axis=2, keepdims=True)
    assert np.abs(c - rc).max() <= 2e-9 * cscale.max() and (np.abs(c - rc) / (np.abs(rc) + 1e-3 * cscale)).max() < 1e-6
    assert np.abs(phi - rphi).max() <= 2e-9 * max(np.abs(rphi).max(), 0.025)
    d = np.abs(its.astype(int) - np.asarray(rit, int))
    assert d.max() <= 1 and (d != 0).mean() <= 0.1, (its, rit)


def run_newton_case(case, seed):
    f32 = dict(case.env).get('LANE_RECORDS') == 'f32'
    lanes = list(range(case.B)) if f32 else [0, case.B // 2, case.B - 1]
    (c, phi, its, st), ref = run_both(lanes=lanes, **newton_args(case, seed))
    assert np.all(st == 0), st                                             # every lane of the batch converged
    got = (c[lanes], phi[lanes], its[lanes], st)
    (assert_close_f32_records if f32 else assert_close)(got, ref)


# compat mode: neutral bulk states of catint_amd.synthetic.make_batch (40 Debye lengths whatever the grid) perturbed by 1 %, Poisson
# boundary values and wall fluxes drawn as tests/fuzz/fuzz_compat.py draws them
BRANCHES = ('dd', 'vwall_gbulk', 'gwall_vbulk', 'vwall_gwall', 'vbulk_gbulk')


def compat_inputs(case, pb_name, seed):
    N, nx, B = case.N, case.nx, case.B
    # (the timesteps of tests/test_gpu_stream.py; a perturbation small enough for the reference scheme to stay stable on every grid)
    # (on the long grids at most D dt / dx^2 = 0.5 for Crank-Nicolson, 0.2 for FTCS)
    dt_factor = min(1e-4, 0.5 * 40.0 / (nx - 1) ** 2) if case.method == 'CN' else min(2e-5, 0.2 * 40.0 / (nx - 1) ** 2)
    p, c0, pb, vz, fl = make_batch(B, N, nx, seed=seed, phi_max=0.02, dt_factor=dt_factor)
    rng = np.random.default_rng(seed)
    c0 = c0 * (1 + 0.01 * rng.uniform(-1, 1, c0.shape))
    pb = np.full((B, 4), np.nan)
    vw, vb = rng.uniform(-0.02, 0.02, B), rng.uniform(-0.002, 0.002, B)
    gw, gb = rng.uniform(-2e4, 2e4, B), rng.uniform(-1e4, 1e4, B)
    cols = {'dd': (vw, vb, None, None), 'vwall_gbulk': (vw, None, None, gb), 'gwall_vbulk': (None, vb, gw, None),
            'vwall_gwall': (vw, None, gw, None), 'vbulk_gbulk': (None, vb, None, gb)}[pb_name]
    for j, v in enumerate(cols):
        if v is not None:
            pb[:, j] = v
    fl = rng.uniform(-1e-4, 1e-4, (B, N))
    vz = vw.copy()                     # (vzeta: the wall potential of the lane, as make_batch sets it)
    p.pb = pb[0].copy()
    if case.rates:
        p.reactions = [([1], [0], 1e6, 5e5)] if N == 2 else [([0, 1], [2], 3e6, 2e8), ([2], [1], 1e8, 5e7)]
    return p, c0, pb, vz, fl


def run_compat_case(case, seed):
    method = {'CN': 'Crank-Nicolson', 'FTCS': 'FTCS'}[case.method]
    nsteps, spl = 4, (1 if case.launch == 'step' else 0)
    for pb_name in (BRANCHES if case.pb == 'all' else (case.pb,)):
        p, c0, pb, vz, fl = compat_inputs(case, pb_name, seed)
        with solver_from_problem(p, method, batch_capacity=case.B) as s:
            s.set_batch(c0, pb, vz, fl)
            s.step(nsteps, spl)
            c, v, g, l = s.get_state()
            st = s.get_status()
        assert np.all(st == 0), (pb_name, st)
        sub = [0, case.B // 2, case.B - 1]
        oc = np.ascontiguousarray(c0[sub].reshape(len(sub), case.N, case.nx).copy())
        ov, og, ol = CO.steps(p, method, oc, pb[sub], vz[sub], fl[sub], nsteps)
        for name, a, b in (('c', c[sub], oc), ('phi', v[sub], ov), ('grad', g[sub], og), ('lapl', l[sub], ol)):
            err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
            assert err < 1e-9, (pb_name, name, err)


@pytest.mark.parametrize('instance', sorted(CENSUS))
def test_instance_matches_the_oracle(instance, monkeypatch):
    case = CENSUS[instance]
    for k in OPTIONS:
        monkeypatch.delenv('CATINT_' + k, raising=False)
    if case.path == 'newton':
        monkeypatch.setenv('CATINT_NEWTON_KERNEL', case.kernel)
    for k, v in case.env:
        monkeypatch.setenv('CATINT_' + k, str(v))
    seed = zlib.crc32(instance.encode())
    if case.path == 'newton':
        run_newton_case(case, seed)
    else:
        run_compat_case(case, seed)


MOL_PB = {'dd': [0.02, 0.0, np.nan, np.nan], 'vwall_gbulk': [0.02, np.nan, np.nan, 1e4], 'gwall_vbulk': [np.nan, 0.0, 1e5, np.nan],
          'vwall_gwall': [0.01, np.nan, 1e5, np.nan], 'vbulk_gbulk': [np.nan, 0.0, np.nan, -1e4]}


@pytest.mark.parametrize('nx,pb_name,lf', [(5, 'dd', False), (66, 'vwall_gbulk', True), (67, 'gwall_vbulk', False), (130, 'vwall_gwall', True),
                                          (131, 'vbulk_gbulk', False), (258, 'dd', True), (259, 'vwall_gbulk', False),
                                          (514, 'gwall_vbulk', True), (515, 'vwall_gwall', False), (1026, 'vbulk_gbulk', True)])
def test_method_of_lines_rhs_matches_the_oracle(nx, pb_name, lf):
    """mol_rhs_kernel<P> (P = 1, 2, 4, 8, 16: the last grid of one P and the first of the next) against ode_func of the oracle; the
    grids beyond one wave take another path (tests/test_gpu_fullsize.py::test_method_of_lines_rhs_on_grids_beyond_one_wave)."""
    rng = np.random.default_rng(nx)
    N = 3
    p = R.Problem(D=np.array([1.957e-9, 2.032e-9, 1.185e-9]), charges=np.array([1, -1, -1]) * 96485.33289, beta=1 / (8.3144598 * 298.14),
                  eps=78.36 * 8.854187817e-12, dx=2e-11, nx=nx, dt=1e-12, pb=np.array(MOL_PB[pb_name]), vzeta=0.01,
                  flux_bound=np.array([1e-5, 0.0, -2e-5]), lax_friedrich=lf)
    y = rng.uniform(5.0, 15.0, (3, N * nx))
    y[:, :nx] = y[:, nx:2 * nx] + y[:, 2 * nx:]                     # neutral states: the potential stays moderate
    with solver_from_problem(p, 'FTCS', batch_capacity=3) as s:
        s.set_batch(y, np.stack([p.pb] * 3), [p.vzeta] * 3, np.stack([p.flux_bound] * 3))
        f = s.mol_rhs(y)
    for b in range(3):
        ref = R.mol_rhs(y[b], p, solver='banded')
        assert np.abs(f[b] - ref).max() <= 1e-9 * np.abs(ref).max(), b
