"""pnp_set_lane_mask on every stepper of the physical mode: a lane masked out of a call keeps its state, status, iteration counter AND its
BDF2 / predictor history -- a masked-out call is a skipped call.  For every lane, a sequence of pnp_step calls, some of them under a mask,
must give what an unmasked run of the same kernel family gives when it makes only the calls that lane took part in (same splits).
Within one family that is a comparison to the bit: a lane's arithmetic depends neither on the other lanes nor on its slot
(tests/test_gpu_lane.py: test_points_ordered_by_expected_iterations_give_the_same_bits), and split calls equal one call
(tests/test_gpu_newton.py: test_bdf2_steps_split_over_calls_and_second_order_in_time).  One small configuration per stepper is anchored
to the CPU oracle oracle/pnp_physical.py, and so are the lanes a stationary solve or pnp_set_lanes put back to a first step."""
import numpy as np
import pytest

from catint_amd import _capi
from oracle import pnp_physical as PH
from tests.test_gpu_newton import BETA, EPS, F, assert_close, make_lanes

pytestmark = pytest.mark.gpu

# kernel family -> (N, nx, B, options).  Batches are no multiples of the lane kernels' points per group (8 / 16 / 32).
FAMILIES = {
    'pair': (3, 128, 40, {}),                                                       # the library's choice: workgroup pair kernel
    'teams': (2, 1100, 9, {}),                                                      # ... lane teams (grid too long for the pair kernel)
    'team': (6, 96, 40, {'NEWTON_KERNEL': 'team'}),
    'generic': (3, 100, 9, {'NEWTON_KERNEL': 'generic'}),
    'sweep': (6, 96, 9, {'NEWTON_KERNEL': 'sweep'}),
    'both': (7, 80, 9, {'NEWTON_KERNEL': 'both'}),
    'lane': (6, 64, 70, {'NEWTON_KERNEL': 'lane', 'LANE_FUSED': '0'}),
    'lane-fused': (6, 64, 70, {'NEWTON_KERNEL': 'lane', 'LANE_FUSED': '1'}),
    'lane2': (6, 80, 37, {'NEWTON_KERNEL': 'lane2'}),
    'lane4': (8, 64, 37, {'NEWTON_KERNEL': 'lane4'}),
    'lane-f32': (8, 64, 70, {'NEWTON_KERNEL': 'lane', 'LANE_RECORDS': 'f32'}),
    # one group of workspace: the launcher walks the batch in chunks and moves the history in and out per chunk
    'lane-groups1': (6, 64, 70, {'NEWTON_KERNEL': 'lane', 'NEWTON_LANE_GROUPS': '1'}),
    'lane2-groups1': (6, 80, 37, {'NEWTON_KERNEL': 'lane2', 'NEWTON_LANE_GROUPS': '1'}),
    'lane4-groups1': (8, 64, 37, {'NEWTON_KERNEL': 'lane4', 'NEWTON_LANE_GROUPS': '1'}),
}

STEPPERS = {
    'euler': {},
    'bdf2': dict(time_order=2),
    'predictor': dict(predictor=True),
    'bdf2+predictor': dict(time_order=2, predictor=True),
    'predictor+steric': dict(predictor=True, mpb_radius=3.5e-10),      # the predictor's crowding guard reads the ion volumes
}


def newton_kw(stepper, N):
    kw = dict(STEPPERS[stepper])
    if 'mpb_radius' in kw:
        kw['mpb_radius'] = [kw['mpb_radius']] * N
    return kw


class Case:
    """One batch of make_lanes operating points and the handles that run it."""

    def __init__(self, N, nx, B, seed, options, kw):
        self.N, self.nx, self.B, self.options, self.kw = N, nx, B, dict(options), dict(kw)
        self.D, self.q, self.cb, self.dx, self.phiM = make_lanes(N, nx, B, seed)
        self.dt = 0.1 * (6 * self.dx) * (nx * self.dx) / self.D.max()
        self.c0 = np.repeat(self.cb[:, :, None], nx, axis=2)
        self.pb = np.zeros((B, 4))
        self.pb[:, 0] = self.phiM

    def solver(self, options=None):
        s = _capi.PnpSolver(self.N, self.nx, self.dx, self.dt, BETA, EPS, self.D, self.q, method='Newton', batch_capacity=self.B)
        opts = {'NEWTON_KERNEL': ''}
        opts.update(self.options if options is None else options)
        for k, v in opts.items():
            s.set_option(k, v)
        s.set_newton(**self.kw)
        s.set_batch(self.c0, self.pb, np.zeros(self.B), np.zeros((self.B, self.N)))
        return s

    def run(self, calls):
        """calls: [(nsteps, mask or None)].  Returns the final (c, phi) and, per call, (status, iteration counts) after it."""
        after = []
        with self.solver() as s:
            for n, mask in calls:
                s.set_lane_mask(mask)
                s.step(n)
                after.append((s.get_status().copy(), s.newton_iterations().copy()))
            s.set_lane_mask(None)
            c, phi = s.get_state()[:2]
        return c, phi, after


def active(calls, B):
    """[call][lane] bool: the lanes each call solves."""
    return np.array([np.ones(B, bool) if m is None else np.asarray(m) != 0 for _, m in calls])


def check_skipped_calls_are_skipped(case, calls, refs):
    """The property: every lane ends where the unmasked run of the calls it took part in ends, to the bit; after every call the active
    lanes report that run's status and iteration counts of the call, the others what they reported before.  refs: the unmasked runs
    made so far, by their sequence of calls."""
    B = case.B
    act = active(calls, B)
    c, phi, after = case.run(calls)
    for pattern in {tuple(act[:, b]) for b in range(B)}:
        lanes = np.flatnonzero((act == np.array(pattern)[:, None]).all(axis=0))
        own = tuple(n for (n, _), a in zip(calls, pattern) if a)
        assert own, 'every schedule gives every lane a call'
        if own not in refs:
            refs[own] = case.run([(n, None) for n in own])
        rc, rphi, rafter = refs[own]
        rc = rc.reshape(B, -1)
        assert np.array_equal(c.reshape(B, -1)[lanes], rc[lanes]), ('state', pattern, lanes)
        assert np.array_equal(phi[lanes], rphi[lanes]), ('potential', pattern, lanes)
        st_prev, it_prev = np.zeros(len(lanes), np.int32), np.zeros(len(lanes), np.int32)
        j = 0
        for i, a in enumerate(pattern):
            st, it = after[i][0][lanes], after[i][1][lanes]
            if a:
                assert np.array_equal(st, rafter[j][0][lanes]) and np.array_equal(it, rafter[j][1][lanes]), ('call', i, pattern, it, rafter[j][1][lanes])
                j += 1
            else:
                assert np.array_equal(st, st_prev) and np.array_equal(it, it_prev), ('masked-out call', i, pattern, it, it_prev)
            st_prev, it_prev = st, it
        assert (st_prev == 0).all()


def masks(B, kind):
    m = np.ones(B, np.int32)
    if kind == 'third-off':
        m[2::3] = 0
    else:                                           # 'single-on'
        m[:] = 0
        m[B // 2] = 1
    return m


# (a) mask on the middle call, (b) on the first, (c) two complementary masks in a row, (d) a mask without a lane, (e) a mask of every lane
# (the same bits as no mask: its reference is the unmasked run of the same calls)
SCHEDULES = {
    'a-middle': lambda m: [(2, None), (1, m), (2, None)],
    'b-first': lambda m: [(1, m), (3, None)],
    'c-complementary': lambda m: [(2, m), (2, 1 - m), (1, None)],
    'd-all-zero': lambda m: [(2, None), (1, 0 * m), (2, None)],
    'e-all-ones': lambda m: [(2, None), (1, 0 * m + 1), (2, None)],
}
_REFS = {}      # (family, stepper) -> the unmasked runs by their sequence of calls, shared by the schedules


@pytest.mark.parametrize("schedule,pattern", [(k, p) for k in SCHEDULES for p in ('third-off', 'single-on')
                                               if p == 'third-off' or k not in ('d-all-zero', 'e-all-ones')])
@pytest.mark.parametrize("stepper", list(STEPPERS))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_masked_out_call_is_a_skipped_call(family, stepper, schedule, pattern):
    N, nx, B, options = FAMILIES[family]
    case = Case(N, nx, B, 5 + N, options, newton_kw(stepper, N))
    check_skipped_calls_are_skipped(case, SCHEDULES[schedule](masks(B, pattern)), _REFS.setdefault((family, stepper), {}))


def oracle_problem(case, b):
    return PH.PhysicalProblem(D=case.D, charges=case.q, beta=BETA, eps=EPS, dx=case.dx, nx=case.nx, c_bulk=case.cb[b], phiM=case.phiM[b],
                              flux=np.zeros(case.N), mpb_radius=case.kw.get('mpb_radius'))


def oracle_integrate(case, b, c, phi, nsteps):
    if nsteps == 0:
        return c, phi, 0
    cc, ph, its = PH.integrate(oracle_problem(case, b), c.copy(), phi.copy(), case.dt, nsteps, bdf2=case.kw.get('time_order', 1) == 2,
                               predictor=bool(case.kw.get('predictor', False)), tol=1e-10, maxit=50, dphi_max=0.05)
    return cc, ph, sum(its)


@pytest.mark.parametrize("stepper", ['euler', 'bdf2', 'predictor', 'bdf2+predictor'])
@pytest.mark.parametrize("family", ['pair', 'lane'])
def test_masked_middle_call_matches_the_oracle(family, stepper):
    """Schedule [2, 1 under a mask, 2] on 8 lanes: the active lanes against the oracle's 5 steps, the skipped ones against its 4 (states to
    assert_close's tolerances, summed iteration counts equal)."""
    N, nx, B = 3, 64, 8
    case = Case(N, nx, B, 29, FAMILIES[family][3], newton_kw(stepper, N))
    m = masks(B, 'third-off')
    calls = [(2, None), (1, m), (2, None)]
    act = active(calls, B)
    c, phi, after = case.run(calls)
    its = sum(np.where(act[i], after[i][1], 0) for i in range(len(calls)))
    ref = [oracle_integrate(case, b, case.c0[b], np.zeros(nx), 5 if m[b] else 4) for b in range(B)]
    assert_close((c.reshape(B, N, nx), phi, its, after[-1][0]),
                 (np.array([r[0] for r in ref]), np.array([r[1] for r in ref]), np.array([r[2] for r in ref])))


@pytest.mark.parametrize("how", ['stationary', 'surface'])
@pytest.mark.parametrize("family,stepper", [('pair', 'bdf2+predictor'), ('lane', 'bdf2+predictor'), ('lane', 'bdf2'),
                                            ('lane4', 'bdf2'), ('team', 'bdf2')])
def test_stationary_solve_under_a_mask_restarts_only_the_lanes_it_solves(family, stepper, how):
    """In the middle of a BDF2 (and predictor) trajectory a stationary solve -- pnp_solve_stationary or pnp_solve_surface(nsteps = 0) --
    restricted to some lanes: the lanes it did not touch continue their trajectory to the bit; the solved ones start a new one with a
    backward-Euler step (oracle: the stationary solve from the state after two steps, then two steps from there)."""
    N, nx, B, options = FAMILIES[family]
    nx = min(nx, 64)
    case = Case(N, nx, B, 31, options, newton_kw(stepper, N))
    m = masks(B, 'third-off')
    solved = np.flatnonzero(m)[:4]
    m[:] = 0
    m[solved] = 1
    with case.solver() as s:
        s.step(2)
        c2, phi2 = (a.copy() for a in s.get_state()[:2])
        s.set_lane_mask(m)
        st = s.solve_stationary() if how == 'stationary' else s.solve_surface(nsteps=0)[3]
        it_stat = s.newton_iterations().copy()
        s.set_lane_mask(None)
        s.step(2)
        c, phi = s.get_state()[:2]
        st, its = s.get_status(), s.newton_iterations()
    assert (st == 0).all()
    untouched = m == 0
    rc, rphi, _ = case.run([(2, None), (2, None)])
    assert np.array_equal(c[untouched], rc[untouched]) and np.array_equal(phi[untouched], rphi[untouched])
    c2 = c2.reshape(B, N, nx)
    for b in solved:
        p = oracle_problem(case, b)
        cs, ps, it, _ = PH.newton_step(p, c2[b].copy(), phi2[b].copy(), c2[b].copy(), np.inf, tol=1e-10, maxit=50, dphi_max=0.05)
        assert it_stat[b] == it
        cc, ph, n_it = oracle_integrate(case, b, cs, ps, 2)
        assert_close((c.reshape(B, N, nx)[b:b + 1], phi[b:b + 1], its[b:b + 1], st[b:b + 1]), (cc[None], ph[None], np.array([n_it])))


@pytest.mark.parametrize("family,stepper", [('pair', 'bdf2'), ('pair', 'bdf2+predictor'), ('lane', 'bdf2'), ('lane2', 'bdf2'),
                                            ('sweep', 'predictor')])
def test_set_lanes_restarts_only_the_patched_lanes(family, stepper):
    """pnp_set_lanes in the middle of a BDF2 / predictor trajectory: the patched lanes start over with a backward-Euler step (here they
    are put back to their initial state: they end where a fresh two-step run ends, and on the oracle's two steps); every other lane
    keeps its history and ends where the run without the patch ends, to the bit."""
    N, nx, B, options = FAMILIES[family]
    nx = min(nx, 64)
    case = Case(N, nx, B, 37, options, newton_kw(stepper, N))
    lanes = np.array([1, B // 2, B - 1])
    with case.solver() as s:
        s.step(2)
        s.set_lanes(lanes, case.c0[lanes], np.zeros((len(lanes), nx)))
        s.step(2)
        c, phi = s.get_state()[:2]
        st, its = s.get_status(), s.newton_iterations()
    assert (st == 0).all()
    others = np.setdiff1d(np.arange(B), lanes)
    rc, rphi, _ = case.run([(2, None), (2, None)])
    assert np.array_equal(c[others], rc[others]) and np.array_equal(phi[others], rphi[others])
    fc, fphi, fafter = case.run([(2, None)])
    assert np.array_equal(c[lanes], fc[lanes]) and np.array_equal(phi[lanes], fphi[lanes]) and np.array_equal(its[lanes], fafter[0][1][lanes])
    ref = [oracle_integrate(case, b, case.c0[b], np.zeros(nx), 2) for b in lanes]
    assert_close((c.reshape(B, N, nx)[lanes], phi[lanes], its[lanes], st[lanes]),
                 (np.array([r[0] for r in ref]), np.array([r[1] for r in ref]), np.array([r[2] for r in ref])))


def test_family_change_under_a_mask_keeps_the_meaning_of_the_history(monkeypatch):
    """N = 8, nx = 16, B = 1024 is the lane-quad kernel's batch (test_default_family_follows_the_measured_thresholds); a mask of five
    lanes makes it a workgroup-per-point batch.  BDF2 [2, 1 under the mask, 2]: the history the lane-quad kernel left in the handle is
    read by the per-step path of the workgroup kernels -- the active lanes agree with the unmasked lane-quad run to the Newton tolerance,
    the skipped ones are the unmasked two-call run to the bit."""
    N, nx, B = 8, 16, 1024
    case = Case(N, nx, B, 43, {}, dict(time_order=2, mpb_radius=[3.5e-10] * N))
    m = np.zeros(B, np.int32)
    m[[3, 200, 511, 700, 1023]] = 1
    with case.solver() as s:
        assert s.default_family() == 'lane4'
        s.set_lane_mask(m)
        assert s.default_family() == 'workgroup'
        s.set_lane_mask(None)
    c, phi, after = case.run([(2, None), (1, m), (2, None)])
    assert (after[-1][0] == 0).all()
    rc, rphi, _ = case.run([(2, None), (1, None), (2, None)])
    on, off = m == 1, m == 0
    scale = np.abs(rc[on]).max()
    assert np.abs(c[on] - rc[on]).max() <= 1e-9 * scale and np.abs(phi[on] - rphi[on]).max() <= 1e-9 * max(np.abs(rphi[on]).max(), 0.025)
    sc, sphi, _ = case.run([(2, None), (2, None)])
    assert np.array_equal(c[off], sc[off]) and np.array_equal(phi[off], sphi[off])


def test_scf_cycle_keeps_the_callers_mask():
    """pnp_scf_cycle runs its own per-lane activity; a mask the caller set before it is in force again afterwards: the next step leaves
    the masked-out lanes alone."""
    N, nx, B = 3, 64, 6
    case = Case(N, nx, B, 47, {}, {})
    k = np.linspace(1e-5, 5e-5, B)[:, None]
    with case.solver() as s:
        s.set_wall_kinetics([2], [[0.0, 0.0, -1.0]], k)
        assert (s.solve_stationary() == 0).all()
        cs, vs, es = s.get_surface()
        m = np.ones(B, np.int32)
        m[[1, 4]] = 0
        s.set_lane_mask(m)
        state = {'surface_concentration': cs.copy(), 'surface_concentration_old': cs.copy(), 'flux': np.zeros((B, N)),
                 'current_density_old': np.zeros((B, N)), 'mix': np.full(B, 0.5), 'accuracy': np.full(B, np.inf),
                 'surface_pH': np.full(B, 7.0), 'surface_potential': vs, 'surface_efield': es,
                 'step_to_check': np.full(B, 1), 'active': np.ones(B, np.int32), 'failed': np.zeros(B, np.int32)}
        s.scf_cycle(state, istep=1, max_iter=4, tau_scf=1e-12, faraday=F)
        c0, phi0 = (a.copy() for a in s.get_state()[:2])
        st0, it0 = s.get_status().copy(), s.newton_iterations().copy()
        s.step(1)
        c1, phi1 = s.get_state()[:2]
        st1, it1 = s.get_status(), s.newton_iterations()
    off, on = m == 0, m == 1
    assert np.array_equal(c1[off], c0[off]) and np.array_equal(phi1[off], phi0[off])
    assert np.array_equal(st1[off], st0[off]) and np.array_equal(it1[off], it0[off])
    assert (it1[on] > 0).all()


def test_scf_cycle_leaves_the_wall_kinetics_in_the_jacobian():
    """pnp_scf_cycle's transport solves take the wall kinetics as prescribed fluxes; that holds for the call alone.  The step after
    it equals, to the bit, the step of a fresh handle given the same state, flux and kinetics: a switch that outlived the call would
    drop the kinetics from the Jacobian and change the iterates."""
    N, nx, B = 3, 64, 6
    case = Case(N, nx, B, 47, {}, {})
    k = np.linspace(1e-5, 5e-5, B)[:, None]

    def step_once(s):
        s.step(1)
        return s.get_state()[:2] + (s.get_status(), s.newton_iterations())
    with case.solver() as s:
        s.set_wall_kinetics([2], [[0.0, 0.0, -1.0]], k)
        assert (s.solve_stationary() == 0).all()
        cs, vs, es = s.get_surface()
        state = {'surface_concentration': cs.copy(), 'surface_concentration_old': cs.copy(), 'flux': np.zeros((B, N)),
                 'current_density_old': np.zeros((B, N)), 'mix': np.full(B, 0.5), 'accuracy': np.full(B, np.inf),
                 'surface_pH': np.full(B, 7.0), 'surface_potential': vs, 'surface_efield': es,
                 'step_to_check': np.full(B, 1), 'active': np.ones(B, np.int32), 'failed': np.zeros(B, np.int32)}
        s.scf_cycle(state, istep=1, max_iter=4, tau_scf=1e-12, faraday=F)
        c0, phi0 = (a.copy() for a in s.get_state()[:2])
        flux = state['flux'].copy()
        after = step_once(s)
    assert np.abs(flux).max() > 0.0 and (after[3] > 0).all()
    with case.solver() as s:
        s.set_batch(c0, case.pb, np.zeros(B), flux)
        s.set_potential(phi0)
        s.set_wall_kinetics([2], [[0.0, 0.0, -1.0]], k)
        fresh = step_once(s)
    for a, b in zip(after, fresh):
        assert np.array_equal(a, b)


def test_a_rejected_call_leaves_nothing_behind():
    """A call the library rejects before any launch -- pnp_solve_surface with nsteps = -1, under a mask set for it -- in the middle of a
    BDF2 trajectory of the lane-pair kernel: once the mask is lifted, the steps after it end where step(2); step(2) ends, to the bit."""
    N, nx, B, options = FAMILIES['lane2']
    case = Case(N, nx, B, 5 + N, options, newton_kw('bdf2', N))
    with case.solver() as s:
        s.step(2)
        s.set_lane_mask(masks(B, 'third-off'))
        with pytest.raises(_capi.PnpError) as rejected:
            s.solve_surface(nsteps=-1)
        assert rejected.value.code == -1                # PNP_EINVAL
        s.set_lane_mask(None)
        s.step(2)
        got = s.get_state()[:2] + (s.get_status(), s.newton_iterations())
    rc, rphi, rafter = case.run([(2, None), (2, None)])
    for a, b in zip(got, (rc, rphi) + rafter[-1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("mask_during_tune", [True, False])
def test_autotune_under_a_mask_leaves_history_counters_and_mask_alone(mask_during_tune, monkeypatch):
    """BDF2 with a mask on the first call: the masked-in lanes have a history, the others none.  pnp_autotune (every family's trials,
    under that mask or with both kinds of lanes in one batch) leaves state, status, iteration counts, the per-lane history and the mask
    as they were: the steps after it continue exactly as with the chosen family forced from there on."""
    N, nx, B = 6, 64, 150
    case = Case(N, nx, B, 53, {}, dict(time_order=2, mpb_radius=[3.5e-10] * N))
    m = masks(B, 'third-off')

    def rest(s):
        if mask_during_tune:
            s.step(1)                          # (still under the mask)
            s.set_lane_mask(None)
        s.step(2)
        return s.get_state()[:2] + (s.newton_iterations(), s.get_status())
    with case.solver() as s:
        s.set_lane_mask(m)
        s.step(2)
        if not mask_during_tune:
            s.set_lane_mask(None)
        before = tuple(a.copy() for a in s.get_state()[:2]) + (s.newton_iterations().copy(), s.get_status().copy())
        name, ms = s.autotune(2)
        after = s.get_state()[:2] + (s.newton_iterations(), s.get_status())
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        if mask_during_tune:
            s.step(1)
            c, phi = s.get_state()[:2]
            assert np.array_equal(c[m == 0], before[0][m == 0]) and np.array_equal(s.newton_iterations()[m == 0], before[2][m == 0])
            s.set_lane_mask(None)
            s.step(2)
            tuned = s.get_state()[:2] + (s.newton_iterations(), s.get_status())
        else:
            tuned = rest(s)
    assert (tuned[3] == 0).all()
    forced = {'lane+fused': {'NEWTON_KERNEL': 'lane', 'LANE_FUSED': '1'}, 'lane': {'NEWTON_KERNEL': 'lane', 'LANE_FUSED': '0'}}.get(name, {'NEWTON_KERNEL': name})
    with case.solver() as s:
        s.set_lane_mask(m)
        s.step(2)
        if not mask_during_tune:
            s.set_lane_mask(None)
        for k, v in forced.items():
            s.set_option(k, v)
        ref = rest(s)
    for a, b in zip(tuned, ref):
        assert np.array_equal(a, b)
