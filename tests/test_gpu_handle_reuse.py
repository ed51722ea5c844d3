"""GPU: a handle that is used again computes what a fresh handle computes.

Production callers keep one pnp_handle alive and run many calls on it -- the continuation stages, the rerun ladder, the SCF loop, the
descriptor sweeps -- with different batch sizes, integrators and options, while the handle carries state that outlives a call: the
charge-row ping-pong and the step parity, per-lane BDF2 / predictor history, the lane order, the caller's mask, workspaces that are
zeroed once and then assumed clean.  Every test here runs a history of other calls on a USED handle, then a final upload and a final
call, and compares with a FRESH handle that gets the final upload and call alone: state, derived potential rows, surface values,
status, Newton iteration counts and the integrators' idid / stats / t_end, bit for bit (np.array_equal: both runs execute the same
kernels on the same rows).  In every family the fresh handle's result is tied to the CPU oracle the sibling tests use, at their
tolerances, so that the two handles cannot agree on a wrong answer.

Three places the suite could not see before, each with a named test:
  * the explicit integrators' shared workspace (ode_buf: DOP853's twelve buffers, DOPRI5's per-lane reals inside DOP853's ninth,
    RKC clearing five of them): test_integrators_share_one_workspace -- the code was right;
  * pnp_set_potential and the BDF2 / predictor history: test_set_potential_restarts_the_history -- it was a bug, the next step
    extrapolated from the potential the caller had just replaced; pnp_set_potential now clears the history of the lanes it overwrites;
  * a smaller batch after a larger one: test_compat_shrink_and_grow_over_poisoned_rows, test_newton_shrink_grow_and_permute -- the
    code was right.

The two cases that are not bitwise are documented where they stand (test_physics_switches_leave_nothing_behind: set_grid;
test_steps_continue_from_an_integrated_state: RKC).

That the tests bite was checked once with scratch builds of the library (not committed), each with one reset taken out:
  lane_hist.assign in pnp_set_batch                      -> test_upload_ends_the_bdf2_history (12 of 12), test_upload_drops_the_lane_mask (6 of 6)
  user_mask_set = false in pnp_set_batch                 -> test_upload_drops_the_lane_mask (6 of 6)
  h->cur = 0; launch_charge_row after the integrators    -> test_steps_continue_from_an_integrated_state (6 of 6)
  the history reset of pnp_set_potential (it was new)    -> test_set_potential_restarts_the_history (12 of 12)
and nothing else turned red in any of them.  Measured on an MI355X: the module's 252 cases take 6.5 s, the slowest 0.3 s
(tests/test_gpu_ode.py: 9.2 s, tests/test_gpu_stream.py: 11.6 s, tests/test_gpu_lane_mask.py: 12.8 s)."""
import dataclasses

import numpy as np
import pytest

from catint_amd import _capi
from oracle import c_oracle as CO
from oracle import pnp_ref as R
from tests import reuse_cases as RC
from tests.reuse_cases import NewtonCase, call, differing, snapshot
from tests.test_gpu_lane_mask import masks, oracle_integrate
from tests.test_gpu_newton import assert_close
from tests.test_gpu_ode import oracle_run, relerr, rkc_oracle_run

pytestmark = pytest.mark.gpu


def assert_same(got, want, what):
    """Bit for bit, every array; the message names the ones that differ (counted from the end: the snapshot's arrays come last)"""
    bad = differing(got, want)
    n = len(got)
    assert not bad, (what, ['%d of %d' % (i, n) for i in bad])


# =========================================================================================================================================
# compat mode (FTCS and Crank-Nicolson handles)
# =========================================================================================================================================
_PROBLEMS, _FRESH = {}, {}


def compat(key):
    """(method, capacity, problem, batch) of a compat case, built once"""
    if key not in _PROBLEMS:
        method = 'Crank-Nicolson' if key == 'two-waves' else key
        N, nx, B, cap, ratio = RC.TWO_WAVES if key == 'two-waves' else RC.COMPAT[key]
        p, c0, pb, vz, fl = RC.compat_problem(N, nx, B, ratio, seed=nx + N)
        _PROBLEMS[key] = (method, cap, p, (c0, pb, vz, fl))
    return _PROBLEMS[key]


def other_batch(key, B, seed):
    """Another batch for the same handle (same species, grid and timestep)"""
    method, cap, p, _ = compat(key)
    p2, c0, pb, vz, fl = RC.compat_problem(len(p.D), p.nx, B, 1.0, seed=seed)
    assert p2.dx == p.dx
    return c0, pb, vz, fl


def final_run(s, batch, final):
    s.set_batch(*batch)
    return call(s, final) + snapshot(s)


def fresh_result(key, final, batch=None, tag='own'):
    """The final upload and call on a handle that did nothing else: computed once per (case, call, batch), shared and left unchanged"""
    if (key, final, tag) not in _FRESH:
        method, cap, p, own = compat(key)
        with RC.compat_solver(p, method, cap) as s:
            _FRESH[(key, final, tag)] = final_run(s, own if batch is None else batch, final)
    return _FRESH[(key, final, tag)]


def used_result(key, history, final, batch=None, history_batch=None):
    method, cap, p, own = compat(key)
    with RC.compat_solver(p, method, cap) as s:
        s.set_batch(*(own if history_batch is None else history_batch))
        for name in history:
            call(s, name)
        return final_run(s, own if batch is None else batch, final)


@pytest.mark.parametrize('final', list(RC.OPS))
@pytest.mark.parametrize('history', list(RC.OPS))
@pytest.mark.parametrize('key', ['FTCS', 'Crank-Nicolson'])
def test_every_call_after_every_other_call(key, history, final):
    """The square: every stepper and integrator as the final call after every other one as the only history"""
    assert_same(used_result(key, [history], final), fresh_result(key, final), (key, history, final))


CHAINS = {
    'dop853-dopri5-dop853': (['dop853', 'dopri5'], 'dop853'),
    'rkc-dopri5': (['rkc'], 'dopri5'),
    'dopri5-dop853-rkc-dopri5': (['dopri5', 'dop853', 'rkc'], 'dopri5'),
    'long-chain-step': (RC.LONG_CHAIN, 'step1'),
    'long-chain-dop853': (RC.LONG_CHAIN, 'dop853'),
    'long-chain-rkc': (RC.LONG_CHAIN, 'rkc'),
}


@pytest.mark.parametrize('chain', list(CHAINS))
@pytest.mark.parametrize('key', ['FTCS', 'Crank-Nicolson', 'two-waves'])
def test_integrators_share_one_workspace(key, chain):
    """ode_buf is zeroed when it is allocated and kept: after DOP853 it has twelve state-sized buffers, a later DOPRI5 puts its per-lane
    reals at the start of DOP853's ninth (with B = 33 lanes of 10 reals they run over the pad columns of its first rows), RKC clears
    the first five only.  Every kernel reads and writes the first nx columns of a row alone, so none of this reaches a result -- which is
    what the orders DOP853 -> DOPRI5 -> DOP853 and RKC -> DOPRI5 and the long interleaving of every call show here, also on a grid of
    two waves per system (the point-wise right-hand side behind the multi-wave Poisson solve)."""
    history, final = CHAINS[chain]
    assert_same(used_result(key, history, final), fresh_result(key, final), (key, chain))


@pytest.mark.parametrize('final', ['step1', 'fused', 'mol_rhs', 'rkc', 'dop853', 'dopri5'])
@pytest.mark.parametrize('method', ['FTCS', 'Crank-Nicolson'])
def test_compat_shrink_and_grow_over_poisoned_rows(method, final):
    """64 lanes of large values with a NaN lane and a negative lane among rows 5 .. 63, stepped and integrated; then 5 other lanes, then
    33: what the first batch left in rows [B, 64) of every buffer reaches neither of the later batches -- their results are a fresh
    handle's, finite, with status 0 everywhere."""
    N, nx = 2, 66
    key = ('shrink', method)
    if key not in _PROBLEMS:
        p, c0, pb, vz, fl = RC.compat_problem(N, nx, 64, 0.4, seed=64)
        _PROBLEMS[key] = (method, 70, p, (c0, pb, vz, fl))
    _, cap, p, (c64, pb64, vz64, fl64) = compat(key)
    c64 = 50.0 * c64
    c64[40, 5] = np.nan
    c64[11, :nx] = -3.0
    small, medium = other_batch(key, 5, seed=5), other_batch(key, 33, seed=33)
    with RC.compat_solver(p, method, cap) as s:
        s.set_batch(c64, pb64, vz64, fl64)
        s.step(3, 1)
        st = s.get_status()
        assert st[40] != 0 and st[11] != 0                    # the poison took
        s.integrate_dop853(1, [0], nsteps=20)
        s.integrate_rkc(1, [0], nsteps=20)
        got5 = final_run(s, small, final)
        got33 = final_run(s, medium, final)
    for got, batch, tag in ((got5, small, 'B=5'), (got33, medium, 'B=33')):
        assert_same(got, fresh_result(key, final, batch, tag), (method, final, tag))
        assert (got[-1] == 0).all() and all(np.isfinite(a).all() for a in got), tag


@pytest.mark.parametrize('streams,B', [(None, 33), ('3', 770)])
@pytest.mark.parametrize('method', ['FTCS', 'Crank-Nicolson'])
def test_odd_step_parity_ends_with_the_upload(method, streams, B, monkeypatch):
    """Every other one-step launch walks the rows backwards (ALTERNATE_ROWS) and the charge row ping-pongs: three steps leave both odd.
    After an upload two steps are a fresh handle's two steps -- also with the batch cut into three row chunks on streams of their own
    (770 operating points: the smallest batch STEP_STREAMS = 3 cuts three ways is 768)."""
    monkeypatch.setenv('CATINT_PNP_ALTERNATE_ROWS', '1')
    if streams:
        monkeypatch.setenv('CATINT_PNP_STEP_STREAMS', streams)
    p, c0, pb, vz, fl = RC.compat_problem(2, 66, B, 0.4, seed=B)
    first = RC.compat_problem(2, 66, B, 0.4, seed=B + 1)[1:]
    results = []
    for history in (True, False):
        with RC.compat_solver(p, method, B) as s:
            if history:
                s.set_batch(*first)
                assert s.step_row_chunks(3) == (3 if streams else 1)
                s.step(3, 1)
            s.set_batch(c0, pb, vz, fl)
            s.step(2, 1)
            results.append(snapshot(s))
    assert_same(results[0], results[1], (method, streams))
    sub = np.arange(0, B, max(1, B // 3))[:3]
    oc = np.ascontiguousarray(c0[sub].reshape(len(sub), 2, 66).copy())
    ov, og, ol = CO.steps(p, method, oc, pb[sub], vz[sub], fl[sub], 2)
    c, v, g = results[1][:3]
    assert relerr(c[sub], oc) < 1e-9 and relerr(v[sub], ov) < 1e-9 and relerr(g[sub], og) < 1e-9


@pytest.mark.parametrize('final', ['dopri5', 'dop853', 'rkc'])
@pytest.mark.parametrize('history', ['dopri5', 'dop853', 'rkc'])
def test_lanes_that_ended_early_leave_no_record(history, final):
    """An integrator whose step budget is too small freezes its lanes with idid = -2; their per-lane records (time, step size, counters,
    the inactive flag) belong to that call: the next run on the handle is a fresh handle's."""
    key = 'Crank-Nicolson'
    method, cap, p, own = compat(key)
    with RC.compat_solver(p, method, cap) as s:
        s.set_batch(*own)
        fn = {'dopri5': s.integrate_dopri5, 'dop853': s.integrate_dop853, 'rkc': s.integrate_rkc}[history]
        _, idid, _, t_end = fn(3, [0, 1, 2], nsteps=1)
        assert (idid == -2).all() and (t_end < 3 * p.dt).all()
        got = final_run(s, own, final)
    assert_same(got, fresh_result(key, final), (history, final))
    assert (got[1] == 1).all()                                # idid of the final run


@pytest.mark.parametrize('integrator', ['rkc', 'dop853', 'dopri5'])
@pytest.mark.parametrize('key', ['FTCS', 'Crank-Nicolson'])
def test_steps_continue_from_an_integrated_state(key, integrator):
    """An integrator leaves the handle as an upload of its final state would: charge row of that state in the first buffer, step parity
    even.  After three one-step launches (both odd) and an integrator, the potential read back and two more steps are those of a fresh
    handle that was given the integrated state.

    RKC's two steps are held to the project's fp64 parity bound, 1e-9 relative, not to the bit: the right-hand side is exactly zero at
    the bulk point, which DOPRI5 and DOP853 therefore return untouched (y + h * 0), but RKC's stage recurrence
    (1 - mu - nu) y_0 + mu y_j-1 + nu y_j-2 rounds it away from its value by an ulp or two.  The upload of the fresh handle takes its
    Dirichlet value from that last point, the used handle keeps the one of its own upload: the two differ in the last bits (printed),
    and so do the steps.  No sum is reordered; the read-back, which does not involve the bulk value, is bitwise for all three."""
    method, cap, p, (c0, pb, vz, fl) = compat(key)
    with RC.compat_solver(p, method, cap) as s:
        s.set_batch(c0, pb, vz, fl)
        s.step(3, 1)
        out = call(s, integrator)
        assert (out[1] == 1).all()
        after = snapshot(s)
        s.step(2, 1)
        later = snapshot(s)
    bulk0, bulk1 = c0.reshape(after[0].shape)[:, :, -1], after[0][:, :, -1]
    drift = np.abs(bulk1 - bulk0).max() / np.abs(bulk0).max()
    print('REUSE | %s | %s | bulk point moved by %.2e relative |' % (key, integrator, drift))
    assert drift <= 8 * 2.0 ** -52 and (integrator == 'rkc' or drift == 0.0)
    with RC.compat_solver(p, method, cap) as s:
        s.set_batch(after[0], pb, vz, fl)
        assert_same(snapshot(s), after, (key, integrator, 'read-back'))
        s.step(2, 1)
        fresh = snapshot(s)
    if integrator != 'rkc':
        assert_same(fresh, later, (key, integrator, 'two steps on'))
    else:
        assert np.array_equal(fresh[-1], later[-1])
        for a, b in zip(fresh[:-1], later[:-1]):
            assert np.abs(a - b).max() <= 1e-9 * np.abs(b).max(), (key, np.abs(a - b).max(), np.abs(b).max())


@pytest.mark.parametrize('B', [5, 770])
def test_potential_follows_set_pb_without_a_step(B):
    """get_state before and after set_pb without any step: the derived potential is the new boundary values', not a cached one (a
    batch of 768 and more computes it at the upload already)."""
    p, c0, pb, vz, fl = RC.compat_problem(2, 66, B, 0.4, seed=B)
    pb2 = pb.copy()
    pb2[:, 0] = -1.5 * pb[:, 0] + 0.004
    vz2 = pb2[:, 0].copy()
    with RC.compat_solver(p, 'Crank-Nicolson', B) as s:
        s.set_batch(c0, pb, vz, fl)
        before = snapshot(s)
        s.set_pb(pb2, vz2)
        after = snapshot(s)
    with RC.compat_solver(p, 'Crank-Nicolson', B) as s:
        s.set_batch(c0, pb2, vz2, fl)
        fresh = snapshot(s)
    assert_same(after, fresh, B)
    assert not np.array_equal(before[1], after[1]) and np.array_equal(before[0], after[0])


# ---- the oracle anchors of the compat cases: the fresh handle's results against the CPU --------------------------------------------------
@pytest.mark.parametrize('key', ['FTCS', 'Crank-Nicolson', 'two-waves'])
def test_fresh_compat_results_match_the_cpu_oracles(key):
    """What the differential tests compare with is right: the fresh handle's steppers against the C oracle (1e-9, as
    tests/test_gpu_stream.py), its right-hand side against oracle/pnp_ref.py (1e-9 per species row), its integrators against the
    pinned oracles driving the device right-hand side of a handle of their own (same step sequence; 1e-12 DOPRI5, 1e-9 DOP853, 1e-10 RKC,
    as tests/test_gpu_ode.py), on two or three lanes."""
    method, cap, p, (c0, pb, vz, fl) = compat(key)
    N, nx, B = len(p.D), p.nx, c0.shape[0]
    lanes = sorted({0, B // 2, B - 1})
    sub = np.array(lanes)
    n_int = 4 if method == 'FTCS' else 3                     # pnp_integrate(nt = 4): passes 0 .. 3 (FTCS), 1 .. 3 (Crank-Nicolson)
    for final, nsteps in (('step1', 3), ('fused', 5), ('integrate', n_int)):
        res = fresh_result(key, final)
        c, v, g = res[-8], res[-7], res[-6]
        oc = np.ascontiguousarray(c0[sub].reshape(len(sub), N, nx).copy())
        ov, og, ol = CO.steps(p, method, oc, pb[sub], vz[sub], fl[sub], nsteps)
        assert (res[-1] == 0).all()
        assert relerr(c[sub], oc) < 1e-9 and relerr(v[sub], ov) < 1e-9 and relerr(g[sub], og) < 1e-9, final
        if final == 'integrate':
            assert np.array_equal(res[0][-1].reshape(B, N, nx), c)
    with RC.compat_solver(p, method, cap) as s:
        s.set_batch(c0, pb, vz, fl)
        y = RC.rhs_argument(s)
    f = fresh_result(key, 'mol_rhs')[0]
    for b in lanes:
        pl = dataclasses.replace(p, pb=pb[b].copy(), vzeta=float(vz[b]), flux_bound=fl[b].copy())
        ref = R.mol_rhs(y[b], pl, use_reactions=False, solver='banded').reshape(N, nx)
        err = np.abs(f[b].reshape(N, nx) - ref).max(axis=1) / np.abs(ref).max(axis=1)
        assert err.max() < 1e-9, (b, err)
    b = lanes[-1]
    with RC.compat_solver(p, method, cap) as s:               # the oracles' right-hand side: a handle of its own
        s.set_batch(c0, pb, vz, fl)
        for final, order in (('dopri5', 5), ('dop853', 8)):
            cout, idid, stats, t_end = fresh_result(key, final)[:4]
            o, ref = oracle_run(s, c0.copy(), B, b, 2, order=order, **RC.ODE_KW)
            assert idid[b] == 1 and o.idid == 1 and stats[b][0] == len(o.log) and stats[b][3] == o.nfcn
            assert relerr(cout[-1, b], ref[-1]) < (1e-12 if order == 5 else 1e-9) and abs(t_end[b] - o.t) <= 1e-13 * o.t
        cout, idid, stats, t_end = fresh_result(key, 'rkc')[:4]
        o, ref = rkc_oracle_run(s, c0.copy(), b, 2)
        assert idid[b] == 1 and list(stats[b][:4]) == [o.nsteps, o.naccpt, o.nrejct, o.nfe] and relerr(cout[-1, b], ref[-1]) < 1e-10


# =========================================================================================================================================
# physical (Newton) mode
# =========================================================================================================================================
FAMS = list(RC.NEWTON_FAMILIES)
BDF2P = dict(time_order=2, predictor=True)


def steps(s, n):
    s.step(n)
    return snapshot(s)


def anchor(case, lanes, got, nsteps, c=None, phi=None):
    """The lanes `lanes` of a snapshot against oracle/pnp_physical.py: nsteps timesteps of the case's stepper from its bulk state (or
    from c, phi), tests/test_gpu_newton.py's assert_close (2e-9 of the profile scale, identical iteration counts)"""
    ref = [oracle_integrate(case, b, case.c0[b] if c is None else c[b], np.zeros(case.nx) if phi is None else phi[b], nsteps) for b in lanes]
    lanes = np.asarray(lanes)
    assert_close((got[0].reshape(-1, case.N, case.nx)[lanes], got[1][lanes], got[8][lanes], got[7][lanes]),
                 (np.array([r[0] for r in ref]), np.array([r[1] for r in ref]), np.array([r[2] for r in ref])))


@pytest.mark.parametrize('predictor', [False, True])
@pytest.mark.parametrize('family', FAMS)
def test_upload_ends_the_bdf2_history(family, predictor):
    """Three BDF2 steps, then set_batch with a new state, then two steps: the fresh handle gets the second upload and its two steps."""
    kw = dict(time_order=2, predictor=predictor)
    a = NewtonCase(family, 61, kw)
    b = a.other(seed=62)
    with a.handle() as s:
        a.upload(s)
        s.step(3)
        b.upload(s)
        got = steps(s, 2)
    with b.handle() as s:
        b.upload(s)
        want = steps(s, 2)
    assert_same(got, want, (family, predictor))
    assert (want[7] == 0).all()
    anchor(b, [0, b.B - 1], want, 2)


@pytest.mark.parametrize('stepper', ['predictor', 'bdf2'])
@pytest.mark.parametrize('family', FAMS)
def test_set_potential_restarts_the_history(family, stepper):
    """Steps with a history, then set_potential, then one step: pnp_set_potential clears the history of the lanes it overwrites (all of
    them), so the step is a fresh handle's first step from the same state and potential -- backward Euler from the rows the caller
    gave, not an extrapolation through the potential they replaced."""
    kw = dict(predictor=True) if stepper == 'predictor' else dict(time_order=2)
    a = NewtonCase(family, 63, kw)
    with a.handle() as s:
        a.upload(s)
        s.step(2)
        c, phi = (x.copy() for x in s.get_state()[:2])
        guess = 0.5 * phi
        s.set_potential(guess)
        got = steps(s, 1)
    with a.handle() as s:
        a.upload(s, c, guess)
        want = steps(s, 1)
    assert_same(got, want, (family, stepper))
    assert (want[7] == 0).all()
    anchor(a, [1, a.B - 2], want, 1, c.reshape(a.B, a.N, a.nx), guess)


@pytest.mark.parametrize('how', ['host', 'device'])
@pytest.mark.parametrize('family', FAMS)
def test_set_lanes_on_a_subset(family, how):
    """set_lanes / set_lanes_device on three lanes in the middle of a BDF2 + predictor trajectory: the untouched lanes continue as in a
    run without the call, the replaced ones behave as freshly uploaded ones (rows from a donor handle that took one step; on the
    device path they come from its resample onto its own grid, which is the identity to the bit)."""
    a = NewtonCase(family, 65, BDF2P)
    lanes = np.array([1, a.B // 2, a.B - 1])
    with a.handle(kw={}) as donor:
        a.upload(donor)
        donor.step(1)
        dc, dphi = donor.get_state()[:2]
        with a.handle() as s:
            a.upload(s)
            s.step(2)
            if how == 'host':
                s.set_lanes(lanes, dc[lanes], dphi[lanes])
            else:
                c_dev, phi_dev = donor.resample(donor.grid, lanes=lanes, to_host=False)
                s.set_lanes_device(c_dev, phi_dev, lanes=lanes)
            got = steps(s, 2)
    with a.handle() as s:
        a.upload(s)
        s.step(2)
        plain = steps(s, 2)
    cm, pm = a.c0.copy(), np.zeros((a.B, a.nx))
    cm[lanes], pm[lanes] = dc.reshape(a.B, a.N, a.nx)[lanes], dphi[lanes]
    with a.handle() as s:
        a.upload(s, cm, pm)
        new = steps(s, 2)
    others = np.setdiff1d(np.arange(a.B), lanes)
    assert_same([x[others] for x in got], [x[others] for x in plain], (family, how, 'untouched'))
    assert_same([x[lanes] for x in got], [x[lanes] for x in new], (family, how, 'replaced'))
    assert (got[7] == 0).all()
    anchor(a, lanes[:2], got, 2, cm, pm)


@pytest.mark.parametrize('family', FAMS)
def test_switching_time_order_and_predictor_between_steps(family):
    """time_order 1 -> 2 -> 1 -> 2 with the predictor switched on and off on the way: every change of the stepper ends the history,
    so the last two steps are those of a fresh handle that was given the state and the final setting only (its first step is backward
    Euler)."""
    a = NewtonCase(family, 67, dict(time_order=2))
    with a.handle(kw=dict(time_order=1)) as s:
        a.upload(s)
        s.step(1)
        s.set_newton(time_order=2)
        s.step(2)
        s.set_newton(time_order=1, predictor=True)
        s.step(2)
        s.set_newton(time_order=2, predictor=True)
        s.step(2)
        c, phi = (x.copy() for x in s.get_state()[:2])
        s.set_newton(time_order=2)
        got = steps(s, 2)
    with a.handle() as s:
        a.upload(s, c, phi)
        want = steps(s, 2)
    assert_same(got, want, family)
    anchor(a, [0, a.B - 1], want, 2, c.reshape(a.B, a.N, a.nx), phi)


@pytest.mark.parametrize('family', FAMS)
def test_upload_drops_the_lane_mask(family):
    """set_lane_mask, then set_batch: the mask belonged to the batch it was set for -- every lane of the new batch advances and equals
    the fresh handle's."""
    a = NewtonCase(family, 69, dict(time_order=2))
    b = a.other(seed=70)
    with a.handle() as s:
        a.upload(s)
        s.set_lane_mask(masks(a.B, 'third-off'))
        s.step(2)
        b.upload(s)
        got = steps(s, 2)
    with b.handle() as s:
        b.upload(s)
        want = steps(s, 2)
    assert_same(got, want, family)
    assert (got[8] > 0).all() and not np.array_equal(got[0], b.c0.reshape(b.B, b.N, b.nx))
    anchor(b, [2, 5], want, 2)                                # (lanes the mask had switched off)


@pytest.mark.parametrize('family', FAMS)
def test_stationary_solve_then_steps(family):
    """solve_stationary moves every lane off its trajectory: the BDF2 + predictor steps after it are those of a fresh handle given the
    stationary state."""
    a = NewtonCase(family, 71, BDF2P)
    with a.handle() as s:
        a.upload(s)
        s.step(2)
        assert (s.solve_stationary() == 0).all()
        c, phi = (x.copy() for x in s.get_state()[:2])
        got = steps(s, 2)
    with a.handle() as s:
        a.upload(s, c, phi)
        want = steps(s, 2)
    assert_same(got, want, family)
    anchor(a, [0, a.B - 1], want, 2, c.reshape(a.B, a.N, a.nx), phi)


@pytest.mark.parametrize('family', ['lane', 'lane2', 'lane4'])
def test_tune_placement_in_the_middle_of_a_bdf2_sequence(family):
    """pnp_tune_placement reallocates the lane workspace and times steps from the current state: state, history, status and iteration
    counts continue as if the call had not happened."""
    a = NewtonCase(family, 73, dict(time_order=2))
    out = []
    for tune in (True, False):
        with a.handle() as s:
            a.upload(s)
            s.step(2)
            before = snapshot(s)
            if tune:
                assert len(s.tune_placement(nsteps=1, trials=2)) >= 1
                assert_same(snapshot(s), before, (family, 'put back'))
            out.append(steps(s, 2))
    assert_same(out[0], out[1], family)


def test_autotune_in_the_middle_of_a_bdf2_sequence():
    """pnp_autotune tries every family from the current state and puts it back; the steps after it are those of the same sequence with
    the chosen family forced from that point on (families agree to the Newton tolerance only, so the reference changes family too)."""
    a = NewtonCase('lane', 75, dict(time_order=2, mpb_radius=[3.5e-10] * 6))
    a.options = {}
    with a.handle() as s:
        a.upload(s)
        s.step(2)
        before = snapshot(s)
        name, ms = s.autotune(1)
        assert_same(snapshot(s), before, 'put back')
        got = steps(s, 2)
    forced = {'lane+fused': {'NEWTON_KERNEL': 'lane', 'LANE_FUSED': '1'}, 'lane': {'NEWTON_KERNEL': 'lane', 'LANE_FUSED': '0'}}.get(name, {'NEWTON_KERNEL': name})
    with a.handle() as s:
        a.upload(s)
        s.step(2)
        for k, v in forced.items():
            s.set_option(k, v)
        want = steps(s, 2)
    assert_same(got, want, name)
    assert (got[7] == 0).all()


@pytest.mark.parametrize('family', FAMS)
def test_newton_shrink_grow_and_permute(family):
    """A large batch with a NaN lane and a negative lane among rows 5 and up ('lane': 70 operating points, dealt to the slots by the
    iteration counts of the call before), then 5 other lanes, then a batch of the first size whose lanes are a permutation of a third
    one: the small batch is a fresh handle's (status 0, finite, iteration counts of length B), the permuted one is the fresh handle's
    result permuted the same way."""
    a = NewtonCase(family, 77, dict(time_order=2))
    small, third = a.other(B=5, seed=78), a.other(seed=79)
    perm = np.random.default_rng(7).permutation(a.B)
    poisoned = a.c0.copy()
    poisoned[a.B - 2, 0, 3] = np.nan
    poisoned[6] = -1.0
    with a.handle() as s:
        a.upload(s, 20.0 * poisoned)
        s.step(2)
        s.step(1)
        small.upload(s)
        got5 = steps(s, 2)
        third.upload(s, lanes=perm)
        s.step(1)
        gotp = steps(s, 2)
    with small.handle() as s:
        small.upload(s)
        want5 = steps(s, 2)
    with third.handle() as s:
        third.upload(s)
        s.step(1)
        wantp = steps(s, 2)
    assert_same(got5, want5, (family, 'B=5'))
    assert len(got5[8]) == 5 and (got5[7] == 0).all() and all(np.isfinite(x).all() for x in got5)
    assert_same(gotp, [x[perm] for x in wantp], (family, 'permuted'))
    assert len(gotp[8]) == a.B and (gotp[7] == 0).all()
    anchor(small, [0, 4], want5, 2)


def _wall(s, case, on):
    if on:
        s.set_wall_kinetics([case.N - 1], [[0.0] * (case.N - 1) + [-1.0]], np.linspace(1e-5, 5e-5, case.B)[:, None])
    else:
        s.set_wall_kinetics([], [], None)


def _reactions(s, case, on):
    s.set_reactions([([0, 1], [2], 1e2, 1.2e5)] if on else [])


def _convection(s, case, on):
    s.set_convection(3.0 * case.D.max() / ((case.nx - 1) * case.dx) if on else 0.0)


def _grid(s, case, on):
    x = np.arange(case.nx) * case.dx
    s.set_grid(x * (1.0 + 0.5 * x / x[-1]) if on else x)


SWITCHES = {'wall_kinetics': _wall, 'reactions': _reactions, 'convection': _convection, 'grid': _grid}


@pytest.mark.parametrize('switch', list(SWITCHES))
@pytest.mark.parametrize('family', FAMS)
def test_physics_switches_leave_nothing_behind(family, switch):
    """set_wall_kinetics, set_reactions, set_convection and set_grid, each turned on, stepped, turned off again, then stepped: the last
    steps are those of a handle that never had the switch and was given the same state.

    set_grid is the one case that cannot be bitwise against a handle that never had it: pnp_create gives the uniform grid the weights
    1 exactly, pnp_set_grid computes dx / (x[i+1] - x[i]) from the nodes i * dx, which is 1 to a rounding -- the difference quotients of
    every flux are scaled by another last bit, no sum is reordered.  There the bitwise reference is a fresh handle that is given the
    same uniform nodes through set_grid, and the handle that never had the call is held to the project's fp64 parity bound, 1e-9
    relative."""
    a = NewtonCase(family, 81, {})
    toggle = SWITCHES[switch]
    with a.handle() as s:
        a.upload(s)
        toggle(s, a, True)
        s.step(1)
        on_state = s.get_state()[0].copy()
        toggle(s, a, False)
        c, phi = (x.copy() for x in s.get_state()[:2])
        got = steps(s, 2)
    with a.handle() as s:
        a.upload(s, c, phi)
        never = steps(s, 2)
    with a.handle() as s:
        a.upload(s)
        s.step(1)
        assert not np.array_equal(s.get_state()[0], on_state), 'the switch changed nothing: the case does not test it'
    if switch != 'grid':
        assert_same(got, never, (family, switch))
    else:
        with a.handle() as s:
            a.upload(s, c, phi)
            toggle(s, a, False)
            assert_same(got, steps(s, 2), (family, switch))
        assert np.array_equal(got[7], never[7]) and np.array_equal(got[8], never[8])
        for x, y in zip(got[:7], never[:7]):
            assert np.abs(x - y).max() <= 1e-9 * np.abs(y).max()
    assert (got[7] == 0).all()
    if switch == 'wall_kinetics':
        anchor(a, [0, a.B - 1], never, 2, c.reshape(a.B, a.N, a.nx), phi)


# =========================================================================================================================================
# satellite libraries: one library object, a large case first, then a small one
# =========================================================================================================================================
# entry point -> the attributes of PnpSolver that hold the library objects it uses
SATELLITES = {
    'resample': ('_regridder',), 'equilibrium': ('_equilibrator',), 'get_electrolyte': ('_observer',), 'get_balance': ('_balancer',),
    'get_response': ('_responder',), 'get_kinetics': ('_kinetics',), 'get_rate_control': ('_rate_control', '_kinetics'),
    'get_coupling': ('_coupler', '_kinetics'), 'get_sensitivities': ('_sensitizer',), 'get_relaxation': ('_mode_solver',),
}
CHUNK_ENV = {'get_response': 'CATRESP_WORKSPACE_BYTES', 'get_relaxation': 'CATMODES_WORKSPACE_BYTES'}
_SAT = {}


def make_satellite_handle(nx, B):
    """tests/test_gpu_kinetics.py's handle (cation, anion and a neutral species at a Stern wall, |phiM| <= 0.12 V) at nx points, solved"""
    from tests.test_gpu_newton import BETA, EPS, F
    D, q, cb = np.array([1.957e-9, 1.185e-9, 1.9e-9]), np.array([F, -F, 0.0]), np.array([10.0, 10.0, 1.0])
    dx = np.sqrt(EPS / BETA / (q ** 2 * cb).sum()) / 6.0
    s = _capi.PnpSolver(3, nx, dx, 1.0, BETA, EPS, D, q, method='Newton', batch_capacity=B)
    s.set_newton(wall_bc='stern', stern_capacitance=0.2, phi_pzc=0.0)
    pb = np.zeros((B, 4))
    pb[:, 0] = np.linspace(-0.12, 0.06, B)
    s.set_batch(np.repeat(np.repeat(cb[None, :, None], nx, axis=2), B, axis=0), pb, np.zeros(B), np.zeros((B, 3)))
    assert (s.solve_stationary() == 0).all()
    return s


def satellite_handle(nx, B):
    """make_satellite_handle(nx, B), one per nx for the module"""
    if nx not in _SAT:
        _SAT[nx] = make_satellite_handle(nx, B)
    return _SAT[nx]


@pytest.fixture(scope='module')
def satellite_handles():
    yield satellite_handle
    for s in _SAT.values():
        s.close()
    _SAT.clear()


def satellite_call(name, s, lanes):
    """The entry point on the lanes `lanes` (None: all; the observables and the balance take the whole batch), as a flat dict"""
    from tests import kinetics_cases as KC
    model = KC.co2r_model('two_site')
    if name == 'resample':
        c, phi = s.resample(np.linspace(0.0, s.grid[-1], s.nx // 2 + 3), lanes=lanes)
        out = {'c': c, 'phi': phi}
    elif name == 'equilibrium':
        out = s.equilibrium(lanes=lanes)
    elif name == 'get_electrolyte':
        out = s.get_electrolyte()
    elif name == 'get_balance':
        out = s.get_balance()
    elif name == 'get_response':
        out = s.get_response(omega=(0.0, 1e5), lanes=lanes, profiles=True)
    elif name == 'get_kinetics':
        out = s.get_kinetics(model, lanes=lanes, fields=('theta', 'rate', 'flux', 'dflux_dc', 'dflux_dphi'))
    elif name == 'get_rate_control':
        out = s.get_rate_control(model, lanes=lanes)
    elif name == 'get_coupling':
        kin = s.get_kinetics(model, lanes=lanes, fields=('flux', 'dflux_dc', 'dflux_dphi'))
        out = s.get_coupling(None, kin, lanes=lanes)
    elif name == 'get_sensitivities':
        out = s.get_sensitivities(['phiM', ('flux', 0), ('c_bulk', 1), 'stern_capacitance'], lanes=lanes)
        out = dict(out, **{'elasticity_' + k: v for k, v in out['elasticity'].items()})
    else:
        out = s.get_relaxation(nmodes=2, subspace=4, iterations=3, lanes=lanes)
    return {k: np.asarray(v) for k, v in out.items() if isinstance(v, np.ndarray) and v.dtype.kind in 'fciu'}


@pytest.mark.parametrize('name,chunked', [(n, False) for n in SATELLITES] + [(n, True) for n in CHUNK_ENV])
def test_satellite_library_objects_carry_nothing_over(name, chunked, satellite_handles, monkeypatch):
    """Each of the ten device libraries through its PnpSolver entry point: the library object is called on a large case (1030 grid
    points, all 18 lanes), then on a small one (66 points, three lanes, not in order).  Its context keeps a device buffer, the uploaded
    tables and the kernel choice between calls; the small result equals, to the bit, that of a library object that only ever saw the
    small case.  For the response and the relaxation modes also with the record workspace capped at one wave (one byte), so that the
    large case walks its systems in chunks."""
    if chunked:
        monkeypatch.setenv(CHUNK_ENV[name], '1')
    big, small = satellite_handles(1030, 18), satellite_handles(66, 7)
    lanes = None if name in ('get_electrolyte', 'get_balance') else [5, 0, 3]
    attrs = SATELLITES[name]

    def drop(s):
        for a in attrs:
            if getattr(s, a, None) is not None:
                getattr(s, a).close()
            setattr(s, a, None)
    drop(big), drop(small)
    want = satellite_call(name, small, lanes)                 # library objects that only ever see the small case
    drop(small)
    large = satellite_call(name, big, None)
    for a in attrs:                                           # ... and the ones that saw the large case first
        setattr(small, a, getattr(big, a))
        setattr(big, a, None)
    got = satellite_call(name, small, lanes)
    assert sorted(got) == sorted(want) and len(want) >= 2
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k], equal_nan=want[k].dtype.kind in 'fc'), (name, k)
    for res in (large, want):                                 # (both cases were solved: the comparison is not one of NaN rows)
        if 'status' in res:
            assert (res['status'] == 0).all(), (name, res['status'])


def test_close_destroys_every_satellite_context():
    """Every entry point that opens a library object, once, on a handle of this test's own (66 points, seven lanes): the ten of
    satellite_call, then the transient, the kinetic admittance, the impedance and the steady state of an interacting model.  All thirteen
    attributes of PnpSolver.SATELLITES then hold a context; after close() every one is None and the context behind it is destroyed."""
    from tests import interact_cases as IC
    from tests import kinetics_cases as KC
    table = _capi.PnpSolver.SATELLITES
    assert {a for attrs in SATELLITES.values() for a in attrs} <= set(table)
    assert len(table) == 13
    lanes, model = [5, 0, 3], KC.co2r_model('two_site')
    s = make_satellite_handle(66, 7)
    try:
        for name in SATELLITES:
            assert len(satellite_call(name, s, None if name in ('get_electrolyte', 'get_balance') else lanes)) >= 2, name
        assert s.get_kinetics_transient(model, [1e-6, 1e-3], lanes=lanes)['flux'].shape == (3, 2, 3)
        assert s.get_kinetic_admittance(model, (0.0, 1e3), lanes=lanes)['Kc'].shape == (3, 2, 3, 3)
        assert s.get_impedance(model, (0.0, 1e3), lanes=lanes)['impedance'].shape == (3, 2)
        assert s.get_kinetics(IC.case('co2r_one_site_weak').tables, lanes=lanes)['ramp_reached'].shape == (3,)
        handles = {a: getattr(s, a) for a in table}
        assert all(h is not None and h._h.value for h in handles.values()), [a for a, h in handles.items() if h is None]
    finally:
        s.close()
    for a, h in handles.items():
        assert getattr(s, a) is None and not h._h.value, a
