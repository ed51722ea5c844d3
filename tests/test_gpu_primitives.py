"""The shared device primitives, one by one, on the device (tests/csrc/primitives_harness.hip through tests/primitives.py).

Scalar functions against multiprecision values at ulp level (the header comments' own accuracy claims), the DPP moves, scans, row and
window helpers bit for bit (including what the buffer resources do beyond their end: loads return 0, stores are dropped), and all 30
instances of tridiag_wave<P, G, DPP1> against multiprecision solutions up to the Crank-Nicolson limit |a| + |c| -> 1.  The helpers that
assert are those of tests/primitives.py; tests/test_primitives_ref.py shows without a GPU that each of them bites.  Every worst case is
printed as a line starting with 'primitives:'; profiles/primitives_unit.md records them."""
import numpy as np
import pytest

from tests import primitives as U

pytestmark = pytest.mark.gpu


def report(msg):
    print('primitives: ' + msg)


# ---- scalar functions -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rcp_ref():
    x = U.rcp_args()
    return x, U.ref_rcp(x)


@pytest.mark.parametrize('name, bar', [('fast_rcp', U.RCP1_BAR), ('fast_rcp2', U.RCP2_BAR), ('nrcp', U.RCP2_BAR)])
def test_reciprocals(name, bar, rcp_ref):
    x, ref = rcp_ref
    got = U.scalar(name, x)
    err = U.rel_error(got, ref)
    k = int(np.argmax(err))
    report('%s: worst relative error %.3e at x = %r (bar %.1e)' % (name, err[k], float(x[k]), bar))
    U.check_rel(got, ref, bar, x, what=name)


def test_fast_rcp2_and_nrcp_are_the_same_function(rcp_ref):
    x, _ = rcp_ref
    same = np.array_equal(U.scalar('fast_rcp2', x), U.scalar('nrcp', x))
    report('fast_rcp2 and nrcp bit-identical: %s' % same)
    assert same      # the same five instructions under two names


def test_expm1_sc():
    u = U.expm1_args()
    ref = U.ref_expm1(u)
    got = U.scalar('expm1_sc', u)
    err = U.ulp_error(got, ref)
    for lab, sel in (('|u| in [0.05, ln2/2)', np.abs(u) < 0.5 * np.log(2.0)), ('u >= ln2/2', u >= 0.5 * np.log(2.0)), ('u <= -ln2/2', u <= -0.5 * np.log(2.0))):
        k = np.nonzero(sel)[0][int(np.argmax(err[sel]))]
        report('expm1_sc, %s: worst %.3f ulp at u = %r' % (lab, err[k], float(u[k])))
    report('expm1_sc: worst %.3f ulp at u = %r (bar < %g)' % (U.check_ulp(got, ref, U.ULP_BAR, u, strict=True, what='expm1_sc') + (U.ULP_BAR,)))
    below, above = U.scalar('expm1_sc', U.EXPM1_BELOW), U.scalar('expm1_sc', U.EXPM1_ABOVE)
    assert np.array_equal(below, np.full(below.shape, -1.0)), below
    assert np.array_equal(above, np.full(above.shape, np.inf)), above


def test_log1p_sc():
    x = U.log1p_args()
    ref = U.ref_log1p(x)
    got = U.scalar('log1p_sc', x)
    err = U.ulp_error(got, ref)
    for lab, sel in (('x = -f', (x < 0) & (x >= -0.1)), ('x = -(1 - f)', x < -0.8), ('x = 1 - f', x > 0), ('1 + x around sqrt(1/2)', (x < -0.29) & (x > -0.3))):
        k = np.nonzero(sel)[0][int(np.argmax(err[sel]))]
        report('log1p_sc, %s: worst %.3f ulp at x = %r' % (lab, err[k], float(x[k])))
    report('log1p_sc: worst %.3f ulp at x = %r (bar < %g)' % (U.check_ulp(got, ref, U.ULP_BAR, x, strict=True, what='log1p_sc') + (U.ULP_BAR,)))
    zero = U.scalar('log1p_sc', np.zeros(1))
    assert zero[0] == 0.0


@pytest.fixture(scope='module')
def bern():
    u = U.bernoulli_args()
    ref_B, ref_dB = U.ref_bernoulli(u)
    return u, ref_B, ref_dB


def test_bernoulli_both_copies(bern):
    u, ref_B, ref_dB = bern
    post = U.scalar('bernoulli', u)
    lane, dB = U.edge_flux(u)
    for name, B in (('post::bernoulli', post), ('lane_edge_flux', lane)):
        report('B, %s: worst %.3f ulp at u = %r (bar %g)' % ((name,) + U.check_ulp(B, ref_B, U.B_ULP_BAR, u, what=name) + (U.B_ULP_BAR,)))
        sw = U.check_bernoulli_switch(u, B)
        for side in (0.05, -0.05):
            report('B, %s at u = %+.2f: series side %r, other side %r, %.3f ulp apart (bar %g)' % ((name, side) + sw[side] + (U.B_ULP_BAR,)))
        report('B, %s: detailed balance |B(-u) - (B(u) + u)| worst %.3f ulp at u = %r (bar %g)' % ((name,) + U.check_bernoulli_balance(u, B) + (U.B_ULP_BAR,)))
    assert post[u == 0.0][0] == 1.0 and lane[u == 0.0][0] == 1.0
    differ = np.nonzero(post != lane)[0]
    report('post::bernoulli and lane_edge_flux bit-identical: %s (%d of %d arguments differ%s)' % (
        differ.size == 0, differ.size, u.size, '' if differ.size == 0 else ', at most %.2f ulp' % (np.abs(post - lane) / np.spacing(np.abs(post)))[differ].max()))
    report('dB, lane_edge_flux: worst relative error %.3e at u = %r (bar %.0e)' % (U.check_rel(dB, ref_dB, U.DB_REL_BAR, u, what='dB') + (U.DB_REL_BAR,)))
    err = U.rel_error(dB, ref_dB)
    for side in (0.05, -0.05):
        near = np.abs(u - side) < 1e-13
        k = np.nonzero(near)[0][int(np.argmax(err[near]))]
        report('dB around u = %+.2f: worst relative error %.3e at u = %r' % (side, err[k], float(u[k])))


# ---- wave moves and scans: bit for bit ----------------------------------------------------------------------------------------------------
def test_lane_moves():
    v = np.arange(64) + 0.5
    prev, nxt = U.wave_moves(v, -7.0)
    assert prev[0, 0] == -7.0 and np.array_equal(prev[0, 1:], v[:-1]), prev
    assert nxt[0, 63] == -7.0 and np.array_equal(nxt[0, :-1], v[1:]), nxt
    for lo, hi in ((15, 16), (31, 32), (47, 48)):      # across the DPP rows and the two halves of the wave
        assert prev[0, hi] == v[lo] and nxt[0, lo] == v[hi]


def test_read_lane():
    v = np.random.default_rng(1).standard_normal(64)
    out = U.read_lane(v)
    assert np.array_equal(out, np.repeat(v[:, None], 64, axis=1))


@pytest.mark.parametrize('W', [2, 4])
def test_column_lane_exchanges(W):
    """pnp_lane_cols.h: lane = 2 W point + W direction + column lane; every lane feeds its id plus 0.25"""
    U.check_col_lanes(W, *U.col_lanes(W, U.lane_ids()))


@pytest.mark.parametrize('P', U.PS)
def test_pick_blocked(P):
    a = np.random.default_rng(P).standard_normal(64 * P)
    out = U.pick_blocked(P, a)
    assert np.array_equal(out, np.repeat(a[:, None], 64, axis=1))


@pytest.mark.parametrize('bc', [False, True], ids=['wave_scan_incl', 'wave_scan_incl_bc'])
def test_wave_scan(bc):
    U.check_scan_onehot(U.wave_scan(np.eye(64), bc))
    v = np.random.default_rng(3).integers(0, 1 << 20, (16, 64)).astype(float)
    assert np.array_equal(U.wave_scan(v, bc), np.cumsum(v, axis=1))


def test_the_two_wave_scans_are_bit_identical():
    rng = np.random.default_rng(4)
    v = rng.standard_normal((64, 64)) * 10.0 ** rng.integers(-6, 7, (64, 64))
    assert np.array_equal(U.wave_scan(v, False), U.wave_scan(v, True))


def scan_inputs(P):
    rng = np.random.default_rng(100 + P)
    ints = rng.integers(0, 1 << 20, (8, 64 * P)).astype(float)
    x = rng.uniform(-1.0, 1.0, (8, 64 * P)) * 10.0 ** rng.integers(-3, 4, (8, 64 * P))
    return ints, x


@pytest.mark.parametrize('rev', [False, True], ids=['forward', 'reverse'])
@pytest.mark.parametrize('P', U.PS)
def test_blocked_scan(P, rev):
    eye = np.eye(64 * P)
    xo, total, base = U.blocked_scan(P, rev, eye)
    U.check_scan_onehot(xo, rev)
    U.check_blocked_scan(eye, xo, total, base, P, rev)
    ints, x = scan_inputs(P)
    U.check_blocked_scan(ints, *U.blocked_scan(P, rev, ints), P, rev)
    ratio = U.check_scan_bound(x, U.blocked_scan(P, rev, x)[0], U.ref_prefix(x, rev), P)
    report('blocked_scan<%d, %s>: random doubles, worst error %.3f of (P + 6) 2^-53 sum|x|' % (P, str(rev).lower(), ratio))


@pytest.mark.parametrize('P', U.PS)
def test_blocked_scan_sum(P):
    rng = np.random.default_rng(200 + P)
    eye = np.eye(64 * P)
    w1 = rng.integers(0, 1 << 20, (64 * P, 64)).astype(float)
    xo, total, base, wtotal = U.blocked_scan_sum(P, eye, w1)
    U.check_scan_onehot(xo)
    U.check_blocked_scan(eye, xo, total, base, P)
    assert np.array_equal(wtotal, np.repeat(w1.sum(axis=1)[:, None], 64, axis=1))
    ints, x = scan_inputs(P)
    w = rng.integers(0, 1 << 20, (8, 64)).astype(float)
    xo, total, base, wtotal = U.blocked_scan_sum(P, ints, w)
    U.check_blocked_scan(ints, xo, total, base, P)
    assert np.array_equal(wtotal, np.repeat(w.sum(axis=1)[:, None], 64, axis=1))
    # one-hot w: every lane's contribution reaches the wave's sum once
    xo, total, base, wtotal = U.blocked_scan_sum(P, np.zeros((64, 64 * P)), np.eye(64))
    assert np.array_equal(wtotal, np.ones((64, 64))) and not xo.any()
    wr = rng.standard_normal((8, 64))
    xo, total, base, wtotal = U.blocked_scan_sum(P, x, wr)
    ratio = U.check_scan_bound(x, xo, U.ref_prefix(x), P)
    wsum = np.array([float(sum(U.mpf(float(t)) for t in row)) for row in wr])
    assert (np.abs(wtotal - wsum[:, None]) <= 7 * 2.0 ** -53 * np.abs(wr).sum(axis=1)[:, None]).all()
    report('blocked_scan_sum<%d>: random doubles, worst error %.3f of (P + 6) 2^-53 sum|x|' % (P, ratio))


# ---- rows and windows: bit for bit ------------------------------------------------------------------------------------------------------
def row_pitches(P):
    return list(range(16, 64 * P + 17, 16)) + [3, 5, 17, 64 * P + 1, 64 * P + 2, 64 * P + 3]


@pytest.mark.parametrize('P', U.PS)
def test_load_row_reads_zero_beyond_the_pitch(P):
    n = U.row_alloc(P)
    assert n == 128 * (P // 2 + 1) and n >= 64 * P + 16
    for ldx in row_pitches(P):
        src = np.concatenate([U.distinct(ldx), U.canaries(n + 16 - ldx)])      # canaries from ldx to beyond the last byte a lane can address
        U.check_load(U.load_row(P, src, ldx), src, ldx)


@pytest.mark.parametrize('aux', [0, 2])
@pytest.mark.parametrize('P', U.PS)
def test_store_row_drops_what_lies_beyond_the_pitch(P, aux):
    n = U.row_alloc(P)
    vals = U.distinct(n)
    for ldx in row_pitches(P):
        before = U.canaries(n + 16)
        U.check_store(U.store_row(P, aux, vals, before, ldx), before, vals, ldx)


# (nx, P): the shapes of pnp::post::choose_shape; load_window and store_rows exist for even P only
GRIDS = [(5, 1), (66, 1), (67, 2), (130, 2), (131, 4), (1026, 16)]


@pytest.mark.parametrize('nx, P', GRIDS)
def test_window_loads_read_zero_beyond_the_resource(nx, P):
    n = U.win_alloc(P)
    assert n == 64 * P + 2 and nx <= n
    for which in U.LOAD_WINDOW:
        if P == 1 and which != 'post::load_win<P>':
            continue
        for nrec in (nx, nx - 1):
            row = np.concatenate([U.distinct(nrec), U.canaries(n + 8 - nrec)])
            U.check_window_load(U.load_window(P, which, row, nrec), row, nrec, P)


@pytest.mark.parametrize('nx, P', GRIDS)
def test_window_stores_drop_what_lies_beyond_the_resource(nx, P):
    n = U.win_alloc(P)
    v = U.distinct(64 * (P + 2)).reshape(64, P + 2)
    for mode in U.STORE_WINDOW:
        if P == 1 and mode == 'store_rows<P>':
            continue
        for nrec in (nx, nx - 1):
            before = U.canaries(n + 8)
            U.check_window_store(U.store_window(P, mode, v, before, nrec), before, v, nrec, P, mode)


# ---- tridiag_wave<P, G, DPP1> -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', U.PS)
def test_tridiag_wave(P):
    """All six instances of one P: forward error of every real row of every system, padded rows are don't-care, DPP1 equals the LDS path,
    no mixing between the systems of a call."""
    ms = U.row_counts(P)
    groups = [[U.system(P, m, cls, g) for g in range(3)] for m in ms for cls in U.CLASSES]       # the systems of one G-wide call
    worst, alone = {}, {}
    identical_alone = True
    for G in (1, 2, 3):
        # G = 1: every system on its own; G > 1: systems 0 .. G-1 of each group together
        calls = [[s] for grp in groups for s in grp] if G == 1 else [grp[:G] for grp in groups]
        a, c, d = (np.array([[getattr(s, n) for s in call] for call in calls]) for n in 'acd')
        a2, c2, d2 = (np.array([[getattr(s, n) for s in call] for call in calls]) for n in ('a2', 'c2', 'd2'))
        x = {dpp: U.tridiag(P, G, dpp, a, c, d) for dpp in (False, True)}
        x2 = {dpp: U.tridiag(P, G, dpp, a2, c2, d2) for dpp in (False, True)}
        # 3. DPP1 equals the LDS path, padded rows included
        assert np.array_equal(x[False], x[True]) and np.array_equal(x2[False], x2[True]), 'tridiag_wave<%d, %d>: DPP1 differs from the LDS path' % (P, G)
        for dpp in (False, True):
            assert np.isfinite(x[dpp]).all() and np.isfinite(x2[dpp]).all()
            for k, call in enumerate(calls):
                for g, s in enumerate(call):
                    # 1. forward error
                    ratio = U.check_tridiag(s.a, s.c, s.d, x[dpp][k, g], P, s.m, s.x_ref, s.bar)
                    key = (G, dpp, s.cls)
                    worst[key] = max(worst.get(key, 0.0), ratio)
                    # 2. padded rows are don't-care
                    assert np.array_equal(x[dpp][k, g, :s.m], x2[dpp][k, g, :s.m]), 'tridiag_wave<%d, %d, %s>: m = %d, %s: the padded rows reach the real ones' % (P, G, dpp, s.m, s.cls)
                    # 4. no mixing between systems
                    if G == 1:
                        alone[(s.m, s.cls, s.g, dpp)] = x[dpp][k, 0]
                    else:
                        one = alone[(s.m, s.cls, s.g, dpp)]
                        apart = np.abs(one[:s.m] - x[dpp][k, g, :s.m]).max() / np.abs(s.x_ref).max()
                        assert apart <= s.bar, 'tridiag_wave<%d, %d, %s>: m = %d, %s: system %d is %.3e from itself solved alone (bar %.3e)' % (P, G, dpp, s.m, s.cls, g, apart, s.bar)
                        identical_alone &= np.array_equal(one[:s.m], x[dpp][k, g, :s.m])
    for G in (1, 2, 3):
        for dpp in (False, True):
            report('tridiag_wave<%d, %d, %s>: worst forward error / (kappa_inf (P + 6) 2.2e-15): %s' % (
                P, G, str(dpp).lower(), ', '.join('%s %.4f' % (cls, worst[(G, dpp, cls)]) for cls in U.CLASSES)))
    report('tridiag_wave<%d>: system g of a G-wide call bit-identical to the same system alone: %s; DPP1 bit-identical to the LDS path: True' % (P, identical_alone))


# ---- the damped Newton update (pnp_math.h): decisions exactly, values in ulp of the twin evaluated in multiprecision ---------------------------------
# (bars: U.RULE_BARS, twice the worst error measured on the MI355X: profiles/primitives_unit.md)
@pytest.mark.parametrize('N', U.RULE_NS)
def test_newton_rule(N):
    rows = U.newton_rule_rows(N)
    fp, exact = U.newton_rule_twin(rows), U.newton_rule_twin(rows, exact=True)
    got = U.newton_rule(N, rows)
    free = {k: np.inf for k in U.RULE_VALUES}
    worst = U.check_newton_rule(got, fp, exact, free, rows['kind'])          # the decisions; the figures before anything is held to them
    report('newton rule, N = %d: worst ulp %s; %d rows, floor in %d, backtrack in %d (1e-12 floor of the free volume in %d), damped %d' % (
        N, ', '.join('%s %.3f' % (k, worst[k]) for k in U.RULE_VALUES), len(rows['lam']), got['floor'].any(axis=1).sum(), got['back'].sum(),
        exact['free_min'].sum(), got['damped'].sum()))
    same = all(np.array_equal(got[k], fp[k], equal_nan=True) for k in U.RULE_VALUES)
    report('newton rule, N = %d: bit-identical to the fp64 twin with the header\'s multiply-adds: %s' % (N, same))
    bad = ~np.isfinite(rows['du']).all(axis=1) | ~np.isfinite(rows['dphi'])
    assert bad.sum() >= 6 and all(np.array_equal(got[k][bad], fp[k][bad], equal_nan=True) for k in U.RULE_VALUES)
    U.check_newton_rule(got, fp, exact, U.RULE_BARS, rows['kind'])


def test_newton_accept():
    t, what = U.newton_accept_tuples()
    acc, prev = U.newton_accept(t)
    report('newton_accept: %d tuples, %d accepted' % (len(what), acc.sum()))
    U.check_newton_accept(acc, prev, t, what)


# ---- the per-lane LU of pnp_kin.h (factor, substitute): every stored word against the fp64 replay of the same operation order ---------
@pytest.mark.parametrize('T', U.LU_TS)
def test_lu_factor_and_substitute_bit_for_bit(T):
    """One launch, one wave, 64 systems (U.lu_cases: the site row with 5e-8 on the diagonal, the tie, the dead row, the singular and the
    infinite matrix, 59 random ones), two right-hand sides each.  No contraction in the header's functions, divisions and multiply-subtracts
    single IEEE operations: the factors, the packed pivot rows, the bad-pivot flags and the solutions equal the replay's bit for bit."""
    A, b, want = U.lu_cases(T)
    got = U.lu(T, A, b)
    ref = U.emul_lu(A, b)
    diff = sum(int((np.ascontiguousarray(g).view(np.uint64) != np.ascontiguousarray(r).view(np.uint64)).sum()) for g, r in zip(got, ref))
    report('lu, T = %d: %d of %d words differ from the replay; flags set in lanes %s; pivot row of step 0 in the site-row lane %d, in the tie lane %d' % (
        T, diff, 64 * (T * T + 2 + 2 * T), np.nonzero(got[2])[0].tolist(), int(got[1][0]) & 15, int(got[1][1]) & 15))
    assert U.check_lu(got, ref) == 64 * (T * T + 2 + 2 * T)
    assert np.nonzero(got[2])[0].tolist() == [3, 4]
    assert (int(got[1][0]) & 15) == want['exchange'] and (int(got[1][1]) & 15) == want['tie rows'][0]
