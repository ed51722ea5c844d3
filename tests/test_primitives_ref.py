"""The unit tests of the shared device primitives, without a GPU (tests/test_gpu_primitives.py is the device half).

The harness library builds for gfx950, exports exactly its catunit_* entry points and holds only catunit:: kernels.  The multiprecision
references of tests/primitives.py are checked against identities they must satisfy, and oracle/pnp_physical.py's bernoulli is held to
the bars of the device functions over the same arguments (it had never been checked at its own SERIES_U switch).  Every assertion
helper the GPU tests use is shown to bite: a plain fp64 NumPy emulation of the operation passes it and each mutant fails it --
reciprocals of seed accuracy (4.6e-8) in the Thomas solve, a prefix scan with one of its six stages skipped or with the row_bcast:31
stage written into rows 1, 3, the 1/30240 coefficient of B replaced by 1/30000, a system whose c[m-1] is not zeroed, a store (and a
load) whose range check ends one double late; for the damped Newton update (pnp_math.h) a twin with each branch of the rule taken out,
moved or taken always."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pnp_physical as PH
from tests import kernel_census as K
from tests import primitives as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fails(f, *a, **kw):
    try:
        f(*a, **kw)
    except AssertionError:
        return True
    return False


# ---- the library ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_unittest_library
    return build_unittest_library()


def test_the_harness_builds_for_gfx950(libpath):
    from catint_amd import build
    assert libpath == build.UNITTEST_LIB and os.path.exists(libpath) and not build.unittest_needs_build()
    assert '--offload-arch=gfx950' in build.FLAGS
    assert build.UNITTEST_SOURCES == ['primitives_harness.hip'] and os.path.isdir(build.UNITTEST_DIR)
    assert os.path.realpath(build.UNITTEST_DIR) == os.path.join(ROOT, 'tests', 'csrc')
    assert 'build_unittest_library(' in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    # test infrastructure: no source of a product library, and no module of the package loads it
    assert not any('harness' in s or 'unittest' in s for s in build.SOURCES + build.OBSERVE_SOURCES + build.BALANCE_SOURCES + build.REGRID_SOURCES + build.EQUIL_SOURCES)
    pkg = os.path.join(ROOT, 'catint_amd')
    for f in os.listdir(pkg):
        if f.endswith('.py') and f != 'build.py':
            assert 'unittest' not in open(os.path.join(pkg, f)).read(), f


def test_the_harness_includes_only_the_shared_headers():
    src = open(os.path.join(ROOT, 'tests', 'csrc', 'primitives_harness.hip')).read()
    quoted = sorted(os.path.basename(n) for n in re.findall(r'^\s*#\s*include\s+"([^"]+)"', src, flags=re.M))
    assert quoted == ['pnp_kin.h', 'pnp_lane_cols.h', 'pnp_lane_common.h', 'pnp_math.h', 'pnp_post.h', 'pnp_wave.h']


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    src = open(os.path.join(ROOT, 'tests', 'csrc', 'primitives_harness.hip')).read()
    declared = sorted(set(re.findall(r'\bint\s+(catunit_[a-z0-9_]+)\s*\(', src)))
    assert declared == sorted(U.SYMBOLS) and len(declared) == 19
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(catunit_[a-z0-9_]+)\b', exported))) == declared


def test_every_kernel_is_in_namespace_catunit_and_every_tridiag_instance_is_there(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert compiled and all(n.startswith('catunit::') for n in compiled), sorted(n for n in compiled if not n.startswith('catunit::'))
    tri = {'catunit::tridiag_kernel<%d, %d, %s>' % (P, G, d) for P in U.PS for G in (1, 2, 3) for d in ('false', 'true')}
    assert len(tri) == 30 and tri <= compiled, sorted(tri - compiled)
    for fam, count in (('scalar_kernel', 6), ('newton_rule_kernel', 4), ('newton_accept_kernel', 1), ('col_lanes_kernel', 2), ('pick_blocked_kernel', 5), ('wave_scan_kernel', 2), ('blocked_scan_kernel', 10),
                       ('blocked_scan_sum_kernel', 5), ('load_row_kernel', 5), ('store_row_kernel', 10), ('load_window_kernel', 13),
                       ('store_window_kernel', 14), ('lu_kernel', 1)):
        assert sum(K.family(n) == 'catunit::' + fam for n in compiled) == count, fam


def test_the_product_libraries_gained_no_kernel():
    from catint_amd import build
    for f in (build.build_library, build.build_observe_library, build.build_balance_library, build.build_regrid_library, build.build_equil_library):
        f()
    try:
        compiled = set()
        for lib in (build.LIB, build.OBSERVE_LIB, build.BALANCE_LIB, build.REGRID_LIB, build.EQUIL_LIB):
            compiled |= K.compiled_kernels(lib=lib)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert not [n for n in compiled if 'catunit' in n]


def test_invalid_arguments_are_refused_before_any_device_call(libpath):
    """hipErrorInvalidValue (1) for what would break a launch rule: a P that is no shape, a buffer smaller than the largest offset a lane
    can form, a resource longer than its allocation.  (This machine may have no device at all.)"""
    lib = U.load_library()
    d = np.zeros(8)
    p = U._p(d)
    assert lib.catunit_row_alloc(3) == -1 and lib.catunit_win_alloc(0) == -1
    assert [lib.catunit_row_alloc(P) for P in U.PS] == [128 * (P // 2 + 1) for P in U.PS]
    assert [lib.catunit_win_alloc(P) for P in U.PS] == [64 * P + 2 for P in U.PS]
    assert lib.catunit_load_row(2, p, 8, 3, p) == 1               # allocation below row_alloc
    assert lib.catunit_store_row(2, 1, p, p, 256, 3) == 1         # aux
    assert lib.catunit_load_window(2, 0, p, 8, 3, p) == 1
    assert lib.catunit_load_window(1, 0, p, 66, 3, p) == 1        # load_window needs an even P
    assert lib.catunit_store_window(1, 0, p, p, 66, 3) == 1
    assert lib.catunit_store_window(2, 1, p, p, 8, 3) == 1
    assert lib.catunit_tridiag(3, 1, 0, p, p, p, p, 1) == 1 and lib.catunit_tridiag(2, 4, 0, p, p, p, p, 1) == 1
    assert lib.catunit_scalar(6, p, p, 8) == 1 and lib.catunit_scalar(0, p, p, 0) == 0
    assert lib.catunit_col_lanes(3, p, p, p, p) == 1 and lib.catunit_col_lanes(8, p, p, p, p) == 1
    assert lib.catunit_pick_blocked(5, p, p) == 1 and lib.catunit_blocked_scan(3, 0, p, p, p, p, 1) == 1
    assert lib.catunit_newton_rule(3, 1, *([p] * 11)) == 1 and lib.catunit_newton_rule(2, 0, *([p] * 11)) == 1      # N is 1, 2, 7 or 8
    assert lib.catunit_newton_accept(0, *([p] * 7)) == 1
    assert lib.catunit_lu(0, *([p] * 5)) == 1 and lib.catunit_lu(10, *([p] * 5)) == 1                                # T is 1 .. 9


# ---- the references --------------------------------------------------------------------------------------------------------------------
def test_argument_sets_hold_what_the_design_asks_for():
    for args in (U.rcp_args(), U.expm1_args(), U.log1p_args(), U.bernoulli_args()):
        assert args.size <= 1 << 16 and np.isfinite(args).all()
    r = U.rcp_args()
    assert r.min() == -1e150 and r.max() == 1e150 and np.abs(r).min() == 1e-150 and ((r >= 0.5) & (r <= 2.0)).sum() >= 4096
    e = U.expm1_args()
    assert np.abs(e).min() == 0.05 and e.max() == 709.0 and e.min() == -709.0 and {0.05, -0.05, -60.0, 709.0} <= set(e)
    assert np.nextafter(-60.0, 0.0) in e and np.nextafter(-60.0, -np.inf) in e
    for k in range(-4, 5):
        t = (k + 0.5) * math.log(2.0)
        assert ((e > t - 1e-12) & (e < t + 1e-12)).sum() >= 513
    assert (U.EXPM1_BELOW < -60.0).all() and (U.EXPM1_ABOVE > 709.0).all()
    lg = U.log1p_args()
    assert 0.0 in lg and lg.min() > -1.0 and -1e-18 in lg and (np.abs(lg + (1.0 - math.sqrt(0.5))) < 1e-13).sum() == 513
    b = U.bernoulli_args()
    assert 0.0 in b and np.abs(b).max() == 700.0 and np.abs(b[b != 0]).min() == 1e-12
    for s in (1.0, -1.0):
        assert s * 0.05 in b and np.nextafter(s * 0.05, 0.0) in b
        assert (np.abs(b - s * 0.05) < 1e-13).sum() == 4097
        assert (np.abs(b[np.abs(b - s * 0.05) < 1e-13]) < 0.05).sum() == 2048


def test_references_satisfy_their_identities():
    x = np.array([3.0, -7.0, 1e-150, 0.7, 1e150])
    hi, lo = U.ref_rcp(x)
    assert np.array_equal(hi, 1.0 / x) and (np.abs(lo) <= 0.5 * np.spacing(np.abs(hi))).all()      # IEEE division is correctly rounded
    u = np.array([0.05, -0.05, 1.0, -60.0, 709.0, 1e-3])
    hi, lo = U.ref_expm1(u)
    assert (U.ulp_error(np.expm1(u), (hi, lo)) < 1.0).all() and hi[3] == -1.0 and 0 < lo[3] < 1e-26
    hi, lo = U.ref_log1p(np.array([-1e-18, -0.5, 0.0, -(1.0 - 2.0 ** -53)]))
    assert hi[0] == -1e-18 and hi[1] == math.log(0.5) and hi[2] == 0.0 and hi[3] == -53 * math.log(2.0)
    (B, _), dB = U.ref_bernoulli(np.array([0.0, 1e-12, -1e-12, 30.0, -30.0]))
    assert B[0] == 1.0 and dB[0] == -0.5 and B[1] == 1.0 - 5e-13 and B[3] + 30.0 == B[4] and abs(dB[1] + 0.5) < 1e-12 and abs(dB[4] + 1.0) < 1e-11
    rng = np.random.default_rng(5)
    v = rng.uniform(-1, 1, (2, 128)) * 10.0 ** rng.integers(-8, 8, (2, 128))
    p = U.ref_prefix(v)
    assert all(p[i, j] == math.fsum(v[i, :j + 1]) for i in range(2) for j in range(128))
    assert np.array_equal(U.ref_prefix(v, rev=True)[:, ::-1], U.ref_prefix(v[:, ::-1]))
    s = U.system(2, 65, 'cn r=1e2', 1)
    T = U.dense(s.a, s.c, s.m)
    assert np.abs(T @ s.x_ref - s.d[:s.m]).max() <= 4 * 2.0 ** -53 * (np.abs(T) @ np.abs(s.x_ref)).max()
    assert s.c[s.m - 1] == 0.0 and s.a[0] == 0.0 and s.a[s.m] != 0.0


# ---- the oracle's Bernoulli function at the bars of the device functions -------------------------------------------------------------------
@pytest.fixture(scope='module')
def bern():
    u = U.bernoulli_args()
    ref_B, ref_dB = U.ref_bernoulli(u)
    return u, ref_B, ref_dB


def test_the_oracle_s_bernoulli_meets_the_device_bars(bern):
    u, ref_B, ref_dB = bern
    assert PH.SERIES_U == U.SERIES_U
    B, dB = PH.bernoulli(u)
    print('oracle B: %.2f ulp at u = %r' % U.check_ulp(B, ref_B, U.B_ULP_BAR, u, what='oracle B'))
    print('oracle dB: %.2e relative at u = %r' % U.check_rel(dB, ref_dB, U.DB_REL_BAR, u, what='oracle dB'))
    print('oracle B at the switch: %r' % U.check_bernoulli_switch(u, B))
    print('oracle balance: %.2f ulp at u = %r' % U.check_bernoulli_balance(u, B))


# ---- the helpers bite ----------------------------------------------------------------------------------------------------------------------
def test_scalar_helpers_pass_fp64_and_fail_seed_accuracy():
    x = U.rcp_args()[::7]
    ref = U.ref_rcp(x)
    U.check_rel(1.0 / x, ref, U.RCP2_BAR)
    seed = (1.0 / x) * (1.0 + U.SEED_REL)
    assert fails(U.check_rel, seed, ref, U.RCP1_BAR) and fails(U.check_rel, seed, ref, U.RCP2_BAR)
    one_step = (1.0 / x) * (1.0 + 2.2e-15)                       # the documented error of fast_rcp misses the bar of fast_rcp2
    U.check_rel(one_step, ref, U.RCP1_BAR)
    assert fails(U.check_rel, one_step, ref, U.RCP2_BAR)
    u = U.expm1_args()[::5]
    ref = U.ref_expm1(u)
    U.check_ulp(np.expm1(u), ref, U.ULP_BAR, u, strict=True)
    assert fails(U.check_ulp, np.expm1(u) * (1.0 + 5 * 2.0 ** -52), ref, U.ULP_BAR, u, strict=True)
    assert fails(U.check_ulp, np.exp(u) - 1.0, ref, U.ULP_BAR, u, strict=True)             # the cancellation expm1 exists to avoid
    assert fails(U.check_ulp, np.where(u == 709.0, np.inf, np.expm1(u)), ref, U.ULP_BAR, u, strict=True)
    assert fails(U.check_ulp, np.where(u == u[3], np.nan, np.expm1(u)), ref, U.ULP_BAR, u, strict=True)             # a NaN is no pass
    xl = U.log1p_args()[::5]
    refl = U.ref_log1p(xl)
    U.check_ulp(np.log1p(xl), refl, U.ULP_BAR, xl, strict=True)
    assert fails(U.check_ulp, np.log(1.0 + xl), refl, U.ULP_BAR, xl, strict=True)


def test_bernoulli_helpers_pass_the_emulation_and_fail_the_coefficient_mutant(bern):
    u, ref_B, ref_dB = bern
    B, dB = U.emul_bernoulli(u)
    U.check_ulp(B, ref_B, U.B_ULP_BAR, u)
    U.check_rel(dB, ref_dB, U.DB_REL_BAR, u)
    U.check_bernoulli_switch(u, B)
    U.check_bernoulli_balance(u, B)
    Bm, _ = U.emul_bernoulli(u, k30240=1.0 / 30000.0)
    assert fails(U.check_ulp, Bm, ref_B, U.B_ULP_BAR, u)
    assert fails(U.check_bernoulli_switch, u, Bm)
    # a B that breaks detailed balance by 1e-15 relative on one side only, and a dB with a wrong u^5 coefficient
    assert fails(U.check_bernoulli_balance, u, np.where(u < 0, B * (1.0 + 2e-15), B))
    us = np.where(np.abs(u) < U.SERIES_U, u, 0.0)
    assert fails(U.check_rel, dB + us ** 5 * (1.0 / 5000.0 - 1.0 / 5040.0), ref_dB, U.DB_REL_BAR, u)


@pytest.mark.parametrize('W', [2, 4])
def test_column_lane_helper_passes_the_emulation_and_fails_the_mutants(W):
    U.check_col_lanes(W, *U.emul_col_lanes(W, U.lane_ids()))
    for mutant in U.COL_LANE_MUTANTS:
        if W == 4 and mutant == U.COL_LANE_MUTANTS[0]:
            continue          # (the quad's own control)
        assert fails(U.check_col_lanes, W, *U.emul_col_lanes(W, U.lane_ids(), mutant)), mutant
    # the other width's map is not this one's
    assert fails(U.check_col_lanes, W, *(t[:W] if t.ndim == 2 else t for t in U.emul_col_lanes(6 - W, U.lane_ids())))


def test_wave_scan_helper_identifies_every_stage_and_row_mask():
    eye = np.eye(64)
    U.check_scan_onehot(U.emul_wave_scan(eye))
    for k in range(6):
        assert fails(U.check_scan_onehot, U.emul_wave_scan(eye, skip=k)), U.SCAN_STAGES[k]
    assert fails(U.check_scan_onehot, U.emul_wave_scan(eye, bcast31_rows=(1, 3)))
    v = np.random.default_rng(3).integers(0, 1 << 20, (8, 64)).astype(float)
    assert np.array_equal(U.emul_wave_scan(v), np.cumsum(v, axis=1))
    assert not np.array_equal(U.emul_wave_scan(v, bcast31_rows=(1, 3)), np.cumsum(v, axis=1))


@pytest.mark.parametrize('rev', [False, True])
@pytest.mark.parametrize('P', U.PS)
def test_blocked_scan_helpers_pass_the_emulation_and_fail_a_skipped_stage(P, rev):
    rng = np.random.default_rng([P, rev])
    eye = np.eye(64 * P)
    xo, total, base = U.emul_blocked_scan(eye, P, rev)
    U.check_scan_onehot(xo, rev)
    U.check_blocked_scan(eye, xo, total, base, P, rev)
    ints = rng.integers(0, 1 << 20, (4, 64 * P)).astype(float)
    U.check_blocked_scan(ints, *U.emul_blocked_scan(ints, P, rev), P, rev)
    x = rng.uniform(-1.0, 1.0, (4, 64 * P)) * 10.0 ** rng.integers(-3, 4, (4, 64 * P))
    ref = U.ref_prefix(x, rev)
    assert U.check_scan_bound(x, U.emul_blocked_scan(x, P, rev)[0], ref, P) <= 1.0
    for k in range(6):
        assert fails(U.check_scan_onehot, U.emul_blocked_scan(eye, P, rev, skip=k)[0], rev)
        assert fails(U.check_blocked_scan, ints, *U.emul_blocked_scan(ints, P, rev, skip=k), P, rev)
        assert fails(U.check_scan_bound, x, U.emul_blocked_scan(x, P, rev, skip=k)[0], ref, P)
    # a base that is not zero in the first (rev: last) lane, a total that is not the same in every lane
    xo, total, base = U.emul_blocked_scan(ints, P, rev)
    b2 = base.copy()
    b2[0, 63 if rev else 0] = 1.0
    t2 = total.copy()
    t2[1, 17] += 1.0
    assert fails(U.check_blocked_scan, ints, xo, total, b2, P, rev) and fails(U.check_blocked_scan, ints, xo, t2, base, P, rev)


@pytest.mark.parametrize('P', U.PS)
def test_tridiag_helper_passes_fp64_thomas_on_every_system_and_fails_the_mutants(P):
    worst = {}
    for m in U.row_counts(P):
        ss = [s for s in U.systems(P) if s.m == m]
        a, c, d = (np.array([getattr(s, n) for s in ss]) for n in 'acd')
        plain = U.emul_tridiag(a, c, d)
        seed = U.emul_tridiag(a, c, d, rcp_rel=U.SEED_REL)
        other = U.emul_tridiag(np.array([s.a2 for s in ss]), np.array([s.c2 for s in ss]), np.array([s.d2 for s in ss]))
        for k, s in enumerate(ss):
            ratio = U.check_tridiag(s.a, s.c, s.d, plain[k], P, m, s.x_ref, s.bar)
            worst[s.cls] = max(worst.get(s.cls, 0.0), ratio)
            if s.cls in U.CN_CLASSES:
                assert fails(U.check_tridiag, s.a, s.c, s.d, seed[k], P, m, s.x_ref, s.bar), (m, s.cls, s.g)
            # the second filling of the padded rows: the same real rows to the last bit
            assert np.array_equal(other[k][:m], plain[k][:m])
            assert np.isfinite(plain[k]).all() and np.isfinite(other[k]).all()
        if m < 64 * P:              # c[m-1] not zeroed: the padding reaches the real rows
            c_bad = c.copy()
            c_bad[:, m - 1] = -0.25
            bad = U.emul_tridiag(a, c_bad, d)
            for k, s in enumerate(ss):
                assert fails(U.check_tridiag, s.a, s.c, s.d, bad[k], P, m, s.x_ref, s.bar), (m, s.cls, s.g)
    # the bar computed inside the helper is the cached one
    s = U.system(P, U.row_counts(P)[2], 'cn r=1e4 alt', 2)
    assert U.check_tridiag(s.a, s.c, s.d, U.emul_tridiag(s.a, s.c, s.d), P, s.m) <= 1.0
    print('P = %d: fp64 Thomas, worst error / bar per class: %s' % (P, {k: round(v, 4) for k, v in worst.items()}))


def test_the_systems_of_a_call_differ_and_cover_the_classes():
    for P in U.PS:
        ss = U.systems(P)
        assert len(ss) == 63
        for s in ss:
            lim = 0.5 if s.cls == 'dominant' else 1.0
            assert (np.abs(s.a) + np.abs(s.c) <= lim).all() and np.isfinite(s.bar)
        for m in U.row_counts(P):
            for cls in U.CLASSES:
                g = [U.system(P, m, cls, k) for k in range(3)]
                assert not np.array_equal(g[0].a, g[1].a) and not np.array_equal(g[1].d, g[2].d) and not np.array_equal(g[0].d, g[2].d)
    s = U.system(16, 1024, 'cn r=1e4', 0)
    assert 0.9998 < (np.abs(s.a) + np.abs(s.c))[1:-1].min() and (s.d > 0).all()
    s = U.system(16, 1023, 'cn r=1e4 alt', 0)
    assert (s.d[::2] > 0).all() and (s.d[1::2] < 0).all()


@pytest.mark.parametrize('P', U.PS)
def test_row_and_window_helpers_fail_a_range_check_that_ends_one_double_late(P):
    n = 128 * (P // 2 + 1)
    for ldx in (3, 5, 17, 64 * P + 1, 64 * P + 16):
        src = np.concatenate([U.distinct(ldx), U.canaries(n + 8 - ldx)])
        U.check_load(U.emul_load(src, ldx, n), src, ldx)
        assert fails(U.check_load, U.emul_load(src, ldx, n, overrun=1), src, ldx)
        before, vals = U.canaries(n + 8), U.distinct(n)
        U.check_store(U.emul_store(before, vals, ldx), before, vals, ldx)
        assert fails(U.check_store, U.emul_store(before, vals, ldx, overrun=1), before, vals, ldx)
    na = 64 * P + 2
    for nrec in (5, 64 * P + 1, 64 * P + 2):
        row = np.concatenate([U.distinct(nrec), U.canaries(na - nrec)])
        U.check_window_load(U.emul_window_load(row, nrec, P), row, nrec, P)
        if nrec < na:
            assert fails(U.check_window_load, U.emul_window_load(row, nrec, P, overrun=1), row, nrec, P)
        v = U.distinct(64 * (P + 2)).reshape(64, P + 2)
        for mode in U.STORE_WINDOW:
            before = U.canaries(na)
            good = U.window_store_expected(before, v, nrec, P, mode)
            U.check_window_store(good, before, v, nrec, P, mode)
            late = U.window_store_expected(before, v, nrec + 1, P, mode)
            if not np.array_equal(late, good):
                assert fails(U.check_window_store, late, before, v, nrec, P, mode)
            assert fails(U.check_window_store, before, before, v, nrec, P, mode)      # nothing stored at all


# ---- the damped Newton update: the twin (oracle/pnp_physical.py: newton_step, at_rounding_floor) and its mutants ---------------------------------
# the fp64 twin with the header's multiply-adds is held to the bars of the device (U.RULE_BARS; on the MI355X the two agree bit for bit)
TWIN_BARS = U.RULE_BARS


@pytest.fixture(scope='module', params=U.RULE_NS)
def rule(request):
    rows = U.newton_rule_rows(request.param)
    return rows, U.newton_rule_twin(rows), U.newton_rule_twin(rows, exact=True)


def test_newton_rule_rows_hold_what_the_design_asks_for(rule):
    rows, fp, exact = rule
    kind = np.array(rows['kind'])
    N = rows['c'].shape[1]
    assert 100 <= kind.size <= 400 and FREE_MIN_IS_THE_ORACLES()
    assert exact['floor'][kind == 'floor'].any(axis=1).all() and not exact['floor'][kind == 'plain'].any()
    assert exact['back'][kind == 'backtrack'].all() and not exact['back'][kind == 'plain'].any()
    if N > 1:          # floor and backtrack in one row
        assert (exact['floor'].any(axis=1) & exact['back']).any()
    fm = kind == 'free_min'
    assert fm.sum() >= 12 and exact['free_min'][fm].all() and not exact['free_min'][~fm].any() and not exact['back'][kind == 'free_min, shrinking'].any()
    free = 1.0 - (rows['vol'] * rows['c']).sum(axis=1)
    assert (0.1 * free[fm] < U.FREE_MIN).all() and (free[fm] > 4 * U.FREE_MIN).all()
    assert exact['damped'].sum() >= 10 and (~exact['damped'] & (rows['dphi_max'] > 0)).sum() >= 4 and (np.abs(rows['dphi'])[rows['dphi_max'] <= 0] > 0.05).any()
    assert (rows['lam'] < 1.0).sum() >= 20 and (rows['lam'] == 1.0).sum() >= 20
    for bad in (np.isnan, np.isposinf, np.isneginf):
        assert bad(rows['du']).any() and bad(rows['dphi']).any()
    assert np.isinf(fp['upd'][np.isnan(rows['du']).any(axis=1)]).all() and np.isinf(fp['mphi'][np.isnan(rows['dphi'])]).all()


def FREE_MIN_IS_THE_ORACLES():
    return U.FREE_MIN == PH.FREE_MIN


def test_newton_rule_twin_passes_its_own_helper_and_every_mutant_fails(rule):
    rows, fp, exact = rule
    worst = U.check_newton_rule(fp, fp, exact, TWIN_BARS, rows['kind'])
    print('N = %d: fp64 twin against exact arithmetic, worst ulp: %s' % (rows['c'].shape[1], {k: round(v, 3) for k, v in worst.items()}))
    for mutant in U.RULE_MUTANTS:
        assert fails(U.check_newton_rule, U.newton_rule_twin(rows, mutant=mutant), fp, exact, TWIN_BARS), mutant
    # theta = 1 applied where the backtrack is not taken changes no decision and, in exact arithmetic, no value: the helper cannot see it
    # (the kernels' bits can: profiles/newton_rule.md); a theta that is 1e-12 off is seen
    off = dict(fp, theta=fp['theta'] * (1.0 + 1e-12))
    assert fails(U.check_newton_rule, off, fp, exact, TWIN_BARS)


def test_newton_rule_decisions_do_not_sit_at_a_tie(rule):
    """a relative perturbation of 1e-12 of every input (fused against unfused multiply-add moves far less) flips no decision"""
    rows, fp, _ = rule
    for seed in range(4):
        moved = U.newton_rule_twin(U.perturbed(rows, 1e-12, seed))
        for k in U.RULE_DECISIONS + ('free_min',):
            assert np.array_equal(moved[k], fp[k]), k


def test_newton_accept_tuples_hold_what_the_design_asks_for():
    t, what = U.newton_accept_tuples()
    acc, prev, fired = U.newton_accept_twin(t)
    alone = {'tol': (True, False, False), 'estimate': (False, True, False), 'rounding floor': (False, False, True)}
    for name, pattern in alone.items():
        rows = [k for k, w in enumerate(what) if w.startswith(name) and 'alone' in w]
        assert rows and all(tuple(fired[k]) == pattern and acc[k] for k in rows), name
    damped = t[:, 0] < 1.0
    assert damped.sum() >= 3 and not acc[damped].any() and np.isinf(prev[damped]).all() and np.array_equal(prev[~damped], t[~damped, 1])
    first = np.array(['first iteration' in w for w in what])
    assert (first & (t[:, 4] != 0) & np.isinf(t[:, 2])).any() and not acc[first & (t[:, 1] > U.RULE_TOL)].any()
    lin = np.array([w.startswith('linear sequence') for w in what])
    assert lin.sum() >= 40 and not fired[lin][:, 2].any()                      # never through the rounding-floor rule
    assert np.array_equal(acc[lin & (t[:, 4] == 0)], (t[:, 1] < U.RULE_TOL)[lin & (t[:, 4] == 0)])
    assert (lin & (t[:, 1] < 100 * U.RULE_TOL) & (t[:, 2] < 100 * U.RULE_TOL) & ~acc).sum() >= 10      # ... while inside its window


def test_newton_accept_twin_is_the_oracle_s_rule_and_every_mutant_fails():
    t, what = U.newton_accept_tuples()
    acc, prev, fired = U.newton_accept_twin(t)
    for k, (lam, upd, up, tol, est) in enumerate(t):
        if lam == 1.0:
            assert fired[k][2] == PH.at_rounding_floor(upd, up, tol), what[k]
    U.check_newton_accept(acc, prev, t, what)
    for mutant in U.ACCEPT_MUTANTS:
        a, p, _ = U.newton_accept_twin(t, mutant=mutant)
        assert fails(U.check_newton_accept, a, p, t), mutant
    for seed in range(4):          # no tie: 1e-12 on every number of every tuple flips no decision
        rng = np.random.default_rng(seed)
        moved = t.copy()
        moved[:, 1:4] *= 1.0 + 1e-12 * rng.choice([-1.0, 1.0], (t.shape[0], 3))
        assert np.array_equal(U.newton_accept_twin(moved)[0], acc) and np.array_equal(U.newton_accept_twin(moved)[2], fired)


# ---- the per-lane LU of pnp_kin.h: the replay itself ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', U.LU_TS)
def test_lu_replay_solves_its_systems_and_the_special_lanes_show_what_they_are_there_for(T):
    """The fp64 replay of factor / substitute that the GPU test compares bit for bit: on the 62 non-singular lanes the normwise backward
    error ||A x - b||_inf / (||A||_inf ||x||_inf + ||b||_inf) stays within 8 T 2^(T-1) 2^-53 (partial pivoting at its worst-case growth: a
    loose bound, there to catch a wrong replay); the special lanes make the decisions they were built for; check_lu passes the replay
    against itself and fails the replay with a non-strict pivot comparison and (T > 1) the one with contracted multiply-subtracts."""
    A, b, want = U.lu_cases(T)
    f, pivs, bad, x = U.emul_lu(A, b)
    err = U.lu_backward_error(A, x, b)[U.LU_NONSINGULAR]
    print('T = %d: worst backward error %.2e, bound %.2e' % (T, err.max(), U.lu_backward_bar(T)))
    assert err.shape == (62, 2) and np.isfinite(x[U.LU_NONSINGULAR]).all() and err.max() <= U.lu_backward_bar(T)
    assert np.array_equal(bad != 0, ~U.LU_NONSINGULAR)                        # the flag in the singular and the infinite lane, nowhere else
    assert not np.isnan(f).any() and not np.isnan(x).any()                    # no stored word is a NaN: bitwise equality is defined
    assert np.isposinf(x[3]).all() and (x[4, :, 0] == 0.0).all()
    step0 = (pivs & np.uint64(15)).astype(int)
    assert step0[0] == want['exchange'] and (T == 1 or step0[0] != 0)          # 5e-8 is not the pivot
    i1, i2 = want['tie rows']
    assert step0[1] == i1 and abs(A[1, i1, 0]) == abs(A[1, i2, 0]) == np.abs(A[1, :, 0]).max()
    assert T == 1 or (A[2, T - 1] == np.eye(T)[T - 1]).all()
    for k in range(T, 16):                                                    # nothing above the T fields of four bits
        assert not (pivs >> np.uint64(4 * k)).any()
    assert U.check_lu((f, pivs, bad, x), U.emul_lu(A, b)) == 64 * (T * T + 2 + 2 * T)
    if T > 1:
        assert fails(U.check_lu, U.emul_lu(A, b, strict=False), (f, pivs, bad, x))
        assert fails(U.check_lu, U.emul_lu(A, b, contract=True), (f, pivs, bad, x))
    # a lane's result is its own: the random lanes alone, in other lanes, give the same words
    A2, b2 = np.roll(A, 7, axis=0), np.roll(b, 7, axis=0)
    U.check_lu(tuple(np.roll(v, 7, axis=0) for v in (f, pivs, bad, x)), U.emul_lu(A2, b2))
