"""pnp_scf_cycle -- the kinetics <-> transport self-consistency loop on the device (catint_amd/csrc/pnp_scf.hip, the host loop in
pnp_capi.hip) -- against tests/scf_ref.py, a CPU restatement of the loop over the oracle's Newton solve, on the case table of
tests/scf_cases.py: stuck lanes (from the first device iteration, and only after a converged one), the 1e-20 clamp, the
negative-concentration fallback, the mix decay, both pH paths and none, zeroth-order / saturating / Butler-Volmer rate laws, K = 0 and
negative-only current densities, NaN inputs, lanes inactive on entry -- in every Newton kernel family that takes the shape.

Integers (active, failed, step_to_check, the returned iteration count, which lanes are stuck) and mix are compared exactly:
tests/test_scf_ref.py keeps every accuracy a factor 1.5 away from tau.  Floats to the bar of tests.test_gpu_newton.assert_close,
R = 2e-9 of the row's scale (the same for single-precision lane records: assert_close_f32_records); the accuracy, a difference of two
current densities over one of them, to 4 R + R |acc|; the surface field to 2 R max|phi| / (x1 - x0); the pH to the relative bar of its
concentration over ln 10.  Worst measured |device - reference| / bar per family over all cases (MI355X):
    default (pair / lane teams) 1.3e-6, generic 1.2e-6, team 7.0e-7, sweep 7.7e-7, lane 1.2e-6, lane2 7.7e-7, lane4 7.4e-7,
    lane with f32 records 9.9e-7, lane with one workspace group 1.2e-6
-- warm-started Newton solves contract quadratically, so both sides sit on their rounding floors.
Properties (check_every, split calls, istep >= max_iter, permutations and subsets, 300 lanes over two blocks, ending by max_iter) are
comparisons to the bit between device runs of one family.
"""
import ctypes as C

import numpy as np
import pytest

from catint_amd import _capi
from tests import scf_cases, scf_ref
from tests.scf_cases import DPHI_MAX, MAXIT, TOL
from tests.test_gpu_newton import BETA, EPS, F

pytestmark = pytest.mark.gpu

R = 2e-9
KEYS = scf_ref.ROWS + scf_ref.SCALARS + scf_ref.FLAGS

# family -> (batch size, options, smallest N, largest N)
FAMILIES = {
    'default': (15, {}, 1, 8),
    'generic': (15, {'NEWTON_KERNEL': 'generic'}, 1, 6),
    'team': (15, {'NEWTON_KERNEL': 'team'}, 5, 8),
    'sweep': (15, {'NEWTON_KERNEL': 'sweep'}, 5, 8),
    'lane': (70, {'NEWTON_KERNEL': 'lane'}, 1, 8),
    'lane2': (37, {'NEWTON_KERNEL': 'lane2'}, 5, 8),
    'lane4': (37, {'NEWTON_KERNEL': 'lane4'}, 5, 8),
    'lane-f32': (70, {'NEWTON_KERNEL': 'lane', 'LANE_RECORDS': 'f32'}, 1, 8),
    'lane-groups1': (70, {'NEWTON_KERNEL': 'lane', 'NEWTON_LANE_GROUPS': '1'}, 1, 8),
}
PARITY = [(c, f) for c in scf_cases.CASES for f, (_, _, lo, hi) in FAMILIES.items() if lo <= scf_cases.get(c).N <= hi]


class Handle(object):
    """A solver holding the lanes idx of a case in the state the loop is entered with: converged at zero wall flux, wall table set."""

    def __init__(self, case, idx, options=None):
        self.case, self.idx = case, np.asarray(idx)
        B, N, nx = len(self.idx), case.N, case.nx
        s = self.s = _capi.PnpSolver(N, nx, case.dx, 1.0, BETA, EPS, case.D, case.q, method='Newton', batch_capacity=B)
        for k, v in dict({'NEWTON_KERNEL': ''}, **(options or {})).items():
            s.set_option(k, v)
        s.set_newton(tol=TOL, maxit=MAXIT, dphi_max=DPHI_MAX, **case.newton_kw)
        if case.x is not None:
            s.set_grid(case.x)
        pb = np.zeros((B, 4))
        pb[:, 0] = case.phiM[self.idx]
        s.set_batch(np.repeat(case.cb[self.idx][:, :, None], nx, axis=2), pb, np.zeros(B), np.zeros((B, N)))
        assert (s.solve_stationary(maxit=50) == 0).all()                      # the caller's first iteration
        w = case.wall
        s.set_wall_kinetics(w['species'], w['nu'], case.K[self.idx], w.get('alpha'), w.get('saturation'))
        self.entry = case.state(*s.get_surface(), idx=self.idx)

    def device(self):
        c, phi = self.s.get_state(derived=False)
        return c.copy(), phi.copy(), self.s.get_status().copy(), self.s.newton_iterations().copy()

    def cycle(self, state, istep=None, max_iter=None, check_every=8):
        case = self.case
        state = {k: np.array(v) for k, v in state.items()}
        it = self.s.scf_cycle(state, case.istep if istep is None else istep, case.max_iter if max_iter is None else max_iter, case.tau, F,
                              check_every=check_every, **case.scf_kw())
        return state, it

    def close(self):
        self.s.close()


class Run(object):
    pass


_RUNS = {}


def run(name, family, idx=None, case=None, **kw):
    """One call of the loop from the entry state; cached.  .state (final arrays), .iterations, .entry (arrays), .before / .after
    (c, phi, status, Newton iterations on the device), .idx."""
    case = scf_cases.get(name) if case is None else case
    B, options = FAMILIES[family][:2]
    idx = case.tile(B) if idx is None else np.asarray(idx)
    key = (name, family, tuple(idx), tuple(sorted(kw.items())))
    if key not in _RUNS:
        h = Handle(case, idx, options)
        try:
            r = Run()
            r.idx, r.entry, r.before = idx, h.entry, h.device()
            r.state, r.iterations = h.cycle(h.entry, **{k: v for k, v in kw.items() if k != 'again'})      # (again: not the cached run)
            r.after = h.device()
        finally:
            h.close()
        _RUNS[key] = r
    return _RUNS[key]


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def assert_same_runs(a, b, lanes_a=None, lanes_b=None, what=''):
    """Two device runs agree to the bit, lane lanes_a[i] of a with lane lanes_b[i] of b: every array, the device state, status, counters."""
    la = np.arange(len(a.idx)) if lanes_a is None else np.asarray(lanes_a)
    lb = la if lanes_b is None else np.asarray(lanes_b)
    for k in KEYS:
        assert same(a.state[k][la], b.state[k][lb]), (what, k)
    for i, part in enumerate(('c', 'phi', 'status', 'newton iterations')):
        assert same(a.after[i][la], b.after[i][lb]), (what, part)


def first_copies(idx):
    return {j: int(np.flatnonzero(idx == j)[0]) for j in np.unique(idx)}


def check_against_reference(case, ref, r, family):
    """The assertions of the module docstring for one device run; returns the worst |device - reference| / bar."""
    idx, st = r.idx, r.state
    first = first_copies(idx)
    firsts = np.array([first[j] for j in idx])
    assert_same_runs(r, r, np.arange(len(idx)), firsts, 'tiled copies equal their first copy')
    worst = 0.0

    def bar(got, want, tol, what):
        nonlocal worst
        ratio = float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / tol)) if np.size(got) else 0.0
        worst = max(worst, ratio)
        assert ratio <= 1.0, (family, what, ratio)
    assert r.iterations == ref.iterations, (r.iterations, ref.iterations)
    for j, b in first.items():
        lane = case.lanes[j]
        for k in scf_ref.FLAGS + ('mix',):
            assert st[k][b] == ref.out[k][j], (family, j, k, st[k][b], ref.out[k][j])
        c, phi = r.after[0][b], r.after[1][b]
        if lane.get('inactive'):
            for k in KEYS:
                assert same(st[k][b], r.entry[k][b]), (j, k)
            for i in range(4):
                assert same(r.after[i][b], r.before[i][b]), (j, i)
            continue
        if lane.get('fails'):
            continue
        stuck = (ref.out['surface_concentration'][j] == -1.0).all()
        assert (st['surface_concentration'][b] == -1.0).all() == stuck, (family, j, st['surface_concentration'][b])
        if lane.get('stuck_from') == case.istep + 1:       # never converged: the lane is back on the state it was handed over with
            assert same(c, r.before[0][b]) and same(phi, r.before[1][b]), (family, j)
        for k in scf_ref.ROWS:
            if stuck and k == 'surface_concentration':
                continue
            scale = np.abs(ref.out[k][j]).max()
            if scale == 0.0:
                assert (st[k][b] == 0.0).all(), (family, j, k)
            else:
                bar(st[k][b], ref.out[k][j], R * scale, (j, k))
        pscale = max(np.abs(ref.phi[j]).max(), 0.025)
        x1 = case.dx if case.x is None else case.x[1] - case.x[0]
        bar(st['surface_potential'][b], ref.out['surface_potential'][j], R * pscale, (j, 'surface_potential'))
        bar(st['surface_efield'][b], ref.out['surface_efield'][j], 2.0 * R * pscale / x1, (j, 'surface_efield'))
        a = ref.out['accuracy'][j]
        if np.isfinite(a):
            bar(st['accuracy'][b], a, 4.0 * R + R * abs(a), (j, 'accuracy'))
        else:
            assert st['accuracy'][b] == a, (family, j, st['accuracy'][b])
        if case.species_H < 0 and case.species_OH < 0:
            assert st['surface_pH'][b] == r.entry['surface_pH'][b]
        else:
            k = case.species_H if case.species_H >= 0 else case.species_OH
            conc = ref.out['surface_concentration_old'][j]          # the mixed iterate the last pH was taken from
            bar(st['surface_pH'][b], ref.out['surface_pH'][j], R * np.abs(conc).max() / abs(conc[k]) / np.log(10.0) + 1e-14, (j, 'surface_pH'))
        cscale = np.abs(ref.c[j]).max()
        bar(c, ref.c[j], R * cscale, (j, 'c'))
        assert (np.abs(c - ref.c[j]) / (np.abs(ref.c[j]) + 1e-3 * np.abs(ref.c[j]).max(axis=1, keepdims=True))).max() < 1e-6
        bar(phi, ref.phi[j], R * pscale, (j, 'phi'))
    return worst


@pytest.mark.parametrize('name,family', PARITY)
def test_device_loop_matches_the_restatement(name, family):
    case = scf_cases.get(name)
    worst = check_against_reference(case, case.reference(), run(name, family), family)
    print('RATIO %s %s %.3g' % (family, name, worst))


def test_stuck_after_a_converged_iteration_goes_back_to_that_iteration():
    """Lane 1 of 'exits': iteration 2 converges, every later one is stuck.  The state the device ends with is the reference's state of
    iteration 2 (checked to the bar above) and NOT the state the lane was handed over with."""
    case, r = scf_cases.get('exits'), run('exits', 'default')
    ref = case.reference()
    b = first_copies(r.idx)[1]
    assert [t['status'] for t in ref.traces[1]][:2] == ['ok', 'stuck']
    moved = np.abs(ref.c[1] - case.entry()[0][1]).max() / np.abs(ref.c[1]).max()
    assert moved > 1e-3
    assert np.abs(r.after[0][b] - r.before[0][b]).max() / np.abs(ref.c[1]).max() > 0.5 * moved
    assert np.abs(r.after[0][b] - ref.c[1]).max() <= R * np.abs(ref.c[1]).max()


@pytest.mark.parametrize('name', ['fallback', 'stern'])
@pytest.mark.parametrize('family', ['default', 'lane'])
def test_a_nan_lane_fails_alone(name, family):
    """A NaN rate constant ('fallback') / a NaN surface concentration handed in ('stern'): that lane ends failed and inactive; every
    other lane ends where it ends in the same batch without the NaN, to the bit."""
    case = scf_cases.get(name)
    finite = {'fallback': scf_cases.case_fallback, 'stern': scf_cases.case_stern}[name](nan=False)
    r, f = run(name, family), run(name + '-finite', family, case=finite)
    bad = np.array([bool(case.lanes[j].get('fails')) for j in r.idx])
    assert bad.any() and same(r.idx, f.idx)
    assert (r.state['failed'][bad] == 1).all() and (r.state['active'][bad] == 0).all()
    assert (f.state['failed'] == 0).all()
    assert_same_runs(r, f, np.flatnonzero(~bad), what='lanes beside the NaN lane')


@pytest.mark.parametrize('family', ['default', 'lane'])
@pytest.mark.parametrize('check_every', [1, 3, 8, 32, 0, 100])
def test_check_every_changes_nothing(family, check_every):
    """The host looks at the active-lane counter every check_every iterations (0: 8, above 32: 32); when it looks decides nothing.
    (8 is the default the other run was made with: a second run of the same call.)"""
    a, b = run('exits', family), run('exits', family, check_every=check_every, again=1)
    assert a.iterations == b.iterations
    assert_same_runs(a, b)
    # every lane leaves, one after the other (one copy of each): the loop ends early, and not before the last lane has left
    case = scf_cases.get('stern')
    a, b = run('stern', family, idx=np.arange(case.P)), run('stern', family, idx=np.arange(case.P), check_every=check_every)
    assert a.iterations == b.iterations == case.reference().iterations < case.max_iter
    assert_same_runs(a, b)


@pytest.mark.parametrize('family', ['default', 'lane'])
@pytest.mark.parametrize('k', [2, 41])
def test_two_calls_equal_one(family, k):
    """istep = 1 -> 45 in one call, and 1 -> k then k -> 45 with the arrays of the first handed to the second.  k = 2: every lane is
    still active, lane 6 is one iteration before its decay; k = 41: the stuck lanes are, one iteration before theirs."""
    case, one = scf_cases.get('exits'), run('exits', family)
    h = Handle(case, one.idx, FAMILIES[family][1])
    try:
        s1, it1 = h.cycle(h.entry, max_iter=k)
        assert it1 == k and s1['active'].any()
        two = Run()
        two.idx = one.idx
        two.state, two.iterations = h.cycle(s1, istep=k)
        two.after = h.device()
    finally:
        h.close()
    stuck = [j for j, l in enumerate(case.lanes) if 'stuck_from' in l]
    assert all(s1['active'][one.idx == j].all() for j in stuck)
    assert two.iterations == one.iterations
    assert_same_runs(one, two)


@pytest.mark.parametrize('istep,max_iter', [(5, 5), (7, 3)])
def test_no_iteration_left_changes_nothing(istep, max_iter):
    case = scf_cases.get('exits')
    h = Handle(case, case.tile(15))
    try:
        before = h.device()
        st, it = h.cycle(h.entry, istep=istep, max_iter=max_iter)
        after = h.device()
    finally:
        h.close()
    assert it == istep
    for k in KEYS:
        assert same(st[k], h.entry[k]), k
    for a, b in zip(before, after):
        assert same(a, b)


@pytest.mark.parametrize('family', ['default', 'lane'])
def test_permuted_lanes_and_subsets(family):
    """A lane's result depends neither on its slot nor on its neighbours."""
    case, base = scf_cases.get('exits'), run('exits', family)
    first = first_copies(base.idx)
    for idx in (base.idx[::-1].copy(), np.array([5, 1, 3]), np.array([3]), np.arange(case.P)):
        r = run('exits', family, idx=idx)
        assert_same_runs(r, base, np.arange(len(idx)), [first[j] for j in idx], 'lanes %s' % (idx,))
        assert r.iterations == max(case.reference().last[j] for j in idx)


def test_300_lanes_over_two_blocks():
    """B = 300: scf_pre_kernel / scf_post_kernel run two blocks and the active-lane counter collects from both; every kind of lane also
    sits beyond index 255.  With lanes that stay active the loop runs to max_iter; when every lane leaves, it ends at the reference's
    iteration count."""
    for name in ('exits', 'stern-finite'):
        case = scf_cases.get(name) if name == 'exits' else scf_cases.case_stern(nan=False)
        idx = case.tile(300)
        assert set(idx[256:]) == set(range(case.P))
        r = run(name, 'default', idx=idx, case=case)
        ref = case.reference()
        check_against_reference(case, ref, r, 'default B=300')
        assert r.iterations == ref.iterations and (ref.iterations < case.max_iter) == (name != 'exits')


@pytest.mark.parametrize('family', ['default', 'lane'])
def test_ending_by_max_iter_leaves_the_last_iterates(family):
    """max_iter = 5 with lanes still active: the arrays are those of iteration 5 and `active` is still 1 where the reference keeps it."""
    case = scf_cases.get('exits')
    ref = case.reference(max_iter=5)
    assert ref.out['active'].sum() >= 4 and ref.iterations == 5
    r = run('exits', family, max_iter=5)
    check_against_reference(case, ref, r, family)


def raw_cycle(s, state, N, istep=1, max_iter=3, species_H=-1, species_OH=-1, struct_size=None, null=None):
    """pnp_scf_cycle through the plain ctypes binding: (return code, message)."""
    st, keep = _capi.PnpScfState(), []
    for name, ctype in _capi.PnpScfState._fields_:
        arr = np.ascontiguousarray(state[name], dtype=np.float64 if ctype == C.POINTER(C.c_double) else np.int32)
        keep.append(arr)
        if name != null:
            setattr(st, name, arr.ctypes.data_as(ctype))
    p = _capi.PnpScfParams(struct_size=C.sizeof(_capi.PnpScfParams) if struct_size is None else struct_size, istep=istep,
                           max_iter=max_iter, check_every=8, species_H=species_H, species_OH=species_OH, tau_scf=1e-6, faraday=F)
    it = C.c_int32(0)
    rc = s._lib.pnp_scf_cycle(s._h, C.byref(p), None, None, C.byref(st), C.byref(it))
    return rc, s._lib.pnp_last_error(s._h).decode()


def test_argument_checks_name_the_cause_and_leave_the_handle_alone():
    case = scf_cases.get('exits')
    idx = np.arange(case.P)
    base = run('exits', 'default', idx=idx)
    N, nx, B = case.N, case.nx, case.P
    with _capi.PnpSolver(N, nx, case.dx, 1e-9, BETA, EPS, case.D, case.q, method='Crank-Nicolson', batch_capacity=B) as s:
        rc, msg = raw_cycle(s, base.entry, N)
        assert rc != 0 and 'PNP_METHOD_NEWTON' in msg
    with _capi.PnpSolver(N, nx, case.dx, 1.0, BETA, EPS, case.D, case.q, method='Newton', batch_capacity=B) as s:
        s.set_newton(tol=TOL, maxit=MAXIT, dphi_max=DPHI_MAX)
        rc, msg = raw_cycle(s, base.entry, N)
        assert rc != 0 and 'pnp_set_batch' in msg
        pb = np.zeros((B, 4))
        pb[:, 0] = case.phiM
        s.set_batch(np.repeat(case.cb[:, :, None], nx, axis=2), pb, np.zeros(B), np.zeros((B, N)))
        rc, msg = raw_cycle(s, base.entry, N)
        assert rc != 0 and 'pnp_set_wall_kinetics' in msg
    h = Handle(case, idx)
    try:
        before = h.device()
        for kw, text in ((dict(istep=0), 'first iteration'), (dict(istep=-3), 'first iteration'), (dict(species_H=N), 'out of range'),
                         (dict(species_OH=N + 2), 'out of range'), (dict(struct_size=C.sizeof(_capi.PnpScfParams) - 8), 'struct_size'),
                         (dict(null='mix'), 'null array'), (dict(null='failed'), 'null array'),
                         (dict(null='surface_concentration'), 'null array')):
            state = {k: v.copy() for k, v in h.entry.items()}
            rc, msg = raw_cycle(h.s, state, N, **kw)
            assert rc != 0 and text in msg, (kw, rc, msg)
            for k in KEYS:
                assert same(state[k], h.entry[k]), (kw, k)
            for a, b in zip(before, h.device()):
                assert same(a, b), kw
        with pytest.raises(_capi.PnpError, match='first iteration'):
            h.cycle(h.entry, istep=0)
        r = Run()                                   # ... and the handle is as good as new: the same call as a fresh handle's, to the bit
        r.idx = idx
        r.state, r.iterations = h.cycle(h.entry)
        r.after = h.device()
    finally:
        h.close()
    assert r.iterations == base.iterations
    assert_same_runs(r, base)
