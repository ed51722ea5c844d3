"""libcatint_scfkin and pnp_scf_cycle_fn on the device: the microkinetic SCF loop without a host round trip per iteration.

Kernel parity: catsk_step_host against catkin_solve (the kernel the host loop calls), bit for bit on flux, theta, flux_scale, status and
iterations, for every case of tests/kinetics_cases.py at 1, 63, 64, 65 and 130 lanes through two successive calls (the second is
warm-started from the coverages the first left on the device); any number of waves; inactive lanes; the uniform start; failures.
Loop parity: pnp_scf_cycle_fn with the library's function against tests/scfkin_ref.py on the cases of tests/scfkin_cases.py.  The
bars are those of tests/test_gpu_scf.py (check_against_reference is its function: integers, mix and the iteration count exact, floats to
R = 2e-9 of the row's scale, the accuracy to 4 R + R |acc|); on top the coverages to R, flux_scale to R of the row's largest, the
kinetic status and the calls exact, the kinetic iterations within 1 per call.  Worst |device - reference| / bar per family is printed
(RATIO lines); measured on an MI355X: case A 0.16 (default, lane, generic), case B 0.25 (default), 0.35 (lane) -- the largest term is
the flux, a difference of gross rates, against R of its row.
Properties (check_every, split calls, permutations and subsets, 300 lanes, inactive lanes, no iteration left) are comparisons to the
bit between device runs.  End to end: Calculator.set_microkinetics(device_loop=True) against device_loop=False, the bars of
tests.test_gpu_calculator.test_device_scf_loop_walks_the_same_iterates_as_the_host_loop; on an MI355X every array came out
bit-identical (23 iterations)."""
import ctypes as C

import numpy as np
import pytest

from catint_amd import _capi, _kinetics
from catint_amd import _scfkin                      # fails without the feature
from tests import kinetics_cases as KC
from tests import scfkin_cases as SC
from tests import scfkin_ref
from tests.scf_cases import DPHI_MAX, MAXIT, TOL
from tests.test_gpu_scf import KEYS, R, Run, assert_same_runs, check_against_reference, first_copies, same

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 130)
F = SC.F
KIN_KEYS = scfkin_ref.KIN_ROWS + scfkin_ref.KIN_FLAGS
FAMILIES = {'default': (15, {}), 'lane': (70, {'NEWTON_KERNEL': 'lane'}), 'generic': (15, {'NEWTON_KERNEL': 'generic'})}
PARITY = [('A', 'default'), ('A', 'lane'), ('A', 'generic'), ('B', 'default'), ('B', 'lane')]


@pytest.fixture(scope='module')
def ks():
    with _kinetics.KineticsSolver(0) as o:
        yield o


def kw_of(case):
    k = case.kw
    return dict(potential_drop='stern' if k['w'] else 'full', stern_capacitance=k['CS'], phi_pzc=k['phi_pzc'])


def tiled(case, n):
    idx = np.arange(n) % len(case.phiM)
    return case.phiM[idx], case.csurf[idx], case.phi_surface[idx]


def start_of(tables):
    return 1.0 / float(np.sum(tables['site_count']))


def host_guess(theta, tables):
    """what the host loop hands catkin_solve: the stored coverages, the uniform ones where a lane has none"""
    return np.where(np.isfinite(theta).all(axis=1)[:, None], theta, start_of(tables))


def assert_call_equals_catkin(got_flux, dev, ref, what):
    """One call of the flux function against catkin_solve at the same inputs, to the bit"""
    ok = ref['status'] == 0
    assert np.array_equal(dev['status'], ref['status']) and np.array_equal(dev['iterations_last'], ref['iterations']), what
    assert same(dev['theta'], ref['theta']) and same(dev['flux_scale'], ref['flux_scale']), what
    assert same(got_flux[ok], ref['flux'][ok]) and np.isnan(got_flux[~ok]).all(), what


# ---- kernel parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', KC.CASE_NAMES)
def test_step_host_gives_the_bits_of_catkin_solve(ks, name):
    case = KC.case(name)
    with _scfkin.ScfKinetics(0) as sk:
        for n in SIZES:
            pm, cs, ps = tiled(case, n)
            sk.begin(case.tables, pm, **kw_of(case))
            guess, total, cold = None, np.zeros(n, np.int64), 0
            for call in range(2):
                cs_call = cs * (1.0 + 0.05 * call)                  # the second call has somewhere to go from its warm start
                flux = sk.step_host(cs_call, ps)
                assert sk.last_kernel == 'catsk::flux_kernel'
                dev = sk.end()
                ref = ks.solve(None, case.tables, pm, csurf=cs_call, phi_surface=ps, theta_guess=guess, fields=('theta', 'flux', 'flux_scale'),
                               **kw_of(case))
                assert_call_equals_catkin(flux, dev, ref, (name, n, call))
                assert (ref['status'] == 0).all() and same(dev['flux_last'], ref['flux'])
                total += ref['iterations']
                assert np.array_equal(dev['iterations_total'], total) and (dev['calls'] == call + 1).all()
                guess = host_guess(dev['theta'], case.tables)
                cold = cold or int(ref['iterations'].max())
            assert ref['iterations'].max() < cold                    # warm


def test_any_number_of_waves_gives_the_same_bits():
    case = KC.case('co2r_two_site')
    pm, cs, ps = tiled(case, 130)
    runs = []
    with _scfkin.ScfKinetics(0) as sk:
        for waves in (0, 1, 2):
            sk.begin(case.tables, pm, max_waves=waves, **kw_of(case))
            flux = [sk.step_host(cs, ps), sk.step_host(1.05 * cs, ps)]
            runs.append((flux, sk.end()))
    for flux, dev in runs[1:]:
        assert same(flux[0], runs[0][0][0]) and same(flux[1], runs[0][0][1])
        for k in KIN_KEYS:
            assert same(dev[k], runs[0][1][k]), k


def test_inactive_lanes_are_not_touched():
    case = KC.case('random_S5')
    n = 130
    pm, cs, ps = tiled(case, n)
    T = len(case.tables['site_count'])
    active = (np.arange(n) % 3 != 1).astype(np.int32)
    active[64:128] = 0                                              # a whole group without an active lane
    on = active != 0
    guess = np.full((n, T), start_of(case.tables))
    guess[~on] = 0.123
    with _scfkin.ScfKinetics(0) as sk:
        sk.begin(case.tables, pm, theta_guess=guess, **kw_of(case))
        flux = sk.step_host(cs, ps, active=active, flux=np.full((n, cs.shape[1]), 7.0))
        dev = sk.end()
        sk.begin(case.tables, pm, theta_guess=guess, **kw_of(case))
        full = sk.step_host(cs, ps)
        ref = sk.end()
    assert (flux[~on] == 7.0).all() and same(flux[on], full[on])
    assert (dev['theta'][~on] == 0.123).all() and (dev['calls'][~on] == 0).all() and (dev['calls'][on] == 1).all()
    for k in KIN_KEYS:
        assert same(dev[k][on], ref[k][on]), k
        if k != 'theta':
            assert (dev[k][~on] == 0).all(), k


def test_a_lane_without_finite_coverages_starts_uniform(ks):
    case = KC.case('co2r_one_site')
    n = 65
    pm, cs, ps = tiled(case, n)
    T = len(case.tables['site_count'])
    cold = ks.solve(None, case.tables, pm, csurf=cs, phi_surface=ps, fields=('theta',), **kw_of(case))
    stored = cold['theta'].copy()
    stored[::3, 0] = np.nan
    stored[1::3, T - 1] = np.inf
    with _scfkin.ScfKinetics(0) as sk:
        sk.begin(case.tables, pm, theta_guess=stored, **kw_of(case))
        flux = sk.step_host(cs, ps)
        dev = sk.end()
    ref = ks.solve(None, case.tables, pm, csurf=cs, phi_surface=ps, theta_guess=host_guess(stored, case.tables),
                   fields=('theta', 'flux', 'flux_scale'), **kw_of(case))
    assert_call_equals_catkin(flux, dev, ref, 'uniform start')
    assert ref['iterations'][2::3].max() <= 2 < ref['iterations'][::3].min()


def test_a_lane_that_fails_gets_nan_fluxes_and_keeps_its_last_good_ones(ks):
    case = KC.case('co2r_one_site')
    n = len(case.phiM)
    pm, cs, ps = case.phiM, case.csurf, case.phi_surface
    with _scfkin.ScfKinetics(0) as sk:
        # a NaN surface concentration in the second call
        sk.begin(case.tables, pm, **kw_of(case))
        first = sk.step_host(cs, ps)
        good = sk.end()
        bad_cs = 1.05 * cs
        bad_cs[3, 0] = np.nan
        second = sk.step_host(bad_cs, ps)
        dev = sk.end()
        ref = ks.solve(None, case.tables, pm, csurf=bad_cs, phi_surface=ps, theta_guess=good['theta'], fields=('theta', 'flux', 'flux_scale'),
                       **kw_of(case))
        assert ref['status'][3] == 2 and (np.delete(ref['status'], 3) == 0).all()
        assert_call_equals_catkin(second, dev, ref, 'NaN concentration')
        assert np.isnan(second[3]).all() and same(dev['flux_last'][3], first[3]) and same(np.delete(dev['flux_last'], 3, axis=0), np.delete(second, 3, axis=0))
        assert np.isnan(dev['theta'][3]).all() and dev['iterations_last'][3] == 0 and dev['calls'][3] == 2
        # maxit = 3 on lanes that need more
        start = start_of(case.tables)
        guess = np.where((np.arange(n) % 2 == 0)[:, None], good['theta'], start)
        sk.begin(case.tables, pm, theta_guess=guess, maxit=3, **kw_of(case))
        flux = sk.step_host(cs, ps)
        dev = sk.end()
        ref = ks.solve(None, case.tables, pm, csurf=cs, phi_surface=ps, theta_guess=guess, maxit=3, fields=('theta', 'flux', 'flux_scale'), **kw_of(case))
        stopped = ref['status'] == 1
        assert stopped.any() and (ref['status'][~stopped] == 0).all()
        assert_call_equals_catkin(flux, dev, ref, 'maxit')
        assert (dev['flux_last'][stopped] == 0.0).all() and same(dev['flux_last'][~stopped], ref['flux'][~stopped])


# ---- the loop ------------------------------------------------------------------------------------------------------------------------
class Handle(object):
    """A solver holding the lanes idx of a case in the state the loop is entered with (converged at zero wall flux, no wall table) and a
    context of the kinetics"""

    def __init__(self, case, idx, options=None):
        self.case, self.idx = case, np.asarray(idx)
        B, N, nx = len(self.idx), case.N, case.nx
        s = self.s = _capi.PnpSolver(N, nx, case.dx, 1.0, case.beta, case.eps, case.D, case.q, method='Newton', batch_capacity=B)
        self.sk = _scfkin.ScfKinetics(0)
        for k, v in dict({'NEWTON_KERNEL': ''}, **(options or {})).items():
            s.set_option(k, v)
        s.set_newton(tol=TOL, maxit=MAXIT, dphi_max=DPHI_MAX, **case.newton_kw)
        if case.x is not None:
            s.set_grid(case.x)
        pb = np.zeros((B, 4))
        pb[:, 0] = case.phiM[self.idx]
        s.set_batch(np.repeat(case.cb[self.idx][:, :, None], nx, axis=2), pb, np.zeros(B), np.zeros((B, N)))
        assert (s.solve_stationary(maxit=50) == 0).all()                      # the caller's first iterations
        self.entry = case.state(*s.get_surface(), idx=self.idx)

    def device(self):
        c, phi = self.s.get_state(derived=False)
        return c.copy(), phi.copy(), self.s.get_status().copy(), self.s.newton_iterations().copy()

    def begin(self, theta_guess=None, lanes=None):
        kin, idx = self.case.kin, self.idx if lanes is None else np.asarray(lanes)
        self.sk.begin(kin.tables, self.case.phiM[idx], potential_drop='stern' if kin.w else 'full', stern_capacitance=kin.CS, phi_pzc=kin.phi_pzc,
                      gamma=None if self.case.gamma is None else self.case.gamma[idx], theta_guess=theta_guess, tol=kin.tol, maxit=kin.maxit)

    def cycle(self, state, istep=None, max_iter=None, check_every=8, flux_fn=None, user=None):
        case = self.case
        state = {k: np.array(v) for k, v in state.items()}
        it = self.s.scf_cycle(state, case.istep if istep is None else istep, case.max_iter if max_iter is None else max_iter, case.tau, F,
                              check_every=check_every, flux_fn=self.sk.flux_fn if flux_fn is None else flux_fn,
                              user=self.sk.user if user is None else user, **case.scf_kw())
        return state, it

    def close(self):
        self.sk.close()
        self.s.close()


_RUNS = {}


def run(name, family, idx=None, **kw):
    """One call of the loop from the entry state; cached.  The members of tests.test_gpu_scf.run's result and .kin (catsk_end)."""
    case = SC.get(name)
    B, options = FAMILIES[family]
    idx = case.tile(B) if idx is None else np.asarray(idx)
    key = (name, family, tuple(idx), tuple(sorted(kw.items())))
    if key not in _RUNS:
        h = Handle(case, idx, options)
        try:
            r = Run()
            r.idx, r.entry, r.before = idx, h.entry, h.device()
            h.begin()
            r.state, r.iterations = h.cycle(h.entry, **{k: v for k, v in kw.items() if k != 'again'})
            r.kin = h.sk.end()
            r.after = h.device()
        finally:
            h.close()
        _RUNS[key] = r
    return _RUNS[key]


def assert_same(a, b, lanes_a=None, lanes_b=None, what=''):
    """assert_same_runs, and the buffers of the kinetics"""
    assert_same_runs(a, b, lanes_a, lanes_b, what)
    la = np.arange(len(a.idx)) if lanes_a is None else np.asarray(lanes_a)
    lb = la if lanes_b is None else np.asarray(lanes_b)
    for k in KIN_KEYS:
        assert same(a.kin[k][la], b.kin[k][lb]), (what, k)


@pytest.mark.parametrize('name,family', PARITY)
def test_device_loop_matches_the_restatement(name, family):
    case, r = SC.get(name), run(name, family)
    ref = case.reference()
    worst = check_against_reference(case, ref, r, family)
    first = first_copies(r.idx)
    assert_same(r, r, np.arange(len(r.idx)), np.array([first[j] for j in r.idx]), 'tiled copies equal their first copy')
    for j, b in first.items():
        for k in ('status', 'calls'):
            assert r.kin[k][b] == ref.kin[k][j], (j, k, r.kin[k][b], ref.kin[k][j])
        assert abs(int(r.kin['iterations_total'][b]) - int(ref.kin['iterations_total'][j])) <= ref.kin['calls'][j], j
        if case.lanes[j].get('inactive'):
            assert np.isnan(r.kin['theta'][b]).all() and (r.kin['flux_scale'][b] == 0).all() and (r.kin['flux_last'][b] == 0).all()
            continue
        if case.lanes[j].get('fails'):
            assert np.isnan(r.state['flux'][b]).all() and np.isnan(r.kin['theta'][b]).all() and (r.kin['flux_last'][b] == 0).all()
            continue
        ratios = [np.abs(r.kin['theta'][b] - ref.kin['theta'][j]).max() / R,
                  np.abs(r.kin['flux_scale'][b] - ref.kin['flux_scale'][j]).max() / (R * np.abs(ref.kin['flux_scale'][j]).max()),
                  np.abs(r.kin['flux_last'][b] - ref.kin['flux_last'][j]).max() / (R * np.abs(ref.kin['flux_last'][j]).max())]
        assert max(ratios) <= 1.0, (family, j, ratios)
        assert same(r.kin['flux_last'][b], r.state['flux'][b])
        worst = max(worst, max(ratios))
    print('RATIO %s %s %.3g' % (family, name, worst))


@pytest.mark.parametrize('family', ['default', 'lane'])
@pytest.mark.parametrize('check_every', [1, 32])
def test_check_every_changes_nothing(family, check_every):
    a, b = run('B', family), run('B', family, check_every=check_every)
    assert a.iterations == b.iterations == SC.get('B').reference().iterations
    assert_same(a, b)


@pytest.mark.parametrize('k', [36, 42])
def test_two_calls_equal_one(k):
    """34 -> 60 in one call, and 34 -> k then k -> 60 with the arrays of the first handed to the second and the coverages read back and
    handed to a new catsk_begin in between (k = 42: the iteration of the decay)"""
    case, one = SC.get('B'), run('B', 'default')
    h = Handle(case, one.idx, FAMILIES['default'][1])
    try:
        h.begin()
        s1, it1 = h.cycle(h.entry, max_iter=k)
        k1 = h.sk.end()
        assert it1 == k and s1['active'].any()
        h.begin(theta_guess=k1['theta'])
        two = Run()
        two.idx = one.idx
        two.state, two.iterations = h.cycle(s1, istep=k)
        two.after, k2 = h.device(), h.sk.end()
    finally:
        h.close()
    assert two.iterations == one.iterations
    assert_same_runs(one, two)
    went_on = k2['calls'] > 0
    assert went_on.any() and same(one.kin['calls'], k1['calls'] + k2['calls']) and same(one.kin['iterations_total'], k1['iterations_total'] + k2['iterations_total'])
    for key in ('theta', 'flux_scale', 'flux_last', 'status', 'iterations_last'):
        assert same(one.kin[key][went_on], k2[key][went_on]) and same(one.kin[key][~went_on], k1[key][~went_on]), key


def test_permuted_lanes_subsets_and_300_lanes():
    """A lane's result depends neither on its slot nor on its neighbours; B = 300: two blocks of the loop's kernels, five groups of
    the kinetics"""
    case, base = SC.get('B'), run('B', 'default')
    first = first_copies(base.idx)
    idx300 = case.tile(300)
    assert set(idx300[256:]) == set(range(case.P))
    for idx in (base.idx[::-1].copy(), np.array([5, 1, 3]), np.array([3]), idx300):
        r = run('B', 'default', idx=idx)
        assert_same(r, base, np.arange(len(idx)), [first[j] for j in idx], 'lanes %s' % (idx,))
        assert r.iterations == max(case.reference().last[j] for j in idx)


def test_a_lane_inactive_at_entry_keeps_everything():
    case, r = SC.get('B'), run('B', 'lane')
    off = np.array([bool(case.lanes[j].get('inactive')) for j in r.idx])
    assert off.any()
    for k in KEYS:
        assert same(r.state[k][off], r.entry[k][off]), k
    for i in range(4):
        assert same(r.after[i][off], r.before[i][off]), i
    assert np.isnan(r.kin['theta'][off]).all() and all((r.kin[k][off] == 0).all() for k in KIN_KEYS if k != 'theta')


@pytest.mark.parametrize('istep,max_iter', [(5, 5), (7, 3)])
def test_no_iteration_left_runs_nothing(istep, max_iter):
    case = SC.get('A')
    h = Handle(case, np.arange(case.P))
    try:
        before = h.device()
        h.begin()
        st, it = h.cycle(h.entry, istep=istep, max_iter=max_iter)
        after, kin = h.device(), h.sk.end()
    finally:
        h.close()
    assert it == istep and (kin['calls'] == 0).all()
    for k in KEYS:
        assert same(st[k], h.entry[k]), k
    for a, b in zip(before, after):
        assert same(a, b)


# ---- argument checks ---------------------------------------------------------------------------------------------------------------
def raw_cycle(s, state, fn, user, istep=2, max_iter=4):
    """pnp_scf_cycle_fn through the plain ctypes binding: (return code, message)"""
    st, keep = _capi.PnpScfState(), []
    for name, ctype in _capi.PnpScfState._fields_:
        arr = np.ascontiguousarray(state[name], dtype=np.float64 if ctype == C.POINTER(C.c_double) else np.int32)
        keep.append(arr)
        setattr(st, name, arr.ctypes.data_as(ctype))
    p = _capi.PnpScfParams(struct_size=C.sizeof(_capi.PnpScfParams), istep=istep, max_iter=max_iter, check_every=8, species_H=-1, species_OH=-1,
                           tau_scf=1e-6, faraday=F)
    it = C.c_int32(0)
    rc = s._lib.pnp_scf_cycle_fn(s._h, C.byref(p), None, None, C.byref(st), fn, user, C.byref(it))
    return rc, s._lib.pnp_last_error(s._h).decode()


def test_argument_checks():
    case = SC.get('A')
    idx = np.arange(case.P)
    base = run('A', 'default', idx=idx)
    N, nx, B = case.N, case.nx, case.P
    calls = []

    def seven(user, d):
        calls.append((d.contents.batch, d.contents.nspecies, d.contents.istep))
        return 7
    seven_fn = _capi.PnpScfFluxFn(seven)
    seven_addr = C.cast(seven_fn, C.c_void_p).value
    with _capi.PnpSolver(N, nx, case.dx, 1e-9, case.beta, case.eps, case.D, case.q, method='Crank-Nicolson', batch_capacity=B) as s:
        rc, msg = raw_cycle(s, base.entry, seven_addr, None)
        assert rc == -1 and 'PNP_METHOD_NEWTON' in msg and not calls
    h = Handle(case, idx)
    try:
        before = h.device()
        rc, msg = raw_cycle(h.s, base.entry, None, None)
        assert rc == -1 and 'pnp_scf_cycle_fn' in msg and 'null flux function' in msg
        # no wall table: refused without a function, accepted with one
        with pytest.raises(_capi.PnpError, match='pnp_set_wall_kinetics'):
            h.s.scf_cycle({k: v.copy() for k, v in h.entry.items()}, case.istep, case.max_iter, case.tau, F)
        # a function that returns 7
        state = {k: v.copy() for k, v in h.entry.items()}
        rc, msg = raw_cycle(h.s, state, seven_addr, None)
        assert rc == -3 and 'returned 7' in msg and calls == [(B, N, 3)]
        for k in KEYS:
            assert same(state[k], h.entry[k]), k
        # catsk_begin with another batch than the handle's
        h.begin(lanes=idx[:-1])
        with pytest.raises(_capi.PnpError, match='returned 3'):
            h.cycle(h.entry)
        assert '%d lanes' % B in h.sk.last_error
        for a, b in zip(before, h.device()):
            assert same(a, b)
        # ... and the handle is as good as new
        r = Run()
        r.idx = idx
        h.begin()
        r.state, r.iterations = h.cycle(h.entry)
        r.after, r.kin = h.device(), h.sk.end()
    finally:
        h.close()
    assert r.iterations == base.iterations
    assert_same(r, base)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_calculator_device_loop_against_the_host_loop():
    from catint_amd.calculator import Calculator
    from tests.test_gpu_kinetics import e2e_model, e2e_transport
    out = {}
    for device_loop in (False, True):
        tp = e2e_transport()
        calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-8)
        calc.set_microkinetics(e2e_model(tp), site_density=2e-6, device_loop=device_loop)
        out[device_loop] = calc.run_scf_cycle(max_iter=200)
    host, dev = out[False], out[True]
    assert 'kinetic_calls' not in host and (dev['kinetic_calls'] > 0).all()
    assert len(dev['history']) < len(host['history']) == host['iterations']
    assert dev['iterations'] == host['iterations'] and np.array_equal(dev['mix'], host['mix'])
    assert dev['converged'].all() and host['converged'].all() and (dev['kinetic_status'] == 0).all()
    for k in ('surface_concentration', 'flux', 'current_density', 'coverage'):
        assert np.allclose(dev[k], host[k], rtol=1e-9, atol=0.0), k
    assert np.allclose(dev['accuracy'], host['accuracy'], rtol=1e-3, atol=1e-12)
    keys = ('surface_concentration', 'flux', 'current_density', 'coverage', 'accuracy', 'surface_pH', 'flux_scale')
    print('IDENTICAL device loop and host loop bit-identical: %s' % {k: bool(np.array_equal(dev[k], host[k])) for k in keys})
