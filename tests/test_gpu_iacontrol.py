"""libcatint_iacontrol on the device against tests/iacontrol_ref.py (the method of tests/test_gpu_drc.py).

Parity: every field on every case of tests/interact_cases.py, at the coverages of the fp64 interact reference (the terrace-and-step case
at the state that file reaches with its one stage), against the same formulas at 60 digits.  The tolerance is measured on the reference
side: per case and field, 10 x the worst error of control_fp64 against control_mp, floor 1e-13, in units of drc_scale (flux: of
flux_scale).
Bit for bit: with one site type and strength 0 the four old families, flux, flux_scale, residual and status are catdrc_solve's; the
normalised fields are the quotient of the raw ones; the view path against the host-surface path; any max_waves and batch size; repeated
lanes; outputs not asked for.  Behaviour: a poisoned point stays alone, a perturbed state (status 1), the dead row, the piecewise
response in its three regimes, dflux_dstrength against central differences of catia_solve.  Solver path:
PnpSolver.get_rate_control(InteractingModel) on the small Stern-wall handle of tests/test_gpu_interact.py.

Measured on an MI355X (printed by the tests): see DESIGN.md section 7t."""
import numpy as np
import pytest

from catint_amd import iacontrol          # fails without the feature
from catint_amd import _drc, _interact
from tests import drc_ref as DR
from tests import iacontrol_ref as CR
from tests import interact_cases as IC
from tests import interact_ref as IR
from tests import kinetics_cases as KC
from tests import kinetics_ref as KR
from tests.test_gpu_interact import kw_of, tiled
from tests.test_gpu_kinetics import open_handle, same

pytestmark = pytest.mark.gpu

ALL = list(iacontrol.FIELDS)
NORMALISED = (('dflux_drc', 'drc'), ('dflux_dG', 'tdrc'))
CACHE = {}


@pytest.fixture(scope='module')
def rc():
    with iacontrol.InteractingRateControl(0) as o:
        yield o


@pytest.fixture(scope='module')
def ia():
    with _interact.InteractingKinetics(0) as o:
        yield o


def references(name):
    """(case, theta of the fp64 interact reference, control_fp64, control_mp, errors of control_fp64) of a case, computed once"""
    if name not in CACHE:
        c = IC.case(name)
        theta = IC.fp64(name)['theta']
        fp = CR.control_fp64(c.tables, c.phiM, c.csurf, c.phi_surface, theta, **c.kw)
        ref = CR.control_mp(c.tables, c.phiM, c.csurf, c.phi_surface, theta, **c.kw)
        CACHE[name] = (c, theta, fp, ref, CR.errors(fp, ref, fp))
    return CACHE[name]


def run(rc, case, theta, n=None, idx=None, fields=ALL, **kw):
    pm, cs, ps = (case.phiM, case.csurf, case.phi_surface) if n is None else tiled(case, n)
    th = theta if n is None else theta[np.arange(n) % len(theta)]
    if idx is not None:
        pm, cs, ps, th = pm[idx], cs[idx], ps[idx], th[idx]
    args = kw_of(case)
    args.update(kw)
    out = rc.solve(None, case.tables, pm, th, csurf=cs, phi_surface=ps, fields=fields, **args)
    assert rc.last_kernel == 'catic::control_kernel' and rc.last_kernel_ms > 0.0
    return out


def quotients(out, tables):
    """the normalised fields as the IEEE quotients of the raw outputs beside them, exactly 0 for a species the mechanism does not touch"""
    idle = ~(np.asarray(tables['nu']) != 0.0).any(axis=0)
    want = {}
    with np.errstate(divide='ignore', invalid='ignore'):
        for raw, norm in NORMALISED:
            want[norm] = out[raw] / out['flux'][:, None, :]
            want[norm][:, :, idle] = 0.0
        want['strength_control'] = float(tables.get('strength', 1.0)) * (out['dflux_dstrength'] / out['flux'])
        want['strength_control'][:, idle] = 0.0
    return want, idle


# ---- parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', IC.CASE_NAMES)
def test_parity_with_60_digits(rc, name):
    case, theta, fp, ref, err_fp = references(name)
    out = run(rc, case, theta)
    assert (out['status'] == 0).all(), out['status']
    assert np.allclose(out['residual'], fp['residual'], rtol=0, atol=1e-13) and out['residual'].max() <= 1e-12
    err = CR.errors(out, ref, fp)
    line, worst = [], {}
    for q, e in err.items():
        tol = max(10.0 * err_fp[q].max(), 1e-13)
        worst[q] = e.max() / tol
        line.append('%s %.1e / %.1e' % (q, e.max(), tol))
    print(name, 'device error / tolerance:', '; '.join(line))
    for q, ratio in worst.items():
        assert ratio <= 1.0, (name, q, ratio)
    assert np.allclose(out['flux_scale'], fp['flux_scale'], rtol=1e-11, atol=0)
    want, idle = quotients(out, case.tables)
    for k, v in want.items():
        assert np.array_equal(out[k], v, equal_nan=True), k
    if idle.any():
        for k in want:
            assert (out[k][..., idle] == 0.0).all() and not np.signbit(out[k][..., idle]).any(), k


# ---- bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['co2r_two_site', 'random_S8'])
def test_one_site_type_at_strength_0_has_the_bits_of_catdrc_solve(rc, name):
    case = KC.case(name)
    theta = KR.solve_fp64(case.tables, case.phiM, case.csurf, case.phi_surface, sens=False, **case.kw)['theta']
    T = len(case.tables['site_count'])
    pm, cs, ps = tiled(case, 70)
    th = theta[np.arange(70) % len(theta)]
    with _drc.RateControl(0) as old:
        want = old.solve(None, case.tables, pm, th, csurf=cs, phi_surface=ps, fields=list(_drc.FIELDS), **kw_of(case))
    assert (want['status'] == 0).all()
    for more in ({}, dict(eps=np.full((T - 1, T - 1), 2.0), eps_ts=np.ones((len(case.tables['lnA']), T - 1))),
                 dict(response='piecewise', cutoff=np.array([0.25]), smoothing=np.array([0.05]))):
        tab = dict(case.tables, site_of=np.zeros(T, np.int32), site_fraction=np.ones(1), eps=np.zeros((T - 1, T - 1)), strength=0.0)
        tab.update(more)
        got = rc.solve(None, tab, pm, th, csurf=cs, phi_surface=ps, fields=ALL, **kw_of(case))
        assert rc.last_kernel == 'catic::control_kernel'
        for k in list(_drc.FIELDS) + ['residual', 'status']:
            assert np.array_equal(got[k], want[k], equal_nan=True), (sorted(more), k)
        assert (got['strength_control'] == 0.0).all()


@pytest.mark.parametrize('name', ['co2r_two_site_weak', 'random_S6_G3_piecewise'])
def test_any_number_of_waves_gives_the_same_bits_and_a_point_its_own(rc, name):
    """130 points = 64 + 64 + 2: the case's points tiled.  One wave, three waves and the library's choice; every point equals the
    point of the plain run of the case, wherever it stands"""
    case, theta, _, _, _ = references(name)
    n0 = len(case.phiM)
    plain = run(rc, case, theta)
    base = run(rc, case, theta, 130)
    for waves in (1, 3):
        same(base, run(rc, case, theta, 130, max_waves=waves))
    for k in base:
        assert np.array_equal(base[k], plain[k][np.arange(130) % n0], equal_nan=True), k
    for n in (1, 63, 65):
        got = run(rc, case, theta, n)
        for k in got:
            assert np.array_equal(got[k], base[k][:n], equal_nan=True), (n, k)


@pytest.fixture(scope='module')
def handle():
    phis = np.linspace(-0.12, 0.06, 130)
    with open_handle(phis) as s:
        assert (s.solve_stationary() == 0).all()
        yield s, phis


def test_the_solver_path_the_view_path_and_repeated_lanes(rc, handle, monkeypatch):
    s, phis = handle
    model = IC.terrace_step_model()
    seen = []

    plain = iacontrol.InteractingRateControl

    class Watched(plain):
        def __exit__(self, *exc):
            seen.append((self.last_kernel, self.last_kernel_ms))
            return plain.__exit__(self, *exc)
    monkeypatch.setattr(iacontrol, 'InteractingRateControl', Watched)
    before = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    cs, vs, _ = s.get_surface()
    kin = s.get_kinetics(model, fields=('theta',), ramp=3)
    assert (kin['status'] == 0).all()
    theta = kin['theta']
    from_view = s.get_rate_control(model, theta=theta, fields=ALL)
    assert seen[-1][0] == 'catic::control_kernel' and seen[-1][1] > 0.0
    # the context was opened for the call and closed after it: no attribute of the solver holds one, and no satellite was opened for it
    assert not [k for k, v in vars(s).items() if isinstance(v, plain)]
    assert s._rate_control is None and len(s.SATELLITES) == 13
    from_host = s.get_rate_control(model, theta=theta, csurf=cs, phi_surface=vs, fields=ALL)
    alone = rc.solve(None, model.tables(), phis, theta, csurf=cs, phi_surface=vs, potential_drop='stern', stern_capacitance=0.2, phi_pzc=0.0, fields=ALL)
    same(from_view, from_host)
    same(from_view, alone)
    # (CO is in the solution here and its desorption is equilibrated: the CO flux is the rounding of gross rates 1e16 times larger and
    # may be exactly 0, where the header gives the normalised entries as inf or NaN; the raw fields are finite everywhere)
    assert (from_view['status'] == 0).all() and from_view['dy_drc'].shape == (130, 7, 7)
    for k in CR.RAW + CR.DY + ('flux', 'flux_scale'):
        assert np.isfinite(from_view[k]).all(), k
    moving = from_view['flux'] != 0.0
    assert np.isfinite(from_view['drc'].transpose(0, 2, 1)[moving]).all() and np.isfinite(from_view['strength_control'][moving]).all()
    assert from_view['tdrc'].shape == (130, 5, 3) and from_view['strength_control'].shape == (130, 3)
    # theta=None: the coverages of get_kinetics at the same arguments (the ramp of the solver's default from the uniform start)
    auto = s.get_rate_control(model, fields=ALL)
    assert (auto['status'] == 0).all()
    assert (np.abs(auto['dflux_drc'] - from_view['dflux_drc']) <= 1e-6 * np.abs(from_view['dflux_drc']) + 1e-9 * from_view['flux_scale'][:, None, :]).all()
    assert sorted(s.get_rate_control(model, theta=theta)) == sorted(iacontrol.DEFAULT_FIELDS + ('status', 'residual'))
    # lane subsets and permutations with repeats, one wave, through the view
    rng = np.random.RandomState(9)
    for lanes in (rng.permutation(130), np.array([129, 0, 0, 64, 63, 65, 129]), np.array([33])):
        got = s.get_rate_control(model, theta=theta[lanes], lanes=lanes, fields=ALL, max_waves=1)
        for k in got:
            assert np.array_equal(got[k], from_view[k][lanes], equal_nan=True), k
    # the handle's state, status and counters are only read
    after = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_apparent_coefficients_from_the_solver_s_own_kinetics_and_coupling(handle):
    s, phis = handle
    model = IC.co2r_model('two_site', 0.3, 0.15)
    lam = model.tables()['strength']
    lanes = np.array([129, 3, 3, 40])
    kin = s.get_kinetics(model, lanes=lanes, fields=('theta', 'flux', 'dflux_dc', 'dflux_dphi'))
    cp = s.get_coupling(None, kin, rf=1.5, lanes=lanes, fields=('T_c', 'T_phi'))
    assert (kin['status'] == 0).all() and (cp['status'] == 0).all()
    plain = s.get_rate_control(model, theta=kin['theta'], lanes=lanes, fields=ALL)
    got = s.get_rate_control(model, theta=kin['theta'], lanes=lanes, fields=ALL, kin=kin, coupling=cp, rf=1.5)
    assert set(got) == set(plain) | {'dflux_drc_apparent', 'dflux_dG_apparent', 'drc_apparent', 'tdrc_apparent', 'dflux_dstrength_apparent',
                                     'strength_control_apparent'}
    same(plain, got, keys=plain)
    for i in range(len(lanes)):
        K = (kin['dflux_dc'][i], kin['dflux_dphi'][i][:, 1], cp['T_c'][i], cp['T_phi'][i])
        for raw in ('dflux_drc', 'dflux_dG'):
            assert np.allclose(got[raw + '_apparent'][i], DR.apparent(got[raw][i], *K, rf=1.5), rtol=1e-12, atol=0), (raw, i)
        assert np.allclose(got['dflux_dstrength_apparent'][i], DR.apparent(got['dflux_dstrength'][i][None, :], *K, rf=1.5)[0], rtol=1e-12, atol=0)
    for raw, norm in NORMALISED:
        assert np.array_equal(got[norm + '_apparent'], got[raw + '_apparent'] / (1.5 * got['flux'])[:, None, :])
    assert np.array_equal(got['strength_control_apparent'], lam * (got['dflux_dstrength_apparent'] / (1.5 * got['flux'])))
    assert np.isfinite(got['strength_control_apparent']).all()
    assert np.array_equal(got['drc_apparent'][1], got['drc_apparent'][2])          # the repeated lane
    few = s.get_rate_control(model, theta=kin['theta'], lanes=lanes, fields=('strength_control',), kin=kin, coupling=cp, rf=1.5)
    assert sorted(few) == sorted(['dflux_dG_apparent', 'dflux_drc_apparent', 'drc_apparent', 'tdrc_apparent', 'dflux_dstrength_apparent',
                                  'strength_control_apparent', 'strength_control', 'residual', 'status'])
    assert np.array_equal(few['strength_control_apparent'], got['strength_control_apparent'])


def test_outputs_not_asked_for_keep_their_sentinel(rc):
    case, theta, _, _, _ = references('random_S5_G2_piecewise')
    N, G, S, R = IR.shape(case.tables)
    out = {k: np.full((3,) + iacontrol.FIELDS[k](N, G + S - 1, R, G), 7.0) for k in ALL}
    out.update(status=np.full(3, 77, np.int32), residual=np.full(3, 7.0))
    two = {k: v[:2] for k, v in out.items()}          # two points of room for three: the third is not the library's to touch
    full = run(rc, case, theta, idx=np.array([0, 1]))
    run(rc, case, theta, idx=np.array([0, 1]), out=two)
    for k, v in out.items():
        assert (v[2] == (77 if v.dtype == np.int32 else 7.0)).all() and np.array_equal(v[:2], full[k]), k
    only = run(rc, case, theta, idx=np.array([0, 1]), fields=['strength_control'])
    assert sorted(only) == ['residual', 'status', 'strength_control'] and np.array_equal(only['strength_control'], full['strength_control'])
    # a family computed for its normalised field alone, each field alone and a few subsets give the bits of the full call
    for fields in [[k] for k in ALL] + [['dy_dstrength', 'tdrc'], ['dflux_dlnkb', 'dy_drc', 'flux'], ['drc', 'dflux_dstrength', 'flux_scale']]:
        got = run(rc, case, theta, idx=np.array([0, 1]), fields=fields)
        assert sorted(got) == sorted(fields + ['residual', 'status'])
        for k in fields:
            assert np.array_equal(got[k], full[k]), (fields, k)


# ---- behaviour ---------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_input_shows_in_its_point_only(rc):
    case, theta, _, _, _ = references('random_S3_G3_linear')
    n = 65
    clean = run(rc, case, theta, n)
    assert (clean['status'] == 0).all()
    th = theta[np.arange(n) % len(theta)].copy()
    th[64, 2] = np.nan
    pm, cs, ps = tiled(case, n)
    got = rc.solve(None, case.tables, pm, th, csurf=cs, phi_surface=ps, fields=ALL, **kw_of(case))
    assert got['status'][64] == 2 and (got['status'][:64] == 0).all() and np.isnan(got['residual'][64])
    for k in ALL:
        assert np.isnan(got[k][64]).all() and np.array_equal(got[k][:64], clean[k][:64]), k
    cs2 = cs.copy()
    cs2[3, 0] = np.inf
    got = rc.solve(None, case.tables, pm, theta[np.arange(n) % len(theta)], csurf=cs2, phi_surface=ps, fields=ALL, **kw_of(case))
    assert got['status'][3] == 2 and (np.delete(got['status'], 3) == 0).all()
    for k in ALL:
        assert np.isnan(got[k][3]).all() and np.array_equal(np.delete(got[k], 3, axis=0), np.delete(clean[k], 3, axis=0)), k


def test_a_lane_the_handle_did_not_solve_reports_2_and_is_alone():
    model = IC.co2r_model('one_site', 0.3, 0.15)
    results = []
    for phis in (np.zeros(5), np.array([0.0, 0.0, -0.8, 0.0, 0.0])):
        with open_handle(phis, maxit=1) as s:
            st = s.solve_stationary()
            theta = s.get_kinetics(model, fields=('theta',), phiM=np.full(5, -0.6), ramp=2)['theta']
            theta[2] = theta[0]          # (the unsolved lane has no coverages of its own: the status must come from the lane)
            results.append((st, s.get_rate_control(model, theta=theta, fields=ALL, phiM=np.full(5, -0.6))))
    (st0, clean), (st1, got) = results
    assert (st0 == 0).all() and st1[2] != 0 and (np.delete(st1, 2) == 0).all()
    assert (clean['status'] == 0).all() and got['status'][2] == 2 and (np.delete(got['status'], 2) == 0).all()
    for k in ALL:
        assert np.isnan(got[k][2]).all(), k
        assert np.array_equal(np.delete(got[k], 2, axis=0), np.delete(clean[k], 2, axis=0)), k


def test_an_adsorbate_nothing_produces_keeps_its_dead_row(rc):
    """A + * <-> A* with a self-interaction, and a second adsorbate no step touches: its row is the identity, every derivative of its
    coverage is 0"""
    from tests.test_kinetics_abi import tables
    dead = tables([[1, 1, 0, 0]], [[0, 0, 1, 0]], [[-1.0]], [1.0, 1.0, 1.0], [[-1.0, 0, 0, 0]])
    dead = dict(dead, site_of=np.zeros(3, np.int32), site_fraction=np.ones(1), eps=np.array([[3.0, 1.0], [1.0, 2.0]]), strength=1.0)
    pm, cs, ps = np.zeros(3), np.array([[0.5], [2.0], [1e-3]]), np.zeros(3)
    kin = IR.solve_fp64(dead, pm, cs, ps, sens=False)
    assert (kin['status'] == 0).all() and (kin['y'][:, 2] == IR.MIN_LOG).all()
    fp = CR.control_fp64(dead, pm, cs, ps, kin['theta'])
    out = rc.solve(None, dead, pm, kin['theta'], csurf=cs, phi_surface=ps, fields=ALL)
    assert (out['status'] == 0).all() and out['residual'].max() <= 1e-14
    assert (out['dy_drc'][:, :, 2] == 0.0).all() and (out['dflux_dG'][:, 1] == 0.0).all() and (out['dy_dstrength'][:, 2] == 0.0).all()
    for k in CR.RAW + CR.DY:
        # an adsorption equilibrium: every flux derivative is a difference of equal terms; in units of those terms
        assert (np.abs(out[k] - fp[k]) <= 1e-13 * fp['drc_scale'][k] + 1e-300).all(), k
    # the coverage falls with the strength of its own repulsion
    assert (out['dy_dstrength'][:, 1] < 0.0).all() and (out['dy_dstrength'][:, 0] > 0.0).all()


def test_a_perturbed_state_reports_1_and_returns_its_numbers(rc):
    case, theta, fp, _, _ = references('co2r_one_site_weak')
    th = theta.copy()
    th[::2, 1] *= 1.0 + 1e-4          # every other point: one coverage off by 1e-4
    out = run(rc, case, th)
    off = np.arange(len(th)) % 2 == 0
    # (a coverage of 1e-58 that is off by 1e-4 moves no residual: status 1 where the residual says so, and only there)
    assert np.array_equal(out['status'], np.where(out['residual'] > 1e-8, 1, 0)) and (out['status'][~off] == 0).all()
    assert (out['status'][off] == 1).sum() >= 10 and out['residual'][out['status'] == 1].min() > 1e-8
    clean = run(rc, case, theta)
    for k in ALL:
        assert np.isfinite(out[k]).all() and np.array_equal(out[k][~off], clean[k][~off]), k
    # the restatement at the same perturbed state agrees: the numbers are the formulas', not a flag's
    ref = CR.control_fp64(case.tables, case.phiM, case.csurf, case.phi_surface, th, **case.kw)
    assert np.array_equal(ref['status'], out['status'])
    for k in ('dflux_drc', 'dflux_dstrength'):
        assert (np.abs(out[k] - ref[k]) <= 1e-11 * ref['drc_scale'][k] + 1e-300).all(), k
    # a looser residual_tol accepts them
    assert (run(rc, case, th, residual_tol=1.0)['status'] == 0).all()


def test_the_piecewise_response_in_its_three_regimes(rc, monkeypatch):
    """random_S6_G3_piecewise holds a site type below its cutoff (f = 0), one inside the smoothing interval and one beyond it; where
    f' is not 0 it is part of the Jacobian: the restatement without it misses the device by far more than the tolerance"""
    name = 'random_S6_G3_piecewise'
    case, theta, fp, ref, err_fp = references(name)
    t = IR._arrays(case.tables)
    regimes = set()
    curved = np.zeros(len(theta), bool)
    for i, th in enumerate(theta):
        crowd = np.zeros(t['G'])
        for k in range(t['G'], t['T']):
            crowd[t['site_of'][k]] += t['ns'][k] * th[k]
        d = crowd / t['x'] - t['cutoff']
        kinds = ['below' if v <= -s else ('inside' if v < s else 'beyond') for v, s in zip(d, t['smooth'])]
        regimes |= set(kinds)
        curved[i] = 'below' != kinds[0] or 'below' != kinds[1] or 'below' != kinds[2]
    assert regimes == {'below', 'inside', 'beyond'} and curved.any()
    out = run(rc, case, theta)
    err = CR.errors(out, ref, fp)
    for q in ('dflux_drc', 'dflux_dG', 'dflux_dstrength', 'dy_drc', 'dy_dstrength'):
        assert err[q].max() <= max(10.0 * err_fp[q].max(), 1e-13), q
    plain = IR.response
    monkeypatch.setattr(IR, 'response', lambda tt, crowd: (plain(tt, crowd)[0], np.zeros(tt['G'])))
    without = CR.control_fp64(case.tables, case.phiM, case.csurf, case.phi_surface, theta, **case.kw)
    gap = np.abs(out['dy_dstrength'] - without['dy_dstrength']).max(axis=1)
    print(name, "|dy_dstrength - the restatement without f'| per point", gap, 'regimes', sorted(regimes))
    assert (gap[curved] > 1e-6).any()


@pytest.mark.parametrize('name', ['co2r_two_site_weak', 'random_S5_G2_piecewise'])
def test_dflux_dstrength_against_central_differences_of_catia_solve(rc, ia, name):
    """(flux(strength (1 + h)) - flux(strength (1 - h))) / (2 h strength), h = 1e-4, both solves on the device from the case's
    coverages.  The bound: 10 x what the same quotient of interact_ref.solve_fp64 misses the restatement's derivative by, in units of
    flux_scale -- the truncation of the difference and what a flux converged to tol leaves of a difference over 2 h."""
    case, theta, fp, _, _ = references(name)
    lam, h = float(case.tables['strength']), 1e-4
    out = run(rc, case, theta, fields=['dflux_dstrength', 'flux_scale'])
    dev, ref = [], []
    for sign in (+1.0, -1.0):
        s = lam * (1.0 + sign * h)
        got = ia.solve(None, case.tables, case.phiM, csurf=case.csurf, phi_surface=case.phi_surface, fields=['flux'], theta_guess=theta, ramp=1,
                       strength=s, **kw_of(case))
        assert (got['status'] == 0).all()
        dev.append(got['flux'])
        ref.append(IR.solve_fp64(case.tables, case.phiM, case.csurf, case.phi_surface, theta_guess=theta, ramp=1, strength=s, sens=False,
                                 **case.kw)['flux'])
    scale = np.where(fp['flux_scale'] > 0, fp['flux_scale'], 1.0)
    bound = 10.0 * (np.abs((ref[0] - ref[1]) / (2.0 * h * lam) - fp['dflux_dstrength']) / scale).max()
    gap = (np.abs((dev[0] - dev[1]) / (2.0 * h * lam) - out['dflux_dstrength']) / scale).max()
    print(name, 'dflux_dstrength against central differences of catia_solve, in units of flux_scale: %.2e, bound %.2e' % (gap, bound))
    print(name, 'largest |dflux_dstrength| / flux_scale %.2e' % (np.abs(out['dflux_dstrength']) / scale).max())
    assert gap <= bound, (gap, bound)
