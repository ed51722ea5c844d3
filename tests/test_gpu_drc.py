"""libcatint_drc on the device against tests/drc_ref.py (the method of tests/test_gpu_kinetics.py).

Parity: every field on every case of tests/kinetics_cases.py, at the coverages of the fp64 kinetics reference, against the same formulas
at 60 digits.  The tolerance is measured on the reference side: per case and field, 10 x the worst error of control_fp64 against
control_mp, floor 1e-13, in units of drc_scale (flux: of flux_scale).
Bit for bit: the normalised fields are the quotient of the raw ones; the view path against the host-surface path; any max_waves and
batch size; repeated lanes; outputs not asked for; a poisoned point stays alone.  Behaviour: the dead row, a perturbed state (status
1), I3 against the kinetics library's own dflux_dphi.  End to end: Calculator.set_microkinetics(scf='newton', rate_control=True) on the
small Stern-wall case of tests/test_gpu_kinetics.py; the apparent degree of rate control of the one transition state for the CO flux
against central differences of converged runs with that transition state shifted.

Measured on an MI355X (printed by the tests): see DESIGN.md section 7k."""
import numpy as np
import pytest

from catint_amd import _drc, _kinetics          # fails without the feature
from tests import drc_ref as DR
from tests import kinetics_cases as KC
from tests import kinetics_ref as KR
from tests.test_gpu_kinetics import E2E_PHIS, e2e_transport, kw_of, open_handle, tiled

pytestmark = pytest.mark.gpu

ALL = list(_drc.FIELDS)
CACHE = {}


@pytest.fixture(scope='module')
def rc():
    with _drc.RateControl(0) as o:
        yield o


@pytest.fixture(scope='module')
def ks():
    with _kinetics.KineticsSolver(0) as o:
        yield o


def references(name):
    """(case, theta of the fp64 kinetics reference, control_fp64, control_mp, errors of control_fp64) of a case, computed once"""
    if name not in CACHE:
        c = KC.case(name)
        theta = KC.references(name)[0]['theta']
        fp = DR.control_fp64(c.tables, c.phiM, c.csurf, c.phi_surface, theta, **c.kw)
        ref = DR.control_mp(c.tables, c.phiM, c.csurf, c.phi_surface, theta, **c.kw)
        CACHE[name] = (c, theta, fp, ref, DR.errors(fp, ref, fp))
    return CACHE[name]


def run(rc, case, theta, n=None, idx=None, fields=ALL, **kw):
    pm, cs, ps = (case.phiM, case.csurf, case.phi_surface) if n is None else tiled(case, n)
    th = theta if n is None else theta[np.arange(n) % len(theta)]
    if idx is not None:
        pm, cs, ps, th = pm[idx], cs[idx], ps[idx], th[idx]
    args = kw_of(case)
    args.update(kw)
    out = rc.solve(None, case.tables, pm, th, csurf=cs, phi_surface=ps, fields=fields, **args)
    assert rc.last_kernel == 'catdrc::control_kernel' and rc.last_kernel_ms > 0.0
    return out


def same(a, b, keys=None):
    for k in (keys or a):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', KC.CASE_NAMES)
def test_parity_with_60_digits(rc, name):
    case, theta, fp, ref, err_fp = references(name)
    out = run(rc, case, theta)
    assert (out['status'] == 0).all(), out['status']
    assert np.allclose(out['residual'], fp['residual'], rtol=0, atol=1e-13) and out['residual'].max() <= 1e-12
    err = DR.errors(out, ref, fp)
    line, worst = [], {}
    for q, e in err.items():
        tol = max(10.0 * err_fp[q].max(), 1e-13)
        worst[q] = e.max() / tol
        line.append('%s %.1e / %.1e' % (q, e.max(), tol))
    print(name, 'device error / tolerance:', '; '.join(line))
    for q, ratio in worst.items():
        assert ratio <= 1.0, (name, q, ratio)
    assert np.allclose(out['flux_scale'], fp['flux_scale'], rtol=1e-11, atol=0)
    # the normalised fields are the IEEE quotient of the raw outputs beside them, exactly 0 for a species the mechanism does not touch
    idle = ~(np.asarray(case.tables['nu']) != 0.0).any(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        for raw, norm in (('dflux_drc', 'drc'), ('dflux_dG', 'tdrc')):
            want = out[raw] / out['flux'][:, None, :]
            want[:, :, idle] = 0.0
            assert np.array_equal(out[norm], want, equal_nan=True), norm
    if idle.any():
        assert (out['drc'][:, :, idle] == 0.0).all() and not np.signbit(out['drc'][:, :, idle]).any()


# ---- bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['co2r_two_site', 'random_S8'])
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
    phis = np.linspace(-0.12, 0.06, 70)
    with open_handle(phis) as s:
        assert (s.solve_stationary() == 0).all()
        yield s, phis


def test_the_view_path_gives_the_bits_of_the_host_surface_path_and_lanes_repeat(rc, handle):
    s, phis = handle
    model = KC.co2r_model('two_site')
    before = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    cs, vs, _ = s.get_surface()
    theta = s.get_kinetics(model, fields=('theta',))['theta']
    from_view = s.get_rate_control(model, theta=theta, fields=ALL)
    assert s._rate_control.last_kernel == 'catdrc::control_kernel'
    from_host = s.get_rate_control(model, theta=theta, csurf=cs, phi_surface=vs, fields=ALL)
    alone = rc.solve(None, model.tables(), phis, theta, csurf=cs, phi_surface=vs, potential_drop='stern', stern_capacitance=0.2, phi_pzc=0.0, fields=ALL)
    same(from_view, from_host)
    same(from_view, alone)
    assert (from_view['status'] == 0).all() and np.isfinite(from_view['drc']).all()
    # theta=None: the coverages of get_kinetics at the same arguments
    same(from_view, s.get_rate_control(model, fields=ALL))
    assert sorted(s.get_rate_control(model)) == sorted(_drc.DEFAULT_FIELDS + ('status', 'residual'))
    # lane subsets and permutations with repeats, one wave, through the view
    rng = np.random.RandomState(9)
    for lanes in (rng.permutation(70), np.array([69, 0, 0, 64, 63, 65, 69]), np.array([33])):
        got = s.get_rate_control(model, theta=theta[lanes], lanes=lanes, fields=ALL, max_waves=1)
        for k in got:
            assert np.array_equal(got[k], from_view[k][lanes], equal_nan=True), k
    # the handle's state, status and counters are only read
    after = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_apparent_coefficients_from_the_solver_s_own_kinetics_and_coupling(handle):
    """get_rate_control(kin=, coupling=): the apparent derivatives are M^-1 (rf dflux) with the M of get_coupling's inputs, per point;
    the intrinsic fields keep their bits; the fields asked for alone come back"""
    s, phis = handle
    model = KC.co2r_model('two_site')
    lanes = np.array([69, 3, 3, 40])
    kin = s.get_kinetics(model, lanes=lanes, fields=('theta', 'flux', 'dflux_dc', 'dflux_dphi'))
    cp = s.get_coupling(None, kin, rf=1.5, lanes=lanes, fields=('T_c', 'T_phi'))
    assert (kin['status'] == 0).all() and (cp['status'] == 0).all()
    plain = s.get_rate_control(model, theta=kin['theta'], lanes=lanes, fields=ALL)
    got = s.get_rate_control(model, theta=kin['theta'], lanes=lanes, fields=ALL, kin=kin, coupling=cp, rf=1.5)
    assert set(got) == set(plain) | {'dflux_drc_apparent', 'dflux_dG_apparent', 'drc_apparent', 'tdrc_apparent'}
    same(plain, got, keys=plain)
    for raw, norm in (('dflux_drc', 'drc'), ('dflux_dG', 'tdrc')):
        for i in range(len(lanes)):
            want = DR.apparent(got[raw][i], kin['dflux_dc'][i], kin['dflux_dphi'][i][:, 1], cp['T_c'][i], cp['T_phi'][i], rf=1.5)
            assert np.allclose(got[raw + '_apparent'][i], want, rtol=1e-12, atol=0), (raw, i)
        assert np.array_equal(got[norm + '_apparent'], got[raw + '_apparent'] / (1.5 * got['flux'])[:, None, :])
        assert np.isfinite(got[norm + '_apparent']).all() and not np.allclose(got[norm + '_apparent'], got[norm], rtol=1e-6)
    assert np.array_equal(got['drc_apparent'][1], got['drc_apparent'][2])          # the repeated lane
    few = s.get_rate_control(model, theta=kin['theta'], lanes=lanes, fields=('drc',), kin=kin, coupling=cp, rf=1.5)
    assert sorted(few) == ['dflux_dG_apparent', 'dflux_drc_apparent', 'drc', 'drc_apparent', 'residual', 'status', 'tdrc_apparent']
    assert np.array_equal(few['drc_apparent'], got['drc_apparent'])
    with pytest.raises(ValueError, match='come together'):
        s.get_rate_control(model, theta=kin['theta'], lanes=lanes, kin=kin)


def test_outputs_not_asked_for_keep_their_sentinel(rc):
    case, theta, _, _, _ = references('random_S5')
    N, S, R = KR.shape(case.tables)
    out = {k: np.full((3,) + _drc.FIELDS[k](N, S, R), 7.0) for k in ALL}
    out.update(status=np.full(3, 77, np.int32), residual=np.full(3, 7.0))
    two = {k: v[:2] for k, v in out.items()}          # two points of room for three: the third is not the library's to touch
    full = run(rc, case, theta, idx=np.array([0, 1]))
    run(rc, case, theta, idx=np.array([0, 1]), out=two)
    for k, v in out.items():
        assert (v[2] == (77 if v.dtype == np.int32 else 7.0)).all() and np.array_equal(v[:2], full[k]), k
    only = run(rc, case, theta, idx=np.array([0, 1]), fields=['tdrc'])
    assert sorted(only) == ['residual', 'status', 'tdrc'] and np.array_equal(only['tdrc'], full['tdrc'])
    # a family computed for its normalised field alone, and each family alone, give the bits of the full call
    for k in ALL:
        assert np.array_equal(run(rc, case, theta, idx=np.array([0, 1]), fields=[k])[k], full[k]), k


# ---- behaviour ---------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_input_shows_in_its_point_only(rc):
    case, theta, _, _, _ = references('random_S4')
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


def test_an_adsorbate_nothing_produces_keeps_its_dead_row(rc):
    """A + * <-> A*, and a second adsorbate no step touches: its row is the identity, every derivative of its coverage is 0"""
    from tests.test_kinetics_abi import tables
    dead = tables([[1, 1, 0, 0]], [[0, 0, 1, 0]], [[-1.0]], [1.0, 1.0, 1.0], [[-1.0, 0, 0, 0]])
    pm, cs, ps = np.zeros(3), np.array([[0.5], [2.0], [1e-3]]), np.zeros(3)
    kin = KR.solve_fp64(dead, pm, cs, ps, sens=False)
    assert (kin['status'] == 0).all() and (kin['y'][:, 2] == KR.MIN_LOG).all()
    fp = DR.control_fp64(dead, pm, cs, ps, kin['theta'])
    out = rc.solve(None, dead, pm, kin['theta'], csurf=cs, phi_surface=ps, fields=ALL)
    assert (out['status'] == 0).all() and out['residual'].max() <= 1e-14
    assert (out['dy_drc'][:, :, 2] == 0.0).all() and (out['dflux_dG'][:, 1] == 0.0).all()
    for k in DR.RAW + ('dy_drc',):
        # an adsorption equilibrium: every flux derivative is a difference of equal terms; in units of those terms
        assert (np.abs(out[k] - fp[k]) <= 1e-13 * fp['drc_scale'][k] + 1e-300).all(), k


def test_a_perturbed_state_reports_1_and_returns_its_numbers(rc):
    case, theta, fp, _, _ = references('co2r_one_site')
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
    ref = DR.control_fp64(case.tables, case.phiM, case.csurf, case.phi_surface, th, **case.kw)
    assert np.array_equal(ref['status'], out['status'])
    assert (np.abs(out['dflux_drc'] - ref['dflux_drc']) <= 1e-11 * ref['drc_scale']['dflux_drc'] + 1e-300).all()
    # a looser residual_tol accepts them
    assert (run(rc, case, th, residual_tol=1.0)['status'] == 0).all()


@pytest.mark.parametrize('name', ['co2r_two_site', 'random_S7'])
def test_chain_rule_against_the_device_s_own_dflux_dphi(rc, ks, name):
    """I3 with both sides from the device: sum_r dflux_dlnkf[r] dlf_r + dflux_dlnkb[r] dlb_r against catkin's dflux_dphi, within the sum
    of the two parity tolerances, each in units of its own term sum"""
    case, _, fp, _, err_fp = references(name)
    kin_fp, _, kin_err = KC.references(name)
    kin = ks.solve(None, case.tables, case.phiM, csurf=case.csurf, phi_surface=case.phi_surface, fields=('theta', 'dflux_dphi'), **kw_of(case))
    out = run(rc, case, kin['theta'], fields=['dflux_dlnkf', 'dflux_dlnkb'])
    t = KR._arrays(case.tables)
    N, R = t['N'], t['R']
    tol_d = max(10.0 * max(err_fp['dflux_dlnkf'].max(), err_fp['dflux_dlnkb'].max()), 1e-13)
    tol_k = max(10.0 * kin_err['dflux_dphi'].max(), 1e-13)
    worst = 0.0
    for i in range(len(case.phiM)):
        V, sg = KR.potential_and_charge(case.phiM[i], case.phi_surface[i], case.kw['w'], case.kw['CS'], case.kw['phi_pzc'], None)
        br = KR.rate_constants(t, V, sg, np.zeros((R, 2)))[2]
        for q, (dV, ds) in enumerate(((1.0, case.kw['CS']), (-1.0 if case.kw['w'] else 0.0, -case.kw['CS']))):
            dlf, dlb = KR.slopes(t, sg, br, dV, ds)
            chain_rule = dlf @ out['dflux_dlnkf'][i] + dlb @ out['dflux_dlnkb'][i]
            bound = tol_d * (np.abs(dlf) @ fp['drc_scale']['dflux_dlnkf'][i] + np.abs(dlb) @ fp['drc_scale']['dflux_dlnkb'][i]) \
                + tol_k * kin_fp['dflux_scale'][i][:, N + q]
            gap = np.abs(chain_rule - kin['dflux_dphi'][i][:, q])
            worst = max(worst, (gap / np.where(bound > 0, bound, 1.0))[bound > 0].max(initial=0.0))
            assert (gap <= bound).all(), (i, q, gap, bound)
    print(name, 'I3 on the device: worst gap / (sum of the two tolerances) %.2f' % worst)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
H_EV = 2e-3
TAU = 2e-9


def e2e_model_shifted(tp, d_ts=0.0):
    """e2e_model of tests/test_gpu_kinetics.py with the energy of its one transition state moved by d_ts eV"""
    from catint_amd.microkinetics import MeanFieldModel
    return MeanFieldModel(list(tp.species.keys()), {'CO2': 1}, ['CO2_g + *_t <-> CO2*_t', 'CO2*_t + 2ele_g <-> TS_t <-> CO_g + *_t; beta=0.5'],
                          {'CO2': (0.10, 0.004, 0.0), 'TS': (0.62 + d_ts, 0.004, 0.0)}, solution_energies={'CO': -0.2}, site_density=2e-6)


def newton_run(d_ts=0.0, rate_control=False):
    from catint_amd.calculator import Calculator
    tp = e2e_transport()
    calc = Calculator(transport=tp, calc='comsol', tau_scf=TAU)
    model = e2e_model_shifted(tp, d_ts)
    calc.set_microkinetics(model, site_density=2e-6, scf='newton', rate_control=rate_control)
    out = calc.run_scf_cycle()
    assert out['converged'].all() and not out['failed'].any()
    return out, tp, model


def test_apparent_rate_control_against_shifted_transition_states_end_to_end():
    """tolerance = 10 |FD(h) - FD(h/2)| + 10 tau_scf / (h / kT), h = 2e-3 eV: the differences' own truncation, and what a flux converged
    to tau_scf leaves of a difference over h / kT"""
    base, tp, model = newton_run(rate_control=True)
    plain, tp0, _ = newton_run()
    assert 'rate_control' not in plain and 'rate_control' not in tp0.alldata[0]['system']
    assert np.array_equal(plain['flux'], base['flux'])          # the option changes nothing of the loop
    rcx = base['rate_control']
    assert set(rcx) == {'drc', 'tdrc', 'status', 'residual', 'kinetic_status', 'drc_apparent', 'tdrc_apparent', 'coupling_status'}
    assert (rcx['status'] == 0).all() and (rcx['kinetic_status'] == 0).all() and (rcx['coupling_status'] == 0).all()
    for i in range(8):
        got = tp.alldata[i]['system']['rate_control']
        assert np.array_equal(got['drc'], rcx['drc'][i]) and np.array_equal(got['drc_apparent'], rcx['drc_apparent'][i])
    names = list(tp.species.keys())
    co, co2, ts = names.index('CO'), names.index('CO2'), 1
    kT = model.kT
    # the transition state is the branch of Ga at the final state of every lane: the table shift moves ln kf and ln kb alike
    t = KR._arrays(dict(model.tables(), site_density=2e-6))
    vs = np.array([tp.alldata[i]['system']['surface_potential'] for i in range(8)])
    for i in range(8):
        V, sg = KR.potential_and_charge(E2E_PHIS[i], vs[i], 1, 0.2, 0.1, None)
        assert KR.rate_constants(t, V, sg, np.zeros((2, 2)))[2][ts] == 0
    fd = {}
    for h in (H_EV, H_EV / 2):
        lo, hi = newton_run(-h)[0]['flux'][:, co], newton_run(+h)[0]['flux'][:, co]
        fd[h] = (lo - hi) / (2 * h / kT) / base['flux'][:, co]          # d ln flux_CO / d(-E_TS / kT)
    tol = 10.0 * np.abs(fd[H_EV] - fd[H_EV / 2]) + 10.0 * TAU / (H_EV / kT)
    apparent, intrinsic = rcx['drc_apparent'][:, ts, co], rcx['drc'][:, ts, co]
    for h in fd:
        print('h = %.0e eV: |drc_apparent - FD| / tolerance per lane' % h, np.array2string(np.abs(apparent - fd[h]) / tol, precision=2))
    print('measured difference |drc_apparent - FD(h/2)|', np.array2string(np.abs(apparent - fd[H_EV / 2]), precision=2), 'tolerance',
          np.array2string(tol, formatter={'float_kind': lambda v: '%.1e' % v}))
    print('intrinsic drc', np.array2string(intrinsic, precision=6), 'apparent', np.array2string(apparent, precision=6),
          'surface CO2 / bulk', np.array2string(base['surface_concentration'][:, co2] / 34.0, precision=3))
    for h in fd:
        assert (np.abs(apparent - fd[h]) <= tol).all(), (h, np.abs(apparent - fd[h]) / tol)
    # where transport holds the surface CO2 below 90 % of the bulk the two differ by far more than the tolerance
    influenced = base['surface_concentration'][:, co2] < 0.9 * 34.0
    assert influenced.any() and (np.abs(apparent - intrinsic)[influenced] > 10.0 * tol[influenced]).all()
    assert (apparent[influenced] < intrinsic[influenced]).all()          # mass transport takes control away from the step
