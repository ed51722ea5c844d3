"""libcatint_interact on the device against tests/interact_ref.py (the method of tests/test_gpu_kinetics.py).

Parity: every case of tests/interact_cases.py (the four-step mechanism in both site variants with a weak and a strong interaction, the
terrace-and-step variant, random networks with one to three site types in both response modes) against the 60-digit solves.  The
tolerance is measured on the reference side: per case and quantity, 10 x the worst error of solve_fp64 against solve_mp, floor 1e-13 --
in |dy| for the coverages, in units of rate_gross / flux_scale for rates and fluxes, relative to the sum of the absolute terms for the
sensitivities, absolute in kT for the energy shifts.  Iteration counts within +-1 per stage of solve_fp64.
Without interactions on one site type: against catkin_solve on the same points, equal statuses and iteration counts, values within the
tolerance of tests/test_gpu_kinetics.py.
Bit for bit: any max_waves, batches of 1, 63, 64, 65 and 130 points, permutations with repeats, the view path against the host-surface
path, outputs not asked for.  Behaviour: five stages reach the state of one stage where both converge; points that stop at maxit in
one stage converge in five; statuses 1 and 2 stay in their lane; warm start.  End to end: the small Stern-wall SCF case of
tests/test_gpu_kinetics.py with a CO2 self-interaction under both loops, the device fluxes compared with the reference at every
iteration's actual state; with the interaction set to zero the run equals the mean-field model's."""
import numpy as np
import pytest

from catint_amd import _interact, _kinetics          # _interact fails without the feature
from tests import interact_cases as IC
from tests import interact_ref as IR
from tests import kinetics_cases as KC
from tests.test_gpu_kinetics import E2E_PHIS, e2e_model, e2e_transport, open_handle, same

pytestmark = pytest.mark.gpu

ALL = list(_interact.FIELDS)
SIZES = (1, 63, 64, 65, 130)
QUANTITIES = ('y', 'rate', 'flux', 'dflux_dc', 'dflux_dphi', 'energy_shift')


@pytest.fixture(scope='module')
def ia():
    with _interact.InteractingKinetics(0) as o:
        yield o


def kw_of(case):
    k = case.kw
    return dict(potential_drop='stern' if k['w'] else 'full', stern_capacitance=k['CS'], phi_pzc=k['phi_pzc'])


def tiled(case, n):
    idx = np.arange(n) % len(case.phiM)
    return case.phiM[idx], case.csurf[idx], case.phi_surface[idx]


def run(ia, case, n=None, idx=None, fields=ALL, **kw):
    pm, cs, ps = (case.phiM, case.csurf, case.phi_surface) if n is None else tiled(case, n)
    if idx is not None:
        pm, cs, ps = pm[idx], cs[idx], ps[idx]
    args = dict(kw_of(case), ramp=case.ramp)
    args.update(kw)
    out = ia.solve(None, case.tables, pm, csurf=cs, phi_surface=ps, fields=fields, **args)
    assert ia.last_kernel == 'catia::interact_kernel' and ia.last_kernel_ms > 0.0
    return out


def tolerances(err_fp):
    return {q: max(10.0 * err_fp[q].max(), 1e-13) for q in QUANTITIES if q in err_fp}


# ---- parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', IC.CASE_NAMES)
def test_parity_with_60_digits(ia, name):
    case = IC.case(name)
    fp, ref, err_fp = IC.references(name)
    assert (fp['status'] == 0).all()
    out = run(ia, case)
    assert (out['status'] == 0).all(), out['status']
    assert (out['ramp_reached'] == case.ramp - 1).all()
    assert np.abs(out['iterations'].astype(int) - fp['iterations']).max() <= case.ramp, (out['iterations'], fp['iterations'])
    err = IC.errors(out, ref, fp)
    tol = tolerances(err_fp)
    print(name, 'device error / tolerance:', '; '.join('%s %.1e / %.1e' % (q, err[q].max(), tol[q]) for q in QUANTITIES))
    for q in QUANTITIES:
        assert err[q].max() <= tol[q], (name, q, err[q].max(), tol[q])
    assert np.allclose(out['rate_gross'], fp['rate_gross'], rtol=1e-11, atol=0) and np.allclose(out['flux_scale'], fp['flux_scale'], rtol=1e-11, atol=0)


@pytest.mark.parametrize('name', ['co2r_one_site', 'co2r_two_site', 'random_S5', 'random_S8'])
def test_without_interactions_on_one_site_type_it_is_catkin_solve(ia, name):
    case = KC.case(name)
    fp, ref, err_fp = KC.references(name)
    T = len(case.tables['site_count'])
    tab = dict(case.tables, site_of=np.zeros(T, np.int32), site_fraction=np.ones(1), eps=np.zeros((T - 1, T - 1)))
    fields = list(_kinetics.FIELDS)
    got = ia.solve(None, tab, case.phiM, csurf=case.csurf, phi_surface=case.phi_surface, fields=fields, **kw_of(case))
    with _kinetics.KineticsSolver(0) as ks:
        want = ks.solve(None, case.tables, case.phiM, csurf=case.csurf, phi_surface=case.phi_surface, fields=fields, **kw_of(case))
    assert np.array_equal(got['status'], want['status']) and (got['status'] == 0).all() and np.array_equal(got['iterations'], want['iterations'])
    assert (got['ramp_reached'] == 0).all()
    err = KC.errors(got, ref, fp)
    for q in ('y', 'rate', 'flux', 'dflux_dc', 'dflux_dphi'):
        tol = max(10.0 * err_fp[q].max(), 1e-13)
        assert err[q].max() <= tol, (name, q, err[q].max(), tol)
    print(name, 'bitwise equal to catkin_solve:', {k: bool(np.array_equal(got[k], want[k])) for k in fields})


# ---- bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['co2r_two_site_weak', 'random_S6_G3_piecewise'])
def test_any_number_of_waves_and_any_batch_size_give_the_same_bits(ia, name):
    case = IC.case(name)
    base = run(ia, case, 130)
    for waves in (1, 2, 3):
        same(base, run(ia, case, 130, max_waves=waves))
    for n in SIZES:
        got = run(ia, case, n)
        for k in got:
            assert np.array_equal(got[k], base[k][:n], equal_nan=True), (n, k)


def test_subsets_and_permutations_with_repeats(ia):
    case = IC.case('random_S5_G2_piecewise')
    base = run(ia, case, 130)
    rng = np.random.RandomState(5)
    for idx in (rng.permutation(130), rng.randint(0, 130, 65), np.array([7]), np.array([129, 129, 0, 64, 63, 64])):
        got = run(ia, case, 130, idx=idx)
        for k in got:
            assert np.array_equal(got[k], base[k][idx], equal_nan=True), k


@pytest.fixture(scope='module')
def handle():
    phis = np.linspace(-0.12, 0.06, 130)
    with open_handle(phis) as s:
        assert (s.solve_stationary() == 0).all()
        yield s, phis


def test_the_view_path_gives_the_bits_of_the_host_surface_path(ia, handle):
    s, phis = handle
    model = IC.terrace_step_model()
    before = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    cs, vs, _ = s.get_surface()
    from_view = s.get_kinetics(model, fields=ALL, ramp=3)
    assert s._interact.last_kernel == 'catia::interact_kernel' and s._kinetics is None
    from_host = s.get_kinetics(model, csurf=cs, phi_surface=vs, fields=ALL, ramp=3)
    alone = ia.solve(None, model.tables(), phis, csurf=cs, phi_surface=vs, potential_drop='stern', stern_capacitance=0.2, phi_pzc=0.0, fields=ALL, ramp=3)
    same(from_view, from_host)
    same(from_view, alone)
    assert (from_view['status'] == 0).all() and np.isfinite(from_view['dflux_dc']).all() and from_view['theta'].shape == (130, 7)
    rng = np.random.RandomState(9)
    for lanes in (rng.permutation(130), np.array([129, 0, 0, 64, 63, 65, 129]), np.arange(63), np.array([77])):
        got = s.get_kinetics(model, lanes=lanes, fields=ALL, max_waves=1, ramp=3)
        for k in got:
            assert np.array_equal(got[k], from_view[k][lanes], equal_nan=True), k
    after = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    with pytest.raises(ValueError, match='mean-field'):
        s.get_kinetics(model, rescue=True)


def test_outputs_not_asked_for_are_untouched(ia):
    case = IC.case('random_S7_G2_linear')
    N, G, S, R = IR.shape(case.tables)
    out = {k: np.full((3,) + _interact.FIELDS[k](N, G + S - 1, R, G), 7.0) for k in ALL}
    out.update({k: np.full(3, 77, np.int32) for k in _interact.FLAGS})
    two = {k: v[:2] for k, v in out.items()}
    run(ia, case, idx=np.array([0, 1]), out=two)
    for k, v in out.items():
        assert (v[2] == (77 if v.dtype == np.int32 else 7.0)).all() and not (v[:2] == (77 if v.dtype == np.int32 else 7.0)).all(), k
    only = run(ia, case, idx=np.array([0, 1]), fields=['flux'])
    assert sorted(only) == ['flux', 'iterations', 'ramp_reached', 'status'] and np.array_equal(only['flux'], out['flux'][:2])
    shifts = run(ia, case, idx=np.array([0, 1]), fields=['energy_shift'])
    assert np.array_equal(shifts['energy_shift'], out['energy_shift'][:2])


# ---- behaviour ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['co2r_one_site_strong', 'random_S2_G2_linear'])
def test_five_stages_reach_the_state_of_one_stage_where_both_converge(ia, name):
    case = IC.case(name)
    tol = tolerances(IC.references(name)[2])
    one, five = run(ia, case, ramp=1), run(ia, case, ramp=5)
    both = (one['status'] == 0) & (five['status'] == 0)
    assert both.sum() >= len(both) // 2 and (five['ramp_reached'][both] == 4).all() and (one['ramp_reached'] == 0).all()
    assert (five['iterations'][both] > one['iterations'][both]).any()
    # each lies within the parity tolerance of the same root
    assert np.abs(np.log(one['theta'][both]) - np.log(five['theta'][both])).max() <= 2.0 * tol['y']
    assert (np.abs(one['flux'][both] - five['flux'][both]) <= 2.0 * tol['flux'] * one['flux_scale'][both]).all()


def test_points_that_stop_at_maxit_in_one_stage_converge_in_five(ia):
    """tests/test_interact_abi.py: in the reference 9 of the 39 points of this case stop at maxit without the ramp"""
    case = IC.case('co2r_two_site_strong')
    one = run(ia, case, ramp=1)
    ref = IR.solve_fp64(case.tables, case.phiM, case.csurf, case.phi_surface, ramp=1, sens=False, **case.kw)
    print('one stage: device statuses', one['status'].tolist(), 'reference', ref['status'].tolist())
    stopped = one['status'] == 1
    assert stopped.any() and (one['iterations'][stopped] == 200).all() and (one['ramp_reached'] == 0).all()
    assert np.isfinite(one['theta'][stopped]).all()          # the numbers of a stopped lane are returned as computed
    five = run(ia, case, ramp=5)
    assert (five['status'] == 0).all() and (five['ramp_reached'] == 4).all()
    # A lane that stops in the middle of the ramp says where, and the lanes beside it go on: from the mean-field state the first stage
    # takes one iteration, and five iterations per stage are too few for the second stage (half strength) where CO2 is plentiful
    # (in the reference: every third point) and enough for both later stages elsewhere
    free = run(ia, case, ramp=1, strength=0.0)
    assert (free['status'] == 0).all() and (free['energy_shift'] == 0.0).all()
    full = run(ia, case, ramp=3, theta_guess=free['theta'])
    short = run(ia, case, ramp=3, theta_guess=free['theta'], maxit=5)
    stage, stopped = short['ramp_reached'], short['status'] == 1
    assert (full['status'] == 0).all() and stopped.any() and (short['status'][~stopped] == 0).all() and (~stopped).sum() >= 13
    assert (stage[stopped] == 1).all() and (stage[~stopped] == 2).all() and (short['iterations'][stopped] == 6).all()
    for k in ALL + ['iterations']:
        assert np.array_equal(short[k][~stopped], full[k][~stopped]), k
    # what a stopped lane returns is its state at the strength of its stage
    t = IR._arrays(case.tables)
    for i in np.flatnonzero(stopped):
        assert np.allclose(short['energy_shift'][i], 0.5 * (t['eps'] @ short['theta'][i, 1:]), rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize('name', ['co2r_two_site_weak', 'random_S8_G1_piecewise'])
def test_a_warm_start_from_the_returned_coverages(ia, name):
    case = IC.case(name)
    cold = run(ia, case)
    warm = run(ia, case, theta_guess=cold['theta'], ramp=1)
    assert (warm['status'] == 0).all() and warm['iterations'].max() <= 2, warm['iterations']
    assert np.abs(np.log(warm['theta']) - np.log(cold['theta'])).max() <= 1e-13


def test_a_non_finite_input_shows_in_its_lane_only(ia):
    case = IC.case('random_S3_G3_linear')
    N, G, S, R = IR.shape(case.tables)
    n = 65
    clean = run(ia, case, n, off=np.zeros((n, R, 2)))
    same(clean, run(ia, case, n))
    for poison in (np.inf, np.nan):
        off = np.zeros((n, R, 2))
        off[64, R - 1, 1] = poison
        got = run(ia, case, n, off=off)
        assert got['status'][64] == 2 and (got['status'][:64] == 0).all() and got['iterations'][64] == 0 and got['ramp_reached'][64] == 0
        for k in ALL:
            assert np.isnan(got[k][64]).all() and np.array_equal(got[k][:64], clean[k][:64]), k
    guess = np.tile(clean['theta'][:1], (n, 1))
    guess[3, 1] = np.nan
    got = run(ia, case, n, theta_guess=guess)
    assert got['status'][3] == 2 and (np.delete(got['status'], 3) == 0).all() and np.isnan(got['energy_shift'][3]).all()


def test_a_lane_the_handle_did_not_solve_reports_2_and_is_alone(ia):
    model = IC.co2r_model('one_site', 0.3, 0.15)
    results = []
    for phis in (np.zeros(5), np.array([0.0, 0.0, -0.8, 0.0, 0.0])):
        with open_handle(phis, maxit=1) as s:
            st = s.solve_stationary()
            results.append((st, s.get_kinetics(model, fields=ALL, phiM=np.full(5, -0.6), ramp=2)))
    (st0, clean), (st1, got) = results
    assert (st0 == 0).all() and st1[2] != 0 and (np.delete(st1, 2) == 0).all()
    assert (clean['status'] == 0).all() and got['status'][2] == 2 and (np.delete(got['status'], 2) == 0).all()
    for k in ALL:
        assert np.isnan(got[k][2]).all(), k
        assert np.array_equal(np.delete(got[k], 2, axis=0), np.delete(clean[k], 2, axis=0)), k


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def interacting_e2e_model(tp, self_eV):
    from catint_amd.interactions import InteractingModel
    return InteractingModel(list(tp.species.keys()), {'CO2': ('t', 1)}, ['CO2_g + *_t <-> CO2*_t', 'CO2*_t + 2ele_g <-> TS_t <-> CO_g + *_t; beta=0.5'],
                            {'CO2': (0.10, 0.004, 0.0), 'TS': (0.62, 0.004, 0.0)}, interactions={('CO2', 'CO2'): self_eV},
                            solution_energies={'CO': -0.2}, site_density=2e-6)


def checked_run(monkeypatch, scf, self_eV, tau, ramp=4):
    """run_scf_cycle with every kinetic call compared with the reference at the state it was made at: (result, iterations per call,
    worst error / tolerance, points retried)"""
    from catint_amd.calculator import Calculator
    tp = e2e_transport()
    calc = Calculator(transport=tp, calc='comsol', tau_scf=tau)
    model = interacting_e2e_model(tp, self_eV)
    calc.set_microkinetics(model, site_density=2e-6, scf=scf, ramp=ramp)
    made, worst, transport = [], [0.0], []
    inner = calc._physical_solver
    monkeypatch.setattr(calc, '_physical_solver', lambda B: transport.append(inner(B)) or transport[-1])

    class Checked(_interact.RampedKinetics):
        def solve(self, view, tables, phiM, **kw):
            out = _interact.RampedKinetics.solve(self, view, tables, phiM, **kw)
            if view is None:
                cs, vs = kw['csurf'], kw['phi_surface']
            else:
                cs, vs, _ = transport[-1].get_surface()
                cs, vs = cs[kw['lanes']], vs[kw['lanes']]
            guess = kw.get('theta_guess')
            ref = IR.solve_fp64(tables, phiM, cs, vs, w=1, CS=kw['stern_capacitance'], phi_pzc=kw['phi_pzc'], theta_guess=guess, sens=False,
                                ramp=ramp if guess is None else 1)
            mp = IR.solve_mp(tables, phiM, cs, vs, ref, w=1, CS=kw['stern_capacitance'], phi_pzc=kw['phi_pzc'], sens=False)
            tol = max(10.0 * IR.mp_err(mp['flux'], ref['flux'], ref['flux_scale']).max(), 1e-13)
            err = IR.mp_err(mp['flux'], out['flux'], ref['flux_scale']).max()
            worst[0] = max(worst[0], err / tol)
            assert err <= tol, (err, tol)
            assert (out['status'] == 0).all() and np.abs(out['iterations'].astype(int) - ref['iterations']).max() <= (ramp if guess is None else 1)
            made.append(out['iterations'].copy())
            return out
    solver = Checked(0, ramp)
    monkeypatch.setattr(calc, '_kinetics_solver', lambda: solver)
    out = calc.run_scf_cycle(max_iter=200)
    return out, made, worst[0], solver.retried, tp, model


@pytest.mark.parametrize('scf, tau', [('mixing', 1e-8), ('newton', 2e-9)])
def test_scf_cycle_with_a_self_interaction_on_the_small_stern_wall_case(monkeypatch, scf, tau):
    out, made, worst, retried, tp, model = checked_run(monkeypatch, scf, 0.3, tau)
    print('%s: SCF iterations %d, kinetic calls %d, worst device flux error / tolerance %.2f, retried %d' % (scf, out['iterations'], len(made), worst, retried))
    assert out['converged'].all() and not out['failed'].any() and (out['kinetic_status'] == 0).all()
    assert made[0].min() > 5 and made[-1].max() <= 3 and retried == 0          # ramped from the uniform start, then warm-started
    assert out['coverage'].shape == (8, 2) and np.allclose(out['coverage'].sum(axis=1), 1.0, atol=1e-12)
    assert (out['flux'][:, 2] < 0).all() and np.allclose(out['flux'][:, 3], -out['flux'][:, 2], rtol=1e-12)
    # the fixed point: the fluxes are the interacting model's at the final surface state, and not the mean-field model's
    tab = dict(model.tables(), site_density=2e-6)
    vs = np.array([tp.alldata[i]['system']['surface_potential'] for i in range(8)])
    end = IR.solve_fp64(tab, np.array(E2E_PHIS), out['surface_concentration'], vs, w=1, CS=0.2, phi_pzc=0.1, sens=False, ramp=4)
    assert np.allclose(end['flux'], out['flux'], rtol=1e-5, atol=1e-30)
    free = IR.solve_fp64(tab, np.array(E2E_PHIS), out['surface_concentration'], vs, w=1, CS=0.2, phi_pzc=0.1, sens=False, strength=0.0)
    assert (np.abs(free['flux'][:, 3] - out['flux'][:, 3]) > 1e-3 * np.abs(out['flux'][:, 3])).any()


@pytest.mark.parametrize('scf, tau', [('mixing', 1e-8), ('newton', 2e-9)])
def test_with_the_interaction_set_to_zero_the_run_is_the_mean_field_model_s(monkeypatch, scf, tau):
    """One stage, so that every kinetic call is the mean-field library's call: the kernel then returns its bits
    (test_without_interactions_on_one_site_type_it_is_catkin_solve prints so), and the whole run is the same run"""
    from catint_amd.calculator import Calculator
    out, made, worst, retried, tp, model = checked_run(monkeypatch, scf, 0.0, tau, ramp=1)
    tp2 = e2e_transport()
    calc = Calculator(transport=tp2, calc='comsol', tau_scf=tau)
    calc.set_microkinetics(e2e_model(tp2), site_density=2e-6, scf=scf)
    want = calc.run_scf_cycle(max_iter=200)
    assert out['iterations'] == want['iterations'] and want['converged'].all()
    for k in ('converged', 'failed', 'flux', 'coverage', 'flux_scale', 'accuracy', 'surface_concentration', 'kinetic_status'):
        assert np.array_equal(out[k], want[k]), k
