"""libcatint_kinetics on the device against tests/kinetics_ref.py (the method of tests/test_gpu_response.py).

Parity: every case of tests/kinetics_cases.py (the four-step mechanism in both site variants with CO2 at 30, 1e-3 and 0 mol/m^3, random
networks for S = 1 .. 8) against the 60-digit solves.  The tolerance is measured on the reference side: per case and quantity, 10 x the
worst error of solve_fp64 against solve_mp, floor 1e-13 -- in |dy| for the coverages, in units of rate_gross / flux_scale for rates and
fluxes, relative to the sum of the absolute terms for the sensitivities (tests/kinetics_ref.py: dflux_scale).  Iteration counts within
+-1 of solve_fp64.
Bit for bit: any max_waves, batches of 1, 63, 64, 65 and 130 points, lane subsets and permutations with repeats, the view path against
the host-surface path, outputs not asked for, the handle's state.  Behaviour: warm start, maxit, status 2 and its confinement to the
lane.  End to end: Calculator.set_microkinetics + run_scf_cycle on a small Stern-wall case, the device fluxes compared with solve_fp64
at every iteration's actual state.

The end-to-end case was first run on the CPU with oracle/pnp_physical.py as the transport and solve_fp64 as the kinetics
(scf_on_the_cpu below, not a test): every lane converges, in 23 iterations, with CO2 drawn down to 19.5 of 34 mol/m^3 at -0.38 V."""
import numpy as np
import pytest

from catint_amd import PnpSolver, _kinetics          # fails without the feature
from tests import kinetics_cases as KC
from tests import kinetics_ref as KR

pytestmark = pytest.mark.gpu

ALL = list(_kinetics.FIELDS)
SIZES = (1, 63, 64, 65, 130)
F = 96485.33289
RATIOS = {}


@pytest.fixture(scope='module')
def ks():
    with _kinetics.KineticsSolver(0) as o:
        yield o


def kw_of(case):
    k = case.kw
    return dict(potential_drop='stern' if k['w'] else 'full', stern_capacitance=k['CS'], phi_pzc=k['phi_pzc'])


def tiled(case, n):
    """n points: the case's, repeated"""
    idx = np.arange(n) % len(case.phiM)
    return case.phiM[idx], case.csurf[idx], case.phi_surface[idx]


def run(ks, case, n=None, idx=None, fields=ALL, **kw):
    pm, cs, ps = (case.phiM, case.csurf, case.phi_surface) if n is None else tiled(case, n)
    if idx is not None:
        pm, cs, ps = pm[idx], cs[idx], ps[idx]
    args = kw_of(case)
    args.update(kw)
    out = ks.solve(None, case.tables, pm, csurf=cs, phi_surface=ps, fields=fields, **args)
    assert ks.last_kernel == 'catkin::steady_kernel' and ks.last_kernel_ms > 0.0
    return out


def same(a, b, keys=None):
    for k in (keys or a):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', KC.CASE_NAMES)
def test_parity_with_60_digits(ks, name):
    case = KC.case(name)
    fp, ref, err_fp = KC.references(name)
    out = run(ks, case)
    assert (out['status'] == 0).all(), out['status']
    assert np.abs(out['iterations'].astype(int) - fp['iterations']).max() <= 1, (out['iterations'], fp['iterations'])
    err = KC.errors(out, ref, fp)
    line = []
    for q in ('y', 'rate', 'flux', 'dflux_dc', 'dflux_dphi'):
        tol = max(10.0 * err_fp[q].max(), 1e-13)
        RATIOS[(name, q)] = err[q].max() / tol
        line.append('%s %.1e / %.1e' % (q, err[q].max(), tol))
    print(name, 'device error / tolerance:', '; '.join(line))
    print(name, 'sensitivities against the plain term sum, device (reference): dflux_dc %.1e (%.1e); dflux_dphi %.1e (%.1e)'
          % (err['dflux_dc_plain'].max(), err_fp['dflux_dc_plain'].max(), err['dflux_dphi_plain'].max(), err_fp['dflux_dphi_plain'].max()))
    for q in ('y', 'rate', 'flux', 'dflux_dc', 'dflux_dphi'):
        assert RATIOS[(name, q)] <= 1.0, (name, q, RATIOS[(name, q)])
    assert np.allclose(out['rate_gross'], fp['rate_gross'], rtol=1e-11, atol=0) and np.allclose(out['flux_scale'], fp['flux_scale'], rtol=1e-11, atol=0)


# ---- bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['co2r_two_site', 'random_S8'])
def test_any_number_of_waves_and_any_batch_size_give_the_same_bits(ks, name):
    case = KC.case(name)
    base = run(ks, case, 130)
    for waves in (1, 2, 3):
        same(base, run(ks, case, 130, max_waves=waves))
    for n in SIZES:
        got = run(ks, case, n)
        for k in got:
            assert np.array_equal(got[k], base[k][:n], equal_nan=True), (n, k)


def test_subsets_and_permutations_with_repeats(ks):
    case = KC.case('co2r_one_site')
    base = run(ks, case, 130)
    rng = np.random.RandomState(5)
    for idx in (rng.permutation(130), rng.randint(0, 130, 65), np.array([7]), np.array([129, 129, 0, 64, 63, 64])):
        got = run(ks, case, 130, idx=idx)
        for k in got:
            assert np.array_equal(got[k], base[k][idx], equal_nan=True), k


def open_handle(phis, maxit=50):
    """Three species (+, -, neutral) at a Stern wall: the surface state of its lanes feeds the three-species mechanism"""
    beta, eps, nx = 1.0 / (8.3144598 * 298.14), 78.36 * 8.854187817e-12, 48
    D, q, cb = np.array([1.957e-9, 1.185e-9, 1.9e-9]), np.array([F, -F, 0.0]), np.array([10.0, 10.0, 1.0])
    dx = np.sqrt(eps / beta / (q ** 2 * cb).sum()) / 6.0
    B = len(phis)
    s = PnpSolver(3, nx, dx, 1.0, beta, eps, D, q, method='Newton', batch_capacity=B)
    s.set_newton(wall_bc='stern', stern_capacitance=0.2, phi_pzc=0.0, maxit=maxit)
    pb = np.zeros((B, 4))
    pb[:, 0] = phis
    s.set_batch(np.repeat(np.repeat(cb[None, :, None], nx, axis=2), B, axis=0), pb, np.zeros(B), np.zeros((B, 3)))
    return s


@pytest.fixture(scope='module')
def handle():
    phis = np.linspace(-0.12, 0.06, 130)
    with open_handle(phis) as s:
        assert (s.solve_stationary() == 0).all()
        yield s, phis


def test_the_view_path_gives_the_bits_of_the_host_surface_path(ks, handle):
    s, phis = handle
    model = KC.co2r_model('two_site')
    before = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    cs, vs, _ = s.get_surface()
    from_view = s.get_kinetics(model, fields=ALL)
    assert s._kinetics.last_kernel == 'catkin::steady_kernel'
    from_host = s.get_kinetics(model, csurf=cs, phi_surface=vs, fields=ALL)
    alone = ks.solve(None, model.tables(), phis, csurf=cs, phi_surface=vs, potential_drop='stern', stern_capacitance=0.2, phi_pzc=0.0, fields=ALL)
    same(from_view, from_host)
    same(from_view, alone)
    assert (from_view['status'] == 0).all() and np.isfinite(from_view['dflux_dc']).all()
    # lane subsets and permutations with repeats, any number of waves, through the view
    rng = np.random.RandomState(9)
    for lanes in (rng.permutation(130), np.array([129, 0, 0, 64, 63, 65, 129]), np.arange(63), np.array([77])):
        got = s.get_kinetics(model, lanes=lanes, fields=ALL, max_waves=1)
        for k in got:
            assert np.array_equal(got[k], from_view[k][lanes], equal_nan=True), k
    # the handle's state, status and counters are only read
    after = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_outputs_not_asked_for_are_untouched(ks):
    case = KC.case('random_S5')
    N, S, R = KR.shape(case.tables)
    out = {k: np.full((3,) + _kinetics.FIELDS[k](N, S, R), 7.0) for k in ALL}
    out.update(status=np.full(3, 77, np.int32), iterations=np.full(3, 77, np.int32))
    two = {k: v[:2] for k, v in out.items()}          # two points of room for three: the third is not the library's to touch
    run(ks, case, idx=np.array([0, 1]), out=two)
    for k, v in out.items():
        assert (v[2] == (77 if v.dtype == np.int32 else 7.0)).all() and not (v[:2] == (77 if v.dtype == np.int32 else 7.0)).all(), k
    only = run(ks, case, idx=np.array([0, 1]), fields=['flux'])
    assert sorted(only) == ['flux', 'iterations', 'status'] and np.array_equal(only['flux'], out['flux'][:2])


# ---- behaviour ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['co2r_two_site', 'random_S6'])
def test_a_warm_start_from_the_returned_coverages(ks, name):
    case = KC.case(name)
    cold = run(ks, case)
    warm = run(ks, case, theta_guess=cold['theta'])
    assert (warm['status'] == 0).all() and warm['iterations'].max() <= 2, warm['iterations']
    assert np.abs(np.log(warm['theta']) - np.log(cold['theta'])).max() <= 1e-13


def test_maxit_3_stops_the_lanes_that_need_more_and_only_those(ks):
    case = KC.case('co2r_one_site')
    n = len(case.phiM)
    cold = run(ks, case)
    start = 1.0 / case.tables['site_count'].sum()
    guess = np.where((np.arange(n) % 2 == 0)[:, None], cold['theta'], start)
    full = run(ks, case, theta_guess=guess)
    short = run(ks, case, theta_guess=guess, maxit=3)
    need_more = full['iterations'] > 3
    assert need_more.any() and (~need_more).any()
    assert np.array_equal(short['status'], np.where(need_more, 1, 0)) and (short['iterations'][need_more] == 3).all()
    for k in ALL:
        assert np.array_equal(short[k][~need_more], full[k][~need_more]), k
        assert np.isfinite(short[k][need_more]).all(), k          # the numbers of a stopped lane are returned as computed


def test_a_lane_the_handle_did_not_solve_reports_2_and_is_alone(ks):
    """A non-zero solver status comes from a stationary solve limited to one iteration (lane 2 at -0.8 V from the bulk state)"""
    model = KC.co2r_model('one_site')
    results = []
    for phis in (np.zeros(5), np.array([0.0, 0.0, -0.8, 0.0, 0.0])):
        with open_handle(phis, maxit=1) as s:
            st = s.solve_stationary()
            results.append((st, s.get_kinetics(model, fields=ALL, phiM=np.full(5, -0.6))))
    (st0, clean), (st1, got) = results
    assert (st0 == 0).all() and st1[2] != 0 and (np.delete(st1, 2) == 0).all()
    assert (clean['status'] == 0).all() and got['status'][2] == 2 and (np.delete(got['status'], 2) == 0).all()
    for k in ALL:
        assert np.isnan(got[k][2]).all(), k
        assert np.array_equal(np.delete(got[k], 2, axis=0), np.delete(clean[k], 2, axis=0)), k
    assert got['iterations'][2] == 0


def test_a_non_finite_input_shows_in_its_lane_only(ks):
    case = KC.case('random_S4')
    N, S, R = KR.shape(case.tables)
    n = 65
    clean = run(ks, case, n, off=np.zeros((n, R, 2)))
    same(clean, run(ks, case, n))                         # zeros are what NULL means
    for poison in (np.inf, np.nan):
        off = np.zeros((n, R, 2))
        off[64, R - 1, 1] = poison
        got = run(ks, case, n, off=off)
        assert got['status'][64] == 2 and (got['status'][:64] == 0).all()
        for k in ALL:
            assert np.isnan(got[k][64]).all() and np.array_equal(got[k][:64], clean[k][:64]), k
    cs = tiled(case, n)[1].copy()
    cs[3, 0] = np.nan
    got = ks.solve(None, case.tables, tiled(case, n)[0], csurf=cs, phi_surface=tiled(case, n)[2], fields=ALL, **kw_of(case))
    assert got['status'][3] == 2 and (np.delete(got['status'], 3) == 0).all() and np.isnan(got['theta'][3]).all()
    assert np.array_equal(np.delete(got['flux'], 3, axis=0), np.delete(clean['flux'], 3, axis=0))
    # per-lane activity coefficients and a prescribed charge enter as the header says: against the reference
    gamma = 0.5 + np.arange(n * N).reshape(n, N) % 7 / 7.0
    sigma = -0.05 - 0.001 * np.arange(n)
    got = run(ks, case, n, gamma=gamma, sigma=sigma)
    pm, cs, ps = tiled(case, n)
    ref = KR.solve_fp64(case.tables, pm, cs, ps, w=case.kw['w'], sigma=sigma, gamma=gamma)
    assert (got['status'] == 0).all() and np.abs(got['iterations'].astype(int) - ref['iterations']).max() <= 1
    assert np.abs(np.log(got['theta']) - ref['y']).max() <= 1e-11
    assert (np.abs(got['flux'] - ref['flux']) <= 1e-11 * ref['flux_scale']).all()
    assert (np.abs(got['dflux_dphi'] - ref['dflux_dphi']) <= 1e-9 * ref['dflux_scale'][:, :, N:] + 1e-300).all()


# ---- end to end --------------------------------------------------------------------------------------------------------------------
E2E_PHIS = list(np.linspace(-0.30, -0.38, 8))


def e2e_transport():
    import collections
    from catint_amd.transport import Transport
    species = collections.OrderedDict([('K+', {'bulk_concentration': 100.0}), ('HCO3-', {'bulk_concentration': 100.0}),
                                       ('CO2', {'bulk_concentration': 34.0}), ('CO', {'bulk_concentration': 0.0})])
    sysd = {'phiM': E2E_PHIS[0], 'boundary thickness': 4e-8, 'Stern capacitance': 20.0, 'phiPZC': 0.1}
    return Transport(species=species, system=sysd, nx=64, descriptors={'phiM': E2E_PHIS})


def e2e_model(tp):
    """CO2 + * <-> CO2*;  CO2* + 2 e- <-> [TS] <-> CO + * (illustrative energies)"""
    from catint_amd.microkinetics import MeanFieldModel
    return MeanFieldModel(list(tp.species.keys()), {'CO2': 1}, ['CO2_g + *_t <-> CO2*_t', 'CO2*_t + 2ele_g <-> TS_t <-> CO_g + *_t; beta=0.5'],
                          {'CO2': (0.10, 0.004, 0.0), 'TS': (0.62, 0.004, 0.0)}, solution_energies={'CO': -0.2}, site_density=2e-6)


def scf_on_the_cpu():
    """The end-to-end case with oracle/pnp_physical.py as the transport and solve_fp64 as the kinetics: (result, calls)"""
    from catint_amd.calculator import Calculator
    from oracle import pnp_physical as PH
    from tests.test_kinetics_abi import FakeKinetics
    tp = e2e_transport()
    calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-8)
    calc.set_microkinetics(e2e_model(tp), site_density=2e-6)
    fake = FakeKinetics()
    calc._kinetics_solver = lambda: fake
    cb = [tp.species[sp]['bulk_concentration'] for sp in tp.species]
    c0 = tp.c0.reshape(tp.nspecies, tp.nx)
    state = {}

    def transport_fn(flux):
        cs, vs = np.zeros((len(E2E_PHIS), tp.nspecies)), np.zeros(len(E2E_PHIS))
        for i, phiM in enumerate(E2E_PHIS):
            p = PH.PhysicalProblem(D=tp.D, charges=tp.charges, beta=tp.beta, eps=tp.eps, dx=tp.dx, nx=tp.nx, c_bulk=cb, phiM=phiM, flux=flux[i],
                                   stern_capacitance=0.2, phi_pzc=0.1)
            c, phi = state.get(i, (c0, np.zeros(tp.nx)))
            c, phi, it, _ = PH.newton_step(p, c, phi, c, np.inf, tol=1e-8, maxit=50)
            state[i] = (c, phi)
            cs[i], vs[i] = c[:, 0], phi[0]
        return cs, vs, np.zeros(len(E2E_PHIS))
    return calc.run_scf_cycle(transport_fn=transport_fn, max_iter=200), fake.calls


def test_scf_cycle_with_microkinetics_on_a_small_stern_wall_case(monkeypatch):
    from catint_amd.calculator import Calculator
    tp = e2e_transport()
    calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-8)
    model = e2e_model(tp)
    calc.set_microkinetics(model, site_density=2e-6)
    tab = dict(model.tables(), site_density=2e-6)
    made, worst = [], [0.0]

    class Checked(_kinetics.KineticsSolver):
        def solve(self, view, tables, phiM, **kw):
            out = _kinetics.KineticsSolver.solve(self, view, tables, phiM, **kw)
            ref = KR.solve_fp64(tables, phiM, kw['csurf'], kw['phi_surface'], w=1, CS=kw['stern_capacitance'], phi_pzc=kw['phi_pzc'],
                                theta_guess=kw['theta_guess'], sens=False)
            mp = KR.solve_mp(tables, phiM, kw['csurf'], kw['phi_surface'], ref, w=1, CS=kw['stern_capacitance'], phi_pzc=kw['phi_pzc'], sens=False)
            tol = max(10.0 * KR.mp_err(mp['flux'], ref['flux'], ref['flux_scale']).max(), 1e-13)
            err = KR.mp_err(mp['flux'], out['flux'], ref['flux_scale']).max()
            worst[0] = max(worst[0], err / tol)
            assert err <= tol, (err, tol)
            assert (out['status'] == 0).all() and np.abs(out['iterations'].astype(int) - ref['iterations']).max() <= 1
            made.append(out['iterations'].copy())
            return out
    monkeypatch.setattr(calc, '_kinetics_solver', lambda: Checked(0))
    out = calc.run_scf_cycle(max_iter=200)
    print('SCF iterations %d, worst device flux error / tolerance over all calls %.2f' % (out['iterations'], worst[0]))
    assert out['converged'].all() and not out['failed'].any() and 3 <= out['iterations'] <= 40
    assert made[0].min() > 5 and made[-1].max() <= 3          # warm-started
    assert out['coverage'].shape == (8, 2) and np.allclose(out['coverage'].sum(axis=1), 1.0, atol=1e-12)
    assert (out['flux'][:, 2] < 0).all() and np.allclose(out['flux'][:, 3], -out['flux'][:, 2], rtol=1e-12)
    assert np.all(np.diff(out['flux'][:, 3]) > 0)            # more CO at the more negative potential
    for i in range(8):
        assert np.array_equal(tp.alldata[i]['system']['coverage'], out['coverage'][i])
    # the fixed point: the fluxes are the model's at the final surface state
    end = KR.solve_fp64(tab, np.array(E2E_PHIS), out['surface_concentration'], np.array([tp.alldata[i]['system']['surface_potential'] for i in range(8)]),
                        w=1, CS=0.2, phi_pzc=0.1, sens=False)
    assert np.allclose(end['flux'], out['flux'], rtol=1e-5, atol=1e-30)
