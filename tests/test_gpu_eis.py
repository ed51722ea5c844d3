"""libcatint_eis on the device (catint_amd._eis.Impedance, PnpSolver.get_kinetic_admittance / get_impedance) against the restatement of
include/catint_eis.h in tests/eis_ref.py, which tests/test_eis_ref.py pins to known answers.

Kinetic kernel: the networks of tests/kinetics_cases.py (both CO2 reduction variants, random S = 1, 4, 8) and the Langmuir step, n = 70
points (one full wave and a partial one: the case's points, repeated), omega = (0, lam, 1e3 lam) with lam the geometric mean over the
points of max_s D_s / theta_s, the gross turnover per coverage.  Error of K = [Kc | Kphi] against eis_ref.kinetic relative to the sum of
the absolute terms of each entry (eis_ref: 'scale', the dflux_scale convention of tests/kinetics_ref.py).  Bound, measured on the
reference side as tests/test_gpu_kinetics.py measures its own: per case 10 x the worst error of eis_ref.kinetic against the 60-digit
evaluation of the same formulas (eis_ref.kinetic_mp), with no floor.  K(0) against get_kinetics(fields=('dflux_dc', 'dflux_dphi')) on the
device under the same bound, for the same six cases.
Measured on the MI355X (also in profiles/eis_probe.md), device error / bound with the reference's own error against 60 digits in
brackets: co2r_one_site 0.31 (6.4e-11), co2r_two_site 0.05 (1.0e-10), random_S1 0.12 (5.9e-12), random_S4 0.001 (5.5e-14), random_S8 0.13
(3.3e-10), Langmuir 0.026 (7.3e-16); K(0) against get_kinetics at most 1.8e-15 of the term sum (co2r_one_site), worst ratio 0.017
(Langmuir, whose bound is 7.3e-15).

Coupled electrode: tests/response_cases.py small(N, nx, stern=True) for N = 1, 3, 4 at nx = 5 and 21, case G8 at nx = 7 and 34 (block
size 9, the partial team), a steric case and case G (reactions and convection), five lanes (the case's phiM times 1, 0.75, 0.5, 0.25,
0.1), F = 3 including 0 (0, 1 / tau_DL, 100 / tau_DL of the case), with the three-step mechanism of tests/eis_cases.py at the wall and rf chosen so that rf (Kc T_c + Kphi0 (x)
T_phi) has a row-sum norm of 0.5 at the first lane and omega = 0.  Tolerance: per output and system, 10 x the disagreement of the
reference's two transport solvers (banded LU; block elimination) on that system, not below 1e-11 -- the project's rule from
tests/test_gpu_response.py; that disagreement must itself stay below 1e-8 (asserted, and checked on the CPU by tests/test_eis_ref.py).
The same rule holds for the transfer functions against get_response and get_coupling and for the blocking electrode against
get_response('phiM').
Measured on the MI355X: worst device error / tolerance 0.15 (G8, nx = 34), every other case 0.09 .. 0.12, with reference disagreements up
to 7.3e-10 (case G, the admittance at omega = 0); the transfer functions against get_response / get_coupling 0.04 at worst, and bit for
bit those of get_response (printed, not asserted).  Every compiled instance, NB = 2 .. 9, is launched by a test of its own (N = 1 .. 8
at nx = 5, three lanes the device solved from the bulk state) and its transfer functions are held to the same rule: 0.008 .. 0.032.

End to end: the scf='newton' case of tests/test_gpu_couple.py at phiM = -0.34 V and phiM +- delta, +- delta / 2, delta = 4 mV, in one
batch.  Re Y(0) of the middle lane against the central difference of the converged current sum_k q_k rf flux_k.  The finite difference
is the reference.  Tolerance: twice the Richardson estimate |FD(delta) - FD(delta / 2)| plus the share of the SCF tolerance,
2 tau_scf max|q flux| / delta (each converged flux carries a relative residual of at most tau_scf = 2e-9, taken through a Newton matrix
whose inverse has norm <= 1: transport limitation only lowers the answer of the flux to the potential).  The mechanism of that case
turns neutral CO2 into neutral CO, so its current is an exact 0 on both sides; the same case runs once more with two HCO3- released
per CO (the anion of its electrolyte in the place of the two OH- of the real reaction), where the current is -2 F per turnover.
Measured on the MI355X: Re Y(0) = 1.401522e6 against FD(delta / 2) = 1.401705e6 and FD(delta) = 1.402251e6 A m^-2 V^-1, tolerance 1.09e3,
error / tolerance 0.167 (the difference is the truncation error of the finite difference, a quarter of the Richardson estimate).
The option of the Calculator also runs after the mixing loop, on the host and with device_loop=True: status 0 everywhere, the
admittance 1.2e-9 from the Newton loop's (asserted to 1e-3: the mixing loops stop on the change per iteration).

Every test prints its worst ratio error / tolerance."""
import numpy as np
import pytest

from catint_amd import PnpSolver, _eis          # fails without the feature
from tests import couple_ref as CR
from tests import eis_cases as EC
from tests import eis_ref as ER
from tests import kinetics_cases as KC
from tests import kinetics_ref as KR
from tests import response_cases as RC
from tests import response_ref as RR
from tests.test_eis_abi import INSTANCES
from tests.test_eis_ref import ELECTROLYTES, omegas_of
from tests.test_gpu_couple import load, open_solver

pytestmark = pytest.mark.gpu

B = len(RC.SCALES)
N_KIN = 70
KFIELDS = ('Kc', 'Kphi', 'dy', 'residual')
EFIELDS = list(ER.ELECTRODE)
_cache = {}


@pytest.fixture(scope='module')
def eis():
    with _eis.Impedance(0) as o:
        yield o


@pytest.fixture(scope='module', autouse=True)
def close_all():
    yield
    for entry in _cache.values():
        entry[0].close()
    _cache.clear()


def same(a, b, keys=None):
    for k in (keys or a):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- the kinetic kernel ------------------------------------------------------------------------------------------------------------
Kin = KC.Case


def langmuir_case():
    phiM, csurf, phi0 = EC.langmuir_points()
    return Kin('langmuir', EC.langmuir_tables(), phiM, csurf, phi0, dict(w=1, CS=0.2, phi_pzc=0.05))


KIN_NAMES = ['co2r_one_site', 'co2r_two_site', 'random_S1', 'random_S4', 'random_S8', 'langmuir']


def kin_case(name):
    """(case, theta [points][T], omegas [3], reference {Kc, Kphi, dy, scale, residual} per unique point, bound) once per session"""
    key = ('kin', name)
    if key not in _cache:
        case = langmuir_case() if name == 'langmuir' else KC.case(name)
        fp = KR.solve_fp64(case.tables, case.phiM, case.csurf, case.phi_surface, sens=False, **case.kw)
        assert (fp['status'] == 0).all()
        theta = fp['theta']
        n = len(case.phiM)
        lams = [ER.kinetic(case.tables, case.phiM[i], case.csurf[i], case.phi_surface[i], theta[i], 0.0, **case.kw)['lam'] for i in range(n)]
        lam = float(np.exp(np.mean(np.log(lams))))
        omegas = np.array([0.0, lam, 1e3 * lam])
        ref = ER.kinetic_batch(case.tables, case.phiM, case.csurf, case.phi_surface, theta, omegas, **case.kw)
        spread = 0.0
        for i in range(n):
            for f, om in enumerate(omegas):
                Kmp = ER.kinetic_mp(case.tables, case.phiM[i], case.csurf[i], case.phi_surface[i], theta[i], om, **case.kw)
                K = np.concatenate([ref['Kc'][i, f], ref['Kphi'][i, f]], axis=1)
                spread = max(spread, ER.mp_err(Kmp, K, ref['scale'][i, f]))
        _cache[key] = (_Closed(), case, theta, omegas, ref, spread)
    return _cache[key][1:]


class _Closed(object):
    def close(self):
        pass


def kw_of(case):
    k = case.kw
    return dict(potential_drop='stern' if k['w'] else 'full', stern_capacitance=k['CS'], phi_pzc=k['phi_pzc'])


def run_kinetic(eis, case, theta, omegas, idx, fields=KFIELDS, **kw):
    args = kw_of(case)
    args.update(kw)
    out = eis.kinetic(None, case.tables, case.phiM[idx], theta[idx], omegas, csurf=case.csurf[idx], phi_surface=case.phi_surface[idx], fields=fields,
                      **args)
    assert eis.last_kernel == 'cateis::kinetic_kernel' and eis.last_kernel_ms > 0.0
    return out


def scaled_error(K, Kref, scale):
    """max |K - Kref| / scale; an entry whose term sum is 0 must be an exact 0"""
    zero = scale == 0
    assert (K[zero] == 0).all() and (Kref[zero] == 0).all()
    return float((np.abs(K - Kref)[~zero] / scale[~zero]).max()) if (~zero).any() else 0.0


@pytest.mark.parametrize('name', KIN_NAMES)
def test_kinetic_admittance_against_the_reference(eis, name):
    case, theta, omegas, ref, spread = kin_case(name)
    n = len(case.phiM)
    idx = np.arange(N_KIN) % n
    out = run_kinetic(eis, case, theta, omegas, idx)
    assert out['Kc'].shape == (N_KIN, 3) + ref['Kc'].shape[2:] and out['dy'].dtype == np.complex128
    assert (out['status'] == 0).all(), out['status']
    assert (out['Kc'][:, 0].imag == 0).all() and (out['Kphi'][:, 0].imag == 0).all() and (out['dy'][:, 0].imag == 0).all()
    bound = 10.0 * spread
    K = np.concatenate([out['Kc'], out['Kphi']], axis=3)
    Kref = np.concatenate([ref['Kc'], ref['Kphi']], axis=3)[idx]
    err = scaled_error(K, Kref, ref['scale'][idx])
    dy_err = float(np.abs(out['dy'] - ref['dy'][idx]).max() / max(np.abs(ref['dy']).max(), 1e-300))
    print('%s: K against eis_ref / term sum %.2e, bound %.2e (reference against 60 digits %.2e), ratio %.3f; dy %.1e; residual %.1e; omega %s'
          % (name, err, bound, spread, err / bound, dy_err, out['residual'].max(), omegas))
    assert err <= bound, (name, err, bound)
    assert np.allclose(out['residual'], ref['residual'][idx], rtol=0, atol=1e-12)
    # a repeated point is the same point
    for k in KFIELDS + ('status',):
        assert np.array_equal(out[k], out[k][idx]), k


@pytest.mark.parametrize('name', KIN_NAMES)
def test_zero_frequency_is_the_sensitivity_of_libcatint_kinetics(eis, name):
    from catint_amd import _kinetics
    case, _, omegas, ref, spread = kin_case(name)
    with _kinetics.KineticsSolver(0) as ks:
        kin = ks.solve(None, case.tables, case.phiM, csurf=case.csurf, phi_surface=case.phi_surface, fields=('theta', 'dflux_dc', 'dflux_dphi'),
                       **kw_of(case))
    assert (kin['status'] == 0).all()
    out = run_kinetic(eis, case, kin['theta'], [0.0], np.arange(len(case.phiM)), fields=('Kc', 'Kphi'))
    K = np.concatenate([out['Kc'][:, 0], out['Kphi'][:, 0]], axis=2)
    assert (K.imag == 0).all()
    bound = 10.0 * spread
    err = scaled_error(K.real, np.concatenate([kin['dflux_dc'], kin['dflux_dphi']], axis=2), ref['scale'][:, 0])
    print('%s: K(0) against get_kinetics / term sum %.2e, bound %.2e, ratio %.3f' % (name, err, bound, err / bound))
    assert err <= bound


def test_kinetic_waves_order_outputs_frequencies_and_workspace_do_not_change_the_bits(eis, monkeypatch):
    case, theta, omegas, _, _ = kin_case('random_S8')
    n = len(case.phiM)
    idx = np.arange(150) % n
    want = run_kinetic(eis, case, theta, omegas, idx)
    same(run_kinetic(eis, case, theta, omegas, idx, max_waves=1), want)
    same(run_kinetic(eis, case, theta, omegas, idx, max_waves=2), want)
    rng = np.random.RandomState(4)
    perm = rng.permutation(150)
    got = run_kinetic(eis, case, theta, omegas, idx[perm])
    for k in got:
        assert np.array_equal(got[k], want[k][perm]), k
    for fields in (('Kc',), ('Kphi', 'residual'), ('dy',)):
        got = run_kinetic(eis, case, theta, omegas, idx, fields=fields)
        assert sorted(got) == sorted(fields + ('status',))
        same(got, want, fields + ('status',))
    for f in range(3):
        got = run_kinetic(eis, case, theta, omegas[f:f + 1], idx)
        for k in ('Kc', 'Kphi', 'dy', 'status'):
            assert np.array_equal(got[k][:, 0], want[k][:, f]), (k, f)
        assert np.array_equal(got['residual'], want['residual'])
    monkeypatch.setenv('CATEIS_WORKSPACE_BYTES', '1')          # one wavefront's 64 pairs per turn: 450 pairs in 8 turns
    same(run_kinetic(eis, case, theta, omegas, idx), want)


def kin_handle():
    """Three species at a Stern wall, 70 lanes solved on the device: the surface state of the view path"""
    if 'kin_handle' not in _cache:
        from tests.test_gpu_kinetics import open_handle
        phis = np.linspace(-0.12, 0.06, N_KIN)
        s = open_handle(phis)
        assert (s.solve_stationary() == 0).all()
        _cache['kin_handle'] = (s, phis)
    return _cache['kin_handle']


def test_the_view_path_gives_the_bits_of_the_host_surface_path(eis):
    s, phis = kin_handle()
    model = KC.co2r_model('two_site')
    before = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    cs, vs, _ = s.get_surface()
    theta = s.get_kinetics(model, fields=('theta',))['theta']
    om = [0.0, 1e3, 1e7]
    from_view = s.get_kinetic_admittance(model, om, theta=theta, fields=KFIELDS)
    assert s._impedance.last_kernel == 'cateis::kinetic_kernel'
    from_host = s.get_kinetic_admittance(model, om, theta=theta, csurf=cs, phi_surface=vs, fields=KFIELDS)
    alone = eis.kinetic(None, model.tables(), phis, theta, om, csurf=cs, phi_surface=vs, potential_drop='stern', stern_capacitance=0.2, phi_pzc=0.0,
                        fields=KFIELDS)
    same(from_view, from_host)
    same(alone, from_view, KFIELDS + ('status',))
    assert (from_view['status'] == 0).all() and np.isfinite(from_view['Kc']).all()
    solved = s.get_kinetic_admittance(model, om, fields=KFIELDS)          # theta=None: get_kinetics first
    same(solved, from_view)
    lanes = np.array([69, 0, 0, 64, 63, 65, 69])
    got = s.get_kinetic_admittance(model, om, theta=theta[lanes], lanes=lanes, fields=KFIELDS, max_waves=1)
    for k in KFIELDS + ('status',):
        assert np.array_equal(got[k], from_view[k][lanes]), k
    after = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_kinetic_status_codes(eis):
    case, theta, omegas, _, _ = kin_case('co2r_one_site')
    idx = np.arange(5)
    clean = run_kinetic(eis, case, theta, omegas, idx)
    assert (clean['status'] == 0).all()
    th = theta[idx].copy()
    th[1] *= np.array([1.0, 1.0 + 1e-3, 1.0, 1.0 - 1e-3])[:th.shape[1]]          # not stationary any more
    th[3, 0] = np.nan
    got = eis.kinetic(None, case.tables, case.phiM[idx], th, omegas, csurf=case.csurf[idx], phi_surface=case.phi_surface[idx], fields=KFIELDS,
                      **kw_of(case))
    assert np.array_equal(got['status'], np.array([[0] * 3, [4] * 3, [0] * 3, [2] * 3, [0] * 3]))
    assert got['residual'][1] > 1e-8 and np.isfinite(got['Kc'][1]).all()
    for k in KFIELDS:
        assert np.isnan(got[k][3]).all(), k
        assert np.array_equal(np.delete(got[k], [1, 3], axis=0), np.delete(clean[k], [1, 3], axis=0)), k
    loose = eis.kinetic(None, case.tables, case.phiM[idx], th, omegas, csurf=case.csurf[idx], phi_surface=case.phi_surface[idx], fields=KFIELDS,
                        residual_tol=1.0, **kw_of(case))
    assert (loose['status'][1] == 0).all() and np.array_equal(loose['Kc'][1], got['Kc'][1])


# ---- the coupled electrode -----------------------------------------------------------------------------------------------------------
def prepared(name):
    """(solver, phis, [(problem, c, phi)] at the device's own state, tables, theta [B][3], rf) of an electrolyte case, once per session"""
    key = ('el', name)
    if key not in _cache:
        case = ELECTROLYTES[name]()
        phis = case.phiM * np.array(RC.SCALES)
        states, st = [None] * B, None
        for b in np.argsort(np.abs(phis)):                    # continuation from the smallest potential up
            _, c, phi = case.solve(phis[b], start=st, tol=1e-11) if st is not None else case.solve(phis[b], tol=1e-11)
            states[b] = st = (c, phi)
        s = open_solver(case, B)
        load(s, case, phis, states)
        status = s.solve_stationary()
        assert (status == 0).all(), (case.name, status)
        c, phi = s.get_state(derived=False)
        lin = [(case.make(phis[b]), c[b], phi[b]) for b in range(B)]
        tables = EC.chain_tables(case.N)
        kin = s.get_kinetics(tables, fields=('theta',))
        assert (kin['status'] == 0).all(), kin['status']
        p, c0, phi0 = lin[0]
        k0 = ER.kinetic(tables, phis[0], c0[:, 0], phi0[0], kin['theta'][0], 0.0, w=1, CS=case.CS, phi_pzc=0.0)
        Tf = ER.transfer(p, c0, phi0, 0.0)
        X = k0['Kc'] @ Tf[:case.N, :case.N] + np.outer(k0['Kphi'][:, 1], Tf[case.N, :case.N])
        rf = 0.5 / np.abs(X).sum(axis=1).max()
        _cache[key] = (s, case, phis, lin, tables, kin['theta'], rf)
    return _cache[key]


def call(s, tables, omegas, theta, rf, **kw):
    kw.setdefault('fields', EFIELDS + ['Kc', 'Kphi', 'residual'])
    out = s.get_impedance(tables, omegas, theta=theta, rf=rf, **kw)
    assert s._impedance.last_kernel_ms > 0.0
    return out


def reference(name, method):
    """[B][F] dicts of eis_ref.electrode with the kinetic admittance of eis_ref.kinetic at the device's state"""
    key = ('ref', name, method)
    if key not in _cache:
        s, case, phis, lin, tables, theta, rf = prepared(name)
        rows = []
        for b, (p, c, phi) in enumerate(lin):
            row = []
            for om in omegas_of(case):
                k = ER.kinetic(tables, phis[b], c[:, 0], phi[0], theta[b], om, w=1, CS=case.CS, phi_pzc=0.0)
                row.append(ER.electrode(p, c, phi, om, k['Kc'], k['Kphi'], rf, method))
            rows.append(row)
        _cache[key] = (_Closed(), rows)
    return _cache[key][1]


@pytest.mark.parametrize('name', sorted(ELECTROLYTES))
def test_the_coupled_electrode_against_the_reference(name):
    s, case, phis, lin, tables, theta, rf = prepared(name)
    omegas = omegas_of(case)
    before = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    got = call(s, tables, omegas, theta, rf)
    assert (got['status'] == 0).all(), got['status']
    assert got['residual'].max() <= 1e-8
    for k in EFIELDS + ['Kc', 'Kphi']:
        assert got[k].dtype == np.complex128 and (got[k][:, 0].imag == 0).all(), k          # omega = 0: exact zeros
    ra, rb = reference(name, 'banded'), reference(name, 'elimination')
    worst, worst_dis, where = 0.0, 0.0, ''
    for b in range(B):
        for f in range(len(omegas)):
            assert ra[b][f]['status'] == 0 and ra[b][f]['cond'] <= 1e3, (name, b, f, ra[b][f]['cond'])
            dis = ER.disagreement(rb[b][f], ra[b][f])
            err = ER.disagreement({k: got[k][b, f] for k in EFIELDS}, ra[b][f])
            for k in EFIELDS:
                assert dis[k] < 1e-8, (name, b, f, k, dis[k])
                tol = max(10.0 * dis[k], 1e-11)
                if err[k] / tol > worst:
                    where = 'point %d, omega %d, %s: error %.2e, reference disagreement %.2e' % (b, f, k, err[k], dis[k])
                worst, worst_dis = max(worst, err[k] / tol), max(worst_dis, dis[k])
    print('%s: worst device error / tolerance %.3f (reference disagreement up to %.1e; %s); rf %.3e, |Y| %.2e .. %.2e, faradaic share %.2f'
          % (name, worst, worst_dis, where, rf, np.abs(got['admittance']).min(), np.abs(got['admittance']).max(),
             np.abs(got['faradaic'][:, 1] / got['admittance'][:, 1]).max()))
    assert worst <= 1.0, (name, worst, where)
    # the pieces add up, and dtheta is the chain rule on the returned pieces
    assert np.array_equal(got['admittance'], got['double_layer'] + got['faradaic'])
    full = call(s, tables, omegas, theta, rf, fields=None)
    assert full['dtheta'].shape == (B, 3, 3) and np.isfinite(full['dtheta']).all() and 'dy' not in full
    assert np.array_equal(full['admittance'], got['admittance']) and np.array_equal(full['impedance'], 1.0 / got['admittance'])
    assert np.array_equal(full['polarization_resistance'], 1.0 / got['admittance'][:, 0].real)
    # the sites stay conserved: sum_t n_t dtheta_t = 0 (relative to the largest term)
    assert np.abs(full['dtheta'].sum(axis=2)).max() <= 1e-8 * np.abs(full['dtheta']).max()
    after = s.get_state(derived=False) + (s.get_status(), s.newton_iterations())
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


@pytest.mark.parametrize('N', range(1, 9))
def test_every_block_size_runs_its_own_instance(N):
    """Each of the eight compiled instances on three lanes the device solved from the bulk state (nx = 5): the instance launched is the one
    of the block size, and its transfer functions meet the reference linearised at the device's state under the rule above"""
    case = RC.small(N, 5, stern=True)
    phis = case.phiM * np.array([0.1, 0.2, 0.3])
    omegas = omegas_of(case)[[0, 2]]
    with open_solver(case, 3) as s:
        load(s, case, phis, [case.bulk_state()] * 3)
        assert (s.solve_stationary() == 0).all()
        c, phi = s.get_state(derived=False)
        got = s.get_impedance(EC.chain_tables(N), omegas, rf=1.0, fields=['admittance', 'Tc', 'Tphi', 'tc', 'tphi'])
        assert s._impedance.last_kernel == 'cateis::electrode_kernel<%d>' % (N + 1) and s._impedance.last_kernel in INSTANCES
    assert (got['status'] == 0).all() and np.isfinite(got['admittance']).all() and (got['Tc'][:, 0].imag == 0).all()
    worst = 0.0
    for b in range(3):
        p = case.make(phis[b])
        for f, om in enumerate(omegas):
            Ta, Tb = ER.transfer(p, c[b], phi[b], om, 'banded'), ER.transfer(p, c[b], phi[b], om, 'elimination')
            dis = RR.rel_rows(Tb, Ta)
            assert dis < 1e-8
            dev = np.zeros((N + 1, N + 1), complex)
            dev[:N, :N], dev[N, :N], dev[:N, N], dev[N, N] = got['Tc'][b, f], got['Tphi'][b, f], got['tc'][b, f], got['tphi'][b, f]
            worst = max(worst, RR.rel_rows(dev, Ta) / max(10.0 * dis, 1e-11))
    print('N = %d: transfer functions of electrode_kernel<%d> against the reference: worst error / tolerance %.3f' % (N, N + 1, worst))
    assert worst <= 1.0


@pytest.mark.parametrize('name', ['N=3 nx=21', 'G8 nx=34', 'steric'])
def test_transfer_functions_against_the_existing_libraries(name):
    s, case, phis, lin, tables, theta, rf = prepared(name)
    omegas = omegas_of(case)
    N = case.N
    got = call(s, tables, omegas, theta, rf, fields=['Tc', 'Tphi', 'tc', 'tphi'])
    blocked = call(s, tables, omegas, theta, 0.0, fields=['admittance', 'faradaic', 'dflux', 'dc_surface', 'dphi_surface'])
    assert (blocked['status'] == 0).all() and (blocked['dflux'] == 0).all() and (blocked['faradaic'] == 0).all()
    tols = np.zeros((B, len(omegas)))
    for b, (p, c, phi) in enumerate(lin):
        for f, om in enumerate(omegas):
            dis = RR.rel_rows(ER.transfer(p, c, phi, om, 'elimination'), ER.transfer(p, c, phi, om, 'banded'))
            assert dis < 1e-8
            tols[b, f] = max(10.0 * dis, 1e-11)
    worst, exact = 0.0, True

    def compare(a, r):
        nonlocal worst, exact
        for b in range(B):
            for f in range(len(omegas)):
                worst = max(worst, RR.rel_rows(np.atleast_1d(a[b, f]).reshape(1, -1), np.atleast_1d(r[b, f]).reshape(1, -1)) / tols[b, f])
        exact = exact and np.array_equal(a, r)
    for j in range(N):
        r = s.get_response(omega=omegas, perturbation=('flux', j))
        assert (r['status'] == 0).all()
        compare(got['Tc'][:, :, :, j], r['dc_surface'])
        compare(got['Tphi'][:, :, j], r['dphi_surface'])
    r = s.get_response(omega=omegas, perturbation='phiM')
    compare(got['tc'], r['dc_surface'])
    compare(got['tphi'], r['dphi_surface'])
    compare(blocked['admittance'], r['admittance'])
    compare(blocked['dc_surface'], r['dc_surface'])
    zero = {'flux': np.zeros((B, N)), 'dflux_dc': np.zeros((B, N, N)), 'dflux_dphi': np.zeros((B, N, 2))}
    cp = s.get_coupling(np.zeros((B, N)), zero, fields=['T_c', 'T_phi'])
    for b in range(B):
        worst = max(worst, CR.rel_T(got['Tc'][b, 0].real, cp['T_c'][b]) / tols[b, 0], CR.rel(got['Tphi'][b, 0].real, cp['T_phi'][b]) / tols[b, 0])
    print('%s: transfer functions against get_response / get_coupling: worst difference / tolerance %.3f; bit-identical to get_response: %s'
          % (name, worst, exact))
    assert worst <= 1.0


@pytest.mark.parametrize('name', ['N=3 nx=21', 'G8 nx=7'])
def test_waves_lanes_outputs_frequencies_and_workspace_do_not_change_the_bits(name, monkeypatch):
    s, case, phis, lin, tables, theta, rf = prepared(name)
    omegas = omegas_of(case)
    rng = np.random.RandomState(11)
    lanes = np.concatenate([rng.permutation(B), rng.randint(0, B, 18)])          # 23 systems x 3 frequencies: more than one wave's teams
    keys = EFIELDS + ['Kc', 'Kphi', 'residual', 'status']
    base = call(s, tables, omegas, theta, rf)
    want = call(s, tables, omegas, theta[lanes], rf, lanes=lanes)
    for k in keys:
        assert np.array_equal(want[k], base[k][lanes]), k
    same(call(s, tables, omegas, theta[lanes], rf, lanes=lanes, max_waves=1), want, keys)
    same(call(s, tables, omegas, theta[lanes], rf, lanes=lanes, max_waves=2), want, keys)
    for fields in (['admittance'], ['dflux', 'tphi'], ['Tc', 'dc_surface', 'Kphi'], ['dsigma', 'residual']):
        got = call(s, tables, omegas, theta[lanes], rf, lanes=lanes, fields=fields)
        assert sorted(k for k in got if k in _eis.FIELDS or k == 'status') == sorted(fields + ['status'])
        same(got, want, fields + ['status'])
    for f in range(len(omegas)):
        got = call(s, tables, omegas[f:f + 1], theta[lanes], rf, lanes=lanes)
        for k in keys:
            if k != 'residual':
                assert np.array_equal(got[k][:, 0], want[k][:, f]), (k, f)
    monkeypatch.setenv('CATEIS_WORKSPACE_BYTES', '1')          # 64 pairs per turn: 69 pairs in two turns
    same(call(s, tables, omegas, theta[lanes], rf, lanes=lanes), want, keys)


def test_an_unsolved_lane_and_perturbed_coverages_report_in_their_lane_only():
    case = RC.Case('unconverged', RC.D2, RC.Q2, [100.0, 100.0], RC.kornyshev().x, -0.8, CS=0.2, radii=[4e-10, 4e-10])
    tables = EC.chain_tables(2)
    om = [0.0, 1e4]
    results = []
    for phis in (np.zeros(B), np.array([0.0, 0.0, -0.8, 0.0, 0.0])):
        with open_solver(case, B, maxit=1) as s:
            load(s, case, phis, [case.bulk_state()] * B)
            status = s.solve_stationary()
            theta = s.get_kinetics(tables, fields=('theta',))['theta']
            if phis.any():
                theta[2] = results[0][2][2]
            results.append((status, call(s, tables, om, theta, 1.0), theta))
            if not phis.any():
                off = theta.copy()
                off[4] *= np.array([1.0 - 1e-4, 1.0 + 1e-3, 1.0])
                moved = call(s, tables, om, off, 1.0)
    (st0, clean, _), (st1, got, _) = results
    assert (st0 == 0).all() and st1[2] != 0 and (np.delete(st1, 2) == 0).all()
    assert (clean['status'] == 0).all()
    keys = EFIELDS + ['Kc', 'Kphi']
    assert (got['status'][2] == 2).all() and (np.delete(got['status'], 2, axis=0) == 0).all()
    assert np.isnan(got['residual'][2])
    for k in keys:
        assert np.isnan(got[k][2]).all(), k
        assert np.array_equal(np.delete(got[k], 2, axis=0), np.delete(clean[k], 2, axis=0)), k
    assert (moved['status'][4] == 4).all() and (np.delete(moved['status'], 4, axis=0) == 0).all()
    assert moved['residual'][4] > 1e-8 and np.isfinite(moved['admittance'][4]).all()
    for k in keys:
        assert np.array_equal(np.delete(moved[k], 4, axis=0), np.delete(clean[k], 4, axis=0)), k


def test_a_singular_closure_is_reported_for_its_lane_only():
    """A step that RELEASES the species it consumes (nu = +1 on the adsorbing species) makes Kc positive against a positive T_c: the
    scalar 1 - rf (Kc T_c + Kphi0 T_phi) of N = 1 vanishes at rf = 1 / (Kc T_c + Kphi0 T_phi), formed from the returned pieces of one
    lane"""
    s, case, phis, lin, _, _, _ = prepared('N=1 nx=21')
    tables = EC.chain_tables(1)
    tables['nu'] = -tables['nu']
    theta = s.get_kinetics(tables, fields=('theta',))['theta']
    first = call(s, tables, [0.0], theta, 1.0, fields=['Kc', 'Kphi', 'Tc', 'Tphi', 'admittance', 'dflux'])
    x = (first['Kc'][:, 0, 0, 0] * first['Tc'][:, 0, 0, 0] + first['Kphi'][:, 0, 0, 1] * first['Tphi'][:, 0, 0]).real
    lane = 2
    assert x[lane] > 0 and np.abs(x / x[lane] - 1.0)[np.arange(B) != lane].min() > 1e-6, x
    rf = 1.0 / x[lane]
    got = call(s, tables, [0.0], theta, rf, fields=['Kc', 'Kphi', 'Tc', 'Tphi', 'admittance', 'dflux'])
    want = np.zeros((B, 1), np.int32)
    want[lane] = 3
    assert np.array_equal(got['status'], want), got['status']
    same(got, first, ['Kc', 'Kphi', 'Tc', 'Tphi'])
    ok = call(s, tables, [0.0], theta, 0.5 * rf, fields=['admittance'])
    assert (ok['status'] == 0).all()


def test_a_wall_table_is_refused():
    case = RC.case_G(5)
    with open_solver(case, 2) as s:
        load(s, case, np.array([-0.01, -0.02]), [case.bulk_state()] * 2)
        sp, nu, k, al, sat = case.wall
        s.set_wall_kinetics(sp, nu, np.tile(np.asarray(k, float), (2, 1)), al, sat)
        with pytest.raises(ValueError, match='wall table'):
            s.get_impedance(EC.chain_tables(case.N), [0.0])


# ---- end to end --------------------------------------------------------------------------------------------------------------------
E2E_PHI, E2E_DELTA, E2E_TAU = -0.34, 4e-3, 2e-9
E2E_PHIS = [E2E_PHI - E2E_DELTA, E2E_PHI - 0.5 * E2E_DELTA, E2E_PHI, E2E_PHI + 0.5 * E2E_DELTA, E2E_PHI + E2E_DELTA]


def e2e_run(impedance, charged=False, tau=E2E_TAU, **micro):
    """(transport, result of run_scf_cycle) of the end-to-end chemistry of tests/test_gpu_kinetics.py at the five potentials.  charged: the
    second step also releases two HCO3- per CO (the anion of this four-species electrolyte in the place of the two OH- of
    CO2* + H2O + 2 e- -> CO + 2 OH-), so that the mechanism carries the current -2 F per turnover"""
    import collections
    from catint_amd.calculator import Calculator
    from catint_amd.transport import Transport
    from tests.test_gpu_kinetics import e2e_model
    species = collections.OrderedDict([('K+', {'bulk_concentration': 100.0}), ('HCO3-', {'bulk_concentration': 100.0}),
                                       ('CO2', {'bulk_concentration': 34.0}), ('CO', {'bulk_concentration': 0.0})])
    tp = Transport(species=species, system={'phiM': E2E_PHIS[0], 'boundary thickness': 4e-8, 'Stern capacitance': 20.0, 'phiPZC': 0.1}, nx=64,
                   descriptors={'phiM': E2E_PHIS})
    tables = e2e_model(tp).tables()
    if charged:
        tables['nu'] = np.array(tables['nu'], float)
        assert tables['nu'].shape == (2, 4) and tables['nu'][1, 3] == 1.0 and tables['nu'][1, 1] == 0.0
        tables['nu'][1, 1] = 2.0
    calc = Calculator(transport=tp, calc='comsol', tau_scf=tau)
    calc.set_microkinetics(tables, site_density=2e-6, impedance=impedance, **micro)
    return tp, calc.run_scf_cycle(max_iter=400)


def slope_check(tp, out, label):
    """Re Y(0) of the middle lane against the central differences of the converged current sum_k q_k flux_k"""
    q = np.asarray(tp.charges, float)
    assert q[0] > 0 and q[1] < 0 and (q[2:] == 0).all()
    flux = out['flux']
    j_fd1 = float(q @ (flux[4] - flux[0])) / (2.0 * E2E_DELTA)
    j_fd2 = float(q @ (flux[3] - flux[1])) / E2E_DELTA
    j_tol = 2.0 * abs(j_fd1 - j_fd2) + 2.0 * E2E_TAU * np.abs(q * flux).max() / E2E_DELTA
    y0 = out['impedance']['admittance'][2, 0].real
    print('end to end (%s): delta %.1e V; Re Y(0) %.6e against FD(delta/2) %.6e (FD(delta) %.6e) A m^-2 V^-1, tolerance %.2e, error / tolerance %.3f'
          % (label, E2E_DELTA, y0, j_fd2, j_fd1, j_tol, abs(y0 - j_fd2) / j_tol if j_tol > 0 else 0.0))
    assert abs(y0 - j_fd2) <= j_tol
    return y0, j_fd2


def test_end_to_end_slope_of_the_polarisation_curve_and_the_calculator_option():
    omega = [0.0, 1e3, 1e6]
    tp, out = e2e_run(omega, scf='newton')
    assert out['converged'].all() and not out['failed'].any()
    imp = out['impedance']
    assert sorted(imp) == ['admittance', 'double_layer', 'faradaic', 'impedance', 'omega', 'status']
    assert (imp['status'] == 0).all() and imp['admittance'].shape == (5, 3) and np.array_equal(imp['omega'], omega)
    assert (imp['admittance'][:, 0].imag == 0).all() and (imp['double_layer'][:, 0] == 0).all()
    for i in range(5):
        d = tp.alldata[i]['system']['impedance']
        assert sorted(d) == sorted(imp) and np.array_equal(d['omega'], omega)
        for k in ('admittance', 'impedance', 'faradaic', 'double_layer', 'status'):
            assert np.array_equal(d[k], imp[k][i]), k
    slope_check(tp, out, 'the neutral mechanism of tests/test_gpu_couple.py: no current on either side')
    # the option changes no other number
    tp0, plain = e2e_run(None, scf='newton')
    assert 'impedance' not in plain and 'impedance' not in tp0.alldata[0]['system']
    for k in plain:
        assert np.array_equal(np.asarray(plain[k]), np.asarray(out[k]), equal_nan=True), k
    for i in range(5):
        a, b = tp0.alldata[i], tp.alldata[i]
        assert sorted(a['system']) == sorted(k for k in b['system'] if k != 'impedance')
        assert all(np.array_equal(a['system'][k], b['system'][k]) for k in a['system'])
        assert all(a['species'][sp][k] == b['species'][sp][k] for sp in a['species'] for k in a['species'][sp])


def test_end_to_end_slope_with_a_charged_product():
    """The same case with two anions released per CO: the faradaic admittance at omega = 0 is not zero, and the finite difference of the
    converged current is its reference"""
    tp, out = e2e_run([0.0], charged=True, scf='newton')
    assert out['converged'].all() and (out['impedance']['status'] == 0).all()
    y0, fd = slope_check(tp, out, 'two HCO3- per CO')
    assert abs(fd) > 0 and out['impedance']['faradaic'][2, 0].real == y0 and (np.abs(out['flux'][:, 1]) > 0).all()


def test_the_option_on_the_mixing_loop_and_on_the_device_loop():
    """set_microkinetics(impedance=...) with scf='mixing': the call at the last transport state of the host loop (the coverages are
    solved for first), and after the hand-over of device_loop=True.  The loops stop at a change of the current of tau per iteration,
    so against the Newton loop's answer the admittance is compared to 1e-3 only"""
    omega = [0.0, 1e3]
    ref = e2e_run(omega, charged=True, scf='newton')[1]['impedance']
    for micro in (dict(), dict(device_loop=True)):
        tp, out = e2e_run(omega, charged=True, tau=1e-8, **micro)
        assert out['converged'].all(), (micro, out['iterations'])
        imp = out['impedance']
        assert sorted(imp) == ['admittance', 'double_layer', 'faradaic', 'impedance', 'omega', 'status']
        assert (imp['status'] == 0).all() and np.isfinite(imp['admittance']).all() and (imp['admittance'][:, 0].imag == 0).all()
        assert np.array_equal(tp.alldata[4]['system']['impedance']['admittance'], imp['admittance'][4])
        dev = np.abs(imp['admittance'] - ref['admittance']).max() / np.abs(ref['admittance']).max()
        print('impedance after the mixing loop (%s, %d iterations): admittance differs from the Newton loop\'s by %.1e' % (micro, out['iterations'], dev))
        assert dev <= 1e-3
