"""The reference of the impedance tests (tests/eis_ref.py) against known answers, on the CPU.

Langmuir: one step A + * <-> A* has K_p(omega) = site_density nu rho_p i omega / (i omega + lam) in closed form
(tests/eis_cases.py: langmuir_answer).  The result is the difference of two larger terms, so errors are stated relative to their sum (the
dflux_scale convention of tests/kinetics_ref.py).  Bound: the reference forms each entry from a 2 x 2 complex solve and a sum of four
terms, a few dozen roundings of 1.1e-16 relative to the term sum; 1e-13 leaves a factor of 20 on top of that.  Measured: 1.1e-15 at
worst over omega / lam in {1e-5, 0.1, 1, 1e3} and seven points; the closed form itself against the 60-digit evaluation 1.1e-15.
K(0): the frequency-dependent matrix at omega = 0 is kinetics_ref.solve_point's, whose dflux_dc / dflux_dphi it must return to the
same bound relative to dflux_scale.
Transport: the two solvers of response_ref agree to 1e-8 on every case the device tests use (their disagreement is the tolerance source
there), the flux columns at omega = 0 are couple_ref's tangent and the phi_M column is response_ref's response.
Closure: rf = 0 is the blocking electrode, Y = i omega C_S (1 - t_phi) exactly; the complex solve_pivoted is couple_ref's on real input;
the whole chain of every device case (mechanism at the wall, rf, closure) agrees between the two transport solvers to 1e-8."""
import numpy as np
import pytest

from tests import couple_ref as CR
from tests import eis_cases as EC
from tests import eis_ref as ER
from tests import kinetics_cases as KC
from tests import kinetics_ref as KR
from tests import response_cases as RC
from tests import response_ref as RR

LANGMUIR_BOUND = 1e-13
KW = dict(w=1, CS=0.2, phi_pzc=0.05)


def test_langmuir_known_answer():
    tab = EC.langmuir_tables()
    phiM, csurf, phi0 = EC.langmuir_points()
    worst, worst_mp = 0.0, 0.0
    for i in range(len(phiM)):
        th, _, lam, _ = EC.langmuir_answer(tab, phiM[i], csurf[i, 0], phi0[i], 0.0)
        for ratio in (1e-5, 0.1, 1.0, 1e3):
            om = ratio * lam
            _, K, _, terms = EC.langmuir_answer(tab, phiM[i], csurf[i, 0], phi0[i], om)
            got = ER.kinetic(tab, phiM[i], csurf[i], phi0[i], th, om, **KW)
            assert got['residual'] < 1e-14, got['residual']
            Kg = np.concatenate([got['Kc'], got['Kphi']], axis=1)
            ok = terms > 0
            assert (Kg[~ok] == 0).all()
            err = (np.abs(Kg - K)[ok] / terms[ok]).max() if ok.any() else 0.0
            worst = max(worst, err)
            Kmp = ER.kinetic_mp(tab, phiM[i], csurf[i], phi0[i], th, om, **KW)
            worst_mp = max(worst_mp, ER.mp_err(Kmp, K, np.where(ok, terms, 1.0)))
    print('Langmuir: worst error of the reference / term sum %.2e, of the closed form against 60 digits %.2e' % (worst, worst_mp))
    assert worst <= LANGMUIR_BOUND and worst_mp <= LANGMUIR_BOUND


def test_langmuir_limits():
    """omega -> infinity: the coverages cannot follow, K is the slope at fixed theta; omega = 0: the adsorption step carries no steady flux"""
    tab = EC.langmuir_tables()
    phiM, csurf, phi0 = EC.langmuir_points()
    th, K, lam, terms = EC.langmuir_answer(tab, phiM[0], csurf[0, 0], phi0[0], 0.0)
    got = ER.kinetic(tab, phiM[0], csurf[0], phi0[0], th, 0.0, **KW)
    assert np.abs(np.concatenate([got['Kc'], got['Kphi']], axis=1)).max() <= LANGMUIR_BOUND * terms.max()
    hi = ER.kinetic(tab, phiM[0], csurf[0], phi0[0], th, 1e9 * lam, **KW)
    _, Kinf, _, _ = EC.langmuir_answer(tab, phiM[0], csurf[0, 0], phi0[0], 1e30 * lam)       # i omega / (i omega + lam) = 1
    Khi = np.concatenate([hi['Kc'], hi['Kphi']], axis=1)
    assert np.abs(Kinf.real).min() > 0
    assert np.abs(Khi - Kinf.real).max() <= 2e-9 * np.abs(Kinf).max()


@pytest.mark.parametrize('name', ['co2r_one_site', 'co2r_two_site', 'random_S1', 'random_S4', 'random_S8'])
def test_zero_frequency_is_the_steady_sensitivity(name):
    case = KC.case(name)
    t = KR._arrays(case.tables)
    worst = 0.0
    for i in range(len(case.phiM)):
        ref = KR.solve_point(t, case.phiM[i], case.csurf[i], case.phi_surface[i], **case.kw)
        assert ref['status'] == 0
        got = ER.kinetic(case.tables, case.phiM[i], case.csurf[i], case.phi_surface[i], ref['theta'], 0.0, **case.kw)
        K = np.concatenate([got['Kc'], got['Kphi']], axis=1)
        assert (K.imag == 0).all()
        want = np.concatenate([ref['dflux_dc'], ref['dflux_dphi']], axis=1)
        sc = ref['dflux_scale']
        assert (np.abs(K.real - want)[sc == 0] == 0).all()
        worst = max(worst, (np.abs(K.real - want)[sc > 0] / sc[sc > 0]).max())
        assert np.allclose(got['scale'], sc, rtol=1e-9, atol=0)
    print(name, 'K(0) against solve_point / dflux_scale: %.2e' % worst)
    assert worst <= 1e-13


ELECTROLYTES = {'N=1 nx=5': lambda: RC.small(1, 5, stern=True), 'N=1 nx=21': lambda: RC.small(1, 21, stern=True),
                'N=3 nx=5': lambda: RC.small(3, 5, stern=True), 'N=3 nx=21': lambda: RC.small(3, 21, stern=True),
                'N=4 nx=5': lambda: RC.small(4, 5, stern=True), 'N=4 nx=21': lambda: RC.small(4, 21, stern=True),
                'steric': lambda: RC.small(3, 21, stern=True, steric=True)}


def without_wall(case):
    case.wall = None
    return case


ELECTROLYTES['G8 nx=7'] = lambda: without_wall(RC.case_G8(7))
ELECTROLYTES['G8 nx=34'] = lambda: without_wall(RC.case_G8(34))
ELECTROLYTES['G nx=21'] = lambda: without_wall(RC.case_G(21))       # reactions and convection


def omegas_of(case):
    return np.array([0.0, 1.0 / case.tau_DL, 100.0 / case.tau_DL])


@pytest.mark.parametrize('name', sorted(ELECTROLYTES))
def test_the_two_transport_solvers_agree_and_match_the_existing_references(name):
    case = ELECTROLYTES[name]()
    p, c, phi = case.solve(0.5 * case.phiM)
    worst = 0.0
    for om in omegas_of(case):
        Ta, Tb = ER.transfer(p, c, phi, om, 'banded'), ER.transfer(p, c, phi, om, 'elimination')
        worst = max(worst, RR.rel_rows(Tb, Ta))
        ra = RR.response(p, c, phi, om, RR.PHIM, 'banded')
        assert np.array_equal(Ta[:p.N, p.N], ra['dc_surface']) and Ta[p.N, p.N] == ra['dphi_surface']
        if om == 0.0:
            assert (Ta.imag == 0).all()
            assert CR.rel_T(Ta[:, :p.N].real, CR.tangent_banded(p, c, phi)) < 1e-9
    print(name, 'disagreement of the two transport solvers: %.2e' % worst)
    assert worst < 1e-8


def test_blocking_electrode_and_the_pivoted_solve():
    case = RC.small(3, 21, stern=True)
    p, c, phi = case.solve(0.5 * case.phiM)
    rng = np.random.RandomState(3)
    Kc, Kphi = rng.randn(3, 3) + 1j * rng.randn(3, 3), rng.randn(3, 2) + 1j * rng.randn(3, 2)
    for om in omegas_of(case):
        Tf = ER.transfer(p, c, phi, om)
        r = ER.closure(p, Tf, Kc, Kphi, om, 0.0)
        assert r['status'] == 0 and (r['dflux'] == 0).all() and r['faradaic'] == 0
        assert r['admittance'] == 1j * om * (p.CS * (1.0 - Tf[3, 3]))
        assert np.array_equal(r['dc_surface'], Tf[:3, 3]) and r['dphi_surface'] == Tf[3, 3]
    A, b = rng.randn(5, 5), rng.randn(5)
    x, s = ER.solve_pivoted(A, b, np.abs(A).max())
    xr, sr = CR.solve_pivoted(A, b, np.abs(A).max())
    # (numpy's complex division rounds a real quotient differently from the real one: the same pivots, the last digits differ)
    assert s == sr and (x.imag == 0).all() and np.allclose(x.real, xr, rtol=1e-12, atol=0)
    A[3] = 2.0 * A[1]
    assert ER.solve_pivoted(A, b, np.abs(A).max())[1] and CR.solve_pivoted(A, b, np.abs(A).max())[1]
    z = rng.randn(4, 4) + 1j * rng.randn(4, 4)
    zb = rng.randn(4) + 1j * rng.randn(4)
    assert np.allclose(ER.solve_pivoted(z, zb, np.abs(z).max())[0], np.linalg.solve(z, zb), rtol=1e-12, atol=0)


@pytest.mark.parametrize('name', sorted(ELECTROLYTES))
def test_the_closed_electrode_agrees_between_the_two_transport_solvers(name):
    """The whole chain of the device cases on the CPU, at the oracle's state: the mechanism of tests/eis_cases.py at the wall, rf from
    the row-sum norm at omega = 0, every output of the closure by both transport solvers.  (With two like-charged species and nothing
    else the mechanism carries no current and the admittance at omega = 0 is rounding noise: such a case cannot be compared.)"""
    case = ELECTROLYTES[name]()
    p, c, phi = case.solve(0.5 * case.phiM)
    tables = EC.chain_tables(case.N)
    kin = KR.solve_point(KR._arrays(tables), p.phiM, c[:, 0], phi[0], w=1, CS=case.CS, phi_pzc=0.0, sens=False)
    assert kin['status'] == 0
    k0 = ER.kinetic(tables, p.phiM, c[:, 0], phi[0], kin['theta'], 0.0, w=1, CS=case.CS, phi_pzc=0.0)
    Tf = ER.transfer(p, c, phi, 0.0)
    rf = 0.5 / np.abs(k0['Kc'] @ Tf[:case.N, :case.N] + np.outer(k0['Kphi'][:, 1], Tf[case.N, :case.N])).sum(axis=1).max()
    worst = 0.0
    for om in omegas_of(case):
        k = ER.kinetic(tables, p.phiM, c[:, 0], phi[0], kin['theta'], om, w=1, CS=case.CS, phi_pzc=0.0)
        assert k['residual'] <= 1e-8
        ra, rb = (ER.electrode(p, c, phi, om, k['Kc'], k['Kphi'], rf, m) for m in ('banded', 'elimination'))
        assert ra['status'] == 0 and ra['cond'] <= 1e3
        dis = ER.disagreement(rb, ra)
        worst = max(worst, max(dis.values()))
        if om == 0.0:
            assert ra['double_layer'] == 0 and abs(ra['faradaic']) > 0
    print(name, 'disagreement of the closed electrode between the two solvers: %.2e (rf %.3e)' % (worst, rf))
    assert worst < 1e-8
