"""Electrolyte observables derived on the device (libcatint_observe, PnpSolver.get_electrolyte, Calculator(derive_on_device=True))
against a NumPy restatement of their definitions (include/catint_observe.h) written here.

Tolerance: the project's fp64 parity tolerance, max|gpu - ref| <= 1e-9 * scale per output array, with scale = max|ref| for the field,
the charge density, gamma, the pH and the conductivity; for the current density the largest sum of the ABSOLUTE terms of an edge,
max_e sum_k |q_k| D_k / h_e (|B(-u)| c_{e+1} + |B(u)| c_e) (the current itself is a difference of them and may vanish); for the two
potential drops the running sum of that bound times h / kappa.  The states make the current a real difference of its terms (|i_el| is
0.1 .. 0.4 of their absolute sum: checked below without a device), so these scales are not generous; on an MI355X the kernel and this
restatement (other summation orders, other exponential) differ by at most 5.7e-16 of them over all cases.
"""
import importlib.util
import os

import numpy as np
import pytest

from catint_amd import PnpSolver, _observe          # fails without the feature
from catint_amd.units import unit_F, unit_R, unit_eps0

N_AVOGADRO = 6.022140857e23
BETA = 1.0 / (unit_R * 298.15)
EPS = 78.36 * unit_eps0
TOL = 1e-9
ROWS = tuple(_observe.FIELDS)


# ---- the comparator ----------------------------------------------------------------------------------------------------------------
def bernoulli(u):
    small = np.abs(u) < 0.05
    us = np.where(small, u, 0.0)
    u2 = us * us
    series = 1.0 - 0.5 * us + u2 * (1.0 / 12.0 + u2 * (-1.0 / 720.0 + u2 * (1.0 / 30240.0)))
    ul = np.where(small, 1.0, u)
    return np.where(small, series, ul / np.expm1(ul))


def reference(c, phi, x, D, q, radii=None, velocity=0.0, sH=-1, sOH=-1, beta=BETA):
    """(outputs, scales): every row of catobs_outputs from c [B][N][nx], phi [B][nx], and the scale its tolerance refers to."""
    B, N, nx = c.shape
    D, q, x = np.asarray(D, float), np.asarray(q, float), np.asarray(x, float)
    h = np.diff(x)
    E = np.empty((B, nx))
    E[:, 1:-1] = -(phi[:, 2:] - phi[:, :-2]) / (x[2:] - x[:-2])
    E[:, 0] = -(phi[:, 1] - phi[:, 0]) / h[0]
    E[:, -1] = -(phi[:, -1] - phi[:, -2]) / h[-1]
    rho = (q[None, :, None] * c).sum(axis=1)
    vol = N_AVOGADRO * (np.zeros(N) if radii is None else np.asarray(radii, float)) ** 3
    phi0 = (vol[None, :, None] * c).sum(axis=1)
    gamma = 1.0 / (1.0 - phi0)
    w = -np.log1p(-phi0)
    with np.errstate(divide='ignore', invalid='ignore'):
        if sH >= 0:
            pH = -np.log10(c[:, sH] / 1000.0) - np.log10(gamma)
        elif sOH >= 0:
            pH = 14.0 + np.log10(c[:, sOH] / 1000.0) - np.log10(gamma)
        else:
            pH = np.full((B, nx), np.nan)
    cl, cr = c[:, :, :-1], c[:, :, 1:]
    kappa = beta * ((q ** 2 * D)[None, :, None] * 0.5 * (cl + cr)).sum(axis=1)
    u = (q * beta)[None, :, None] * np.diff(phi, axis=1)[:, None, :] + np.diff(w, axis=1)[:, None, :] - velocity * h[None, None, :] / D[None, :, None]
    Bp = bernoulli(u)
    Bm = Bp + u
    Dh = D[None, :, None] / h[None, None, :]
    J = -Dh * (Bm * cr - Bp * cl)
    Jd = -Dh * (cr - cl)
    iel = (q[None, :, None] * J).sum(axis=1)
    idf = (q[None, :, None] * Jd).sum(axis=1)
    bound = (np.abs(q)[None, :, None] * Dh * (np.abs(Bm) * np.abs(cr) + np.abs(Bp) * np.abs(cl))).sum(axis=1)
    zero = np.zeros((B, 1))
    with np.errstate(divide='ignore', invalid='ignore'):
        on = kappa > 0
        diR = np.concatenate([zero, np.cumsum(np.where(on, -iel / kappa, 0.0) * h[None, :], axis=1)], axis=1)
        ddf = np.concatenate([zero, np.cumsum(np.where(on, idf / kappa, 0.0) * h[None, :], axis=1)], axis=1)
        drop_scale = np.cumsum(np.where(on, bound / kappa, 0.0) * h[None, :], axis=1).max()
    out = {'efield': E, 'charge_density': rho, 'gamma': gamma, 'pH': pH, 'conductivity': kappa, 'current_density': iel, 'dphi_iR': diR,
           'dphi_diff': ddf}
    dinf = phi[:, -1] - phi[:, 0]
    out['scalars'] = np.stack([phi[:, 0], E[:, 0], gamma[:, 0], pH[:, 0], diR[:, -1], ddf[:, -1], dinf, dinf - diR[:, -1], iel[:, 0],
                               kappa[:, -1]], axis=1)
    amax = lambda a: float(np.nanmax(np.abs(a))) if np.isfinite(a).any() else 1.0
    scales = {'efield': amax(E), 'charge_density': amax(rho), 'gamma': amax(gamma), 'pH': amax(pH), 'conductivity': amax(kappa),
              'current_density': float(bound.max()), 'dphi_iR': float(drop_scale), 'dphi_diff': float(drop_scale)}
    scales['scalars'] = np.array([amax(phi), scales['efield'], scales['gamma'], scales['pH'], drop_scale, drop_scale, amax(phi),
                                  max(amax(phi), drop_scale), scales['current_density'], scales['conductivity']])
    scales['ratio'] = float(np.median(np.abs(iel) / bound))
    return out, scales


# ---- arbitrary (not solved) states ----------------------------------------------------------------------------------------------------
class Case(object):
    def __init__(self, N, nx, B, steric=False, graded=False, velocity=0.0, max_waves=0, table=True):
        self.N, self.nx, self.B, self.steric, self.graded, self.velocity, self.max_waves, self.table = N, nx, B, steric, graded, velocity, max_waves, table

    @property
    def id(self):
        return 'N%d-nx%d-B%d%s%s%s%s' % (self.N, self.nx, self.B, '-steric' if self.steric else '', '-graded' if self.graded else '',
                                         '-conv' if self.velocity else '', '-waves%d' % self.max_waves if self.max_waves else '')

    def instance(self):
        m = self.nx - 2
        P, WY = (16, 4) if m > 2048 else (16, 2) if m > 1024 else (next(p for p in (1, 2, 4, 8, 16) if m <= 64 * p), 1)
        return 'catobs::electrolyte_kernel<%d, %d, %s>' % (P, WY, 'true' if self.steric else 'false')

    def problem(self):
        N, nx = self.N, self.nx
        z = np.array([1, -1, 2, -1, 0, 1, -2, -1][:N], float)
        D = 1e-9 * (1.0 + 0.3 * np.arange(N))
        radii = 3e-10 * (1.0 + 0.1 * np.arange(N)) if self.steric else None
        x = np.concatenate([[0.0], np.cumsum(1e-10 * 1.04 ** np.minimum(np.arange(nx - 1), 150))]) if self.graded else np.arange(nx) * 2e-10
        # the pH comes from H+ (species 0) in the cases with an even number of grid points, from OH- (the last species) in the others
        sH, sOH = (0, -1) if nx % 2 == 0 else (-1, N - 1)
        return z * unit_F, D, radii, x, sH, sOH

    def state(self, seed=0):
        """Smooth positive concentrations and a random-walk potential: steps of 5 .. 15 mV make |i_el| 0.1 .. 0.4 of the sum of its absolute terms"""
        rng = np.random.RandomState(1000 * self.nx + self.N + seed)
        B, N, nx = self.B, self.N, self.nx
        s = np.linspace(0.0, 1.0, nx)
        f = rng.uniform(0.5, 3.0, (B, N, 1))
        p = rng.uniform(0.0, 2 * np.pi, (B, N, 1))
        cb = 10.0 * (1.0 + np.arange(N))[None, :, None] * rng.uniform(0.5, 1.5, (B, N, 1))
        c = cb * np.exp(0.5 * np.sin(2 * np.pi * f * s[None, None, :] + p))
        steps = rng.uniform(0.005, 0.015, (B, nx)) * rng.choice([-1.0, 1.0], (B, nx))
        phi = np.cumsum(steps, axis=1)
        return np.ascontiguousarray(c), np.ascontiguousarray(phi)

    def solver(self):
        q, D, radii, x, _, _ = self.problem()
        s = PnpSolver(self.N, self.nx, float(x[1] - x[0]), 1.0, BETA, EPS, D, q, method='Newton', batch_capacity=self.B)
        s.set_newton(wall_bc='stern', stern_capacitance=0.2, mpb_radius=radii)
        if self.graded:
            s.set_grid(x)
        if self.velocity:
            s.set_convection(self.velocity)
        return s

    def upload(self, s, c, phi):
        B = len(c)
        s.set_batch(c, np.zeros((B, 4)), np.zeros(B), np.zeros((B, self.N)))
        s.set_potential(phi)

    def reference(self, c, phi):
        q, D, radii, x, sH, sOH = self.problem()
        return reference(c, phi, x, D, q, radii, self.velocity, sH, sOH)

    def derive(self, s, **kw):
        _, _, _, _, sH, sOH = self.problem()
        kw.setdefault('max_waves', self.max_waves)
        return s.get_electrolyte(species_H=sH, species_OH=sOH, **kw)


CASES = [
    # the shapes of the issue: (N, nx, B)
    Case(1, 5, 3), Case(3, 66, 37), Case(3, 67, 37, steric=True, graded=True), Case(8, 130, 37, steric=True, velocity=0.3),
    Case(5, 259, 5), Case(7, 514, 5), Case(4, 1026, 3), Case(7, 1027, 2), Case(2, 2051, 2, steric=True), Case(2, 4098, 2),
    # every wave walks several operating points, the last round is ragged (300 = 37 * 8 + 4)
    Case(3, 67, 300, steric=True, graded=True, max_waves=8),
    # the instances the shapes above leave out (every instance is steric or not: both are compiled)
    Case(2, 34, 4, steric=True, table=False), Case(2, 100, 4, table=False), Case(3, 200, 3, velocity=-0.2, table=False),
    Case(3, 258, 3, steric=True, table=False), Case(3, 300, 3, steric=True, graded=True, table=False), Case(2, 1000, 2, steric=True, table=False),
    Case(2, 2050, 2, steric=True, table=False),
]


def test_the_states_are_the_ones_the_tolerance_was_worked_out_for():
    """No device: the cases cover every compiled instance, and the random-walk potential makes the current a real difference of its terms."""
    from tests.test_observe_abi import INSTANCES
    assert {c.instance() for c in CASES} == INSTANCES
    for case in CASES:
        if case.nx > 600 or case.B > 40:
            continue
        _, scales = case.reference(*case.state())
        assert 0.1 <= scales['ratio'] <= 0.4, (case.id, scales['ratio'])


@pytest.fixture(scope='module')
def derived():
    """Every case once: {case id: (device outputs, reference outputs, scales, kernel name)}."""
    out = {}
    for case in CASES:
        c, phi = case.state()
        with case.solver() as s:
            case.upload(s, c, phi)
            got = case.derive(s)
            name = s._observer.last_kernel
        ref, scales = case.reference(c, phi)
        out[case.id] = (got, ref, scales, name)
    return out


def assert_close(got, ref, scales, what):
    for key in ROWS + ('scalars',):
        err = np.abs(got[key] - ref[key])
        rel = (err / scales[key]).max() if key == 'scalars' else err.max() / scales[key]
        print('%s %s: max|gpu - ref| / scale = %.3e' % (what, key, rel))
        assert np.isfinite(got[key]).all(), (what, key)
        assert rel <= TOL, (what, key, rel)


# ---- (a) parity on arbitrary states ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_arbitrary_state_parity(case, derived):
    got, ref, scales, name = derived[case.id]
    assert name == case.instance()
    for key in ROWS:
        assert got[key].shape == ref[key].shape
    assert_close(got, ref, scales, case.id)


# ---- (b) every compiled instance was run ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_compiled_instance_is_run(derived):
    from catint_amd.build import OBSERVE_LIB
    from tests import kernel_census as K
    launched = {name for (_, _, _, name) in derived.values()}
    assert launched == K.compiled_kernels(lib=OBSERVE_LIB)


# ---- (c) null outputs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('case', [CASES[2], CASES[3], Case(2, 1030, 3)], ids=lambda c: c.id)
def test_null_outputs_leave_the_others_bit_for_bit(case):
    c, phi = case.state()
    with case.solver() as s:
        case.upload(s, c, phi)
        full = case.derive(s)
        subsets = [((r,), False) for r in ROWS] + [((), True), (('efield', 'pH'), False), (('current_density',), True),
                                                   (tuple(r for r in ROWS if r != 'dphi_iR'), True), (('dphi_diff', 'gamma'), False)]
        for rows, scalars in subsets:
            got = case.derive(s, fields=list(rows), scalars=scalars)
            assert sorted(got) == sorted(rows + (('scalars',) if scalars else ()))
            for key in got:
                assert np.array_equal(got[key], full[key]), (rows, scalars, key)
    sc = full['scalars']
    for col, (row, idx) in enumerate([(phi, 0), (full['efield'], 0), (full['gamma'], 0), (full['pH'], 0), (full['dphi_iR'], -1),
                                      (full['dphi_diff'], -1), (None, None), (None, None), (full['current_density'], 0),
                                      (full['conductivity'], -1)]):
        if row is not None:
            assert np.array_equal(sc[:, col], row[:, idx]), col
    assert np.array_equal(sc[:, 6], phi[:, -1] - phi[:, 0])
    assert np.array_equal(sc[:, 7], (phi[:, -1] - phi[:, 0]) - full['dphi_iR'][:, -1])


# ---- (d) operating points are independent; the handle is only read ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('case', [Case(3, 67, 37, steric=True, graded=True, max_waves=5), Case(2, 1100, 7, max_waves=6)], ids=lambda c: c.id)
def test_operating_points_are_independent(case):
    c, phi = case.state()
    perm = np.random.RandomState(5).permutation(case.B)
    with case.solver() as s:
        case.upload(s, c, phi)
        status0 = s.get_status()
        full = case.derive(s)
        c1, phi1 = s.get_state(derived=False)
        assert np.array_equal(c1, c) and np.array_equal(phi1, phi) and np.array_equal(s.get_status(), status0)     # only read
        case.upload(s, c[perm], phi[perm])
        shuffled = case.derive(s)
        for key in full:
            assert np.array_equal(shuffled[key], full[key][perm]), key
        bad = case.B // 2
        cn, pn = c.copy(), phi.copy()
        cn[bad, 0, case.nx // 3] = np.nan
        pn[bad, 2] = np.nan
        case.upload(s, cn, pn)
        poisoned = case.derive(s)
        keep = np.arange(case.B) != bad
        for key in full:
            assert np.array_equal(poisoned[key][keep], full[key][keep]), key
        assert np.isnan(poisoned['scalars'][bad]).any()


@pytest.mark.gpu
def test_device_view_and_errors_on_real_handles():
    from catint_amd._capi import PnpError
    case = CASES[1]
    c, phi = case.state()
    with case.solver() as s:
        with pytest.raises(PnpError) as e:
            s.device_view()
        assert e.value.code == -4                                         # PNP_ESTATE before set_batch
        case.upload(s, c, phi)
        v = s.device_view()
        assert (v.struct_size, v.method, v.nspecies, v.nx, v.row_pitch, v.batch) == (
            __import__('ctypes').sizeof(_observe.PnpDeviceView), 2, case.N, case.nx, s.row_pitch, case.B)
        assert v.c_dev and v.phi_dev and v.status_dev and v.stream
    q, D, _, x, _, _ = case.problem()
    with PnpSolver(case.N, case.nx, float(x[1]), 1e-9, BETA, EPS, D, q, method='Crank-Nicolson', batch_capacity=2) as s:
        s.set_batch(c[:2], np.zeros((2, 4)), np.zeros(2), np.zeros((2, case.N)))
        assert s.device_view().phi_dev is None                            # the compat mode keeps no potential in its state
        with pytest.raises(_observe.ObserveError) as e:
            s.get_electrolyte()
        assert e.value.code == _observe.EINVAL


# ---- (e) physics: the current the solver conserves ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('velocity', [0.0, 0.05])
def test_stationary_solutions_carry_the_prescribed_current(velocity):
    from oracle import pnp_physical as PH
    N, nx = 3, 96
    D = np.array([1.957e-9, 1.185e-9, 1.5e-9])
    q = np.array([unit_F, -unit_F, 0.0])
    cb = np.array([10.0, 10.0, 3.0])
    dx = np.sqrt(EPS / BETA / (q ** 2 * cb).sum()) / 6.0
    fluxes = [np.zeros(N), np.array([0.02, -0.01, 0.03]), np.array([-0.015, 0.0, -0.02])]
    cs, phis = [], []
    for j in fluxes:
        p = PH.PhysicalProblem(D=D, charges=q, beta=BETA, eps=EPS, dx=dx, nx=nx, c_bulk=cb, phiM=-0.10, flux=j, stern_capacitance=0.2,
                               velocity=velocity)
        c0 = np.repeat(cb[:, None], nx, axis=1)
        c, phi, it, _ = PH.newton_step(p, c0, np.zeros(nx), c0, np.inf, tol=1e-10)
        assert it <= 50
        cs.append(c)
        phis.append(phi)
    c, phi = np.stack(cs), np.stack(phis)
    x = np.arange(nx) * dx
    ref, scales = reference(c, phi, x, D, q, None, velocity)
    with PnpSolver(N, nx, dx, 1.0, BETA, EPS, D, q, method='Newton', batch_capacity=len(fluxes)) as s:
        s.set_newton(wall_bc='stern', stern_capacitance=0.2)
        if velocity:
            s.set_convection(velocity)
        s.set_batch(c, np.zeros((len(fluxes), 4)), np.zeros(len(fluxes)), np.stack(fluxes))
        s.set_potential(phi)
        got = s.get_electrolyte()
    assert 'pH' not in got
    want = np.array([(q * j).sum() for j in fluxes])                     # F sum_k z_k j_k on every edge of a stationary solution
    err = np.abs(got['current_density'] - want[:, None]).max()
    print('stationary current: max|i_el - F sum z j| / scale = %.3e' % (err / scales['current_density']))
    assert err <= 1e-8 * scales['current_density']
    assert abs(got['scalars'][0, 4]) <= 1e-8 * scales['dphi_iR']          # zero flux: no ohmic drop
    assert np.array_equal(got['scalars'][:, 6], phi[:, -1] - phi[:, 0])
    for key in got:
        if key != 'scalars':
            assert np.abs(got[key] - ref[key]).max() <= TOL * scales[key], key


# ---- (f) the calculator's two paths ---------------------------------------------------------------------------------------------------------
def _co2r_run(derive_on_device):
    from catint_amd.calculator import Calculator
    spec = importlib.util.spec_from_file_location('co2r_physical_sweep', os.path.join(os.path.dirname(__file__), '..', 'examples',
                                                                                       'co2r_physical_sweep.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    tp, _ = ex.build(6, 96, phimin=-0.5, phimax=-0.9)
    calc = Calculator(transport=tp, calc='comsol', derive_on_device=derive_on_device)
    tp.newton = {'tol': 1e-9, 'maxit': 80}
    calc.set_surface_kinetics([{'species': 'CO2', 'rate': ex.tafel_rate(tp), 'stoichiometry': {'CO2': -1.0, 'CO': 1.0, 'OH-': 2.0}}])
    calc.run()
    assert np.all(calc.status == 0)
    return tp, calc


@pytest.mark.gpu
def test_calculator_paths_agree(tmp_path):
    from catint_amd.results_io import save_all, read_all
    from tests import results_walk
    tp_h, calc_h = _co2r_run(False)
    tp_d, calc_d = _co2r_run(True)
    assert calc_h.observables is None and calc_d.observables.shape == (6, _observe.NSCALARS)
    names = list(tp_h.species.keys())
    radii = [float(tp_h.species[sp].get('MPB_radius', 0.0)) for sp in names]
    special = {'electrolyte_current_density': 'current_density', 'delta_phi_iR': 'dphi_iR', 'delta_phi_diff': 'dphi_diff',
               'delta_phi_iR_inf': 'dphi_iR', 'delta_phi_diff_inf': 'dphi_iR', 'delta_phi_inf_min_iR': None}
    for i in range(6):
        dh, dd = tp_h.alldata[i], tp_d.alldata[i]
        c = np.array([dh['species'][sp]['concentration'] for sp in names])
        _, scales = reference(c[None], np.asarray(dh['system']['potential'])[None], tp_h.xmesh, tp_h.D, tp_h.charges, radii, 0.0,
                              names.index('H+'), -1, beta=tp_h.beta)
        assert sorted(dh['system']) == sorted(dd['system'])
        for key, a in dh['system'].items():
            b = dd['system'][key]
            if isinstance(a, str) or key == 'Stern_epsilon_func':
                assert a == b, key
                continue
            a, b = np.asarray(a, float), np.asarray(b, float)
            scale = np.abs(a).max()
            if key in special:
                scale = scales[special[key]] if special[key] else max(scales['dphi_iR'], abs(dh['system']['delta_phi_inf']))
            assert a.shape == b.shape and np.abs(a - b).max() <= TOL * max(scale, 1e-300), (i, key, np.abs(a - b).max(), scale)
        assert list(dh['species']) == list(dd['species'])
        for sp in names:
            assert sorted(dh['species'][sp]) == sorted(dd['species'][sp])
            for key, a in dh['species'][sp].items():
                a, b = np.asarray(a, float), np.asarray(dd['species'][sp][key], float)
                assert a.shape == b.shape and np.abs(a - b).max() <= TOL * max(np.abs(a).max(), 1e-300), (i, sp, key)
        o = calc_d.observables[i]
        assert o[0] == dd['system']['surface_potential'] and o[3] == dd['system']['surface_pH'] and o[4] == dd['system']['delta_phi_iR_inf']
    folder = str(tmp_path / 'CO2R_results_device')
    save_all(tp_d, folder)

    class Bare(object):
        pass
    got = results_walk.walk(read_all(Bare(), folder, only=['alldata', 'species', 'system', 'xmesh', 'descriptors', 'electrode_reactions']))
    import json
    manifest = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'results_manifest.json')))
    assert sorted(got) == sorted(manifest)
    for key, (kind, n) in manifest.items():
        assert got[key][0] == kind, (key, got[key], kind)
        if n is not None and kind in ('list', 'ndarray') and key != "descriptors['phiM']":
            assert got[key][1] == tp_d.nx, (key, got[key])
