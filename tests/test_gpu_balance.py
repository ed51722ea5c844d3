"""Species fluxes, reaction rates, wall terms and the discrete mass balance derived on the device (libcatint_balance,
PnpSolver.get_balance, Calculator(balance_on_device=True)) against a NumPy restatement of their definitions
(include/catint_balance.h) written here -- and that restatement against the oracle the solver is tested with.

Tolerance: the project's fp64 parity tolerance, max|gpu - ref| <= 1e-9 * scale per output array, with scale = the largest sum of the
ABSOLUTE terms that enter an element of that output (the outputs are differences and may vanish): for the flux
(D_k / h_e) (|B(-u) c_{e+1}| + |B(u) c_e|), for a reaction rate |forward| + |backward|, for the source the same times the
multiplicities, for the wall flux |prescribed| + sum_r |nu wall_rate_r|, for the imbalance all of these over the control volume, for
the integrals their V-weighted sums.  MAX_IMBALANCE_REL is a ratio of an imbalance to its own scale: an error of the imbalance of
1e-9 of its scale moves it by 1e-9, so its scale is 1.
On an MI355X the kernel and this restatement (other summation orders, other exponential) differ by at most 4.1e-16 of these scales
over all cases (printed per output by the parity test; the worst one by test_every_compiled_instance_is_run).
"""
import collections
import types

import numpy as np
import pytest

from catint_amd import PnpSolver, _balance          # fails without the feature
from catint_amd.units import unit_F, unit_R, unit_eps0

N_AVOGADRO = 6.022140857e23
BETA = 1.0 / (unit_R * 298.15)
EPS = 78.36 * unit_eps0
TOL = 1e-9
ROWS = tuple(_balance.FIELDS)
COL = {n: i for i, n in enumerate(_balance.SCALARS)}


# ---- the comparator ----------------------------------------------------------------------------------------------------------------
def bernoulli(u):
    small = np.abs(u) < 0.05
    us = np.where(small, u, 0.0)
    u2 = us * us
    series = 1.0 - 0.5 * us + u2 * (1.0 / 12.0 + u2 * (-1.0 / 720.0 + u2 * (1.0 / 30240.0)))
    ul = np.where(small, 1.0, u)
    return np.where(small, series, ul / np.expm1(ul))


def control_volumes(x):
    h = np.diff(x)
    V = np.empty(len(x))
    V[1:-1] = 0.5 * (h[1:] + h[:-1])
    V[0], V[-1] = 0.5 * h[0], 0.5 * h[-1]
    return h, V


def reference(c, phi, x, D, q, flux, phiM, radii=None, velocity=0.0, reactions=(), wall=None, beta=BETA):
    """(outputs, scales): every row of catbal_outputs from c [B][N][nx], phi [B][nx], and the scale its tolerance refers to."""
    B, N, nx = c.shape
    D, q, x, flux, phiM = (np.asarray(a, float) for a in (D, q, x, flux, phiM))
    h, V = control_volumes(x)
    vol = N_AVOGADRO * (np.zeros(N) if radii is None else np.asarray(radii, float)) ** 3
    phi0 = (vol[None, :, None] * c).sum(axis=1)
    gamma = 1.0 / (1.0 - phi0)
    w = -np.log1p(-phi0)
    cl, cr = c[:, :, :-1], c[:, :, 1:]
    u = (q * beta)[None, :, None] * np.diff(phi, axis=1)[:, None, :] + np.diff(w, axis=1)[:, None, :] - velocity * h[None, None, :] / D[None, :, None]
    Bp = bernoulli(u)
    Bm = Bp + u
    Dh = D[None, :, None] / h[None, None, :]
    J = -Dh * (Bm * cr - Bp * cl)
    Ja = Dh * (np.abs(Bm * cr) + np.abs(Bp * cl))
    R = len(reactions)
    rate, rabs = np.zeros((B, R, nx)), np.zeros((B, R, nx))
    source, sabs = np.zeros((B, N, nx)), np.zeros((B, N, nx))
    for r, (lhs, rhs, kf, kr) in enumerate(reactions):
        side = []
        for idx, kk in ((lhs, kf), (rhs, kr)):
            v = np.zeros((B, nx))
            if kk != 0.0:
                v = kk * gamma ** len(idx)
                for j in idx:
                    v = v * c[:, j]
            side.append(v)
        rate[:, r] = side[0] - side[1]
        rabs[:, r] = np.abs(side[0]) + np.abs(side[1])
        for j in lhs:
            source[:, j] -= rate[:, r]
            sabs[:, j] += rabs[:, r]
        for j in rhs:
            source[:, j] += rate[:, r]
            sabs[:, j] += rabs[:, r]
    W = 0 if not wall else len(wall['species'])
    wall_rate = np.zeros((B, W))
    wall_flux, wabs = flux.copy(), np.abs(flux)
    for r in range(W):
        s = wall['species'][r]
        cs = c[:, s, 0] if s >= 0 else np.ones(B)
        al = 0.0 if wall.get('alpha') is None else wall['alpha'][r]
        ks = 0.0 if wall.get('saturation') is None else wall['saturation'][r]
        wall_rate[:, r] = np.asarray(wall['k'], float)[:, r] * cs / (1.0 + ks * cs) * np.exp(al * (phiM - phi[:, 0]))
        wall_flux += np.asarray(wall['nu'], float)[r][None, :] * wall_rate[:, r, None]
        wabs += np.abs(np.asarray(wall['nu'], float)[r][None, :] * wall_rate[:, r, None])
    imb, scl = np.zeros((B, N, nx)), np.zeros((B, N, nx))
    imb[:, :, 1:-1] = (J[:, :, :-1] - J[:, :, 1:]) / V[1:-1] + source[:, :, 1:-1]
    scl[:, :, 1:-1] = (Ja[:, :, :-1] + Ja[:, :, 1:]) / V[1:-1] + sabs[:, :, 1:-1]
    imb[:, :, 0] = (wall_flux - J[:, :, 0]) / V[0] + source[:, :, 0]
    scl[:, :, 0] = (wabs + Ja[:, :, 0]) / V[0] + sabs[:, :, 0]
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(scl > 0, np.abs(imb) / scl, 0.0)[:, :, :-1].max(axis=2)
    Vi = V[None, None, :-1]
    scalars = np.stack([wall_flux, J[:, :, -1], (Vi * source[:, :, :-1]).sum(axis=2), (Vi * imb[:, :, :-1]).sum(axis=2), ratio,
                        (V[None, None, :] * c).sum(axis=2)], axis=2)
    out = {'flux': J, 'reaction_rate': rate, 'source': source, 'wall_rate': wall_rate, 'wall_flux': wall_flux, 'imbalance': imb,
           'scalars': scalars}
    amax = lambda a: float(np.abs(a).max()) if a.size else 0.0      # noqa: E731
    scales = {'flux': amax(Ja), 'reaction_rate': amax(rabs), 'source': amax(sabs), 'wall_rate': amax(wall_rate), 'wall_flux': amax(wabs),
              'imbalance': amax(scl), 'imbalance_pointwise': scl}
    scales['scalars'] = np.array([amax(wabs), amax(Ja), amax((Vi * sabs[:, :, :-1]).sum(axis=2)), amax((Vi * scl[:, :, :-1]).sum(axis=2)), 1.0,
                                  amax((V[None, None, :] * np.abs(c)).sum(axis=2))])
    # how real a difference the flux is: |J| over the sum of its absolute terms
    scales['ratio'] = float(np.median(np.abs(J) / Ja))
    return out, scales


# ---- reaction and wall tables ---------------------------------------------------------------------------------------------------------
def reaction_table(name, N):
    """[(lhs, rhs, kf, kr)] over N species; the rate constants keep forward and backward terms within a few decades of each other at
    concentrations of 5 .. 200 mol/m^3."""
    if name == 'none':
        return []
    if name == 'abc':                    # A + B <-> C
        return [([0, 1], [2], 3.0, 40.0)]
    if name == 'dimer':                  # 2 A <-> B: a repeated species
        return [([0, 0], [1], 0.7, 25.0)]
    if name == 'empty':                  # an empty side (an excluded species of constant activity) and kr = 0
        return [([], [0], 12.5, 0.0)]
    if name == 'four':                   # four reactants on a side
        return [([0, 1, 0, 1], [N - 1], 2e-4, 30.0), ([N - 1], [0], 5.0, 0.0)]
    if name == 'buffer':                 # the shape of the CO2R table: five reactions, one with an empty side
        return [([0, 1], [2], 3.0, 40.0), ([2, 1], [3], 1.5, 60.0), ([0], [4], 9.0, 4.0), ([4, 1], [3], 0.8, 11.0), ([], [1, 5], 2.4, 0.09)]
    if name == 'many':                   # 16 reactions over 8 species
        rng = np.random.RandomState(16)
        out = []
        for r in range(16):
            nl, nr = rng.randint(1, 4), rng.randint(1, 4)
            out.append(([int(v) for v in rng.randint(0, N, nl)], [int(v) for v in rng.randint(0, N, nr)],
                        float(10.0 ** rng.uniform(0, 1) * 30.0 ** (1 - nl)), float(10.0 ** rng.uniform(0, 1) * 30.0 ** (1 - nr))))
        return out
    raise KeyError(name)


def wall_table(name, N, B, seed=0):
    rng = np.random.RandomState(77 + seed)
    if name == 'none':
        return None
    if name == 'first':
        nu = np.zeros((1, N))
        nu[0, 0], nu[0, N - 1] = -1.0, (1.0 if N > 1 else -1.0)
        return {'species': [0], 'nu': nu, 'k': rng.uniform(1e-6, 1e-5, (B, 1)), 'alpha': None, 'saturation': None}
    if name == 'zeroth':
        return {'species': [-1], 'nu': rng.choice([-1.0, 1.0, 2.0], (1, N)), 'k': rng.uniform(1e-5, 1e-4, (B, 1)), 'alpha': None, 'saturation': None}
    if name == 'eight':                  # Butler-Volmer and Langmuir factors
        return {'species': [int(v) for v in rng.randint(-1, N, 8)], 'nu': rng.choice([-2.0, -1.0, 0.0, 1.0, 2.0], (8, N)),
                'k': rng.uniform(1e-7, 1e-6, (B, 8)), 'alpha': rng.uniform(-12.0, 12.0, 8) * (rng.uniform(size=8) < 0.75),
                'saturation': rng.uniform(0.0, 0.05, 8) * (rng.uniform(size=8) < 0.6)}
    raise KeyError(name)


# ---- arbitrary (not solved) states ----------------------------------------------------------------------------------------------------
class Case(object):
    def __init__(self, N, nx, B, rx='none', wk='none', steric=False, graded=False, velocity=0.0, max_waves=0):
        self.N, self.nx, self.B, self.rx, self.wk = N, nx, B, rx, wk
        self.steric, self.graded, self.velocity, self.max_waves = steric, graded, velocity, max_waves

    @property
    def id(self):
        return 'N%d-nx%d-B%d-%s-%s%s%s%s%s' % (self.N, self.nx, self.B, self.rx, self.wk, '-steric' if self.steric else '',
                                               '-graded' if self.graded else '', '-conv' if self.velocity else '',
                                               '-waves%d' % self.max_waves if self.max_waves else '')

    def shape(self):
        m = self.nx - 2
        return (16, 4) if m > 2048 else (16, 2) if m > 1024 else (next(p for p in (1, 2, 4, 8, 16) if m <= 64 * p), 1)

    def instance(self):
        return 'catbal::species_kernel<%d, %d, %s>' % (self.shape() + ('true' if self.steric else 'false',))

    def problem(self):
        N, nx = self.N, self.nx
        z = np.array([1, -1, 2, -1, 0, 1, -2, -1][:N], float)
        D = 1e-9 * (1.0 + 0.3 * np.arange(N))
        radii = 3e-10 * (1.0 + 0.1 * np.arange(N)) if self.steric else None
        x = np.concatenate([[0.0], np.cumsum(1e-10 * 1.04 ** np.minimum(np.arange(nx - 1), 150))]) if self.graded else np.arange(nx) * 2e-10
        return z * unit_F, D, radii, x

    def tables(self):
        return reaction_table(self.rx, self.N), wall_table(self.wk, self.N, self.B, self.nx)

    def state(self, seed=0):
        """Smooth positive concentrations and a random-walk potential with steps of 5 .. 15 mV (Case.state of test_gpu_observe.py,
        restated): every flux is a real difference of its terms.  Prescribed wall fluxes of both signs, electrode potentials in -1 .. 0 V."""
        rng = np.random.RandomState(1000 * self.nx + self.N + seed)
        B, N, nx = self.B, self.N, self.nx
        s = np.linspace(0.0, 1.0, nx)
        f = rng.uniform(0.5, 3.0, (B, N, 1))
        p = rng.uniform(0.0, 2 * np.pi, (B, N, 1))
        cb = 10.0 * (1.0 + np.arange(N))[None, :, None] * rng.uniform(0.5, 1.5, (B, N, 1))
        c = cb * np.exp(0.5 * np.sin(2 * np.pi * f * s[None, None, :] + p))
        steps = rng.uniform(0.005, 0.015, (B, nx)) * rng.choice([-1.0, 1.0], (B, nx))
        phi = np.cumsum(steps, axis=1)
        flux = rng.uniform(-2e-4, 2e-4, (B, N))
        phiM = rng.uniform(-1.0, 0.0, B)
        return np.ascontiguousarray(c), np.ascontiguousarray(phi), flux, phiM

    def solver(self):
        q, D, radii, x = self.problem()
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

    def reference(self, c, phi, flux, phiM):
        q, D, radii, x = self.problem()
        rx, wk = self.tables()
        return reference(c, phi, x, D, q, flux, phiM, radii, self.velocity, rx, wk)

    def derive(self, s, bal, flux, phiM, wall=None, **kw):
        """The tables go to the library as this case states them (the handle is only the owner of the state)."""
        q, D, radii, x = self.problem()
        rx, wk = self.tables()
        kw.setdefault('max_waves', self.max_waves)
        return bal.species(s.device_view(), D, q, x, BETA, flux, phiM, mpb_radius=radii, velocity=self.velocity, reactions=rx,
                           wall=wk if wall is None else wall, **kw)


CASES = [
    # the shapes of the issue (N, nx, B), crossed with its reaction and wall tables
    Case(1, 5, 3, 'empty', 'zeroth'), Case(3, 66, 37, 'abc', 'first'), Case(3, 67, 37, 'dimer', 'none', steric=True, graded=True),
    Case(8, 130, 37, 'many', 'eight', steric=True, velocity=0.3), Case(5, 259, 5, 'four', 'none'), Case(7, 514, 5, 'none', 'first'),
    Case(4, 1026, 3, 'abc', 'zeroth'), Case(7, 1027, 2, 'buffer', 'eight'), Case(2, 2051, 2, 'dimer', 'first', steric=True),
    Case(2, 4098, 2, 'empty', 'zeroth'),
    # every wave walks several operating points, the last round is ragged (300 = 37 * 8 + 4)
    Case(3, 67, 300, 'abc', 'eight', steric=True, graded=True, max_waves=8),
    # the instances the shapes above leave out (every instance is steric or not: both are compiled), with the tables rotated on
    Case(2, 34, 4, 'four', 'eight', steric=True), Case(2, 100, 4, 'none', 'none'), Case(3, 200, 3, 'abc', 'first', velocity=-0.2),
    Case(3, 258, 3, 'dimer', 'zeroth', steric=True), Case(6, 300, 3, 'buffer', 'first', steric=True, graded=True),
    Case(2, 1000, 2, 'empty', 'eight', steric=True), Case(2, 2050, 2, 'four', 'none', steric=True),
    Case(2, 4000, 2, 'dimer', 'eight', steric=True),
]
BY_ID = {c.id: c for c in CASES}


def test_the_cases_cover_every_instance_and_every_table():
    """No device: the cases' instance names are exactly the compiled instances, every reaction and wall table of the issue is used, and
    the random-walk potential makes the flux a real difference of its terms."""
    from tests.test_balance_abi import INSTANCES
    assert {c.instance() for c in CASES} == INSTANCES
    assert {c.rx for c in CASES} >= {'none', 'abc', 'dimer', 'empty', 'four', 'many'}
    assert {c.wk for c in CASES} == {'none', 'first', 'zeroth', 'eight'}
    assert len(reaction_table('many', 8)) == 16 and {j for (l, r, _, _) in reaction_table('many', 8) for j in l + r} == set(range(8))
    for case in CASES:
        if case.nx > 600 or case.B > 40:
            continue
        _, scales = case.reference(*case.state())
        assert 0.05 <= scales['ratio'] <= 0.6, (case.id, scales['ratio'])


# ---- (a) the comparator against the oracle (no device) ----------------------------------------------------------------------------------
@pytest.mark.parametrize('N, nx, rx, wk, velocity', [(3, 41, 'abc', 'first', 0.0), (8, 57, 'many', 'eight', 0.25), (2, 30, 'four', 'zeroth', -0.1),
                                                     (6, 64, 'buffer', 'eight', 0.0)])
def test_the_comparator_states_the_oracle_s_residual(N, nx, rx, wk, velocity):
    from oracle import pnp_physical as PH
    case = Case(N, nx, 2, rx, wk, steric=True, graded=True, velocity=velocity)
    q, D, radii, x = case.problem()
    c, phi, flux, phiM = case.state()
    table, wall = case.tables()
    ref, scales = case.reference(c, phi, flux, phiM)
    h, V = control_volumes(x)
    dx = float(x[1] - x[0])
    for b in range(case.B):
        wks = [] if wall is None else [{'species': wall['species'][r], 'k': wall['k'][b, r], 'nu': wall['nu'][r],
                                        'alpha': 0.0 if wall['alpha'] is None else wall['alpha'][r],
                                        'saturation': 0.0 if wall['saturation'] is None else wall['saturation'][r]} for r in range(len(wall['species']))]
        p = PH.PhysicalProblem(D=D, charges=q, beta=BETA, eps=EPS, dx=dx, nx=nx, c_bulk=c[b, :, -1], phiM=phiM[b], flux=flux[b],
                               stern_capacitance=0.2, mpb_radius=radii, reactions=[{'lhs': l, 'rhs': r, 'kf': f, 'kr': g} for (l, r, f, g) in table],
                               wall_kinetics=wks, x=x, velocity=velocity)
        F = PH.residual(p, c[b], phi[b], c[b], np.inf)
        want = -F[:N, :-1] * D[:, None] / (dx * V[None, :-1])
        err = np.abs(ref['imbalance'][b, :, :-1] - want).max()
        assert err <= 1e-12 * scales['imbalance'], ('imbalance', err / scales['imbalance'])
        assert np.all(ref['imbalance'][b, :, -1] == 0.0)
        assert np.abs(ref['source'][b] - PH.reaction_rates(p, c[b])[0]).max() <= 1e-12 * scales['source']
        for r, wk_ in enumerate(wks):
            assert abs(ref['wall_rate'][b, r] - wk_['k'] * PH.wall_rate_law(p, wk_, c[b], phi[b])[0]) <= 1e-12 * scales['wall_rate']


# ---- (b) parity on arbitrary states -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def derived():
    """Every case once: {case id: (device outputs, reference outputs, scales, kernel name)}."""
    out = {}
    with _balance.Balancer(0) as bal:
        for case in CASES:
            c, phi, flux, phiM = case.state()
            with case.solver() as s:
                case.upload(s, c, phi)
                got = case.derive(s, bal, flux, phiM)
                name = bal.last_kernel
            ref, scales = case.reference(c, phi, flux, phiM)
            out[case.id] = (got, ref, scales, name)
    return out


def ratios(got, ref, scales):
    """{output: max|gpu - ref| / scale}; an output whose scale is 0 must be reproduced exactly (ratio 0) or counts as infinite."""
    out = {}
    for key in ROWS + ('scalars',):
        if got[key].size == 0:
            continue
        err = np.abs(got[key] - ref[key])
        if key == 'scalars':
            err, scale = err.reshape(-1, _balance.NSCALARS).max(axis=0), scales[key]
        else:
            err, scale = np.array([err.max()]), np.array([scales[key]])
        with np.errstate(divide='ignore', invalid='ignore'):
            out[key] = float(np.where(err == 0.0, 0.0, err / scale).max())
    return out


def assert_close(got, ref, scales, what, tol=TOL):
    for key, rel in ratios(got, ref, scales).items():
        print('%s %s: max|gpu - ref| / scale = %.3e' % (what, key, rel))
        assert np.isfinite(got[key]).all(), (what, key)
        assert rel <= tol, (what, key, rel)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_arbitrary_state_parity(case, derived):
    got, ref, scales, name = derived[case.id]
    assert name == case.instance()
    for key in ROWS + ('scalars',):
        assert got[key].shape == ref[key].shape, key
    assert_close(got, ref, scales, case.id)


@pytest.mark.gpu
def test_every_compiled_instance_is_run(derived):
    from catint_amd.build import BALANCE_LIB
    from tests import kernel_census as K
    launched = {name for (_, _, _, name) in derived.values()}
    assert launched == K.compiled_kernels(lib=BALANCE_LIB)
    worst = max(max(ratios(got, ref, scales).values()) for (got, ref, scales, _) in derived.values())
    print('worst parity ratio over all cases and outputs: %.3e' % worst)


# ---- (c) the telescoping sum, on the device's own numbers -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_defect_is_wall_minus_bulk_plus_source(case, derived):
    got, _, _, _ = derived[case.id]
    sc = got['scalars']
    lhs = sc[..., COL['defect']]
    rhs = sc[..., COL['wall_flux']] - sc[..., COL['bulk_flux']] + sc[..., COL['source_integral']]
    # the absolute sum: every edge flux enters the sum of the V_i imbalance_i twice with opposite signs, the wall flux and every
    # V_i R_k,i once -- recomputed here from the device's own rows
    q, D, radii, x = case.problem()
    h, V = control_volumes(x)
    bound = (np.abs(got['wall_flux']) + 2.0 * np.abs(got['flux']).sum(axis=2) + (V[None, None, :-1] * np.abs(got['source'][:, :, :-1])).sum(axis=2))
    rel = (np.abs(lhs - rhs) / bound).max()
    print('%s: |DEFECT - (WALL - BULK + SOURCE)| / absolute sum = %.3e' % (case.id, rel))
    assert rel <= TOL
    assert np.array_equal(sc[..., COL['wall_flux']], got['wall_flux']) and np.array_equal(sc[..., COL['bulk_flux']], got['flux'][:, :, -1])


# ---- (d) locality ---------------------------------------------------------------------------------------------------------------------------
LOCAL = [Case(3, 40, 2, 'abc', 'first', steric=True), Case(3, 100, 2, 'dimer', 'eight'), Case(3, 200, 2, 'abc', 'first', steric=True, graded=True),
         Case(3, 400, 2, 'four', 'zeroth', velocity=0.2), Case(2, 1000, 2, 'dimer', 'first', steric=True), Case(2, 1500, 2, 'dimer', 'first'),
         Case(2, 3000, 2, 'four', 'eight', steric=True)]


@pytest.mark.gpu
@pytest.mark.parametrize('case', LOCAL, ids=[c.id for c in LOCAL])
def test_a_changed_concentration_moves_only_its_neighbourhood(case):
    """One concentration changed at an interior point (the last point of a thread, and where there are several of a wave: its right
    neighbour belongs to the next thread / wave), then one at the wall: everything outside the stencil stays bit for bit."""
    c, phi, flux, phiM = case.state()
    P, WY = case.shape()
    i = 64 * P if 64 * P < case.nx - 2 else (3 * P if 3 * P < case.nx - 2 else case.nx // 2)
    b0, k0 = 1, case.N - 1 if case.rx != 'dimer' else 0
    with _balance.Balancer(0) as bal, case.solver() as s:
        case.upload(s, c, phi)
        base = case.derive(s, bal, flux, phiM)
        for point in (i, 0):
            c2 = c.copy()
            c2[b0, k0, point] *= 1.25
            case.upload(s, c2, phi)
            got = case.derive(s, bal, flux, phiM)
            pts = np.ones(case.nx, bool)
            pts[max(point - 1, 0):point + 2] = False
            one = np.ones(case.nx, bool)
            one[point] = False
            edges = np.ones(case.nx - 1, bool)
            edges[max(point - 1, 0):point + 1] = False
            assert np.array_equal(got['imbalance'][:, :, pts], base['imbalance'][:, :, pts])
            assert np.array_equal(got['source'][:, :, one], base['source'][:, :, one])
            assert np.array_equal(got['reaction_rate'][:, :, one], base['reaction_rate'][:, :, one])
            assert np.array_equal(got['flux'][:, :, edges], base['flux'][:, :, edges])
            other = np.arange(case.B) != b0
            for key in got:
                assert np.array_equal(got[key][other], base[key][other]), key
            # ... and inside the stencil something did move
            assert not np.array_equal(got['flux'][b0, k0], base['flux'][b0, k0])
            assert not np.array_equal(got['imbalance'][b0], base['imbalance'][b0])


# ---- (e) null outputs; operating points are independent; the handle is only read ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('case', [BY_ID[CASES[2].id], BY_ID[CASES[3].id], Case(2, 1030, 3, 'dimer', 'first')], ids=lambda c: c.id)
def test_null_outputs_leave_the_others_bit_for_bit(case):
    c, phi, flux, phiM = case.state()
    with _balance.Balancer(0) as bal, case.solver() as s:
        case.upload(s, c, phi)
        full = case.derive(s, bal, flux, phiM)
        subsets = [((r,), False) for r in ROWS] + [((), True), (('wall_rate',), True), (('flux', 'wall_flux'), False), (('reaction_rate', 'imbalance'), False),
                                                   (tuple(r for r in ROWS if r != 'reaction_rate'), True), (('source',), True)]
        for rows, scalars in subsets:
            got = case.derive(s, bal, flux, phiM, fields=list(rows), scalars=scalars)
            assert sorted(got) == sorted(rows + (('scalars',) if scalars else ()))
            for key in got:
                assert np.array_equal(got[key], full[key]), (rows, scalars, key)


@pytest.mark.gpu
@pytest.mark.parametrize('case', [Case(3, 67, 37, 'abc', 'eight', steric=True, graded=True, max_waves=5), Case(2, 1100, 7, 'dimer', 'first', max_waves=6)],
                         ids=lambda c: c.id)
def test_operating_points_are_independent(case):
    c, phi, flux, phiM = case.state()
    _, wk = case.tables()
    perm = np.random.RandomState(5).permutation(case.B)
    with _balance.Balancer(0) as bal, case.solver() as s:
        case.upload(s, c, phi)
        status0 = s.get_status()
        full = case.derive(s, bal, flux, phiM)
        c1, phi1 = s.get_state(derived=False)
        assert np.array_equal(c1, c) and np.array_equal(phi1, phi) and np.array_equal(s.get_status(), status0)     # only read
        case.upload(s, c[perm], phi[perm])
        shuffled = case.derive(s, bal, flux[perm], phiM[perm], wall=dict(wk, k=wk['k'][perm]))
        for key in full:
            assert np.array_equal(shuffled[key], full[key][perm]), key


# ---- (f) solved states -------------------------------------------------------------------------------------------------------------------
class Solved(object):
    """A small problem the solver's defaults converge on from the bulk state: 2 x 96 (a binary electrolyte, point ions), or 7 x 130 with
    a two-reaction buffer C <-> D <-> E in equilibrium in the bulk, steric ions and one Butler-Volmer wall reaction C -> E."""

    def __init__(self, big, velocity=0.0):
        self.big, self.velocity = big, velocity
        if big:
            self.N, self.nx = 7, 130
            z = np.array([1, -1, 0, 0, 0, 1, -1], float)
            self.cb = np.array([10.0, 10.0, 4.0, 8.0, 2.0, 5.0, 5.0])
            self.D = 1e-9 * np.array([1.957, 1.185, 1.6, 1.3, 1.1, 1.0, 2.0])
            self.radii = np.full(7, 3.5e-10)
            self.reactions = [([2], [3], 2.0e3, 1.0e3), ([3], [4], 0.5e3, 2.0e3)]          # 4 -> 8 -> 2 mol/m^3 in the bulk
            nu = np.zeros((1, 7))
            nu[0, 2], nu[0, 4] = -1.0, 1.0
            self.wall = {'species': [2], 'nu': nu, 'alpha': np.array([-8.0]), 'saturation': np.array([0.0])}
            self.k0 = 2e-3
        else:
            self.N, self.nx = 2, 96
            z = np.array([1, -1], float)
            self.cb = np.array([10.0, 10.0])
            self.D = np.array([1.957e-9, 1.185e-9])
            self.radii, self.reactions, self.wall = None, [], None
        self.q = z * unit_F
        self.dx = float(np.sqrt(EPS / BETA / (self.q ** 2 * self.cb).sum()) / 6.0)
        self.x = np.arange(self.nx) * self.dx
        self.phiM = np.array([-0.10, -0.04, 0.06])
        self.B = len(self.phiM)
        self.flux = np.zeros((self.B, self.N))
        self.flux[:, 0] = [0.0, 2e-3, -1e-3]
        self.flux[:, 1] = [0.0, 2e-3, -1e-3]
        self.dt = 0.05 * (self.nx * self.dx) ** 2 / self.D.max()
        self.tol = 1e-10

    def solver(self):
        s = PnpSolver(self.N, self.nx, self.dx, self.dt, BETA, EPS, self.D, self.q, method='Newton', batch_capacity=self.B)
        s.set_newton(wall_bc='stern', stern_capacitance=0.2, mpb_radius=self.radii)          # tol, maxit, dphi_max: the defaults
        if self.velocity:
            s.set_convection(self.velocity)
        if self.reactions:
            s.set_reactions(self.reactions)
        pb = np.zeros((self.B, 4))
        pb[:, 0] = self.phiM
        self.c0 = np.repeat(self.cb[None, :, None], self.B, axis=0).repeat(self.nx, axis=2)
        s.set_batch(self.c0, pb, np.zeros(self.B), self.flux)
        if self.wall:
            s.set_wall_kinetics(self.wall['species'], self.wall['nu'], np.full((self.B, 1), self.k0), self.wall['alpha'], self.wall['saturation'])
        return s

    def reference(self, c, phi):
        wall = None if not self.wall else dict(self.wall, k=np.full((self.B, 1), self.k0))
        return reference(c, phi, self.x, self.D, self.q, self.flux, self.phiM, self.radii, self.velocity, self.reactions, wall)


SOLVED = [Solved(False), Solved(True), Solved(True, velocity=0.02)]
SOLVED_IDS = ['2x96', '7x130', '7x130-conv']


def test_the_solved_problems_converge_on_the_oracle():
    """No device: the oracle's Newton iteration (the device's, restated) converges on the larger problem from the bulk state, so a
    failure of the GPU tests below is not the problem's."""
    from oracle import pnp_physical as PH
    pr = SOLVED[2]
    p = PH.PhysicalProblem(D=pr.D, charges=pr.q, beta=BETA, eps=EPS, dx=pr.dx, nx=pr.nx, c_bulk=pr.cb, phiM=pr.phiM[0], flux=pr.flux[0],
                           stern_capacitance=0.2, mpb_radius=pr.radii, reactions=[{'lhs': l, 'rhs': r, 'kf': f, 'kr': g} for (l, r, f, g) in pr.reactions],
                           wall_kinetics=[{'species': 2, 'k': pr.k0, 'nu': pr.wall['nu'][0], 'alpha': -8.0}], velocity=pr.velocity)
    c0 = np.repeat(pr.cb[:, None], pr.nx, axis=1)
    c, phi, it, _ = PH.newton_step(p, c0, np.zeros(pr.nx), c0, np.inf)
    assert it <= 50
    ref, scales = reference(c[None], phi[None], pr.x, pr.D, pr.q, pr.flux[:1], pr.phiM[:1], pr.radii, pr.velocity, pr.reactions,
                            dict(pr.wall, k=np.full((1, 1), pr.k0)))
    assert ref['scalars'][0, :, COL['max_imbalance_rel']].max() < 1e-6           # a solution of the oracle balances


@pytest.mark.gpu
@pytest.mark.parametrize('pr', SOLVED, ids=SOLVED_IDS)
def test_stationary_solutions(pr):
    from catint_amd.calculator import Calculator
    with pr.solver() as s:
        st = s.solve_stationary()
        assert (st == 0).all(), st
        c, phi = s.get_state(derived=False)
        got = s.get_balance()
    ref, scales = pr.reference(c, phi)
    assert_close(got, ref, scales, 'stationary')
    worst = got['scalars'][:, :, COL['max_imbalance_rel']].max()
    print('stationary %s: MAX_IMBALANCE_REL = %.3e (comparator on the same state: %.3e)' % (
        'N%d nx%d v%g' % (pr.N, pr.nx, pr.velocity), worst, ref['scalars'][:, :, COL['max_imbalance_rel']].max()))
    if pr.wall:
        calc = Calculator.__new__(Calculator)            # surface_kinetic_fluxes reads the species names and the table, nothing else
        calc.tp = types.SimpleNamespace(species=collections.OrderedDict((chr(65 + k), {}) for k in range(pr.N)))
        calc.surface_kinetics = [{'species': 'C', 'rate': pr.k0, 'stoichiometry': {'C': -1.0, 'E': 1.0}, 'alpha': -8.0}]
        host = calc.surface_kinetic_fluxes(c[:, :, 0], pr.phiM, vsurf=phi[:, 0])
        assert np.abs(got['wall_flux'] - pr.flux - host).max() <= TOL * scales['wall_flux']
        assert np.abs(got['wall_rate'][:, 0] - host[:, 4]).max() <= TOL * scales['wall_rate']
        assert np.abs(host).max() > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('pr', SOLVED[:2], ids=SOLVED_IDS[:2])
def test_one_backward_euler_step(pr):
    """The imbalance of the state after one step is the time derivative the step realised: (c - c_old) / dt, to the parity tolerance
    plus what the solver's own stopping rule leaves (its scaled update below tol: tol (c + c_bulk) / dt)."""
    with pr.solver() as s:
        s.step(1)
        assert (s.get_status() == 0).all()
        c, phi = s.get_state(derived=False)
        got = s.get_balance()
    ref, scales = pr.reference(c, phi)
    assert_close(got, ref, scales, 'timestep')
    dcdt = (c - pr.c0) / pr.dt
    bound = TOL * scales['imbalance_pointwise'] + pr.tol * (np.abs(c) + pr.cb[None, :, None]) / pr.dt
    miss = (np.abs(got['imbalance'] - dcdt) / bound)[:, :, :-1].max()
    print('timestep: max |imbalance - (c - c_old) / dt| / bound = %.3e' % miss)
    assert miss <= 1.0
    assert np.abs(dcdt).max() > 0.0 and np.all(got['imbalance'][:, :, -1] == 0.0)


# ---- (g) the Python layer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_defaults_are_what_the_solver_was_given():
    """get_balance() without arguments uses the recorded problem: equal, bit for bit, to the library called with the same tables."""
    pr = SOLVED[2]
    with pr.solver() as s, _balance.Balancer(0) as bal:
        assert (s.solve_stationary() == 0).all()
        got = s.get_balance()
        explicit = bal.species(s.device_view(), pr.D, pr.q, pr.x, BETA, pr.flux, pr.phiM, mpb_radius=pr.radii, velocity=pr.velocity,
                               reactions=pr.reactions, wall=dict(pr.wall, k=np.full((pr.B, 1), pr.k0)))
        assert sorted(got) == sorted(explicit) == sorted(ROWS + ('scalars',))
        for key in got:
            assert np.array_equal(got[key], explicit[key]), key
        few = s.get_balance(fields=['wall_rate'], scalars=True)
        assert sorted(few) == ['scalars', 'wall_rate'] and np.array_equal(few['scalars'], got['scalars'])
        # a new prescribed flux is recorded where it is set
        s.solve_surface(flux=2.0 * pr.flux)
        assert np.array_equal(s.get_balance(fields=['wall_flux'], scalars=False)['wall_flux'],
                              s.get_balance(fields=['wall_flux'], scalars=False, flux=2.0 * pr.flux)['wall_flux'])


def _scf_state(B, N, cs, vs, es):
    return {'surface_concentration': cs.copy(), 'surface_concentration_old': cs.copy(), 'flux': np.zeros((B, N)),
            'current_density_old': np.zeros((B, N)), 'mix': np.full(B, 0.5), 'accuracy': np.full(B, np.inf),
            'surface_pH': np.full(B, 7.0), 'surface_potential': vs, 'surface_efield': es,
            'step_to_check': np.full(B, 1), 'active': np.ones(B, np.int32), 'failed': np.zeros(B, np.int32)}


@pytest.mark.gpu
def test_after_the_scf_loop_the_balance_is_formed_from_the_loop_s_flux_alone():
    """pnp_scf_cycle's solves take the wall reactions through the prescribed flux (evaluated explicitly from the mixed surface state),
    not through the wall table: the state it leaves conserves state['flux'] and nothing else.  get_balance refuses the stale recorded
    flux, and with the loop's flux it equals the comparator called WITHOUT a wall table -- with the table the wall reactions would
    count twice.  A lane whose last solve converged then balances.  Bound: the solver stops when its scaled update is below tol =
    1e-10, so the state is within tol (relative; tol / (beta |q|) in the potential) of the discrete solution; every term of the
    imbalance is linear in c and has a logarithmic derivative of at most 1 + |u| in the potential, and |u| stays below 10 on these
    grids (six points per Debye length, |phiM| < 0.2 V): 1e-8 = 100 tol covers both with a decade to spare."""
    from tests.test_gpu_lane_mask import Case as LaneCase, F
    from tests.test_gpu_newton import BETA as LBETA
    N, nx, B = 3, 64, 6
    case = LaneCase(N, nx, B, 47, {}, {})
    k = np.linspace(1e-5, 5e-5, B)[:, None]
    x = np.arange(nx) * case.dx
    with case.solver() as s:
        s.set_wall_kinetics([2], [[0.0, 0.0, -1.0]], k)
        assert (s.solve_stationary() == 0).all()
        implicit = s.get_balance()
        assert implicit['wall_rate'].shape == (B, 1) and np.abs(implicit['wall_rate']).min() > 0.0
        assert implicit['scalars'][:, :, COL['max_imbalance_rel']].max() <= 1e-8
        cs, vs, es = s.get_surface()
        state = _scf_state(B, N, cs, vs, es)
        s.scf_cycle(state, istep=1, max_iter=4, tau_scf=1e-12, faraday=F)
        with pytest.raises(ValueError):
            s.get_balance()
        got = s.get_balance(flux=state['flux'])
        c, phi = s.get_state(derived=False)
        ok = s.get_status() == 0
        ref, scales = reference(c, phi, x, case.D, case.q, state['flux'], case.phiM, beta=LBETA)       # no wall table
        assert got['wall_rate'].shape == (B, 0)
        assert_close(got, ref, scales, 'after the SCF loop')
        assert np.array_equal(got['wall_flux'], state['flux']) and np.abs(state['flux'][:, 2]).min() > 0.0
        worst = got['scalars'][ok][:, :, COL['max_imbalance_rel']].max()
        print('after the SCF loop: MAX_IMBALANCE_REL of the %d converged lanes = %.3e' % (ok.sum(), worst))
        assert ok.any() and worst <= 1e-8
        # (what the table on top of the loop's flux would have reported: the wall reactions twice)
        twice, _ = reference(c, phi, x, case.D, case.q, state['flux'], case.phiM, wall={'species': [2], 'nu': [[0.0, 0.0, -1.0]], 'k': k}, beta=LBETA)
        assert twice['scalars'][ok][:, 2, COL['max_imbalance_rel']].min() > 1e-8          # ... outside the bound held above
        # the next implicit solve puts the table back; the flux the loop left on the device is still not the recorded one
        assert (s.solve_stationary() == 0).all()
        with pytest.raises(ValueError):
            s.get_balance()
        again = s.get_balance(flux=state['flux'])
        assert again['wall_rate'].shape == (B, 1)
        c, phi = s.get_state(derived=False)
        ref, scales = reference(c, phi, x, case.D, case.q, state['flux'], case.phiM, wall={'species': [2], 'nu': [[0.0, 0.0, -1.0]], 'k': k}, beta=LBETA)
        assert_close(again, ref, scales, 'implicit solve after the SCF loop')
        assert again['scalars'][:, :, COL['max_imbalance_rel']].max() <= 1e-8
        s.set_flux(np.zeros((B, N)))                     # a flux set on the host again: the record is current
        s.get_balance(fields=[], scalars=True)


@pytest.mark.gpu
def test_a_wall_table_of_another_batch_size_is_not_used_silently():
    """pnp_set_batch keeps the handle's wall table; its rate constants were recorded per lane of the batch they were set for.  After a
    set_batch with another size get_balance raises until set_wall_kinetics is called again."""
    from tests.test_gpu_lane_mask import Case as LaneCase
    N, nx, B = 3, 64, 6
    case = LaneCase(N, nx, B, 47, {}, {})
    with case.solver() as s:
        s.set_wall_kinetics([2], [[0.0, 0.0, -1.0]], np.full((B, 1), 2e-5))
        s.set_batch(case.c0, case.pb, np.zeros(B), np.zeros((B, N)))             # the same size: the record holds
        assert s.get_balance(fields=['wall_rate'], scalars=False)['wall_rate'].shape == (B, 1)
        s.set_batch(case.c0[:4], case.pb[:4], np.zeros(4), np.zeros((4, N)))
        with pytest.raises(ValueError, match='set_wall_kinetics'):
            s.get_balance()
        s.set_wall_kinetics([2], [[0.0, 0.0, -1.0]], np.full((4, 1), 2e-5))
        assert s.get_balance(fields=['wall_rate'], scalars=False)['wall_rate'].shape == (4, 1)
        s.set_batch(case.c0[:5], case.pb[:5], np.zeros(5), np.zeros((5, N)))
        s.set_wall_kinetics([], [], [])                                           # the table removed: nothing stale is left
        assert s.get_balance(fields=['wall_rate'], scalars=False)['wall_rate'].shape == (5, 0)


def _small_sweep(balance_on_device):
    import importlib.util
    import os
    from catint_amd.calculator import Calculator
    spec = importlib.util.spec_from_file_location('co2r_physical_sweep', os.path.join(os.path.dirname(__file__), '..', 'examples',
                                                                                       'co2r_physical_sweep.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    tp, _ = ex.build(3, 96, phimin=-0.5, phimax=-0.9)
    calc = Calculator(transport=tp, calc='comsol', balance_on_device=balance_on_device)
    tp.newton = {'tol': 1e-9, 'maxit': 80}
    calc.set_surface_kinetics([{'species': 'CO2', 'rate': ex.tafel_rate(tp), 'stoichiometry': {'CO2': -1.0, 'CO': 1.0, 'OH-': 2.0}}])
    calc.run()
    assert np.all(calc.status == 0)
    return tp, calc


@pytest.mark.gpu
def test_calculator_fills_the_new_keys_only_when_asked():
    tp_h, calc_h = _small_sweep(False)
    tp_d, calc_d = _small_sweep(True)
    assert calc_h.balance is None and sorted(calc_d.balance) == sorted(ROWS + ('scalars',))
    names = list(tp_h.species.keys())
    new_species, new_system = {'flux', 'reaction_source', 'mass_balance_defect'}, {'reaction_rates'}
    # flag off: exactly the keys Calculator._alldata_fill writes on the parent commit, written out (the sweep's descriptors are phiM and
    # temperature, its Stern layer has a constant permittivity, CO is the one species with an electrode reaction)
    species_keys = {'concentration', 'surface_concentration', 'activity_coefficient', 'surface_activity_coefficient', 'electrode_flux'}
    system_keys = {'potential', 'efield', 'charge_density', 'surface_potential', 'surface_efield', 'phiM', 'temperature', 'status', 'pH',
                   'surface_pH', 'activity_coefficient', 'conductivity', 'electrolyte_current_density', 'delta_phi_iR', 'delta_phi_diff',
                   'delta_phi_iR_inf', 'delta_phi_diff_inf', 'delta_phi_inf', 'delta_phi_inf_min_iR', 'Stern_efield', 'Stern_epsilon_func'}
    assert sorted(tp_h.alldata[0]) == sorted(tp_d.alldata[0])
    R = len([rx for rx in tp_d.reactions.values() if 'rates' in rx])
    for i in range(3):
        dh, dd = tp_h.alldata[i], tp_d.alldata[i]
        assert set(dh['system']) == system_keys and set(dd['system']) == system_keys | new_system
        assert np.asarray(dd['system']['reaction_rates']).shape == (R, tp_d.nx)
        for k, sp in enumerate(names):
            hs, ds = dh['species'][sp], dd['species'][sp]
            want = species_keys | ({'electrode_current_density'} if sp == 'CO' else set())
            assert set(hs) == want and set(ds) == want | new_species, (i, sp)
            assert np.asarray(ds['flux']).shape == (tp_d.nx - 1,) and np.asarray(ds['reaction_source']).shape == (tp_d.nx,)
            assert isinstance(ds['mass_balance_defect'], float)
            scale = max(np.abs([dh['species'][s_]['electrode_flux'] for s_ in names]).max(), 1e-300)
            assert abs(ds['electrode_flux'] - hs['electrode_flux']) <= TOL * scale, (i, sp)
            if 'electrode_current_density' in hs:
                assert abs(ds['electrode_current_density'] - hs['electrode_current_density']) <= TOL * abs(hs['electrode_current_density']) + 1e-300
    assert np.abs([tp_h.alldata[i]['species']['CO']['electrode_flux'] for i in range(3)]).max() > 0.0


def test_a_compat_calculator_refuses_the_flag():
    from catint_amd.calculator import Calculator, CalculatorError
    tp = types.SimpleNamespace(calc='Crank-Nicolson', system={}, ntout=1)
    with pytest.raises(CalculatorError, match='balance_on_device is part of the physical mode'):
        Calculator(transport=tp, calc='Crank-Nicolson', balance_on_device=True)
    assert Calculator(transport=tp, calc='Crank-Nicolson').balance_on_device is False       # the same transport passes without the flag
