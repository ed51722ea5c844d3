"""The cases of the linear-response tests (tests/test_response_abi.py on the CPU, tests/test_gpu_response.py on the device): problem
definitions as oracle.pnp_physical.PhysicalProblem builders, their converged oracle states, and the time scales the frequency lists are
made of."""
import numpy as np

from oracle import pnp_physical as PH

F, BETA, EPS = 96485.33289, 1.0 / (8.3144598 * 298.14), 78.36 * 8.854187817e-12
D2 = np.array([1.957e-9, 1.185e-9])
Q2 = np.array([F, -F])
SCALES = (1.0, 0.75, 0.5, 0.25, 0.1)     # the operating points of a device case: the case's phiM times these


def graded_mesh(*a):
    from catint_amd.host import graded_mesh as g
    return g(*a)


def debye(q, cb):
    return float(np.sqrt(EPS / BETA / (np.asarray(q) ** 2 * np.asarray(cb)).sum()))


class Case(object):
    """A problem family: make(phiM) -> PhysicalProblem.  `wall` as the solver takes it (species, nu, k, alpha, saturation) or None;
    reactions as [(lhs, rhs, kf, kr)]"""

    def __init__(self, name, D, q, cb, x, phiM, CS=None, radii=None, velocity=0.0, reactions=(), wall=None, flux=None):
        self.name, self.D, self.q, self.cb, self.x = name, np.asarray(D, float), np.asarray(q, float), np.asarray(cb, float), np.asarray(x, float)
        self.phiM, self.CS, self.radii, self.velocity = float(phiM), CS, None if radii is None else np.asarray(radii, float), float(velocity)
        self.reactions, self.wall = list(reactions), wall
        self.flux = None if flux is None else np.asarray(flux, float)
        self.N, self.nx, self.dx = len(self.D), len(self.x), float(self.x[1] - self.x[0])
        self.lam = debye(self.q, self.cb)
        L = self.x[-1] - self.x[0]
        self.tau_D, self.tau_DL = L * L / self.D.min(), self.lam * L / self.D.max()

    def omegas(self):
        return np.array([0.0, 1.0 / self.tau_D, 1.0 / self.tau_DL, 100.0 / self.tau_DL])

    def make(self, phiM=None, flux=None):
        wk = []
        if self.wall is not None:
            sp, nu, k, al, sat = self.wall
            wk = [{'species': int(sp[r]), 'k': float(k[r]), 'nu': list(np.asarray(nu, float)[r]), 'alpha': float(al[r]), 'saturation': float(sat[r])}
                  for r in range(len(sp))]
        return PH.PhysicalProblem(D=self.D, charges=self.q, beta=BETA, eps=EPS, dx=self.dx, nx=self.nx, c_bulk=self.cb,
                                  phiM=self.phiM if phiM is None else phiM, flux=self.flux if flux is None else flux,
                                  stern_capacitance=self.CS, mpb_radius=self.radii,
                                  reactions=[{'lhs': list(l), 'rhs': list(r), 'kf': kf, 'kr': kr} for (l, r, kf, kr) in self.reactions],
                                  wall_kinetics=wk, x=self.x, velocity=self.velocity)

    def bulk_state(self):
        return np.repeat(self.cb[:, None], self.nx, axis=1), np.zeros(self.nx)

    def solve(self, phiM=None, flux=None, start=None, tol=1e-12):
        """The oracle's stationary state at phiM (from `start` = (c, phi), or from the bulk state by continuation in 0.1 V stages)"""
        target = self.phiM if phiM is None else float(phiM)
        if start is not None:
            p = self.make(target, flux)
            c, phi, it, _ = PH.newton_step(p, start[0], start[1], start[0], np.inf, tol=tol, maxit=80)
            assert it <= 80, (self.name, target, it)
            return p, c, phi
        c, phi = self.bulk_state()
        n = max(1, int(np.ceil(abs(target) / 0.1)))
        for s in range(1, n + 1):
            p = self.make(target * s / n, flux)
            c, phi, it, _ = PH.newton_step(p, c, phi, c, np.inf, tol=tol if s == n else 1e-8, maxit=80)
            assert it <= 80, (self.name, target, s, it)
        return p, c, phi


def debye_hueckel(nx, stern):
    lam = debye(Q2, [10.0, 10.0])
    return Case('Debye-Hueckel nx=%d %s' % (nx, 'stern' if stern else 'dirichlet'), D2, Q2, [10.0, 10.0], np.linspace(0.0, 10.0 * lam, nx), 0.0,
                CS=0.2 if stern else None)


def kornyshev():
    lam = debye(Q2, [100.0, 100.0])
    return Case('Kornyshev', D2, Q2, [100.0, 100.0], graded_mesh(30.0 * lam, 0.02e-9, 130), -0.8, radii=[4e-10, 4e-10])


def kornyshev_formula(case, phiM):
    gam = 2.0 * case.cb[0] * case.radii[0] ** 3 * PH.N_AVOGADRO
    u = F * BETA * abs(phiM)
    s = 2.0 * gam * np.sinh(0.5 * u) ** 2
    if s == 0.0:
        return EPS / case.lam
    return EPS / case.lam * np.cosh(0.5 * u) / (1.0 + s) * np.sqrt(s / np.log1p(s))


def case_F(flux=None):
    """N = 3, every term of the physics"""
    q, cb = np.array([1.0, -1.0, -2.0]) * F, [120.0, 100.0, 10.0]
    lam = debye(q, cb)
    return Case('F', [1.957e-9, 1.185e-9, 0.923e-9], q, cb, graded_mesh(60.0 * lam, lam / 8.0, 33), -0.4, CS=0.2, radii=[4e-10, 3e-10, 3.5e-10],
                velocity=-1e-3, reactions=[([0, 1], [2], 1e2, 1.2e5)],
                wall=([1], [[0.0, -1.0, 0.5]], [2e-6], [-0.15 * F * BETA], [0.002]), flux=flux)


E_Z = np.array([1, 1, -1, -1, -2, -1, 1, -1], float)
E_CB = np.array([50, 50, 40, 30, 10, 5, 20, 25], float)
E_D = np.array([1.957, 1.334, 2.032, 1.185, 0.923, 5.273, 2.06, 1.792]) * 1e-9


def case_E(nx):
    """N = 8 (block size 9: seven teams and one idle lane per wave)"""
    q = E_Z * F
    lam = debye(q, E_CB)
    nu = np.zeros((1, 8))
    nu[0, 3], nu[0, 5] = -1.0, 2.0
    return Case('E nx=%d' % nx, E_D, q, E_CB, graded_mesh(80.0 * lam, lam / 10.0, nx), -0.3 if nx == 34 else -0.8, CS=0.2, radii=[3.5e-10] * 8,
                reactions=[([3, 5], [4], 1e3, 1.5e4)], wall=([3], nu, [1e-6], [-0.1 * F * BETA], [0.0]))


def case_G(nx):
    """N = 4, every term of the physics and every shape of a table entry: a dimerisation (a repeated reactant), an empty side with a
    rate, a catalyst with a repeat and a dead backward side, four entries on both sides with a fourfold repeat; at the wall two
    reactions driven by the same species, a zeroth-order one that still depends on the potential, and alpha = 0"""
    q, cb = np.array([1.0, -1.0, 1.0, -1.0]) * F, [60.0, 50.0, 10.0, 20.0]
    lam = debye(q, cb)
    reactions = [([0, 0], [2], 2e4, 5e5), ([], [0, 1], 2e5, 1e2), ([1, 3, 3], [2, 1], 5.0, 0.0), ([0, 1, 2, 3], [3, 3, 3, 3], 1e-2, 1e-3)]
    wall = ([1, -1, 1], [[0.0, -1.0, 0.5, 0.0], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, -1.0, 1.0]], [2e-6, 1e-5, 1e-6],
            np.array([-0.15, 0.1, 0.0]) * F * BETA, [0.002, 0.0, 0.0])
    return Case('G nx=%d' % nx, E_D[:4], q, cb, graded_mesh(20.0 * lam, lam / 6.0, nx), -0.3, CS=0.2, radii=[4e-10, 3e-10, 3.5e-10, 3e-10],
                velocity=-1e-3, reactions=reactions, wall=wall)


def case_G8(nx):
    """N = 8 with both tables full: 16 reactions of 0 .. 4 entries per side (every fifth without a backward rate, reactions 3 and 10
    without a forward one; reaction 3 is ([0, 5, 5], [], 0, 2e5), a constant source), 8 wall reactions (the first of zeroth order, the
    second and third driven by the same species), drawn from a seeded generator in this order; the zeroth-order wall reaction takes
    alpha = 0.1 F beta and no saturation, whatever was drawn"""
    q = E_Z * F
    lam = debye(q, E_CB)
    rng = np.random.RandomState(8)
    reactions = []
    for r in range(16):
        nl, nr = r % 5, (3 * r + 1) % 5
        lhs = [int(v) for v in rng.randint(0, 8, nl)]
        rhs = [int(v) for v in rng.randint(0, 8, nr)]
        kf, kr = 1e5 / 30.0 ** nl, 2e5 / 30.0 ** nr
        if r % 5 == 2:
            kr = 0.0
        if r % 7 == 3:
            kf = 0.0
        reactions.append((lhs, rhs, kf, kr))
    sp = [int(v) for v in rng.randint(-1, 8, 8)]
    sp[0] = -1
    sp[1] = sp[2] = 3
    nu = rng.choice([-2., -1., 0., 1., 2.], (8, 8))
    al = rng.choice([-0.15, 0.0, 0.1], 8) * F * BETA
    al[0] = 0.1 * F * BETA
    sat = rng.choice([0.0, 0.002, 0.05], 8)
    sat[0] = 0.0          # (drawn 0.002: pnp_set_wall_rate_law refuses a saturation on a zeroth-order reaction)
    k = rng.uniform(2e-7, 2e-6, 8)
    return Case('G8 nx=%d' % nx, E_D, q, E_CB, graded_mesh(40.0 * lam, lam / 6.0, nx), -0.3, CS=0.2, radii=[3.5e-10] * 8, velocity=-1e-3,
                reactions=reactions, wall=(sp, nu, k, al, sat))


# Entries that leave every row of case G as it is: a reaction without rates, a reaction whose species stands on both sides alone (net is
# identically 0), and a wall reaction (species, nu, alpha, saturation) whose rate constant is 0 on every lane
NULL_REACTIONS = [([0, 1], [3, 3], 0.0, 0.0), ([2], [2], 3e3, 7e2)]
NULL_WALL = (0, [1.0, -1.0, 0.0, 2.0], -0.1 * F * BETA, 0.01)


def table_properties(s, case, outputs, moves, wall=True):
    """The exact properties of the reaction and wall tables in one of the team-elimination libraries.  s: a solver that holds converged
    states of `case` (case G); outputs(): a dict of the library's output arrays at the handle's present tables.  The tables are
    replaced after the state is fixed, and the exact state is put back before every call.  Appending an entry of NULL_REACTIONS or
    (wall=True) NULL_WALL changes no bit of any output; dropping the case's first reaction changes every output named in `moves`
    (a table that is silently ignored would pass the first half).  The handle is left as it was."""
    n = s.B
    c, phi = s.get_state(derived=False)

    def run():
        s.set_lanes(list(range(n)), c, phi)
        return outputs()

    def differing(a, b):
        assert sorted(a) == sorted(b)
        return sorted(k for k in a if not np.array_equal(a[k], b[k], equal_nan=True))

    def set_wall(extra):
        sp, nu, k, al, sat = case.wall
        kk = np.tile(np.asarray(k, float), (n, 1))
        if extra:
            s.set_wall_kinetics(list(sp) + [NULL_WALL[0]], [list(row) for row in nu] + [NULL_WALL[1]], np.hstack([kk, np.zeros((n, 1))]),
                                list(al) + [NULL_WALL[2]], list(sat) + [NULL_WALL[3]])
        else:
            s.set_wall_kinetics(sp, nu, kk, al, sat)
    want = run()
    assert all(np.isfinite(want[k]).all() for k in moves)
    try:
        for extra in NULL_REACTIONS:
            s.set_reactions(case.reactions + [extra])
            assert not differing(run(), want), extra
        s.set_reactions(case.reactions)
        if wall:
            set_wall(True)
            assert not differing(run(), want), 'wall'
            set_wall(False)
        s.set_reactions(case.reactions[1:])
        moved = differing(run(), want)
        assert set(moves) <= set(moved), (moves, moved)
    finally:
        s.set_reactions(case.reactions)
        if wall:
            set_wall(False)
        s.set_lanes(list(range(n)), c, phi)
    assert not differing(run(), want)


def small(N, nx, stern=False, steric=False):
    """The first N species of case E's lists (N = 1: a single cation against a Dirichlet wall), a short graded grid"""
    q, cb = E_Z[:N] * F, E_CB[:N]
    lam = debye(q, cb)
    return Case('N=%d nx=%d%s%s' % (N, nx, ' stern' if stern else '', ' steric' if steric else ''), E_D[:N], q, cb,
                graded_mesh(20.0 * lam, lam / 6.0, nx), -0.1, CS=0.2 if stern else None, radii=[3.5e-10] * N if steric else None)


SMALL_PIVOT_LANE, SMALL_PIVOT_REACTION = 2, ([0, 1], [0, 0, 1], 0.0, 0.0)


def small_pivot():
    """A system that trips the pivot monitor on data: the autocatalytic step A + C -> 2 A + C puts -(dx^2 / D_0) v kf c_1 on the diagonal of
    species 0, and in the uniform state of lane SMALL_PIVOT_LANE (c_0 = c_1 = 10 (1 - 3e-14)) that cancels the transport part of the
    diagonal, 2, to 6e-14 of it, while the Poisson row below holds (dx^2 / eps) q_0 in the same column.  The other lanes' diagonals are
    0.2 .. 0.8.  Returns (case, [cb per lane]): uniform grid, Dirichlet wall, phiM = 0, no solve needed (and none would converge)."""
    x = np.linspace(0.0, 40e-9, 21)
    case = Case('small pivot', D2, Q2, [10.0, 10.0], x, 0.0)
    kf = 2.0 / (case.dx * case.dx / D2[0] * 10.0)
    case.reactions = [(SMALL_PIVOT_REACTION[0], SMALL_PIVOT_REACTION[1], kf, 0.0)]
    return case, [9.0, 8.0, 10.0 * (1.0 - 3e-14), 6.0, 7.0]
