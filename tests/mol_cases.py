"""The case matrix of the direct tests of the method-of-lines right-hand side (tests/test_gpu_mol_rhs.py on the device,
tests/test_mol_rhs_ref.py for the fp64 oracle's own error): inputs only, no expectations.

Every case is a batch of B = 5 lanes (on a handle of capacity 8) in which every lane has its own state, its own Poisson boundary
values (one boundary combination per batch) and vzeta, and its own wall-flux vector with mixed signs and one zero; the state uploaded
with set_batch is another one than the argument of mol_rhs (twice as large and not neutral)."""
import collections
import functools

import numpy as np

from oracle import pnp_ref as R
from tests import mol_ref as M

B, CAPACITY = 5, 8
MP_MAX_NX = 259                  # the multiprecision restatement is practical up to here
FARADAY, RT = 96485.33289, 8.3144598 * 298.14
DX, DT = 2e-11, 1e-12
# one boundary combination per name: [potential wall, potential bulk, gradient wall, gradient bulk] (the values of the census test)
MOL_PB = collections.OrderedDict([('dd', [0.02, 0.0, np.nan, np.nan]), ('vwall_gbulk', [0.02, np.nan, np.nan, 1e4]),
                                  ('gwall_vbulk', [np.nan, 0.0, 1e5, np.nan]), ('vwall_gwall', [0.01, np.nan, 1e5, np.nan]),
                                  ('vbulk_gbulk', [np.nan, 0.0, np.nan, -1e4])])
D_TABLE = [1.957e-9, 2.032e-9, 1.185e-9, 0.923e-9, 5.273e-9, 1.334e-9, 2.056e-9, 9.311e-9]
Z_CYCLE = [-1, 1, -2, -1, 1, -1]                                  # species 1 ..; species 0 (z = +1) closes neutrality

Case = collections.namedtuple('Case', 'N nx pb lf mig table')


def case_id(c):
    return 'N%d-nx%d-%s%s%s-%s' % (c.N, c.nx, c.pb, '-LF' if c.lf else '', '' if c.mig else '-nomig', c.table)


def table(name, N):
    """[(lhs, rhs, kf, kr)] with rate constants of order one (scaled per case, see make_case)."""
    if name == 'none':
        return []
    if name == 'single':                 # N = 1: 2 A <-> A (the species on both sides), then a source from an empty side that overwrites it
        return [([0, 0], [0], 0.7, 25.0), ([], [0], 12.5, 0.3)]
    if name == 'dimer':                  # N = 2: 2 A <-> B
        return [([0, 0], [1], 0.7, 25.0)]
    if name == 'overwrite':              # N = 3: every species in several reactions, species 1 on both sides of one: the last writer counts
        return [([0, 1], [2], 3.0, 40.0), ([2, 1], [1, 0], 1.5, 6.0), ([0], [2], 9.0, 4.0), ([1], [0, 0], 5.0, 0.8)]
    if name == 'buffer':                 # the shape of the CO2R table (tests/test_gpu_balance.py): five reactions, one with an empty side
        return [([0, 1], [2], 3.0, 40.0), ([2, 1], [3], 1.5, 60.0), ([0], [4], 9.0, 4.0), ([4, 1], [3], 0.8, 11.0), ([], [1, 5], 2.4, 0.09)]
    if name == 'max':                    # PNP_MAX_REACTIONS reactions with PNP_MAX_REACTANTS reactants on a side
        rng = np.random.RandomState(16)
        out = []
        for r in range(16):
            nl, nr = (4, 4) if r % 3 == 0 else (4, int(rng.randint(1, 4))) if r % 3 == 1 else (int(rng.randint(1, 4)), 4)
            out.append(([int(v) for v in rng.randint(0, N, nl)], [int(v) for v in rng.randint(0, N, nr)],
                        float(10.0 ** rng.uniform(0, 1) * 10.0 ** (1 - nl)), float(10.0 ** rng.uniform(0, 1) * 10.0 ** (1 - nr))))
        return out
    raise KeyError(name)


_pb = list(MOL_PB)
GRID_NX = [5, 66, 67, 130, 131, 258, 259, 514, 515, 1026, 1027, 2050]       # both sides of every points-per-lane boundary; two pointwise
GRIDS = [Case(3, nx, _pb[(i + j) % 5], bool(j), True, 'overwrite') for i, nx in enumerate(GRID_NX) for j in (0, 1)]
SPECIES = [Case(N, nx, _pb[(i + j) % 5], bool((i + j) % 2), N > 1, t)
           for i, (N, t) in enumerate([(1, 'single'), (2, 'dimer'), (7, 'buffer'), (16, 'max')]) for j, nx in enumerate((67, 1027))]
TABLES = [Case(N, nx, _pb[(i + 2 * j + 1) % 5], bool((i + j + 1) % 2), True, t)
          for i, (N, t) in enumerate([(7, 'buffer'), (3, 'overwrite'), (16, 'max')]) for j, nx in enumerate((131, 1027))]
NOMIG = [Case(3, nx, _pb[(2 * i + j) % 5], bool(j), False, t) for i, nx in enumerate((67, 1027)) for j, t in enumerate(('none', 'overwrite'))]
ALL = list(collections.OrderedDict.fromkeys(GRIDS + SPECIES + TABLES + NOMIG))
SHORT = [c for c in ALL if c.nx <= MP_MAX_NX]
LONG = [c for c in ALL if c.nx > MP_MAX_NX]

Inputs = collections.namedtuple('Inputs', 'case problems y upload pb vzeta flux')


def charges_of(N):
    return np.array([1] + [Z_CYCLE[(k - 1) % len(Z_CYCLE)] for k in range(1, N)], float)


NOISE = 0.1                      # point-to-point roughness of the states, mol/m^3: sets the diffusion scale D NOISE / dx^2 of the RHS


def random_states(rng, N, nx, lanes=B):
    """Smooth profiles (anions 8 .. 15, further cations 1 .. 3, +- 20 %) with 1 % roughness; species 0 closes neutrality up to an
    excess of +- 0.5 mol/m^3 per lane: on these grids (dx = 0.02 nm) that charge bends the potential by some mV and makes the
    migration term a visible part of the right-hand side, where an exactly neutral state would leave it to the applied field alone."""
    z = charges_of(N)
    x = np.arange(nx)[None, None, :] / float(nx)
    base = np.where(z[None, :, None] < 0, rng.uniform(8.0, 15.0, (lanes, N, 1)), rng.uniform(1.0, 3.0, (lanes, N, 1)))
    y = base * (1.0 + 0.2 * np.sin(2 * np.pi * (rng.uniform(0.5, 2.0, (lanes, N, 1)) * x + rng.uniform(size=(lanes, N, 1)))))
    y = y + NOISE * rng.uniform(-1.0, 1.0, (lanes, N, nx))
    if N > 1:
        y[:, 0] = -(z[None, 1:, None] * y[:, 1:]).sum(axis=1) + rng.uniform(-0.5, 0.5, (lanes, 1)) + 0.1 * NOISE * rng.uniform(-1, 1, (lanes, nx))
    return y.reshape(lanes, N * nx)


@functools.lru_cache(maxsize=None)
def make_case(case, seed=0):
    """Inputs of one case: problems[b] (oracle Problem of lane b), y[B][N*nx] the argument of mol_rhs, upload[B][N*nx] the state given to
    set_batch, pb[B][4], vzeta[B], flux[B][N].  The rate constants are scaled so that the largest rate of lane 0 is 0.3 of the
    diffusion scale D NOISE / dx^2 of the states (rates that would vanish in the sum could be wrong unnoticed)."""
    N, nx = case.N, case.nx
    rng = np.random.default_rng([nx, N, seed, len(case.table)])
    D = np.array([D_TABLE[k % len(D_TABLE)] * (1.0 + 0.01 * (k // len(D_TABLE))) for k in range(N)])
    y = random_states(rng, N, nx)
    upload = 2.0 * y
    upload[:, :nx] += rng.uniform(0.5, 1.5, (B, nx))                      # ... and not neutral
    pb = np.stack([np.array(MOL_PB[case.pb])] * B)
    pb *= rng.uniform(0.6, 1.4, (B, 4)) * np.where(rng.uniform(size=(B, 4)) < 0.3, -1.0, 1.0)
    vzeta = rng.uniform(-0.02, 0.02, B)
    flux = rng.uniform(1.0, 10.0, (B, N)) * (-1.0) ** np.add.outer(np.arange(B), np.arange(N) * (N > 2))     # signs alternate over lanes and species
    for b in range(B):
        flux[b, (b + 1) % N] = 0.0 if N > 1 or b == 2 else flux[b, 0]      # one zero per lane (N = 1: one lane with zero flux)
    base = dict(D=D, charges=charges_of(N) * FARADAY, beta=1.0 / RT, eps=78.36 * 8.854187817e-12, dx=DX, nx=nx, dt=DT,
                lax_friedrich=case.lf, use_migration=case.mig)
    reactions = table(case.table, N)
    if reactions:
        probe = R.Problem(pb=pb[0], vzeta=vzeta[0], flux_bound=flux[0], reactions=reactions, **base)
        scale = 0.3 * D.max() * NOISE / DX ** 2 / np.abs(R.get_rates(y[0].reshape(N, nx), probe)).max()
        reactions = [(l, r, kf * scale, kr * scale) for l, r, kf, kr in reactions]
    problems = tuple(R.Problem(pb=pb[b], vzeta=vzeta[b], flux_bound=flux[b], reactions=reactions, **base) for b in range(B))
    for a in (y, upload, pb, vzeta, flux):
        a.setflags(write=False)
    return Inputs(case, problems, y, upload, pb, vzeta, flux)


def oracle_rhs(inp, solver='banded'):
    return np.stack([R.mol_rhs(inp.y[b], p, use_reactions=bool(p.reactions), solver=solver) for b, p in enumerate(inp.problems)])


@functools.lru_cache(maxsize=None)
def mp_rhs(case):
    inp = make_case(case)
    return tuple(M.mol_rhs(inp.y[b], p, use_reactions=bool(p.reactions)) for b, p in enumerate(inp.problems))


FLOOR = 2.0 ** -53      # the rounding of one fp64 result: no fp64 evaluation can be held to less


@functools.lru_cache(maxsize=None)
def e_oracle(case):
    """E_oracle of a short-grid case: the fp64 oracle's (Thomas / left-to-right sums) largest row-scaled error against the multiprecision
    value, over lanes and species rows; not below the rounding of one result."""
    inp, ref = make_case(case), mp_rhs(case)
    f = oracle_rhs(inp)
    return max(FLOOR, max(float(M.row_errors(f[b], ref[b], case.N).max()) for b in range(B)))


def bar_short(case):
    """16 E_oracle of the case (device and oracle are both fp64 and differ in summation order and FMA contraction only: tree scans of
    depth log2(nx) against left-to-right sums), never looser than the 1e-9 of the older tests."""
    return min(16.0 * e_oracle(case), 1e-9)


@functools.lru_cache(maxsize=None)
def e_oracle_max():
    return max(e_oracle(c) for c in SHORT)


def bar_long(case):
    """grids without a multiprecision value, against the fp64 oracle: 16 x the largest E_oracle of the short grids, times nx/259 for
    the longer prefix sums; never looser than 1e-9."""
    return min(16.0 * e_oracle_max() * case.nx / float(MP_MAX_NX), 1e-9)


def rate_magnitudes(C, p):
    """[N][nx]: |pl kf| + |pr kr| of the reaction that writes each species' rate last (get_rates' overwrite order): the size of the
    two terms whose difference the rate is, i.e. what its rounding error is proportional to."""
    mag = np.zeros_like(C)
    for lhs, rhs, kf, kr in p.reactions:
        pl = np.ones(C.shape[1]); pr = np.ones(C.shape[1])
        for k in lhs:
            pl = pl * C[k]
        for k in rhs:
            pr = pr * C[k]
        for k in list(lhs) + list(rhs):
            mag[k] = np.abs(pl * kf) + np.abs(pr * kr)
    return mag
