"""The cases of tests/test_interact_abi.py and tests/test_gpu_interact.py (test infrastructure, no tests of its own): the four-step CO2
reduction mechanism of tests/kinetics_cases.py in both site variants with a weak (0.3 eV self, 0.15 eV cross) and a strong (1.0 / 0.5 eV)
interaction between all adsorbates, a terrace-and-step variant with two site types, and random reversible networks with G = 1, 2, 3 site
types in both response modes.  The energies are illustrative numbers chosen for this file.  references(name) solves a case once per
session in fp64 (tests/interact_ref.py: solve_fp64) and at 60 digits (solve_mp); every test shares the result and leaves it unchanged."""
import functools
from collections import namedtuple

import numpy as np

from catint_amd.interactions import InteractingModel
from tests import interact_ref as IR
from tests import kinetics_cases as KC
from tests import kinetics_ref as KR

Case = namedtuple('Case', 'name tables phiM csurf phi_surface kw ramp')


def pair_interactions(names, self_eV, cross_eV):
    return {(a, b): (self_eV if a == b else cross_eV) for i, a in enumerate(names) for b in names[i:]}


def co2r_model(variant, self_eV, cross_eV, **kw):
    sites = KC.SITES[variant]
    return InteractingModel(KC.SPECIES, {a: ('t', n) for a, n in sites.items()}, KC.STEPS[variant], KC.ENERGIES,
                            interactions=pair_interactions(list(sites), self_eV, cross_eV), solution=KC.SOLUTION,
                            solution_energies=KC.SOLUTION_ENERGIES, temperature=298.15, cref=1000.0, site_density=1.6e-5, **kw)


def lattice():
    """the operating points of kinetics_cases.co2r_case"""
    c = KC.co2r_case('one_site')
    return c.phiM, c.csurf, c.phi_surface


def co2r_case(variant, self_eV, cross_eV, tag):
    phiM, csurf, phis = lattice()
    return Case('co2r_%s_%s' % (variant, tag), co2r_model(variant, self_eV, cross_eV).tables(), phiM, csurf, phis, dict(KC.STERN), 5)


TERRACE_STEP_ADSORBATES = {'CO2': ('t', 1), 'COOH': ('t', 1), 'CO_t': ('t', 1), 'CO_s': ('s', 1), 'H': ('s', 1)}
TERRACE_STEP_STEPS = ['CO2_g + *_t <-> CO2*_t',
                      'CO2*_t + H2O_g + ele_g <-> COOH*_t + OH_g',
                      'COOH*_t + ele_g <-> COOH-ele_t <-> CO*_t + OH_g; beta=0.5',
                      'CO*_t <-> CO_g + *_t',
                      'CO*_t + *_s <-> CO*_s + *_t',
                      'CO*_s <-> CO_g + *_s',
                      'H2O_g + ele_g + *_s <-> H*_s + OH_g']
TERRACE_STEP_ENERGIES = dict(KC.ENERGIES, CO_t=KC.ENERGIES['CO'], CO_s=(0.10, 0.002, 0.0), H=(1.6, 0.0, 0.0))


def terrace_step_model(**kw):
    """Terrace sites (90 %) carry the mechanism, step sites (10 %) bind CO more strongly and hydrogen; CO repels CO on and across both"""
    inter = {('CO_t', 'CO_t'): 0.3, ('CO_s', 'CO_s'): 0.5, ('H', 'CO_s'): 0.1, ('CO2', 'CO2'): 0.2, ('COOH', 'COOH'): 0.2}
    return InteractingModel(KC.SPECIES, TERRACE_STEP_ADSORBATES, TERRACE_STEP_STEPS, TERRACE_STEP_ENERGIES, interactions=inter,
                            site_fractions={'t': 0.9, 's': 0.1}, solution=KC.SOLUTION, solution_energies=KC.SOLUTION_ENERGIES,
                            temperature=298.15, cref=1000.0, site_density=1.6e-5, **kw)


def terrace_step_case():
    phiM, csurf, phis = (v[np.arange(39) // 3 % 2 == 0] for v in lattice())          # every other potential: 21 points
    # one stage: without the repulsion (the first stage of a ramp) CO saturates the step sites and the damped iteration of the header
    # does not converge from the uniform start at most of these points; at full strength it does at all of them
    return Case('terrace_step', terrace_step_model().tables(), phiM, csurf, phis, dict(KC.STERN), 1)


def random_network(S, G, response, seed):
    """The chain of kinetics_cases.random_network with every adsorbate on a random one of G site types (each type at least once), the
    free sites of each type added to the side that holds fewer of that type; a random symmetric eps in [0, 6] kT, random eps_ts."""
    rng = np.random.RandomState(seed)
    N = min(8, 2 + S // 2)
    T = G + S
    site_of = np.concatenate([np.arange(G), rng.permutation(np.concatenate([np.arange(G), rng.randint(0, G, S - G)]))]).astype(np.int32)
    ns = np.concatenate([np.ones(G), rng.randint(1, 4, S).astype(float)])
    frac = rng.dirichlet(np.full(G, 4.0))
    rows = []

    def step(lhs, rhs, nu):
        of, ob = np.zeros(N + T, np.int32), np.zeros(N + T, np.int32)
        for col, cnt in lhs:
            of[col] += cnt
        for col, cnt in rhs:
            ob[col] += cnt
        for g in range(G):
            on = site_of == g
            diff = float((ns * (ob[N:] - of[N:]))[on].sum())
            if diff > 0:
                of[N + g] += int(diff)
            else:
                ob[N + g] += int(-diff)
        if of.max() > 3 or ob.max() > 3:
            return
        rows.append((of, ob, nu))
    z = np.zeros(N)
    A = N + G - 1          # adsorbate i = 1 .. S is column A + i
    step([(0, 1)], [(A + 1, 1)], -np.eye(N)[0])
    for i in range(1, S):
        step([(A + i, 1)], [(A + i + 1, 1)], z)
    step([(A + S, 1)], [(1, 1)], np.eye(N)[1])
    if S >= 2:
        i, j = rng.choice(np.arange(1, S + 1), 2, replace=False)
        step([(A + i, 2)], [(A + j, 1)], z)
    tries = 0
    while len(rows) < min(16, 2 * S) and S >= 3 and tries < 100:
        tries += 1
        i, j = rng.choice(np.arange(1, S + 1), 2, replace=False)
        if abs(i - j) > 1:
            step([(A + i, 1)], [(A + j, 1)], z)
    R = len(rows)
    dG = np.stack([rng.uniform(-3, 3, R), rng.choice([0.0, 0.0, 19.5], R), rng.uniform(-3, 3, R), rng.uniform(-5, 5, R)], axis=1)
    Ea = np.stack([rng.uniform(0, 8, R), 0.5 * dG[:, 1], rng.uniform(-1, 1, R), np.zeros(R)], axis=1)
    no_ts = rng.rand(R) < 0.4
    Ea[no_ts] = [-np.inf, 0.0, 0.0, 0.0]
    eps = rng.uniform(0, 6, (S, S))
    eps = 0.5 * (eps + eps.T)
    eps_ts = rng.uniform(0, 6, (R, S))
    eps_ts[no_ts] = 0.0
    tables = {'order_f': np.stack([r[0] for r in rows]), 'order_b': np.stack([r[1] for r in rows]), 'nu': np.stack([r[2] for r in rows]),
              'cref': np.full(N, 1000.0), 'site_count': ns, 'dG': dG, 'Ea': Ea, 'lnA': 29.4 + rng.uniform(-2, 2, R), 'site_density': 1e-5,
              'site_of': site_of, 'site_fraction': frac, 'eps': eps, 'eps_ts': eps_ts, 'response': response,
              'cutoff': rng.uniform(0.1, 0.4, G), 'smoothing': rng.uniform(0.03, 0.1, G), 'strength': 1.0}
    phiM = np.array([-0.2, -0.5, -0.8, -1.1])
    csurf = np.zeros((4, N))
    csurf[:, 0] = [10.0, 1.0, 0.0, 25.0]
    csurf[:, 1] = [1e-2, 0.0, 5.0, 1e-6]
    csurf[:, 2:] = 1.0
    return Case('random_S%d_G%d_%s' % (S, G, response), tables, phiM, csurf, 0.2 * phiM, dict(w=1 if S % 2 else 0, CS=0.15, phi_pzc=0.05), 4)


# (S, G, response) -> seed.  As in kinetics_cases.SEEDS every seed was checked on the CPU to converge at all four points in every stage
# (tests/test_interact_abi.py asserts it); a network that does not is replaced by another seed, not skipped.
RANDOM = {(3, 1, 'linear'): 109, (8, 1, 'piecewise'): 115, (2, 2, 'linear'): 111, (5, 2, 'piecewise'): 120, (7, 2, 'linear'): 107,
          (3, 3, 'linear'): 121, (6, 3, 'piecewise'): 139}


def all_cases():
    out = [co2r_case(v, s, c, tag) for v in ('one_site', 'two_site') for s, c, tag in ((0.3, 0.15, 'weak'), (1.0, 0.5, 'strong'))]
    out.append(terrace_step_case())
    return out + [random_network(S, G, resp, seed) for (S, G, resp), seed in RANDOM.items()]


CASE_NAMES = ['co2r_one_site_weak', 'co2r_one_site_strong', 'co2r_two_site_weak', 'co2r_two_site_strong', 'terrace_step'] + \
    ['random_S%d_G%d_%s' % k for k in RANDOM]


@functools.lru_cache(maxsize=None)
def case(name):
    return {c.name: c for c in all_cases()}[name]


@functools.lru_cache(maxsize=None)
def fp64(name):
    """the fp64 result of a case at its ramp, computed once"""
    c = case(name)
    return IR.solve_fp64(c.tables, c.phiM, c.csurf, c.phi_surface, ramp=c.ramp, **c.kw)


@functools.lru_cache(maxsize=None)
def references(name):
    """(fp64 result, 60-digit result, errors of the fp64 result per point) of a case at its ramp, computed once"""
    c = case(name)
    fp = fp64(name)
    ref = IR.solve_mp(c.tables, c.phiM, c.csurf, c.phi_surface, fp, **c.kw)
    return fp, ref, errors(fp, ref, fp)


def errors(res, ref, fp):
    """kinetics_cases.errors, and 'energy_shift' as an absolute error in kT"""
    out = KC.errors(res, ref, fp)
    if 'energy_shift' in res:
        out['energy_shift'] = KR.mp_err(ref['energy_shift'], res['energy_shift'])
    return out
