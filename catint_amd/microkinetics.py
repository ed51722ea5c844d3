"""Host-side description of a mean-field surface microkinetic model: adsorbates on one site type, elementary steps with optional
transition states, free energies that depend on the potential (through the electrons of a step) and on the surface charge.
``MeanFieldModel.tables()`` turns it into the dimensionless arrays of ``include/catint_kinetics.h`` that the device solves
(``catint_amd._kinetics.KineticsSolver``, ``PnpSolver.get_kinetics``, ``Calculator.set_microkinetics``)."""
import math
import re

import numpy as np

from .units import unit_e, unit_kB

PLANCK = 6.62607004e-34        # J s
MAX_ORDER, MAX_SITES = 3, 3
_UC_PER_CM2 = 100.0            # 1 C/m^2 in micro C/cm^2


class MicrokineticsError(ValueError):
    pass


def _term(text):
    """'2*_t' -> (2, '*', 't');  'CO2*_t' -> (1, 'CO2*', 't');  '2OH_g' -> (2, 'OH', 'g')"""
    m = re.match(r'^(\d*)\s*(.+)_([A-Za-z0-9]+)$', text.strip())
    if not m:
        raise MicrokineticsError('cannot read the term %r: expected [count]name_site, e.g. CO2_g, 2*_t, COOH*_t' % text)
    return int(m.group(1) or 1), m.group(2), m.group(3)


def parse_step(expr):
    """CatMAP's rxn_expressions notation with one site type: 'A_g + 2*_t <-> TS_t <-> B*_t + C_g; beta=0.5; prefactor=1e13'.
    Returns (step dict with the raw names of the string, site type or None).  Names: '*' the free site, 'X*' / 'X' on the site type the
    adsorbate X, 'ele_g' an electron, 'X_g' the solution name 'X_g'."""
    head, *opts = [s.strip() for s in expr.split(';')]
    parts = [s.strip() for s in head.split('<->')]
    if len(parts) not in (2, 3):
        raise MicrokineticsError('a step is "reactants <-> products" or "reactants <-> transition state <-> products": %r' % expr)
    step = {'reactants': {}, 'products': {}, 'ts': None, 'electrons': 0, 'beta': 0.5, 'prefactor': None}
    sites = set()

    def side(text, into):
        for term in text.split(' + '):
            count, name, site = _term(term)
            if site == 'g':
                if name == 'ele':
                    step['electrons'] += count if into == 'reactants' else -count
                    continue
                key = name + '_g'
            else:
                sites.add(site)
                key = '*' if name == '*' else name.rstrip('*')
            step[into][key] = step[into].get(key, 0) + count
    side(parts[0], 'reactants')
    side(parts[-1], 'products')
    if len(parts) == 3:
        count, name, site = _term(parts[1])
        if site == 'g' or count != 1:
            raise MicrokineticsError('the transition state of %r must be one species on the surface' % expr)
        sites.add(site)
        step['ts'] = name.rstrip('*')
    for o in opts:
        if not o:
            continue
        k, _, v = o.partition('=')
        if k.strip() not in ('beta', 'prefactor'):
            raise MicrokineticsError('unknown option %r in %r (known: beta, prefactor)' % (k.strip(), expr))
        step[k.strip()] = float(v)
    if len(sites) > 1:
        raise MicrokineticsError('one site type is supported, %r names %s' % (expr, ', '.join(sorted(sites))))
    return step


class MeanFieldModel(object):
    """species: the transport's species names (the columns of the wall flux).  adsorbates: {name: sites it occupies (1 .. 3)}, in the
    order of the coverages.  steps: dicts {'reactants': {name: count}, 'products': {...}, 'ts': name or None, 'electrons': n_e (on the
    reactant side; negative: released), 'beta': symmetry factor, 'prefactor': A in 1/s (None: kT/h)} or strings (parse_step).  Names in
    a step: '*' the free site, an adsorbate, or a solution name; `solution` maps solution names to a transport species or to None (unit
    activity, e.g. {'H2O_g': None}); a name X_g without an entry means the transport species X.
    energies: {adsorbate or transition state: g0 or (g0, g1, g2)}, free energy g0 + g1 sigma + g2 sigma^2 in eV with sigma in micro C/cm^2
    (CatMAP's sigma_params); the free site is 0.  solution_energies: {solution name or transport species: eV}, default 0.
    The numbers handed to the device are in kT: a step with n_e electrons on the reactant side has dG = dG0 + n_e e V and, with a
    transition state, Ea = Ea0 + beta n_e e V."""

    def __init__(self, species, adsorbates, steps, energies, solution=None, solution_energies=None, temperature=298.15, cref=1000.0,
                 site_density=1e-5):
        self.species = list(species)
        self.adsorbates = list(adsorbates.keys())
        self.site_count = np.array([1.0] + [float(adsorbates[a]) for a in self.adsorbates])
        for a in self.adsorbates:
            if adsorbates[a] not in (1, 2, 3):
                raise MicrokineticsError('adsorbate %r occupies %r sites: 1 .. %d are supported' % (a, adsorbates[a], MAX_SITES))
        self.solution = dict(solution or {})
        self.energies = {k: tuple(np.atleast_1d(np.asarray(v, float))) + (0.0,) * (3 - np.size(v)) for k, v in energies.items()}
        self.solution_energies = dict(solution_energies or {})
        self.temperature = float(temperature)
        self.site_density = float(site_density)
        self.cref = np.broadcast_to(np.asarray(cref, float), (len(self.species),)).copy() if not isinstance(cref, dict) else \
            np.array([float(cref.get(s, 1000.0)) for s in self.species])
        self.steps = [parse_step(s) if isinstance(s, str) else dict({'ts': None, 'electrons': 0, 'beta': 0.5, 'prefactor': None}, **s)
                      for s in steps]
        self._check()

    # -- names ---------------------------------------------------------------------------------------------------------------------
    def _column(self, name):
        """('site', t) / ('species', k) / ('unit', None)"""
        if name == '*':
            return 'site', 0
        if name in self.adsorbates:
            return 'site', 1 + self.adsorbates.index(name)
        if name in self.solution:
            sp = self.solution[name]
            if sp is None:
                return 'unit', None
            if sp not in self.species:
                raise MicrokineticsError('%r is mapped to %r, which is not a transport species (%s)' % (name, sp, ', '.join(self.species)))
            return 'species', self.species.index(sp)
        bare = name[:-2] if name.endswith('_g') else name
        if bare in self.species:
            return 'species', self.species.index(bare)
        raise MicrokineticsError('unknown name %r: neither the free site *, an adsorbate (%s), a transport species (%s) nor an entry of '
                                 '`solution`' % (name, ', '.join(self.adsorbates), ', '.join(self.species)))

    def _energy(self, name):
        kind, _ = self._column(name)
        if name == '*':
            return (0.0, 0.0, 0.0)
        if kind == 'site':
            if name not in self.energies:
                raise MicrokineticsError('no free energy for the adsorbate %r' % name)
            return self.energies[name]
        bare = name[:-2] if name.endswith('_g') else name
        for key in (name, bare, self.solution.get(name)):
            if key in self.solution_energies:
                return (float(self.solution_energies[key]), 0.0, 0.0)
        return (0.0, 0.0, 0.0)

    def _check(self):
        for i, st in enumerate(self.steps):
            sites = 0.0
            for sign, side in ((-1, 'reactants'), (1, 'products')):
                for name, count in st[side].items():
                    kind, col = self._column(name)
                    if int(count) != count or not 0 < count <= MAX_ORDER:
                        raise MicrokineticsError('step %d: %r appears %r times, 1 .. %d are supported' % (i, name, count, MAX_ORDER))
                    if kind == 'site':
                        sites += sign * count * self.site_count[col]
            if sites != 0.0:
                raise MicrokineticsError('step %d does not conserve sites: the products hold %+g sites more than the reactants' % (i, sites))
            if st['ts'] is not None and st['ts'] not in self.energies:
                raise MicrokineticsError('step %d: no free energy for the transition state %r' % (i, st['ts']))

    # -- the arrays of include/catint_kinetics.h ---------------------------------------------------------------------------------------
    @property
    def kT(self):
        """eV"""
        return unit_kB * self.temperature / unit_e

    def electrons(self):
        """[R]: the electrons on the reactant side of every step (negative: released), the n_e that tables() puts into dG and Ea; what
        catint_amd.voltammetry.Voltammetry.sweep counts the current with"""
        return np.array([float(st['electrons']) for st in self.steps])

    def tables(self, site_density=None):
        N, T, R = len(self.species), len(self.site_count), len(self.steps)
        kT = self.kT
        of, ob = np.zeros((R, N + T), np.int32), np.zeros((R, N + T), np.int32)
        nu, dG, Ea, lnA = np.zeros((R, N)), np.zeros((R, 4)), np.zeros((R, 4)), np.zeros(R)
        scale = np.array([1.0, _UC_PER_CM2, _UC_PER_CM2 ** 2]) / kT          # eV (micro C/cm^2)^-k -> kT (C/m^2)^-k
        for r, st in enumerate(self.steps):
            g = {'reactants': np.zeros(3), 'products': np.zeros(3)}
            for side, table, sign in (('reactants', of, -1.0), ('products', ob, 1.0)):
                for name, count in st[side].items():
                    kind, col = self._column(name)
                    if kind == 'site':
                        table[r, N + col] += int(count)
                    elif kind == 'species':
                        table[r, col] += int(count)
                        nu[r, col] += sign * count
                    g[side] += count * np.array(self._energy(name))
            ne = float(st['electrons'])
            d = (g['products'] - g['reactants']) * scale
            dG[r] = [d[0], ne / kT, d[1], d[2]]
            if st['ts'] is None:
                Ea[r] = [-np.inf, 0.0, 0.0, 0.0]
            else:
                e = (np.array(self.energies[st['ts']]) - g['reactants']) * scale
                Ea[r] = [e[0], float(st['beta']) * ne / kT, e[1], e[2]]
            A = st['prefactor'] if st['prefactor'] is not None else unit_kB * self.temperature / PLANCK
            lnA[r] = math.log(A)
        return {'order_f': of, 'order_b': ob, 'nu': nu, 'cref': self.cref.copy(), 'site_count': self.site_count.copy(), 'dG': dG, 'Ea': Ea,
                'lnA': lnA, 'site_density': self.site_density if site_density is None else float(site_density)}
