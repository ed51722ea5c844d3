"""Host-side description of a surface microkinetic model with lateral interactions between the adsorbates and several site types
(terrace and step): what ``catint_amd.microkinetics.MeanFieldModel`` leaves out.  ``InteractingModel.tables()`` returns the arrays of
``include/catint_interact.h`` -- the keys of ``MeanFieldModel.tables()`` with one free-site column per type, plus the interaction
matrices in kT -- which ``catint_amd._interact.InteractingKinetics`` solves on the device (``PnpSolver.get_kinetics``,
``Calculator.set_microkinetics`` route a model that carries these keys there)."""
import math

import numpy as np

from .microkinetics import MAX_SITES, MeanFieldModel, MicrokineticsError, _term

MAX_SITE_TYPES, MAX_COLUMNS = 3, 9
RESPONSES = ('linear', 'piecewise')
# the keys of tables() that route a model to libcatint_interact
INTERACTION_KEYS = ('site_of', 'site_fraction', 'eps', 'eps_ts', 'response', 'cutoff', 'smoothing', 'strength')


def has_interactions(tables):
    """Whether the dict carries the keys of include/catint_interact.h (and so cannot go to the mean-field libraries)"""
    return 'site_of' in tables or 'eps' in tables


def parse_step(expr):
    """CatMAP's rxn_expressions notation with the site suffix kept: 'CO2_g + *_t <-> CO2*_t', 'H*_s + CO*_t <-> HCO-TS_t <-> CHO*_t + *_s;
    beta=0.5'.  Returns the step dict of microkinetics.parse_step whose surface names are (name, site) pairs: ('*', 't') the free site of
    type t, ('CO', 't') the adsorbate CO on t; 'ts' is (name, site) or None."""
    head, *opts = [s.strip() for s in expr.split(';')]
    parts = [s.strip() for s in head.split('<->')]
    if len(parts) not in (2, 3):
        raise MicrokineticsError('a step is "reactants <-> products" or "reactants <-> transition state <-> products": %r' % expr)
    step = {'reactants': {}, 'products': {}, 'ts': None, 'electrons': 0, 'beta': 0.5, 'prefactor': None}

    def side(text, into):
        for term in text.split(' + '):
            count, name, site = _term(term)
            if site == 'g':
                if name == 'ele':
                    step['electrons'] += count if into == 'reactants' else -count
                    continue
                key = name + '_g'
            else:
                key = ('*' if name == '*' else name.rstrip('*'), site)
            step[into][key] = step[into].get(key, 0) + count
    side(parts[0], 'reactants')
    side(parts[-1], 'products')
    if len(parts) == 3:
        count, name, site = _term(parts[1])
        if site == 'g' or count != 1:
            raise MicrokineticsError('the transition state of %r must be one species on the surface' % expr)
        step['ts'] = (name.rstrip('*'), site)
    for o in opts:
        if not o:
            continue
        k, _, v = o.partition('=')
        if k.strip() not in ('beta', 'prefactor'):
            raise MicrokineticsError('unknown option %r in %r (known: beta, prefactor)' % (k.strip(), expr))
        step[k.strip()] = float(v)
    return step


class InteractingModel(MeanFieldModel):
    """species, steps, energies, solution, solution_energies, temperature, cref, site_density: as MeanFieldModel.
    adsorbates: {name: (site type, sites it occupies)} in the order of the coverages (or {name: count} with one site type).
    site_fractions: {site type: fraction of all sites}, in the order of the free-site columns; None: one type, the adsorbates', with
    fraction 1.  All coverages count per total site, so those of type g sum to its fraction.
    A step string keeps its site suffix ('H*_s + CO*_t <-> ...'); in a step dict the free site of type t is '*_t' ('*' with one type).
    An adsorbate that lives on two types is two adsorbates, named with the suffix: {'H_s': ('s', 1), 'H_t': ('t', 1)}.
    interactions: {(a, b): eV} per unit coverage, symmetric; a missing cross term is sqrt(eps_aa eps_bb) when both self terms are given
    and positive (the geometric-mean rule), else 0.  strength scales all of them (CatMAP's interaction_strength).
    response: 'linear' (f = 1) or 'piecewise' (CatMAP's smooth piecewise linear function of the crowding of the site type) with cutoff
    and smoothing, numbers or {site type: number}.
    ts_interactions: 'intermediate_state' -- the row of a transition state is the mean of the rows of its initial and final state -- or
    {transition state: {adsorbate: eV}} (a transition state without an entry gets the mean)."""

    def __init__(self, species, adsorbates, steps, energies, interactions=None, site_fractions=None, response='linear', strength=1.0,
                 ts_interactions='intermediate_state', cutoff=0.25, smoothing=0.05, solution=None, solution_energies=None, temperature=298.15,
                 cref=1000.0, site_density=1e-5):
        ads = {a: (v if isinstance(v, (tuple, list)) else (None, v)) for a, v in adsorbates.items()}
        named = [s for s, _ in ads.values() if s is not None]
        if site_fractions is None:
            kinds = sorted(set(named)) or ['t']
            if len(kinds) > 1:
                raise MicrokineticsError('the adsorbates name the site types %s: site_fractions is needed' % ', '.join(kinds))
            site_fractions = {kinds[0]: 1.0}
        self.site_types = list(site_fractions.keys())
        G = len(self.site_types)
        if not 1 <= G <= MAX_SITE_TYPES:
            raise MicrokineticsError('%d site types: 1 .. %d are supported' % (G, MAX_SITE_TYPES))
        self.site_fraction = np.array([float(site_fractions[s]) for s in self.site_types])
        if not (np.isfinite(self.site_fraction).all() and (self.site_fraction > 0).all()):
            raise MicrokineticsError('every site fraction must be positive and finite')
        self.adsorbates = list(ads.keys())
        if G + len(self.adsorbates) > MAX_COLUMNS or not self.adsorbates:
            raise MicrokineticsError('%d adsorbates on %d site types: at least one adsorbate and at most %d columns' % (len(self.adsorbates), G, MAX_COLUMNS))
        site_of = list(range(G))
        for a in self.adsorbates:
            site, count = ads[a]
            site = self.site_types[0] if site is None and G == 1 else site
            if site not in self.site_types:
                raise MicrokineticsError('adsorbate %r is on the site type %r, which has no fraction (%s)' % (a, site, ', '.join(self.site_types)))
            if count not in (1, 2, 3):
                raise MicrokineticsError('adsorbate %r occupies %r sites: 1 .. %d are supported' % (a, count, MAX_SITES))
            site_of.append(self.site_types.index(site))
        self.site_of = np.array(site_of, np.int32)
        self.site_count = np.array([1.0] * G + [float(ads[a][1]) for a in self.adsorbates])
        self.species = list(species)
        self.solution = dict(solution or {})
        self.energies = {k: tuple(np.atleast_1d(np.asarray(v, float))) + (0.0,) * (3 - np.size(v)) for k, v in energies.items()}
        self.solution_energies = dict(solution_energies or {})
        self.temperature = float(temperature)
        self.site_density = float(site_density)
        self.cref = np.broadcast_to(np.asarray(cref, float), (len(self.species),)).copy() if not isinstance(cref, dict) else \
            np.array([float(cref.get(s, 1000.0)) for s in self.species])
        if response not in RESPONSES:
            raise MicrokineticsError('response %r: one of %s' % (response, ', '.join(RESPONSES)))
        self.response = response
        self.strength = float(strength)
        if not math.isfinite(self.strength):
            raise MicrokineticsError('strength must be finite')
        self.cutoff, self.smoothing = self._per_type(cutoff, 'cutoff'), self._per_type(smoothing, 'smoothing')
        if response == 'piecewise' and not (self.smoothing > 0).all():
            raise MicrokineticsError('smoothing must be positive')
        self.steps = [self._resolve(parse_step(s)) if isinstance(s, str) else dict({'ts': None, 'electrons': 0, 'beta': 0.5, 'prefactor': None}, **s)
                      for s in steps]
        self._check()
        self._check_types()
        self.interactions = self._matrix(interactions or {})
        self.ts_interactions = ts_interactions
        if ts_interactions != 'intermediate_state':
            for ts, row in ts_interactions.items():
                for a in row:
                    if a not in self.adsorbates:
                        raise MicrokineticsError('ts_interactions[%r] names %r, which is no adsorbate' % (ts, a))

    def _per_type(self, value, what):
        if isinstance(value, dict):
            out = np.array([float(value[s]) for s in self.site_types])
        else:
            out = np.full(len(self.site_types), float(value))
        if not np.isfinite(out).all():
            raise MicrokineticsError('%s must be finite' % what)
        return out

    # -- names ---------------------------------------------------------------------------------------------------------------------
    def _adsorbate(self, name, site, expr='a step'):
        for key in (name + '_' + site, name):
            if key in self.adsorbates:
                if self.site_types[self.site_of[len(self.site_types) + self.adsorbates.index(key)]] != site:
                    raise MicrokineticsError('%s puts %r on the site type %r, the model has it on another' % (expr, name, site))
                return key
        raise MicrokineticsError('unknown adsorbate %r on the site type %r (%s)' % (name, site, ', '.join(self.adsorbates)))

    def _resolve(self, step):
        """the (name, site) pairs of parse_step as the model's names: '*_t', an adsorbate, a transition state"""
        for side in ('reactants', 'products'):
            out = {}
            for key, count in step[side].items():
                if isinstance(key, tuple):
                    name, site = key
                    if site not in self.site_types:
                        raise MicrokineticsError('unknown site type %r (%s)' % (site, ', '.join(self.site_types)))
                    key = '*_' + site if name == '*' else self._adsorbate(name, site)
                out[key] = out.get(key, 0) + count
            step[side] = out
        if step['ts'] is not None:
            name, site = step['ts']
            step['ts'] = name if name in self.energies or name + '_' + site not in self.energies else name + '_' + site
        return step

    def _column(self, name):
        G = len(self.site_types)
        if name == '*' and G > 1:
            raise MicrokineticsError("'*' names no site type: with %d types the free sites are %s" % (G, ', '.join('*_' + s for s in self.site_types)))
        if isinstance(name, str) and name.startswith('*_') and name[2:] in self.site_types:
            return 'site', self.site_types.index(name[2:])
        if name in self.adsorbates:
            return 'site', G + self.adsorbates.index(name)
        return MeanFieldModel._column(self, name)

    def _energy(self, name):
        if isinstance(name, str) and name.startswith('*'):
            return (0.0, 0.0, 0.0)
        return MeanFieldModel._energy(self, name)

    def _check_types(self):
        G = len(self.site_types)
        for i, st in enumerate(self.steps):
            sites = np.zeros(G)
            for sign, side in ((-1, 'reactants'), (1, 'products')):
                for name, count in st[side].items():
                    kind, col = self._column(name)
                    if kind == 'site':
                        sites[self.site_of[col]] += sign * count * self.site_count[col]
            for g in range(G):
                if sites[g] != 0.0:
                    raise MicrokineticsError('step %d does not conserve the sites of type %r: the products hold %+g more than the reactants'
                                             % (i, self.site_types[g], sites[g]))

    def _matrix(self, given):
        """eps [S][S] in eV: symmetric, missing cross terms by the geometric mean of the self terms"""
        S = len(self.adsorbates)
        eps, known = np.zeros((S, S)), np.zeros((S, S), bool)
        for (a, b), v in given.items():
            for nm in (a, b):
                if nm not in self.adsorbates:
                    raise MicrokineticsError('interactions names %r, which is no adsorbate (%s)' % (nm, ', '.join(self.adsorbates)))
            if not math.isfinite(float(v)):
                raise MicrokineticsError('the interaction of %r and %r is not finite' % (a, b))
            i, j = self.adsorbates.index(a), self.adsorbates.index(b)
            if known[i, j] and eps[i, j] != float(v):
                raise MicrokineticsError('the interaction of %r and %r is given twice with different values' % (a, b))
            eps[i, j] = eps[j, i] = float(v)
            known[i, j] = known[j, i] = True
        for i in range(S):
            for j in range(S):
                if not known[i, j] and i != j and known[i, i] and known[j, j] and eps[i, i] > 0 and eps[j, j] > 0:
                    eps[i, j] = math.sqrt(eps[i, i] * eps[j, j])
        return eps

    # -- the arrays of include/catint_interact.h ---------------------------------------------------------------------------------------
    def tables(self, site_density=None):
        tab = MeanFieldModel.tables(self, site_density)
        N, G, S, R = len(self.species), len(self.site_types), len(self.adsorbates), len(self.steps)
        kT = self.kT
        eps = self.interactions / kT
        of, ob = tab['order_f'][:, N + G:].astype(float), tab['order_b'][:, N + G:].astype(float)
        eps_ts = 0.5 * (of @ eps + ob @ eps)
        if self.ts_interactions != 'intermediate_state':
            for r, st in enumerate(self.steps):
                row = self.ts_interactions.get(st['ts']) if st['ts'] is not None else None
                if row is not None:
                    eps_ts[r] = [float(row.get(a, 0.0)) / kT for a in self.adsorbates]
        for r, st in enumerate(self.steps):
            if st['ts'] is None:
                eps_ts[r] = 0.0
        tab.update(site_of=self.site_of.copy(), site_fraction=self.site_fraction.copy(), eps=eps, eps_ts=eps_ts, response=self.response,
                   cutoff=self.cutoff.copy(), smoothing=self.smoothing.copy(), strength=self.strength)
        return tab
