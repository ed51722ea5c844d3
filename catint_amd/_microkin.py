"""What the ctypes bindings of the libraries that work on a surface microkinetic model (``_kinetics.py``, ``_drc.py``, ``_kintrans.py``,
``_eis.py``, ``_interact.py``, ``_scfkin.py``) share: the limits of ``include/catint_kinetics.h`` (the other headers repeat them) and
``Call``, the marshalling of the tables and the per-point arrays of a call into the members the parameter structs have in common.  The
libraries that take the medium have the counterpart in ``_medium.py``."""
import numpy as np

from ._devlib import _PD, _PI, _PL, _dptr, _f64, _i32, _iptr, _lptr, field_names, lane_list, results  # noqa: F401  (_kinetics.py .. import them here)

MAX_SPECIES, MAX_ADSORBATES, MAX_STEPS, MAX_ORDER, MAX_SITES = 8, 8, 16, 3, 3
MIN_LOG = -700.0
DROP = {'full': 0, 'stern': 1}

# values per operating point from (N, T, R)
_PER_POINT = {'sigma': lambda N, T, R: 1, 'off': lambda N, T, R: R * 2, 'gamma': lambda N, T, R: max(N, 0), 'theta_guess': lambda N, T, R: T,
              'theta': lambda N, T, R: T, 'theta0': lambda N, T, R: T, 'csurf': lambda N, T, R: max(N, 0), 'phi_surface': lambda N, T, R: 1}


class Call(object):
    """The arguments of one solve, validated: names (the requested fields), n, dims = (N, S, R), arrays (the contiguous arrays, which
    live as long as this object) and members: the members catkin_params and catdrc_params have in common, by name.  per_point: the
    per-point arrays by the name of their member (keys of _PER_POINT; None: absent), in the order their sizes are checked."""

    def __init__(self, tables, phiM, lanes, per_point, fields, known, default, potential_drop, stern_capacitance, phi_pzc, max_waves):
        site_count = _f64(tables['site_count']).reshape(-1)
        of, ob = _i32(tables['order_f']), _i32(tables['order_b'])
        T = len(site_count)
        S = T - 1
        R = of.shape[0] if of.ndim == 2 else 0
        N = (of.shape[1] - T) if of.ndim == 2 else 0
        self.names = field_names(fields, known, default)
        pm = _f64(np.atleast_1d(np.asarray(phiM, float))).reshape(-1)
        n = len(pm)
        idx = lane_list(lanes)
        if idx is not None and len(idx) != n:
            raise ValueError('lanes has %d entries, phiM %d' % (len(idx), n))
        nu, cref, dG, Ea, lnA = (_f64(tables[k]) for k in ('nu', 'cref', 'dG', 'Ea', 'lnA'))
        pp = {name: _f64(a) for name, a in per_point.items()}
        for name, a in pp.items():
            size = n * _PER_POINT[name](N, T, R)
            if a is not None and a.size != size:
                raise ValueError('%s has %d values, the call needs %d' % (name, a.size, size))
        for name, a, size in (('order_b', ob, R * (N + T)), ('nu', nu, R * max(N, 0)), ('cref', cref, max(N, 0)), ('dG', dG, R * 4), ('Ea', Ea, R * 4),
                              ('lnA', lnA, R)):
            if a.size != size:
                raise ValueError('%s has %d values, the tables need %d' % (name, a.size, size))
        self.n, self.dims = n, (N, S, R)
        self.arrays = [site_count, of, ob, pm, idx, nu, cref, dG, Ea, lnA] + list(pp.values())
        self.members = dict(max_waves=int(max_waves), nspecies=N, nadsorbates=S, nsteps=R,
                            potential_drop=potential_drop if isinstance(potential_drop, int) else DROP[potential_drop], n=n,
                            lanes=_lptr(idx), order_f=_iptr(of), order_b=_iptr(ob), nu=_dptr(nu),
                            cref=_dptr(cref), site_count=_dptr(site_count), dG=_dptr(dG), Ea=_dptr(Ea), lnA=_dptr(lnA),
                            site_density=float(tables['site_density']), stern_capacitance=float(stern_capacitance), phi_pzc=float(phi_pzc),
                            phiM=_dptr(pm), **{name: _dptr(a) for name, a in pp.items()})

    def results(self, known, out):
        """the dict a solve returns: `out` or a new one, with an array of the field's shape for every requested name that has none"""
        N, S, R = (max(v, 0) for v in self.dims)
        return results(out, {name: known[name](N, S, R) for name in self.names}, (self.n,))
