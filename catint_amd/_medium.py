"""What the ctypes bindings of the libraries that take the medium and its tables (``_response.py``, ``_couple.py``, ``_sens.py``,
``_modes.py``, ``_balance.py`` and ``Impedance.solve`` of ``_eis.py``) share, the counterpart of ``_microkin.Call``: the marshalling of
the medium, the reaction table, the wall table and the lane list of a call into the members the parameter structs have in common, by
name, and the size checks of those arrays."""
from ._capi import flatten_reactions as reaction_table      # the arrays of pnp_set_reactions: the parameter structs take the same form
from ._devlib import _dptr, _f64, _i32, _iptr, _lptr, lane_list

WALL = {'dirichlet': 0, 'stern': 1}


class Medium(object):
    """The medium of one call about the state behind `view`, marshalled: dims = (B, N, nx) of the view, idx (the lane list or None), n
    (the number of operating points of the call), arrays (the contiguous arrays, which live as long as this object) and members: the
    members of the parameter struct by name.  Every struct has D, charges, mpb_radius, x, beta, velocity and the reaction table;
    `given` holds what only some have, each under the name of its argument: eps, dx, stern_capacitance, wall_bc, max_waves, wall (->
    n_wall, wall_species, nu, k, alpha, saturation) and lanes (-> lanes and nlanes, the batch where lanes is None)."""

    def __init__(self, view, D, charges, x, beta, mpb_radius=None, velocity=0.0, reactions=(), **given):
        B, N, _ = self.dims = tuple(max(int(v), 0) for v in (view.batch, view.nspecies, view.nx))
        R, n_lhs, lhs, n_rhs, rhs, kf, kr = reaction_table(list(reactions))
        self.D, self.charges, self.x, self.radius = (_f64(a) for a in (D, charges, x, mpb_radius))
        self.arrays = [n_lhs, lhs, n_rhs, rhs, kf, kr]
        m = self.members = dict(nreactions=R, D=_dptr(self.D), charges=_dptr(self.charges), mpb_radius=_dptr(self.radius), x=_dptr(self.x),
                                beta=float(beta), velocity=float(velocity), n_lhs=_iptr(n_lhs), lhs=_iptr(lhs), n_rhs=_iptr(n_rhs),
                                rhs=_iptr(rhs), kf=_dptr(kf), kr=_dptr(kr))
        for name in ('eps', 'dx', 'stern_capacitance'):
            if name in given:
                m[name] = float(given[name])
        if 'max_waves' in given:
            m['max_waves'] = int(given['max_waves'])
        if 'wall_bc' in given:
            m['wall_bc'] = given['wall_bc'] if isinstance(given['wall_bc'], int) else WALL[given['wall_bc']]
        self.wall_sizes = []
        if 'wall' in given:
            wall = given['wall']
            W = 0 if not wall else len(wall['species'])
            wk = [None] * 5
            if W:
                wk = [_i32(wall['species']), _f64(wall['nu']), _f64(wall.get('k')), _f64(wall.get('alpha')), _f64(wall.get('saturation'))]
            self.arrays += wk
            self.wall_sizes = [('wall k', wk[2], B * W), ('wall nu', wk[1], W * N), ('wall alpha', wk[3], W), ('wall saturation', wk[4], W)]
            m.update(n_wall=W, wall_species=_iptr(wk[0]), nu=_dptr(wk[1]), k=_dptr(wk[2]), alpha=_dptr(wk[3]), saturation=_dptr(wk[4]))
        if 'lanes' in given:
            self.idx = lane_list(given['lanes'])
            self.n = B if self.idx is None else len(self.idx)
            m.update(nlanes=self.n, lanes=_lptr(self.idx))

    def rows(self, n):
        """for the libraries whose call without a lane list has as many points as its per-point arrays have rows, not the batch"""
        self.n = self.members['nlanes'] = n

    def check(self, needs, own=()):
        """The size checks in the order every library makes them: `own` [(name, array or None, size)], the wall table, mpb_radius, then
        D, charges and x against the view.  needs: the library's wording, 'the view needs' or 'the call needs'."""
        _, N, nx = self.dims
        for name, a, size in list(own) + self.wall_sizes + [('mpb_radius', self.radius, N)]:
            if a is not None and a.size != size:
                raise ValueError('%s has %d values, %s %d' % (name, a.size, needs, size))
        if self.D.size < N or self.charges.size < N or self.x.size < nx:
            raise ValueError('D, charges or x shorter than the view')
