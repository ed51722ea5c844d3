"""CPU: what the Python bindings hand to the libraries, member by member, and PnpSolver's table of library objects.

The libraries that take the medium (response, couple, sens, modes, balance, cateis_solve) build their parameter struct from
catint_amd._medium.Medium by member name.  Here Handle.__init__ and Handle._call are replaced by a recorder, every one of them is
called once with a lane list and once without, and each member of the medium part of the recorded struct is compared with the input it
must carry.  All scalars are pairwise distinct and the arrays have distinct lengths where the structs allow it (mpb_radius must have N
entries, alpha and saturation n_wall each: those differ in their values), so two members that changed places cannot pass."""
import ctypes as C
import glob
import importlib
import inspect
import os
import re
import sys

import numpy as np
import pytest

from catint_amd import _capi, _devlib

B, N, NX = 4, 3, 7
D = np.array([1.1e-9, 1.2e-9, 1.3e-9, 1.4e-9])                     # N + 1 values
CHARGES = np.array([1.0, -1.0, 2.0, -2.0, 3.0]) * 96485.0          # N + 2
X = np.cumsum(np.linspace(1.0, 2.0, NX + 2)) * 1e-10                # nx + 2, not uniform
RADII = np.array([3e-10, 4e-10, 5e-10])
SCALARS = dict(beta=0.0404, eps=6.9e-10, dx=1.25e-9, velocity=-2e-3, stern_capacitance=0.21)
MAX_WAVES = 3
REACTIONS = [([0, 1], [2], 1e2, 1.2e5), ([], [0, 0, 1], 2e5, 0.0), ([2], [1], 5.0, 7.0)]
WALL = {'species': [1, -1], 'nu': [[0.0, -1.0, 0.5], [1.0, 0.0, -2.0]], 'k': np.arange(1.0, 1.0 + B * 2).reshape(B, 2) * 1e-6,
        'alpha': [-5.8, 3.9], 'saturation': [0.002, 0.05]}
LANES = [3, 0, 3, 1, 2]
PHIM = np.linspace(-0.3, -0.1, B)


def view():
    return _devlib.PnpDeviceView(struct_size=C.sizeof(_devlib.PnpDeviceView), nspecies=N, nx=NX, row_pitch=16, batch=B)


@pytest.fixture
def recorded(monkeypatch):
    """Handle without a library: the constructor opens nothing, _call keeps (entry, params, outputs) and, so that the arrays the
    pointers mean outlive the call, the local variables of the two frames above it (solve, and cateis_solve's caller of _run)"""
    calls = []

    def call(self, entry, view, params, outputs):
        frame = sys._getframe(1)
        calls.append((entry, params, outputs, dict(frame.f_locals), dict(frame.f_back.f_locals)))
    monkeypatch.setattr(_devlib.Handle, '__init__', lambda self, device=0: setattr(self, '_h', C.c_void_p()))
    monkeypatch.setattr(_devlib.Handle, '_call', call)
    return calls


def tables():
    """a two-adsorbate chain over the N species (the kinetic half of cateis_solve)"""
    of, ob = np.zeros((2, N + 3), np.int32), np.zeros((2, N + 3), np.int32)
    of[0, 0], of[0, N], ob[0, N + 1], of[1, N + 1], ob[1, N + 2] = 1, 1, 1, 1, 1
    return {'order_f': of, 'order_b': ob, 'nu': np.zeros((2, N)), 'cref': np.full(N, 40.0), 'site_count': np.ones(3),
            'dG': np.zeros((2, 4)), 'Ea': np.zeros((2, 4)), 'lnA': np.zeros(2), 'site_density': 1e-6}


def _response(lanes):
    from catint_amd import _response as M
    M.Responder().solve(view(), D, CHARGES, X, SCALARS['beta'], SCALARS['eps'], SCALARS['dx'], PHIM, lanes=lanes, mpb_radius=RADII,
                        wall_bc='stern', stern_capacitance=SCALARS['stern_capacitance'], velocity=SCALARS['velocity'], reactions=REACTIONS,
                        wall=WALL, max_waves=MAX_WAVES)
    return B if lanes is None else len(lanes)


def _couple(lanes):
    from catint_amd import _couple as M
    n = B + 2 if lanes is None else len(lanes)          # (without a lane list the rows of flux count)
    M.Coupler().solve(view(), D, CHARGES, X, SCALARS['beta'], SCALARS['eps'], SCALARS['dx'], np.zeros((n, N)), np.zeros((n, N)),
                      np.zeros((n, N, N)), np.zeros((n, N)), lanes=lanes, mpb_radius=RADII, wall_bc='stern',
                      stern_capacitance=SCALARS['stern_capacitance'], velocity=SCALARS['velocity'], reactions=REACTIONS, max_waves=MAX_WAVES)
    return n


def _sens(lanes):
    from catint_amd import _sens as M
    n = B + 2 if lanes is None else len(lanes)
    M.Sensitizer().solve(view(), D, CHARGES, X, SCALARS['beta'], SCALARS['eps'], SCALARS['dx'], PHIM, np.zeros((n, N)), ['phiM'], lanes=lanes,
                         mpb_radius=RADII, wall_bc='stern', stern_capacitance=SCALARS['stern_capacitance'], velocity=SCALARS['velocity'],
                         reactions=REACTIONS, wall=WALL, max_waves=MAX_WAVES)
    return n


def _modes(lanes):
    from catint_amd import _modes as M
    M.ModeSolver().solve(view(), D, CHARGES, X, SCALARS['beta'], SCALARS['eps'], SCALARS['dx'], PHIM, np.zeros((2, N + 1, NX)), lanes=lanes,
                         mpb_radius=RADII, wall_bc='stern', stern_capacitance=SCALARS['stern_capacitance'], velocity=SCALARS['velocity'],
                         reactions=REACTIONS, wall=WALL, max_waves=MAX_WAVES)
    return B if lanes is None else len(lanes)


def _balance(lanes):
    from catint_amd import _balance as M
    M.Balancer().species(view(), D, CHARGES, X, SCALARS['beta'], np.zeros((B, N)), PHIM, mpb_radius=RADII, velocity=SCALARS['velocity'],
                         reactions=REACTIONS, wall=WALL, max_waves=MAX_WAVES)
    return None          # (catbal_params has no lane list)


def _eis(lanes):
    from catint_amd import _eis as M
    n = B if lanes is None else len(lanes)
    M.Impedance().solve(view(), tables(), np.linspace(-0.3, -0.1, n), np.full((n, 3), 1.0 / 3.0), [0.0, 1e3], D, CHARGES, X, SCALARS['beta'],
                        SCALARS['eps'], SCALARS['dx'], rf=0.9, lanes=lanes, mpb_radius=RADII, wall_bc='stern',
                        stern_capacitance=SCALARS['stern_capacitance'], velocity=SCALARS['velocity'], reactions=REACTIONS, max_waves=MAX_WAVES)
    return n


#            call, the struct's name of the wall species (None: no wall table), of the number of points
LIBRARIES = {'response': (_response, 'wall_species', 'nlanes'), 'couple': (_couple, None, 'nlanes'), 'sens': (_sens, 'wall_species', 'nlanes'),
             'modes': (_modes, 'wall_species', 'nlanes'), 'balance': (_balance, 'species', None), 'eis': (_eis, None, 'n')}


def pointee(ptr, like):
    like = np.asarray(like)
    return np.ctypeslib.as_array(ptr, shape=(like.size,)).reshape(like.shape)


@pytest.mark.parametrize('lanes', [None, LANES], ids=['all', 'lanes'])
@pytest.mark.parametrize('library', list(LIBRARIES))
def test_medium_members_carry_their_inputs(library, lanes, recorded):
    call, wall_species, count = LIBRARIES[library]
    n = call(lanes)
    assert len(recorded) == 1
    p = recorded[0][1]
    members = {name for name, _ in p._fields_}
    for name, a in (('D', D), ('charges', CHARGES), ('x', X), ('mpb_radius', RADII)):
        assert np.array_equal(pointee(getattr(p, name), a), a), name
    for name, v in SCALARS.items():
        if name in members:
            assert getattr(p, name) == v, name
    assert {'beta', 'velocity'} <= members and (library == 'balance' or {'eps', 'dx', 'stern_capacitance', 'wall_bc'} <= members)
    assert p.max_waves == MAX_WAVES and p.struct_size == C.sizeof(type(p))
    if 'wall_bc' in members:
        assert p.wall_bc == 1
    R, n_lhs, lhs, n_rhs, rhs, kf, kr = _capi.flatten_reactions(REACTIONS)
    assert p.nreactions == R == 3
    for name, a in (('n_lhs', n_lhs), ('lhs', lhs), ('n_rhs', n_rhs), ('rhs', rhs), ('kf', kf), ('kr', kr)):
        assert np.array_equal(pointee(getattr(p, name), a), a), name
    if wall_species is not None:
        assert p.n_wall == 2
        for name, key, dtype in ((wall_species, 'species', np.int32), ('nu', 'nu', float), ('k', 'k', float), ('alpha', 'alpha', float),
                                 ('saturation', 'saturation', float)):
            a = np.asarray(WALL[key], dtype)
            assert np.array_equal(pointee(getattr(p, name), a), a), name
    else:
        assert not {'n_wall', 'wall_species', 'alpha', 'saturation'} & members
    if count is not None:
        assert getattr(p, count) == n
        assert bool(p.lanes) == (lanes is not None)
        if lanes is not None:
            assert np.array_equal(pointee(p.lanes, np.asarray(lanes, np.int64)), lanes)
    else:
        assert 'lanes' not in members


def test_no_parameter_struct_is_built_by_position():
    here = os.path.dirname(os.path.abspath(_capi.__file__))
    found = []
    for path in sorted(glob.glob(os.path.join(here, '_*.py'))):
        with open(path) as f:
            for i, line in enumerate(f, 1):
                if not line.startswith('class ') and re.search(r'Cat\w+Params\((?!\s*(\w+\s*=[^=]|\*\*|\)))', line):
                    found.append('%s:%d' % (os.path.basename(path), i))
    assert not found, found


# -- PnpSolver.SATELLITES ---------------------------------------------------------------------------------------------------------------
CALCULATORS_OWN = {'RampedKinetics', 'ScfKinetics'}          # library objects the Calculator holds, not PnpSolver


def test_every_library_object_is_in_the_table():
    here = os.path.dirname(os.path.abspath(_capi.__file__))
    classes = set()
    for path in glob.glob(os.path.join(here, '_*.py')):
        module = importlib.import_module('catint_amd.' + os.path.basename(path)[:-3])
        classes |= {(module.__name__.rsplit('.', 1)[1], name) for name, cls in inspect.getmembers(module, inspect.isclass)
                    if issubclass(cls, _devlib.Handle) and cls is not _devlib.Handle and cls.__module__ == module.__name__}
    table = _capi.PnpSolver.SATELLITES
    assert len(table) == 13 and len(set(table.values())) == 13
    assert {c for c in classes if c[1] not in CALCULATORS_OWN} == set(table.values())
    assert CALCULATORS_OWN <= {c[1] for c in classes}


def test_close_walks_the_table():
    class Fake(object):
        closed = 0

        def close(self):
            self.closed += 1
    s = object.__new__(_capi.PnpSolver)          # (no pnp_handle: close() must take an object whose constructor did not finish)
    fakes = {attr: Fake() for attr in _capi.PnpSolver.SATELLITES}
    for attr, fake in fakes.items():
        setattr(s, attr, fake)
    s.close()
    assert all(f.closed == 1 for f in fakes.values()) and all(getattr(s, attr) is None for attr in fakes)
    s.close()
    assert all(f.closed == 1 for f in fakes.values())
    object.__new__(_capi.PnpSolver).close()          # ... and one that has none of the attributes yet
