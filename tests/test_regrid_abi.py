"""libcatint_regrid without a GPU (the method of tests/test_balance_abi.py): it builds for gfx950 and exports what
include/catint_regrid.h declares, the ctypes mirrors have the compiler's layouts, every validation error is returned before any device
call, the kernels compiled into it are exactly the six instances listed here and none of the other three libraries gained one,
pnp_set_lanes_device is declared, bound and exported.  The header's definition is restated here in NumPy (`resample_ref`, which
tests/test_gpu_regrid.py compares the device with) and checked for what makes it the right interpolant: equilibrium profiles are
reproduced exactly, the weights sum to one, nodes are copied bit for bit, and the sub-edges of a nested refinement carry the parent
edge's flux.  The calculator's two opt-in paths are driven with fake solvers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import kernel_census as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {'catgrid_params': 'CatgridParams', 'catgrid_outputs': 'CatgridOutputs'}

# regrid_kernel<waves per operating point, steric>: max(nx, nx_target) <= 1026 / <= 2050 / larger
INSTANCES = {'catgrid::regrid_kernel<%d, %s>' % (WY, s) for WY in (1, 2, 4) for s in ('false', 'true')}

N_A = 6.022140857e23
F, BETA = 96485.33289, 1.0 / (8.3144598 * 298.14)


# ---- the definition of include/catint_regrid.h, restated ---------------------------------------------------------------------------
def bernoulli(u):
    """B(u) = u / (exp(u) - 1), by its series below |u| = 0.05"""
    u = np.asarray(u, float)
    small = np.abs(u) < 0.05
    us = np.where(small, u, 0.0)
    u2 = us * us
    series = 1.0 - 0.5 * us + u2 * (1.0 / 12.0 + u2 * (-1.0 / 720.0 + u2 * (1.0 / 30240.0)))
    ub = np.where(small, 1.0, u)
    with np.errstate(over='ignore'):
        return np.where(small, series, ub / np.expm1(ub))


def cell_table(x, xt):
    """(e, s) of every target point: the largest e <= nx-2 with x[e] <= X, s = (X - x[e]) / h_e; the last node is (nx-1, 0)"""
    x, xt = np.asarray(x, float), np.asarray(xt, float)
    assert xt.min() >= x[0] and xt.max() <= x[-1]
    e = np.minimum(np.searchsorted(x, xt, side='right') - 1, len(x) - 2)
    s = (xt - x[e]) / (x[e + 1] - x[e])
    at_end = xt == x[-1]
    return np.where(at_end, len(x) - 1, e), np.where(at_end, 0.0, s)


def weights(u, s):
    """(G, H) of the definition; all four B evaluated directly, |u| clamped at 500"""
    u = np.clip(u, -500.0, 500.0)
    G = s * bernoulli(-u) / bernoulli(-u * s)
    H = (1.0 - s) * bernoulli(u) / bernoulli(u * (1.0 - s))
    return G, H


def resample_ref(x, c, phi, xt, charges, beta, D, velocity=0.0, radius=None):
    """c [N][nx], phi [nx] on x -> (c [N][nxt], phi [nxt]) on xt"""
    x, c, phi = np.asarray(x, float), np.asarray(c, float), np.asarray(phi, float)
    nx = len(x)
    e, s = cell_table(x, xt)
    f = np.minimum(e + 1, nx - 1)
    h = np.where(e == nx - 1, x[-1] - x[-2], x[f] - x[e])
    w = np.zeros(nx)
    if radius is not None and np.any(radius):
        w = -np.log1p(-(N_A * np.asarray(radius, float)[:, None] ** 3 * c).sum(axis=0))
    dphi = phi[f] - phi[e]
    phit = np.where(s == 0.0, phi[e], phi[e] + s * dphi)
    ct = np.empty((c.shape[0], len(e)))
    for k in range(c.shape[0]):
        u = charges[k] * beta * dphi + (w[f] - w[e]) - velocity * h / D[k]
        G, H = weights(u, s)
        ct[k] = np.where(s == 0.0, c[k][e], H * c[k][e] + G * c[k][f])
    return ct, phit


def nested_targets(x, rng, per_cell=3):
    """Every source node and per_cell random points inside every cell"""
    inner = x[:-1, None] + np.diff(x)[:, None] * np.sort(rng.uniform(0.02, 0.98, (len(x) - 1, per_cell)), axis=1)
    return np.unique(np.concatenate([x, inner.ravel()]))


def steep_potential(rng, nx, vmax=2.5):
    """Nodes of a random walk rescaled to |phi| <= vmax"""
    phi = np.cumsum(rng.standard_normal(nx))
    phi -= 0.5 * (phi.max() + phi.min())
    return phi * (vmax / np.abs(phi).max())


def test_equilibrium_profiles_are_reproduced_exactly():
    """c = c_b exp(-q beta phi) on the nodes of a piecewise linear potential is an exponential inside every cell: the interpolant
    returns c_b exp(-q beta phi_lin(X)) -- where linear interpolation of c would be off by orders of magnitude (|u| >= 20)."""
    rng = np.random.default_rng(11)
    x = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 2.0, 40))]) * 1e-9
    phi = steep_potential(rng, len(x))
    q, cb = np.array([F, -F, 2 * F]), np.array([100.0, 120.0, 10.0])
    assert np.abs(q[:, None] * BETA * np.diff(phi)).max() >= 20.0
    c = cb[:, None] * np.exp(-q[:, None] * BETA * phi)
    xt = nested_targets(x, rng)
    ct, phit = resample_ref(x, c, phi, xt, q, BETA, np.full(3, 1e-9))
    lin = np.interp(xt, x, phi)
    want = cb[:, None] * np.exp(-q[:, None] * BETA * lin)
    err = np.abs(ct / want - 1.0).max()
    print('equilibrium: max relative error %.2e' % err)
    assert err <= 1e-12
    assert np.abs(phit - lin).max() <= 1e-14 * 2.5
    worst = np.abs(np.stack([np.interp(xt, x, row) for row in c]) / want - 1.0).max()
    assert worst > 1e3           # what the host path's np.interp makes of the same profile


def test_weights_sum_to_one_and_are_not_negative():
    rng = np.random.default_rng(12)
    u = np.concatenate([rng.uniform(-25, 25, 4000), rng.uniform(-0.06, 0.06, 500), [-500.0, 500.0, -700.0, 700.0, 0.0, 12.0, -12.0]])
    s = rng.uniform(0.0, 1.0, len(u))
    s[:7] = [0.0, 1.0, 1e-300, 1.0 - 2.0 ** -53, 0.5, 1e-9, 1 - 1e-9]
    G, H = weights(u, s)
    assert np.isfinite(G).all() and np.isfinite(H).all() and (G >= 0).all() and (H >= 0).all()
    print('G + H - 1: %.2e' % np.abs(G + H - 1.0).max())
    assert np.abs(G + H - 1.0).max() <= 1e-14


def test_identity_bit_for_bit():
    """Onto the own grid, and the nodes among the points of a nested refinement: copies"""
    rng = np.random.default_rng(13)
    x = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 2.0, 30))]) * 1e-9
    phi = steep_potential(rng, len(x))
    c = rng.uniform(1e-3, 1e3, (2, len(x)))
    q, D, r = np.array([F, -F]), np.array([1e-9, 2e-9]), np.array([3e-10, 4e-10])
    ct, phit = resample_ref(x, c, phi, x, q, BETA, D, velocity=1e-3, radius=r)
    assert np.array_equal(ct, c) and np.array_equal(phit, phi)
    xt = nested_targets(x, rng)
    ct, phit = resample_ref(x, c, phi, xt, q, BETA, D, velocity=1e-3, radius=r)
    at = np.searchsorted(xt, x)
    assert np.array_equal(ct[:, at], c) and np.array_equal(phit[at], phi)
    assert (ct > 0).all() and (ct <= np.maximum(c[:, :-1], c[:, 1:]).max(axis=1)[:, None]).all()


def test_sub_edges_of_a_nested_refinement_carry_the_parent_edge_s_flux():
    """The Scharfetter-Gummel flux of every sub-edge, formed from the resampled values with the sub-edge's share of u, is the flux of
    the source edge it lies in: a state resampled onto a nested refinement satisfies the fine grid's conservation law in the
    interior of every source cell."""
    rng = np.random.default_rng(14)
    x = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 2.0, 25))]) * 1e-9
    phi = steep_potential(rng, len(x), 1.5)
    c = np.exp(rng.uniform(-3, 3, (2, len(x))))
    q, D, vel = np.array([F, -2 * F]), np.array([1e-9, 2e-9]), 2e-3
    xt = nested_targets(x, rng)
    ct, phit = resample_ref(x, c, phi, xt, q, BETA, D, velocity=vel)
    worst = 0.0
    for k in range(2):
        def flux(xx, cc, pp):
            h = np.diff(xx)
            u = q[k] * BETA * np.diff(pp) - vel * h / D[k]
            a, b = bernoulli(-u) * cc[1:], bernoulli(u) * cc[:-1]
            return -(D[k] / h) * (a - b), (D[k] / h) * (np.abs(a) + np.abs(b))
        Jp, _ = flux(x, c[k], phi)
        Js, scale = flux(xt, ct[k], phit)
        parent = np.minimum(np.searchsorted(x, xt[:-1], side='right') - 1, len(x) - 2)
        worst = max(worst, (np.abs(Js - Jp[parent]) / scale).max())
    print('sub-edge flux against the parent edge: %.2e of the sum of absolute terms' % worst)
    assert worst <= 1e-12


# ---- the library -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_regrid_library
    return build_regrid_library()


@pytest.fixture(scope='module')
def regridder(libpath):
    from catint_amd import _regrid
    with _regrid.Regridder(0) as o:
        yield o


def header_source(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    from catint_amd import _regrid
    declared = sorted(set(re.findall(r'\b(catgrid_[a-z0-9_]+)\s*\(', header_source('catint_regrid.h'))))
    assert declared == sorted(_regrid.SYMBOLS) and len(declared) == 6
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(catgrid_[a-z0-9_]+)\b', exported))) == declared


def test_the_sources_are_not_part_of_the_other_libraries():
    from catint_amd import build
    assert not any('catgrid' in s or 'regrid' in s for s in build.SOURCES + build.OBSERVE_SOURCES + build.BALANCE_SOURCES)
    assert os.path.dirname(build.REGRID_LIB) == os.path.dirname(build.LIB)
    assert build.REGRID_SOURCES == ['catgrid.hip'] and os.path.isdir(build.REGRID_DIR)
    listed = {os.path.realpath(p) for p in build.REGRID_HEADERS}
    for h in ('catint_regrid.h', 'catint_pnp.h'):
        assert os.path.realpath(os.path.join(ROOT, 'include', h)) in listed
    assert os.path.realpath(os.path.join(build.CSRC, 'pnp_post.h')) in listed
    # every file the source reaches through quoted #include lines is a listed dependency (the walk of tests/test_build_deps.py)
    from tests.test_build_deps import reached
    sources = [os.path.join(build.REGRID_DIR, f) for f in build.REGRID_SOURCES]
    assert not reached(sources) - listed - {os.path.realpath(f) for f in sources}


def header_structs():
    out = {}
    for body, struct in re.findall(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', header_source('catint_regrid.h'), flags=re.S):
        fields = []
        for decl in body.split(';'):
            decl = decl.strip()
            if not decl:
                continue
            names = decl.split(None, 1)[1] if not decl.startswith('const') else decl.split(None, 2)[2]
            fields += [n.strip().lstrip('*').strip() for n in names.split(',')]
        out[struct] = fields
    return out


@pytest.fixture(scope='module')
def compiler_layout(tmp_path_factory):
    structs = header_structs()
    assert set(PAIRS) <= set(structs)
    d = tmp_path_factory.mktemp('regrid_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_regrid.h"', 'int main(void) {']
    for s in PAIRS:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (s, s))
        for f in structs[s]:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    for name, macro in (('maxnx', 'CATGRID_MAX_NX'), ('maxspecies', 'CATGRID_MAX_SPECIES'), ('maxu', '(int)CATGRID_MAX_U')):
        lines.append('  printf("%s n %%d\\n", %s);' % (name, macro))
    lines += ['  return 0;', '}']
    (d / 'abi.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(d / 'abi.c'), '-o', str(d / 'abi')])
    layout = {}
    for line in subprocess.check_output([str(d / 'abi')]).decode().splitlines():
        s, f, v = line.split()
        layout.setdefault(s, {})[f] = int(v)
    return layout


@pytest.mark.parametrize('cname', sorted(PAIRS))
def test_ctypes_mirror_matches_the_compiler(cname, compiler_layout):
    from catint_amd import _regrid
    cls = getattr(_regrid, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_of_the_binding_are_the_header_s(compiler_layout):
    from catint_amd import _regrid
    assert _regrid.MAX_NX == compiler_layout['maxnx']['n'] == 4098 and _regrid.MAX_SPECIES == compiler_layout['maxspecies']['n']
    assert _regrid.MAX_U == compiler_layout['maxu']['n'] == 500
    assert [_regrid.row_pitch(n) for n in (3, 16, 17, 130, 4098)] == [16, 16, 32, 144, 4112]


def fake_view(nx=16, N=2, B=2, phi=0x1000, size=None):
    """A view no device stands behind: validation must reject it without reading it."""
    from catint_amd import _regrid
    return _regrid.PnpDeviceView(C.sizeof(_regrid.PnpDeviceView) if size is None else size, 2, N, nx, (nx + 15) // 16 * 16, 0, B, 0x1000, phi,
                                 0x1000, None)


def call(regridder, view, x=None, x_target=None, D=None, charges=None, beta=0.4, **kw):
    from catint_amd import _regrid
    nx, N = max(view.nx, 1), max(view.nspecies, 1)
    x = np.arange(nx) * 1e-9 if x is None else x
    x_target = np.linspace(x[0], x[-1], 9) if x_target is None else x_target
    with pytest.raises(_regrid.RegridError) as e:
        regridder.resample(view, np.full(N, 1e-9) if D is None else D, np.full(N, 96485.0) if charges is None else charges, x, beta,
                           x_target, **kw)
    return e.value


@pytest.mark.parametrize('what, make, word', [
    ('compat handle: no potential row', lambda: (fake_view(phi=None), {}), 'potential'),
    ('nx below 3', lambda: (fake_view(nx=2), {}), 'nx'),
    ('nx above 4098', lambda: (fake_view(nx=4099, B=1), {}), 'nx'),
    ('more than 8 species', lambda: (fake_view(N=9), {}), 'species'),
    ('x not increasing', lambda: (fake_view(), {'x': np.array([0.0, 1.0, 2.0, 2.0] + list(range(3, 15)), float)}), 'increasing'),
    ('struct_size of the parameters', lambda: (fake_view(), {'struct_size': 8}), 'struct_size'),
    ('struct_size of the view', lambda: (fake_view(size=12), {}), 'struct_size'),
    ('a zero diffusion coefficient', lambda: (fake_view(), {'D': np.array([1e-9, 0.0])}), 'D > 0'),
    ('a NaN diffusion coefficient', lambda: (fake_view(), {'D': np.array([1e-9, np.nan])}), 'D > 0'),
    ('an infinite charge', lambda: (fake_view(), {'charges': np.array([np.inf, 1.0])}), 'finite charge'),
    ('a negative radius', lambda: (fake_view(), {'mpb_radius': np.array([3e-10, -3e-10])}), 'radius'),
    ('beta zero', lambda: (fake_view(), {'beta': 0.0}), 'beta'),
    ('velocity infinite', lambda: (fake_view(), {'velocity': np.inf}), 'velocity'),
    ('negative max_waves', lambda: (fake_view(), {'max_waves': -1}), 'max_waves'),
    ('nx_target below 3', lambda: (fake_view(), {'x_target': np.array([0.0, 1e-9])}), 'nx_target'),
    ('nx_target above 4098', lambda: (fake_view(), {'x_target': np.linspace(0.0, 15e-9, 4099)}), 'nx_target'),
    ('x_target not increasing', lambda: (fake_view(), {'x_target': np.array([0.0, 2e-9, 2e-9, 3e-9])}), 'x_target is not strictly increasing'),
    ('x_target decreasing', lambda: (fake_view(), {'x_target': np.array([3e-9, 2e-9, 1e-9])}), 'x_target is not strictly increasing'),
    ('a target point left of the grid', lambda: (fake_view(), {'x_target': np.array([-1e-12, 2e-9, 3e-9])}), 'outside the source grid'),
    ('a target point right of the grid', lambda: (fake_view(), {'x_target': np.array([0.0, 2e-9, 15e-9 * (1 + 1e-15)])}), 'outside the source grid'),
    ('a NaN target point', lambda: (fake_view(), {'x_target': np.array([0.0, np.nan, 3e-9])}), 'x_target'),
    ('a lane index at the batch size', lambda: (fake_view(), {'lanes': [0, 2]}), 'lane index'),
    ('a negative lane index', lambda: (fake_view(), {'lanes': [-1]}), 'lane index'),
])
def test_validation_errors_come_before_any_device_call(regridder, what, make, word):
    from catint_amd import _regrid
    view, kw = make()
    err = call(regridder, view, **kw)
    assert err.code == _regrid.EINVAL, (what, str(err))
    assert word in str(err), (what, str(err))
    assert regridder.last_kernel == '' and regridder.last_kernel_ms == -1.0


def test_null_arguments_and_null_context(regridder, libpath):
    from catint_amd import _regrid
    lib = _regrid.load_library()
    p = _regrid.CatgridParams(struct_size=C.sizeof(_regrid.CatgridParams))
    o = _regrid.CatgridOutputs()
    v = fake_view()
    assert lib.catgrid_resample(regridder._h, None, C.byref(p), C.byref(o)) == _regrid.EINVAL
    assert b'null' in lib.catgrid_last_error(regridder._h)
    assert lib.catgrid_resample(regridder._h, C.byref(v), None, C.byref(o)) == _regrid.EINVAL
    assert lib.catgrid_resample(regridder._h, C.byref(v), C.byref(p), None) == _regrid.EINVAL
    assert lib.catgrid_resample(None, None, C.byref(p), C.byref(o)) == _regrid.EINVAL
    assert lib.catgrid_create(0, None) == _regrid.EINVAL
    assert lib.catgrid_last_kernel(regridder._h) == b''
    # x_target NULL with a valid nx_target
    x, D = np.arange(16) * 1e-9, np.full(2, 1e-9)
    p = _regrid.CatgridParams(C.sizeof(_regrid.CatgridParams), 0, _regrid._dptr(D), _regrid._dptr(D), None, 0.4, 0.0, _regrid._dptr(x), 5, 0,
                              None, 0, None)
    assert lib.catgrid_resample(regridder._h, C.byref(v), C.byref(p), C.byref(o)) == _regrid.EINVAL
    assert b'x_target' in lib.catgrid_last_error(regridder._h)


def test_an_empty_lane_list_makes_no_device_call(regridder):
    """n == 0: valid, and done before the first device call (this machine may have no device at all)."""
    out = regridder.resample(fake_view(), np.full(2, 1e-9), np.full(2, 96485.0), np.arange(16) * 1e-9, 0.4, np.linspace(0, 15e-9, 7), lanes=[])
    assert out['c'].shape == (0, 2, 7) and out['phi'].shape == (0, 7) and regridder.last_kernel == ''


def test_compiled_kernels_are_the_six_instances(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)


def test_the_other_libraries_gained_no_kernel():
    from catint_amd.build import BALANCE_LIB, OBSERVE_LIB, build_balance_library, build_observe_library
    build_observe_library()
    build_balance_library()
    try:
        compiled = K.compiled_kernels() | K.compiled_kernels(lib=OBSERVE_LIB) | K.compiled_kernels(lib=BALANCE_LIB)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert not [n for n in compiled if 'catgrid' in n or 'regrid' in n]


def test_set_lanes_device_is_declared_bound_and_exported():
    from catint_amd import _capi
    from catint_amd.build import build_library
    assert 'pnp_set_lanes_device' in _capi.SYMBOLS
    assert re.search(r'\bint\s+pnp_set_lanes_device\s*\(\s*pnp_handle\s*\*\s*h\s*,\s*int64_t\s+n\s*,\s*const\s+int64_t\s*\*\s*lanes\s*,'
                     r'\s*const\s+double\s*\*\s*c_dev\s*,\s*const\s+double\s*\*\s*phi_dev\s*\)', header_source('catint_pnp.h'))
    exported = subprocess.check_output(['nm', '-D', '--defined-only', build_library()]).decode()
    assert re.search(r'\bpnp_set_lanes_device\b', exported)
    for name in ('set_lanes_device', 'resample', 'resample_to'):
        assert hasattr(_capi.PnpSolver, name), name
    assert not [s for s in _capi.SYMBOLS if 'catgrid' in s or 'regrid' in s]        # no other pnp_* symbol was added for it


# ---- the calculator's opt-in paths, with fake solvers ------------------------------------------------------------------------------
def ladder_parts():
    from tests.test_host_physical import LadderSolver, make_tp

    class DeviceLadderSolver(LadderSolver):
        """LadderSolver with the device path: resample_to records the call and hands its state over as set_lanes_device would"""

        def __init__(self, *a, **kw):
            grid = kw.pop('grid')
            LadderSolver.__init__(self, *a, **kw)
            self.grid = np.asarray(grid, float)

        def resample_to(self, other, lanes=None, dst_lanes=None):
            lanes = np.arange(self.B) if lanes is None else np.asarray(lanes)
            dst = np.arange(len(lanes)) if dst_lanes is None else np.asarray(dst_lanes)
            self.calls.append(('resample_to', list(lanes), list(dst)))
            other.calls.append(('set_lanes_device', list(dst)))
            other.c[dst] = self.c[lanes][:, :, :1]           # (a recognisable state; the grids differ)
            other.phi[dst] = self.phi[lanes][:, :1]

        def newton_iterations(self):
            return np.full(self.B, 3, np.int32)
    return DeviceLadderSolver, make_tp


@pytest.mark.parametrize('on_device', [False, True])
def test_the_mesh_rung_hands_over_on_the_device_only_when_opted_in(monkeypatch, on_device):
    """tp.newton['regrid_on_device']: the mesh rung calls resample_to exactly for the recovered lanes, and neither get_state nor
    set_lanes; without the option it is get_state + set_lanes as before.  The confirming solve is the main handle's either way."""
    from catint_amd.calculator import Calculator
    Solver, make_tp = ladder_parts()
    phis = np.linspace(-0.5, -2.0, 4)
    tp = make_tp(phis)
    tp.set_graded_mesh(tp.xmesh[1] / 50.0)
    tp.newton = {'retry_rungs': 1, 'retry_mesh_rungs': 1, 'dphi_stage': 0.2}
    if on_device:
        tp.newton['regrid_on_device'] = True
    calc = Calculator(transport=tp, calc='comsol')
    main = Solver(4, tp.nx, 3, stuck=[0, 2, 3], grid=tp.xmesh)
    subs = []

    def fake_sub(B, xmesh=None, **kw):
        # the ramp rung recovers nothing; on the refined mesh the first two of the three failed lanes converge
        s = Solver(B, tp.nx, 3, stuck=[0, 1, 2] if xmesh is None else [2], grid=tp.xmesh if xmesh is None else xmesh)
        s.get_state_calls = 0
        get_state = s.get_state
        def counted():
            s.get_state_calls += 1
            return get_state()
        s.get_state = counted
        subs.append(s)
        return s
    monkeypatch.setattr(calc, '_physical_solver', fake_sub)
    st = calc.solve_physical(main, np.ones((4, 3 * tp.nx)), phis, np.zeros((4, 3)))
    assert [r['mesh_refined'] for r in calc.retry_log] == [False, True] and calc.retry_log[1]['recovered'] == [0, 2]
    assert list(st) == [0, 0, 0, 1]
    mesh_sub = subs[1]
    if on_device:
        assert [c for c in mesh_sub.calls if c[0] == 'resample_to'] == [('resample_to', [0, 1], [0, 2])]
        assert mesh_sub.get_state_calls == 0 and not [c for c in main.calls if c[0] == 'set_lanes']
        assert [c for c in main.calls if c[0] == 'set_lanes_device'] == [('set_lanes_device', [0, 2])]
    else:
        assert not [c for c in mesh_sub.calls if c[0] == 'resample_to'] and mesh_sub.get_state_calls == 1
        assert [c[1] for c in main.calls if c[0] == 'set_lanes'] == [[0, 2]]
        assert not [c for c in main.calls if c[0] == 'set_lanes_device']
    assert [c[1] for c in main.calls if c[0] == 'mask'] == [[0, 2], None]
    # the ramp rung's sub-batch never takes the device path: it shares the batch's mesh
    assert not [c for c in subs[0].calls if c[0] == 'resample_to']


def test_mesh_continuation_with_fakes(monkeypatch):
    """tp.newton['coarse_nx']: the usual path runs on a coarse handle, its converged lanes are resampled onto the main handle, one direct
    solve there decides; a lane that fails it goes through the usual continuation as rung 0 of the ladder."""
    from catint_amd.calculator import Calculator
    Solver, make_tp = ladder_parts()
    phis = np.linspace(-0.5, -2.0, 3)
    tp = make_tp(phis)
    tp.set_graded_mesh(tp.xmesh[1] / 50.0)
    tp.newton = {'coarse_nx': 20, 'retry_rungs': 1, 'retry_mesh_rungs': 0, 'dphi_stage': 0.2}
    calc = Calculator(transport=tp, calc='comsol')
    main = Solver(3, tp.nx, 3, stuck=[1], need=2, grid=tp.xmesh)       # lane 1 fails the one direct solve
    subs = []

    def fake_sub(B, xmesh=None, **kw):
        s = Solver(B, tp.nx if xmesh is None else len(xmesh), 3, grid=tp.xmesh if xmesh is None else xmesh)
        subs.append(s)
        return s
    monkeypatch.setattr(calc, '_physical_solver', fake_sub)
    st = calc.solve_physical(main, np.ones((3, 3 * tp.nx)), phis, np.zeros((3, 3)))
    coarse = subs[0]
    assert coarse.nx == 20 and coarse.grid[0] == tp.xmesh[0] and coarse.grid[-1] == tp.xmesh[-1]
    assert np.isclose(coarse.grid[1] - coarse.grid[0], tp.xmesh[1] - tp.xmesh[0])
    assert [c for c in coarse.calls if c[0] == 'resample_to'] == [('resample_to', [0, 1, 2], [0, 1, 2])]
    assert len([c for c in coarse.calls if c[0] == 'solve']) == calc.continuation_stages == 11      # the usual path, on the coarse grid
    # the main handle: set_batch, the hand-over, ONE solve; then rung 0 patches the lane that failed
    kinds = [c[0] for c in main.calls]
    assert kinds[:3] == ['set_batch', 'set_lanes_device', 'solve']
    assert calc.mesh_continuation == {'coarse_nx': 20, 'coarse_failed': 0, 'failed': 1}
    assert [(r['rung'], r['stages'], r['lanes'], r['recovered']) for r in calc.retry_log] == [(0, 11, [1], [1])]
    assert len(subs) == 2 and subs[1].nx == tp.nx
    assert list(st) == [0, 0, 0]
    # without the option nothing of this happens
    tp.newton = {'retry_rungs': 1, 'retry_mesh_rungs': 0, 'dphi_stage': 0.2}
    main2 = Solver(3, tp.nx, 3, grid=tp.xmesh)
    del subs[:]
    calc.solve_physical(main2, np.ones((3, 3 * tp.nx)), phis, np.zeros((3, 3)))
    assert not subs and not [c for c in main2.calls if c[0] == 'set_lanes_device']
