"""libcatint_equil without a GPU (the method of tests/test_regrid_abi.py).  The NumPy restatement of include/catint_equil.h
(tests/pb_ref.py, which tests/test_gpu_equil.py compares the device with) is checked against the oracle of the physical mode: its result
is a root of the oracle's stationary zero-flux residual, and the oracle's Newton iteration started from it returns at once.  The library
builds for gfx950 and exports what the header declares, the ctypes mirrors have the compiler's layouts, every validation error is
returned before any device call, the kernels compiled into it are exactly the fourteen instances listed here and none of the other four
libraries gained one.  The calculator's opt-in path is driven with fake solvers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pnp_physical as PH
from tests import kernel_census as K
from tests import pb_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {'cateq_params': 'CateqParams', 'cateq_outputs': 'CateqOutputs'}

# pb_kernel<points per lane, waves per operating point, steric>: the shapes of pnp::post::choose_shape
SHAPES = [(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (16, 2), (16, 4)]
INSTANCES = {'cateq::pb_kernel<%d, %d, %s>' % (P, WY, s) for P, WY in SHAPES for s in ('false', 'true')}

F, BETA, EPS = 96485.33289, 1.0 / (8.3144598 * 298.14), 78.36 * 8.854187817e-12
Q = np.array([1.0, -1.0, -2.0]) * F
CB = np.array([120.0, 100.0, 10.0])
DIFF = np.array([1.957e-9, 1.185e-9, 0.923e-9])
RADII = np.array([4e-10, 3e-10, 3.5e-10])


def graded():
    from catint_amd.host import graded_mesh
    return graded_mesh(80e-9, 0.05e-9, 130)


# (name, grid, phiM, Stern capacitance or None, radii or None): the three cases of the design note and one on a uniform grid.  The
# steric cases stay at a Stern wall: the oracle forms 1 - phi0 by subtraction and loses it where the ions saturate
CASES = [('point ions, Dirichlet wall, +0.3 V', graded, 0.3, None, None),
         ('point ions, Stern wall, -0.8 V', graded, -0.8, 0.2, None),
         ('steric ions, Stern wall, -1.0 V', graded, -1.0, 0.2, RADII),
         ('steric ions, Stern wall, uniform grid, +0.6 V', lambda: np.linspace(0.0, 20e-9, 97), 0.6, 0.2, RADII)]


def row_scales(p, c, phi):
    """Sum of the absolute terms of every row of the oracle's stationary residual (zero wall flux, no reactions): [(N+1), nx]"""
    N, nx = c.shape
    S = np.zeros((N + 1, nx))
    w, _ = PH._steric(p, c)
    for k in range(N):
        u = p.q[k] * p.beta * np.diff(phi) + np.diff(w)
        Bp, _ = PH.bernoulli(u)
        T = p.w * (np.abs((Bp + u) * c[k, 1:]) + np.abs(Bp * c[k, :-1]))
        S[k, 1:-1] = T[1:] + T[:-1]
        S[k, 0] = T[0]
        S[k, -1] = abs(c[k, -1]) + abs(p.c_bulk[k])
    pe = p.dx * p.dx / p.eps
    S[N, 1:-1] = np.abs(p.w[1:] * (phi[2:] - phi[1:-1])) + np.abs(p.w[:-1] * (phi[1:-1] - phi[:-2])) + pe * p.v[1:-1] * (np.abs(p.q)[:, None] * c).sum(axis=0)[1:-1]
    if p.CS is None:
        S[N, 0] = abs(phi[0]) + abs(p.phiM)
    else:
        S[N, 0] = abs(p.w[0] * (phi[1] - phi[0])) + (p.dx * p.CS / p.eps) * (abs(p.phiM - p.phi_pzc) + abs(phi[0]))
    S[N, -1] = abs(phi[-1]) + abs(p.phi_bulk)
    return S


@pytest.mark.parametrize('name, grid, phiM, CS, radii', CASES, ids=[c[0] for c in CASES])
def test_the_restatement_is_a_root_of_the_oracle_s_zero_flux_system(name, grid, phiM, CS, radii):
    x = grid()
    nx, dx = len(x), float(x[1] - x[0])
    c, phi, status, its = pb_ref.solve(x, dx, Q, BETA, EPS, CB, phiM, 0.0, radii, CS)
    assert status == 0 and 2 <= its <= 40
    p = PH.PhysicalProblem(D=DIFF, charges=Q, beta=BETA, eps=EPS, dx=dx, nx=nx, c_bulk=CB, phiM=phiM, stern_capacitance=CS, mpb_radius=radii, x=x)
    R = PH.residual(p, c, phi, c, np.inf)
    S = row_scales(p, c, phi)
    worst = (np.abs(R) / np.where(S > 0, S, 1.0)).max()
    assert (np.abs(R) <= 1e-9 * S).all(), worst
    c2, phi2, it2, hist = PH.newton_step(p, c, phi, c, np.inf, tol=1e-10)
    moved = max(np.abs(c2 - c).max() / np.abs(c).max(), np.abs(phi2 - phi).max() / np.abs(phi).max())
    print('%s: %d PB iterations, residual %.1e of the row scale, oracle: %d iteration, update %.1e, moved %.1e' % (name, its, worst, it2, hist[-1], moved))
    assert it2 == 1 and moved < 1e-12
    # and the double layer is there: the counter-ion is enriched at the wall, the wall potential is off the bulk value
    assert abs(phi[0]) > 0.05 and c[0 if phi[0] < 0 else 1, 0] > 5.0 * CB[0 if phi[0] < 0 else 1]


def test_saturation_stays_finite_in_the_restatement():
    """+1 V at a Dirichlet wall with divalent anions: the ions fill the volume at the wall (phi0 = S / (1 + S) rounds to 1, where the
    oracle's 1 - phi0 is lost); 1 / (1 + S) is formed without the subtraction and everything stays finite"""
    x = graded()
    c, phi, status, its = pb_ref.solve(x, float(x[1] - x[0]), Q, BETA, EPS, CB, 1.0, 0.0, RADII, None)
    assert status == 0 and np.isfinite(c).all() and (c >= 0).all()
    phi0 = (pb_ref.N_AVOGADRO * RADII[:, None] ** 3 * c).sum(axis=0)
    assert 0.99 < phi0[0] <= 1.0 + 1e-15 and phi[0] == 1.0 and abs(phi0[-1] - (pb_ref.N_AVOGADRO * RADII ** 3 * CB).sum()) < 1e-15


def test_iteration_limit_of_the_restatement():
    x = graded()
    c, phi, status, its = pb_ref.solve(x, float(x[1] - x[0]), Q, BETA, EPS, CB, -1.0, 0.0, None, 0.2, maxit=2)
    assert status == 1 and its == 2 and np.isfinite(c).all()


# ---- the library -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_equil_library
    return build_equil_library()


@pytest.fixture(scope='module')
def equilibrator(libpath):
    from catint_amd import _equil
    with _equil.Equilibrator(0) as o:
        yield o


def header_source(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    from catint_amd import _equil
    declared = sorted(set(re.findall(r'\b(cateq_[a-z0-9_]+)\s*\(', header_source('catint_equil.h'))))
    assert declared == sorted(_equil.SYMBOLS) and len(declared) == 6
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(cateq_[a-z0-9_]+)\b', exported))) == declared


def test_the_sources_are_not_part_of_the_other_libraries():
    from catint_amd import build
    others = build.SOURCES + build.OBSERVE_SOURCES + build.BALANCE_SOURCES + build.REGRID_SOURCES
    assert not any('cateq' in s or 'equil' in s for s in others)
    assert os.path.dirname(build.EQUIL_LIB) == os.path.dirname(build.LIB)
    assert build.EQUIL_SOURCES == ['cateq.hip'] and os.path.isdir(build.EQUIL_DIR)
    listed = {os.path.realpath(p) for p in build.EQUIL_HEADERS}
    for h in ('catint_equil.h', 'catint_pnp.h'):
        assert os.path.realpath(os.path.join(ROOT, 'include', h)) in listed
    assert os.path.realpath(os.path.join(build.CSRC, 'pnp_post.h')) in listed
    from tests.test_build_deps import reached
    sources = [os.path.join(build.EQUIL_DIR, f) for f in build.EQUIL_SOURCES]
    assert not reached(sources) - listed - {os.path.realpath(f) for f in sources}
    # build() of the driver entry point builds it
    assert 'build_equil_library(' in open(os.path.join(ROOT, '__graft_entry__.py')).read()


def header_structs():
    out = {}
    for body, struct in re.findall(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', header_source('catint_equil.h'), flags=re.S):
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
    d = tmp_path_factory.mktemp('equil_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_equil.h"', 'int main(void) {']
    for s in PAIRS:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (s, s))
        for f in structs[s]:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    for name, macro in (('maxnx', 'CATEQ_MAX_NX'), ('maxspecies', 'CATEQ_MAX_SPECIES'), ('maxexp', '(int)CATEQ_MAX_EXPONENT'),
                        ('maxit', 'CATEQ_MAX_ITERATIONS'), ('dirichlet', 'CATEQ_WALL_DIRICHLET'), ('stern', 'CATEQ_WALL_STERN')):
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
    from catint_amd import _equil
    cls = getattr(_equil, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_of_the_binding_are_the_header_s(compiler_layout):
    from catint_amd import _equil
    assert _equil.MAX_NX == compiler_layout['maxnx']['n'] == 4098 and _equil.MAX_SPECIES == compiler_layout['maxspecies']['n']
    assert _equil.MAX_EXPONENT == compiler_layout['maxexp']['n'] == pb_ref.MAX_EXPONENT
    assert _equil.MAX_ITERATIONS == compiler_layout['maxit']['n'] == 1000
    assert _equil.WALL == {'dirichlet': compiler_layout['dirichlet']['n'], 'stern': compiler_layout['stern']['n']}


def fake_view(nx=16, N=2, B=2, phi=0x1000, size=None):
    """A view no device stands behind: validation must reject it without reading it."""
    from catint_amd import _equil
    return _equil.PnpDeviceView(C.sizeof(_equil.PnpDeviceView) if size is None else size, 2, N, nx, (nx + 15) // 16 * 16, 0, B, 0x1000, phi,
                                0x1000, None)


def good_args(view):
    nx, N = max(view.nx, 1), max(view.nspecies, 1)
    return dict(charges=np.where(np.arange(N) % 2, -F, F), x=np.arange(nx) * 1e-9, beta=0.4, eps=EPS, dx=1e-9, phiM=np.array([0.1, -0.1]),
                phi_bulk=np.zeros(2), c_bulk=np.full((2, N), 10.0))


def call(equilibrator, view, **kw):
    from catint_amd import _equil
    args = good_args(view)
    args.update(kw)
    with pytest.raises(_equil.EquilError) as e:
        equilibrator.solve(view, **args)
    return e.value


@pytest.mark.parametrize('what, make, word', [
    ('compat handle: no potential row', lambda: (fake_view(phi=None), {}), 'potential'),
    ('nx below 3', lambda: (fake_view(nx=2), {}), 'nx'),
    ('nx above 4098', lambda: (fake_view(nx=4099, B=1), {}), 'nx'),
    ('more than 8 species', lambda: (fake_view(N=9), {}), 'species'),
    ('x not increasing', lambda: (fake_view(), {'x': np.array([0.0, 1.0, 2.0, 2.0] + list(range(3, 15)), float)}), 'increasing'),
    ('struct_size of the parameters', lambda: (fake_view(), {'struct_size': 8}), 'cateq_params.struct_size'),
    ('struct_size of the view', lambda: (fake_view(size=12), {}), 'struct_size'),
    ('an infinite charge', lambda: (fake_view(), {'charges': np.array([np.inf, 1.0])}), 'finite charge'),
    ('a negative radius', lambda: (fake_view(), {'mpb_radius': np.array([3e-10, -3e-10])}), 'radius'),
    ('a NaN radius', lambda: (fake_view(), {'mpb_radius': np.array([3e-10, np.nan])}), 'radius'),
    ('beta zero', lambda: (fake_view(), {'beta': 0.0}), 'beta'),
    ('eps zero', lambda: (fake_view(), {'eps': 0.0}), 'eps'),
    ('eps infinite', lambda: (fake_view(), {'eps': np.inf}), 'eps'),
    ('dx negative', lambda: (fake_view(), {'dx': -1e-9}), 'dx'),
    ('dx NaN', lambda: (fake_view(), {'dx': np.nan}), 'dx'),
    ('tol zero', lambda: (fake_view(), {'tol': 0.0}), 'tol'),
    ('tol NaN', lambda: (fake_view(), {'tol': np.nan}), 'tol'),
    ('maxit zero', lambda: (fake_view(), {'maxit': 0}), 'maxit'),
    ('negative max_waves', lambda: (fake_view(), {'max_waves': -1}), 'max_waves'),
    ('an unknown wall', lambda: (fake_view(), {'wall_bc': 2}), 'wall_bc'),
    ('a Stern wall without a capacitance', lambda: (fake_view(), {'wall_bc': 'stern', 'stern_capacitance': 0.0}), 'Stern'),
    ('a Stern wall with a negative capacitance', lambda: (fake_view(), {'wall_bc': 'stern', 'stern_capacitance': -0.2}), 'Stern'),
    ('a Stern wall with a NaN phi_pzc', lambda: (fake_view(), {'wall_bc': 'stern', 'stern_capacitance': 0.2, 'phi_pzc': np.nan}), 'Stern'),
    ('a negative c_bulk', lambda: (fake_view(), {'c_bulk': np.array([[10.0, 10.0], [10.0, -1.0]])}), 'operating point 1'),
    ('a NaN c_bulk', lambda: (fake_view(), {'c_bulk': np.array([[np.nan, 10.0], [10.0, 1.0]])}), 'operating point 0'),
    ('an infinite phiM', lambda: (fake_view(), {'phiM': np.array([0.1, np.inf])}), 'operating point 1'),
    ('a NaN phi_bulk', lambda: (fake_view(), {'phi_bulk': np.array([np.nan, 0.0])}), 'operating point 0'),
    ('ions that fill the bulk', lambda: (fake_view(), {'mpb_radius': np.array([4e-10, 4e-10]), 'c_bulk': np.full((2, 2), 1.3e4)}), 'volume fraction'),
])
def test_validation_errors_come_before_any_device_call(equilibrator, what, make, word):
    from catint_amd import _equil
    view, kw = make()
    err = call(equilibrator, view, **kw)
    assert err.code == _equil.EINVAL, (what, str(err))
    assert word in str(err), (what, str(err))
    assert equilibrator.last_kernel == '' and equilibrator.last_kernel_ms == -1.0


def test_null_arguments_and_null_context(equilibrator, libpath):
    from catint_amd import _equil
    lib = _equil.load_library()
    p = _equil.CateqParams(struct_size=C.sizeof(_equil.CateqParams))
    o = _equil.CateqOutputs()
    v = fake_view()
    assert lib.cateq_solve(equilibrator._h, None, C.byref(p), C.byref(o)) == _equil.EINVAL
    assert b'null' in lib.cateq_last_error(equilibrator._h)
    assert lib.cateq_solve(equilibrator._h, C.byref(v), None, C.byref(o)) == _equil.EINVAL
    assert lib.cateq_solve(equilibrator._h, C.byref(v), C.byref(p), None) == _equil.EINVAL
    assert lib.cateq_solve(None, None, C.byref(p), C.byref(o)) == _equil.EINVAL
    assert lib.cateq_create(0, None) == _equil.EINVAL
    assert lib.cateq_last_kernel(equilibrator._h) == b''
    # charges and x NULL
    assert lib.cateq_solve(equilibrator._h, C.byref(v), C.byref(p), C.byref(o)) == _equil.EINVAL
    assert b'charges and x' in lib.cateq_last_error(equilibrator._h)
    # operating points without their parameters
    a = good_args(v)
    p = _equil.CateqParams(C.sizeof(_equil.CateqParams), 0, _equil._dptr(a['charges']), None, _equil._dptr(a['x']), 0.4, EPS, 1e-9, 0, 100, 0.0,
                           0.0, 1e-10, None, None, None, 2)
    assert lib.cateq_solve(equilibrator._h, C.byref(v), C.byref(p), C.byref(o)) == _equil.EINVAL
    assert b'phiM' in lib.cateq_last_error(equilibrator._h)
    p.nlanes = -1
    assert lib.cateq_solve(equilibrator._h, C.byref(v), C.byref(p), C.byref(o)) == _equil.EINVAL
    assert b'nlanes' in lib.cateq_last_error(equilibrator._h)


def test_an_empty_lane_list_makes_no_device_call(equilibrator):
    """n == 0: valid, and done before the first device call (this machine may have no device at all)."""
    v = fake_view()
    a = good_args(v)
    a.update(phiM=np.zeros(0), phi_bulk=np.zeros(0), c_bulk=np.zeros((0, 2)))
    out = equilibrator.solve(v, **a)
    assert out['c'].shape == (0, 2, 16) and out['phi'].shape == (0, 16) and out['status'].shape == (0,) and equilibrator.last_kernel == ''


def test_compiled_kernels_are_the_fourteen_instances(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert len(INSTANCES) == 14
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)


def test_the_other_libraries_gained_no_kernel():
    from catint_amd.build import (BALANCE_LIB, OBSERVE_LIB, REGRID_LIB, build_balance_library, build_library, build_observe_library,
                                  build_regrid_library)
    build_library()
    build_observe_library()
    build_balance_library()
    build_regrid_library()
    try:
        compiled = K.compiled_kernels() | K.compiled_kernels(lib=OBSERVE_LIB) | K.compiled_kernels(lib=BALANCE_LIB) | K.compiled_kernels(lib=REGRID_LIB)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert not [n for n in compiled if 'cateq' in n or 'pb_kernel' in n]
    from catint_amd import _capi
    assert not [s for s in _capi.SYMBOLS if 'cateq' in s or 'equil' in s]        # no pnp_* symbol was added for it
    for name in ('equilibrium', 'set_equilibrium'):
        assert hasattr(_capi.PnpSolver, name), name


# ---- the calculator's opt-in path, with fake solvers -------------------------------------------------------------------------------
def ladder_parts():
    from tests.test_host_physical import LadderSolver, make_tp

    class EquilLadderSolver(LadderSolver):
        """LadderSolver with set_equilibrium: records the call and leaves a recognisable state; the lanes `pb_fails` report status 1"""

        def __init__(self, *a, **kw):
            self.pb_fails = list(kw.pop('pb_fails', ()))
            LadderSolver.__init__(self, *a, **kw)

        def set_equilibrium(self, phiM=None, lanes=None, tol=1e-10, maxit=100):
            self.calls.append(('set_equilibrium', np.array(phiM, float).copy()))
            self.c[:] = -3.0
            st = np.zeros(self.B, np.int32)
            st[self.pb_fails] = 1
            return {'status': st, 'iterations': np.full(self.B, 9, np.int32)}

        def newton_iterations(self):
            return np.full(self.B, 3, np.int32)
    return EquilLadderSolver, make_tp


def test_without_the_option_the_call_sequence_is_unchanged(monkeypatch):
    from catint_amd.calculator import Calculator
    Solver, make_tp = ladder_parts()
    phis = np.linspace(-0.5, -2.0, 3)
    runs = []
    for newton in ({'retry_rungs': 1, 'retry_mesh_rungs': 0, 'dphi_stage': 0.2},
                   {'retry_rungs': 1, 'retry_mesh_rungs': 0, 'dphi_stage': 0.2, 'equilibrium_start': False}):
        tp = make_tp(phis)
        tp.newton = newton
        calc = Calculator(transport=tp, calc='comsol')
        main = Solver(3, tp.nx, 3)
        monkeypatch.setattr(calc, '_physical_solver', lambda *a, **kw: pytest.fail('no sub-batch is needed'))
        st = calc.solve_physical(main, np.ones((3, 3 * tp.nx)), phis, np.zeros((3, 3)))
        assert list(st) == [0, 0, 0] and calc.continuation_stages == 11
        runs.append([c[0] for c in main.calls])
    assert runs[0] == runs[1] == ['set_batch', 'solve'] + ['set_pb', 'set_flux', 'solve'] * 10
    assert 'set_equilibrium' not in runs[0]


def test_with_the_option_one_solve_from_the_equilibrium_state(monkeypatch):
    from catint_amd.calculator import Calculator
    Solver, make_tp = ladder_parts()
    phis = np.linspace(-0.5, -2.0, 3)
    tp = make_tp(phis)
    tp.newton = {'retry_rungs': 1, 'retry_mesh_rungs': 0, 'dphi_stage': 0.2, 'equilibrium_start': True}
    calc = Calculator(transport=tp, calc='comsol')
    main = Solver(3, tp.nx, 3)
    monkeypatch.setattr(calc, '_physical_solver', lambda *a, **kw: pytest.fail('no sub-batch is needed'))
    flux = np.arange(9.0).reshape(3, 3)
    st = calc.solve_physical(main, np.ones((3, 3 * tp.nx)), phis, flux)
    assert list(st) == [0, 0, 0]
    assert [c[0] for c in main.calls] == ['set_batch', 'set_equilibrium', 'solve']
    # the batch is set at the operating point with the full flux, and the equilibrium is taken at the operating point's potentials
    assert np.array_equal(main.calls[0][1], phis) and np.array_equal(main.calls[0][2], calc.RF * flux)
    assert np.array_equal(main.calls[1][1], phis)
    assert calc.continuation_stages == 1
    assert calc.equilibrium_start == {'pb_failed': 0, 'pb_iterations': 9, 'failed': 0}
    assert calc.newton_iterations_total == 9 and calc.newton_iterations_slowest == 3
    # a sweep close to phiPZC is solved directly, as without the option: the continuation path would not have been taken
    near = np.array([0.1, 0.2, 0.3])
    tp2 = make_tp(near)
    tp2.newton = dict(tp.newton)
    calc2 = Calculator(transport=tp2, calc='comsol')
    main2 = Solver(3, tp2.nx, 3)
    calc2.solve_physical(main2, np.ones((3, 3 * tp2.nx)), near, np.zeros((3, 3)))
    assert [c[0] for c in main2.calls] == ['set_batch', 'solve']


def test_lanes_that_fail_the_one_solve_walk_the_continuation(monkeypatch):
    """... as rung 0 of the ladder, exactly as after mesh continuation; so does a lane whose Poisson-Boltzmann iteration did not converge"""
    from catint_amd.calculator import Calculator
    Solver, make_tp = ladder_parts()
    phis = np.linspace(-0.5, -2.0, 4)
    tp = make_tp(phis)
    tp.newton = {'retry_rungs': 1, 'retry_mesh_rungs': 0, 'dphi_stage': 0.2, 'equilibrium_start': True}
    calc = Calculator(transport=tp, calc='comsol')
    main = Solver(4, tp.nx, 3, stuck=[1], need=2, pb_fails=[3])       # lane 1 fails the one direct solve, lane 3 its PB iteration
    subs = []
    walked = []

    def fake_sub(B, xmesh=None, **kw):
        s = Solver(B, tp.nx, 3)
        subs.append(s)
        return s
    monkeypatch.setattr(calc, '_physical_solver', fake_sub)
    cont = calc._continuation

    def spy(solver, c0, pb, vz, flux, phiM, start, nst, lanes=None):
        walked.append((solver, nst, None if lanes is None else list(lanes)))
        return cont(solver, c0, pb, vz, flux, phiM, start, nst, lanes=lanes)
    monkeypatch.setattr(calc, '_continuation', spy)
    st = calc.solve_physical(main, np.ones((4, 3 * tp.nx)), phis, np.zeros((4, 3)))
    assert [c[0] for c in main.calls][:3] == ['set_batch', 'set_equilibrium', 'solve']
    assert calc.equilibrium_start == {'pb_failed': 1, 'pb_iterations': 9, 'failed': 2}
    assert len(walked) == 1 and walked[0][0] is subs[0] and walked[0][1:] == (11, [1, 3])
    assert [(r['rung'], r['stages'], r['lanes'], r['recovered']) for r in calc.retry_log] == [(0, 11, [1, 3], [1, 3])]
    assert [c[1] for c in main.calls if c[0] == 'set_lanes'] == [[1, 3]]
    assert [c[1] for c in main.calls if c[0] == 'mask'] == [[1, 3], None]
    assert list(st) == [0, 0, 0, 0] and calc.continuation_stages == 1
