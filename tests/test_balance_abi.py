"""libcatint_balance without a GPU: it builds for gfx950 and exports what include/catint_balance.h declares, the header is plain C, the
ctypes mirrors have the compiler's layouts (the method of tests/test_observe_abi.py), every validation error is returned before any
device call, the kernels compiled into it are exactly the instances listed here, and neither of the other two libraries gained one."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import kernel_census as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {'catbal_params': 'CatbalParams', 'catbal_outputs': 'CatbalOutputs'}

# species_kernel<points per lane, waves per operating point, steric>: one wave up to nx = 1026, then 16 points per lane in 2 / 4 waves.
# Reactions and wall tables are loops over a device table, not template parameters: they change no instance.
INSTANCES = {'catbal::species_kernel<%d, %d, %s>' % (P, WY, s)
             for (P, WY) in ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (16, 2), (16, 4)) for s in ('false', 'true')}


@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_balance_library
    return build_balance_library()


@pytest.fixture(scope='module')
def balancer(libpath):
    from catint_amd import _balance
    with _balance.Balancer(0) as o:
        yield o


def header_source(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    from catint_amd import _balance
    declared = sorted(set(re.findall(r'\b(catbal_[a-z0-9_]+)\s*\(', header_source('catint_balance.h'))))
    assert declared == sorted(_balance.SYMBOLS)
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(catbal_[a-z0-9_]+)\b', exported))) == declared


def test_the_sources_are_not_part_of_the_other_libraries():
    from catint_amd import build
    assert not any('catbal' in s or 'balance' in s for s in build.SOURCES + build.OBSERVE_SOURCES)
    assert os.path.dirname(build.BALANCE_LIB) == os.path.dirname(build.LIB)


def header_structs():
    out = {}
    for body, struct in re.findall(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', header_source('catint_balance.h'), flags=re.S):
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
    d = tmp_path_factory.mktemp('balance_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_balance.h"', 'int main(void) {']
    for s in PAIRS:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (s, s))
        for f in structs[s]:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    for name, macro in (('nscalars', 'CATBAL_NSCALARS'), ('maxnx', 'CATBAL_MAX_NX'), ('maxspecies', 'CATBAL_MAX_SPECIES'),
                        ('maxreactions', 'PNP_MAX_REACTIONS'), ('maxreactants', 'PNP_MAX_REACTANTS'), ('maxwall', 'PNP_MAX_WALL_REACTIONS'),
                        ('col_wall_flux', 'CATBAL_WALL_FLUX'), ('col_bulk_flux', 'CATBAL_BULK_FLUX'), ('col_source_integral', 'CATBAL_SOURCE_INTEGRAL'),
                        ('col_defect', 'CATBAL_DEFECT'), ('col_max_imbalance_rel', 'CATBAL_MAX_IMBALANCE_REL'), ('col_inventory', 'CATBAL_INVENTORY')):
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
    from catint_amd import _balance
    cls = getattr(_balance, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_of_the_binding_are_the_header_s(compiler_layout):
    from catint_amd import _balance
    assert _balance.NSCALARS == compiler_layout['nscalars']['n'] == 6
    assert _balance.MAX_NX == compiler_layout['maxnx']['n'] and _balance.MAX_SPECIES == compiler_layout['maxspecies']['n']
    assert (_balance.MAX_REACTIONS, _balance.MAX_REACTANTS, _balance.MAX_WALL_REACTIONS) == (
        compiler_layout['maxreactions']['n'], compiler_layout['maxreactants']['n'], compiler_layout['maxwall']['n'])
    for col, name in enumerate(_balance.SCALARS):
        assert compiler_layout['col_' + name]['n'] == col
    assert C.sizeof(_balance.CatbalOutputs) == 7 * 8
    assert list(_balance.FIELDS) + ['scalars'] == [n for n, _ in _balance.CatbalOutputs._fields_]


def fake_view(nx=16, N=2, B=2, phi=0x1000, size=None):
    """A view no device stands behind: validation must reject it without reading it."""
    from catint_amd import _balance
    return _balance.PnpDeviceView(C.sizeof(_balance.PnpDeviceView) if size is None else size, 2, N, nx, (nx + 15) // 16 * 16, 0, B, 0x1000, phi,
                                  0x1000, None)


DEFAULT = object()


def call(balancer, view, x=None, flux=DEFAULT, phiM=DEFAULT, D=None, charges=None, beta=0.4, **kw):
    from catint_amd import _balance
    nx, N, B = max(view.nx, 1), max(view.nspecies, 1), view.batch
    x = np.arange(nx) * 1e-9 if x is None else x
    flux = np.zeros((B, view.nspecies)) if flux is DEFAULT else flux
    phiM = np.zeros(B) if phiM is DEFAULT else phiM
    with pytest.raises(_balance.BalanceError) as e:
        balancer.species(view, np.full(N, 1e-9) if D is None else D, np.full(N, 96485.0) if charges is None else charges, x, beta, flux, phiM, **kw)
    return e.value


def wall(n=1, species=None, k=DEFAULT, B=2, N=2):
    return {'species': [0] * n if species is None else species, 'nu': np.ones((n, N)), 'k': np.ones((B, n)) if k is DEFAULT else k}


@pytest.mark.parametrize('what, make, word', [
    ('compat handle: no potential row', lambda: (fake_view(phi=None), {}), 'potential'),
    ('nx below 3', lambda: (fake_view(nx=2), {}), 'nx'),
    ('nx above 4098', lambda: (fake_view(nx=4099, B=1), {}), 'nx'),
    ('more than 8 species', lambda: (fake_view(N=9), {}), 'species'),
    ('x not increasing', lambda: (fake_view(), {'x': np.array([0.0, 1.0, 2.0, 2.0] + list(range(3, 15)), float)}), 'increasing'),
    ('x decreasing', lambda: (fake_view(), {'x': -np.arange(16.0)}), 'increasing'),
    ('struct_size of the parameters', lambda: (fake_view(), {'struct_size': 8}), 'struct_size'),
    ('struct_size of the view', lambda: (fake_view(size=12), {}), 'struct_size'),
    ('a zero diffusion coefficient', lambda: (fake_view(), {'D': np.array([1e-9, 0.0])}), 'D > 0'),
    ('a negative diffusion coefficient', lambda: (fake_view(), {'D': np.array([-1e-9, 1e-9])}), 'D > 0'),
    ('a NaN diffusion coefficient', lambda: (fake_view(), {'D': np.array([1e-9, np.nan])}), 'D > 0'),
    ('an infinite charge', lambda: (fake_view(), {'charges': np.array([np.inf, 1.0])}), 'finite charge'),
    ('a negative radius', lambda: (fake_view(), {'mpb_radius': np.array([3e-10, -3e-10])}), 'radius'),
    ('beta zero', lambda: (fake_view(), {'beta': 0.0}), 'beta'),
    ('beta NaN', lambda: (fake_view(), {'beta': np.nan}), 'beta'),
    ('velocity infinite', lambda: (fake_view(), {'velocity': np.inf}), 'velocity'),
    ('reaction species above N - 1', lambda: (fake_view(), {'reactions': [([0, 2], [1], 1.0, 1.0)]}), 'species index'),
    ('reaction species negative', lambda: (fake_view(), {'reactions': [([0], [1], 1.0, 1.0), ([1], [-1], 1.0, 1.0)]}), 'species index'),
    ('five reactants on the left', lambda: (fake_view(), {'reactions': [([0] * 5, [1], 1.0, 1.0)]}), 'n_lhs'),
    ('five reactants on the right', lambda: (fake_view(), {'reactions': [([0], [1] * 5, 1.0, 1.0)]}), 'n_rhs'),
    ('seventeen reactions', lambda: (fake_view(), {'reactions': [([0], [1], 1.0, 1.0)] * 17}), 'nreactions'),
    ('nine wall reactions', lambda: (fake_view(), {'wall': wall(9)}), 'n_wall'),
    ('wall species above N - 1', lambda: (fake_view(), {'wall': wall(2, [0, 2])}), 'wall reaction'),
    ('wall species below -1', lambda: (fake_view(), {'wall': wall(1, [-2])}), 'wall reaction'),
    ('wall table without rate constants', lambda: (fake_view(), {'wall': wall(1, k=None)}), 'rate constants'),
    ('no prescribed flux', lambda: (fake_view(), {'flux': None}), 'flux'),
    ('no electrode potential', lambda: (fake_view(), {'phiM': None}), 'phiM'),
])
def test_validation_errors_come_before_any_device_call(balancer, what, make, word):
    from catint_amd import _balance
    view, kw = make()
    err = call(balancer, view, **kw)
    assert err.code == _balance.EINVAL, (what, str(err))
    assert word in str(err), (what, str(err))
    assert balancer.last_kernel == '' and balancer.last_kernel_ms == -1.0


def test_null_arguments_and_null_context(balancer, libpath):
    from catint_amd import _balance
    lib = _balance.load_library()
    p = _balance.CatbalParams(struct_size=C.sizeof(_balance.CatbalParams))
    o = _balance.CatbalOutputs()
    v = fake_view()
    assert lib.catbal_species(balancer._h, None, C.byref(p), C.byref(o)) == _balance.EINVAL
    assert b'null' in lib.catbal_last_error(balancer._h)
    assert lib.catbal_species(balancer._h, C.byref(v), None, C.byref(o)) == _balance.EINVAL
    assert lib.catbal_species(balancer._h, C.byref(v), C.byref(p), None) == _balance.EINVAL
    assert lib.catbal_species(None, None, C.byref(p), C.byref(o)) == _balance.EINVAL
    assert lib.catbal_create(0, None) == _balance.EINVAL
    assert lib.catbal_last_kernel(balancer._h) == b''


def test_a_call_that_asks_for_nothing_makes_no_device_call(balancer):
    """Every output NULL: valid, and done before the first device call (this machine may have no device at all)."""
    view = fake_view()
    out = balancer.species(view, np.full(2, 1e-9), np.full(2, 96485.0), np.arange(16) * 1e-9, 0.4, np.zeros((2, 2)), np.zeros(2), fields=[],
                           scalars=False)
    assert out == {} and balancer.last_kernel == ''


def test_the_solver_binding_offers_the_balance():
    from catint_amd import _capi
    assert hasattr(_capi.PnpSolver, 'get_balance')
    assert not [s for s in _capi.SYMBOLS if 'catbal' in s or 'balance' in s]        # no pnp_* symbol was added for it


def test_compiled_kernels_are_the_listed_instances(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)


def test_the_other_libraries_gained_no_kernel():
    from catint_amd.build import OBSERVE_LIB, build_observe_library
    build_observe_library()
    try:
        compiled = K.compiled_kernels() | K.compiled_kernels(lib=OBSERVE_LIB)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert not [n for n in compiled if 'catbal' in n or 'balance' in n]
