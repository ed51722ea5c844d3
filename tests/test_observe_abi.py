"""libcatint_observe without a GPU: it builds for gfx950 and exports what include/catint_observe.h declares, the header is plain C, the
ctypes mirrors have the compiler's layouts (the method of tests/test_abi_layout.py), every validation error is returned before any
device call, and the kernels compiled into it are exactly the instances listed here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import kernel_census as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = {'pnp_device_view': 'catint_pnp.h', 'catobs_params': 'catint_observe.h', 'catobs_outputs': 'catint_observe.h'}
PAIRS = {'pnp_device_view': 'PnpDeviceView', 'catobs_params': 'CatobsParams', 'catobs_outputs': 'CatobsOutputs'}

# electrolyte_kernel<points per lane, waves per operating point, steric>: one wave up to nx = 1026, then 16 points per lane in 2 / 4 waves
INSTANCES = {'catobs::electrolyte_kernel<%d, %d, %s>' % (P, WY, s)
             for (P, WY) in ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (16, 2), (16, 4)) for s in ('false', 'true')}


@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_observe_library
    return build_observe_library()


@pytest.fixture(scope='module')
def observer(libpath):
    from catint_amd import _observe
    with _observe.Observer(0) as o:
        yield o


def header_source(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_the_library_exports_every_declared_symbol(libpath):
    from catint_amd import _observe
    declared = sorted(set(re.findall(r'\b(catobs_[a-z0-9_]+)\s*\(', header_source('catint_observe.h'))))
    assert declared == sorted(_observe.SYMBOLS)
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s


def test_the_sources_are_not_part_of_the_solver_library():
    from catint_amd import build
    assert not any('catobs' in s or 'observe' in s for s in build.SOURCES)
    assert os.path.dirname(build.OBSERVE_LIB) == os.path.dirname(build.LIB)


def header_structs():
    out = {}
    for name in set(HEADERS.values()):
        for body, struct in re.findall(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', header_source(name), flags=re.S):
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
    d = tmp_path_factory.mktemp('observe_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_observe.h"', 'int main(void) {']
    for s in PAIRS:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (s, s))
        for f in structs[s]:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    lines += ['  printf("nscalars n %d\\n", CATOBS_NSCALARS);', '  printf("maxnx n %d\\n", CATOBS_MAX_NX);', '  return 0;', '}']
    (d / 'abi.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(d / 'abi.c'), '-o', str(d / 'abi')])
    layout = {}
    for line in subprocess.check_output([str(d / 'abi')]).decode().splitlines():
        s, f, v = line.split()
        layout.setdefault(s, {})[f] = int(v)
    return layout


@pytest.mark.parametrize('cname', sorted(PAIRS))
def test_ctypes_mirror_matches_the_compiler(cname, compiler_layout):
    from catint_amd import _observe
    cls = getattr(_observe, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_of_the_binding_are_the_header_s(compiler_layout):
    from catint_amd import _observe
    assert _observe.NSCALARS == compiler_layout['nscalars']['n'] == 10
    assert _observe.MAX_NX == compiler_layout['maxnx']['n']
    assert C.sizeof(_observe.CatobsOutputs) == 9 * 8          # nine rows: a scalars-only call moves NSCALARS * 8 = 80 bytes per point


def fake_view(nx=16, N=2, B=2, phi=0x1000, size=None):
    """A view no device stands behind: validation must reject it (or, valid, fail at the first device call) without reading it."""
    from catint_amd import _observe
    return _observe.PnpDeviceView(C.sizeof(_observe.PnpDeviceView) if size is None else size, 2, N, nx, (nx + 15) // 16 * 16, 0, B, 0x1000, phi,
                                  0x1000, None)


def call(observer, view, nx=None, N=None, x=None, **kw):
    from catint_amd import _observe
    nx = view.nx if nx is None else nx
    N = view.nspecies if N is None else N
    x = np.arange(max(nx, 1)) * 1e-9 if x is None else x
    with pytest.raises(_observe.ObserveError) as e:
        observer.electrolyte(view, np.full(max(N, 1), 1e-9), np.full(max(N, 1), 96485.0), x, 0.4, **kw)
    return e.value


@pytest.mark.parametrize('what, make, word', [
    ('compat handle: no potential row', lambda: (fake_view(phi=None), {}), 'potential'),
    ('nx below 3', lambda: (fake_view(nx=2), {}), 'nx'),
    ('nx above 4098', lambda: (fake_view(nx=4099, B=1), {}), 'nx'),
    ('more than 8 species', lambda: (fake_view(N=9), {}), 'species'),
    ('x not increasing', lambda: (fake_view(), {'x': np.array([0.0, 1.0, 2.0, 2.0] + list(range(3, 15)), float)}), 'increasing'),
    ('x decreasing', lambda: (fake_view(), {'x': -np.arange(16.0)}), 'increasing'),
    ('struct_size of the parameters', lambda: (fake_view(), {'struct_size': 8}), 'struct_size'),
    ('struct_size of the view', lambda: (fake_view(size=12), {}), 'struct_size'),
    ('pH species out of range', lambda: (fake_view(), {'species_H': 2}), 'species_H'),
])
def test_validation_errors_come_before_any_device_call(observer, what, make, word):
    from catint_amd import _observe
    view, kw = make()
    err = call(observer, view, **kw)
    assert err.code == _observe.EINVAL, (what, str(err))
    assert word in str(err), (what, str(err))


def test_null_view_and_null_context(observer, libpath):
    from catint_amd import _observe
    lib = _observe.load_library()
    p = _observe.CatobsParams(struct_size=C.sizeof(_observe.CatobsParams))
    o = _observe.CatobsOutputs()
    assert lib.catobs_electrolyte(observer._h, None, C.byref(p), C.byref(o)) == _observe.EINVAL
    assert b'null' in lib.catobs_last_error(observer._h)
    assert lib.catobs_electrolyte(None, None, C.byref(p), C.byref(o)) == _observe.EINVAL
    assert lib.catobs_create(0, None) == _observe.EINVAL
    assert lib.catobs_last_kernel(observer._h) == b''


def test_device_view_needs_a_batch_and_is_declared():
    """pnp_get_device_view is declared next to the read-back calls and bound; PNP_ESTATE before pnp_set_batch needs a handle, i.e. a
    device: tests/test_gpu_observe.py."""
    from catint_amd import _capi
    assert 'pnp_get_device_view' in _capi.SYMBOLS
    assert hasattr(_capi.PnpSolver, 'device_view') and hasattr(_capi.PnpSolver, 'get_electrolyte')
    assert re.search(r'\bint\s+pnp_get_device_view\s*\(\s*pnp_handle\s*\*\s*h\s*,\s*pnp_device_view\s*\*\s*out\s*\)', header_source('catint_pnp.h'))


def test_compiled_kernels_are_the_listed_instances(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)


def test_the_solver_library_gained_no_kernel():
    """The census of libcatint_pnp.so is tests/test_kernel_census.py's; here only that nothing of this library's got into it."""
    try:
        compiled = K.compiled_kernels()
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert not [n for n in compiled if 'catobs' in n or 'electrolyte' in n]
