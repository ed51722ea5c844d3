"""libcatint_scfkin and the seam pnp_scf_cycle_fn without a GPU (the method of tests/test_kinetics_abi.py): the library builds for gfx950
and exports exactly what include/catint_scfkin.h declares and no pnp_* symbol, the ctypes mirrors have the compiler's layouts, every
validation error is returned before any device call, the library holds the one kernel, the other eleven libraries gained none, and
its sources are in no other library's list.  Calculator.set_microkinetics(device_loop=True) is driven with fakes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import kernel_census as K
from tests.test_kinetics_abi import FakeKinetics, chain, edit, header_source, poke, scf_parts, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {'catsk_params': 'CatskParams', 'catsk_outputs': 'CatskOutputs'}
INSTANCES = {'catsk::flux_kernel'}
MACROS = {'maxspecies': 'CATSK_MAX_SPECIES', 'maxads': 'CATSK_MAX_ADSORBATES', 'maxsteps': 'CATSK_MAX_STEPS', 'minlog': '(int)CATSK_MIN_LOG',
          'full': 'CATSK_DROP_FULL', 'stern': 'CATSK_DROP_STERN', 'converged': 'CATSK_CONVERGED', 'maxit': 'CATSK_MAXIT', 'input': 'CATSK_INPUT',
          'pivot': 'CATSK_PIVOT', 'einval': 'CATSK_EINVAL', 'enomem': 'CATSK_ENOMEM', 'edevice': 'CATSK_EDEVICE'}


@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_scfkin_library
    return build_scfkin_library()


@pytest.fixture(scope='module')
def sk(libpath):
    from catint_amd import _scfkin
    with _scfkin.ScfKinetics(0) as o:
        yield o


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    from catint_amd import _scfkin
    declared = sorted(set(re.findall(r'\b(catsk_[a-z0-9_]+)\s*\(', header_source('catint_scfkin.h'))))
    assert declared == sorted(_scfkin.SYMBOLS) and len(declared) == 8
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(catsk_[a-z0-9_]+)\b', exported))) == declared
    assert not re.findall(r'\bpnp_[a-z0-9_]+\b', exported)          # and no pnp_* symbol


def test_the_seam_is_declared_exported_and_mirrored():
    from catint_amd import _capi
    from catint_amd.build import build_library
    src = header_source('catint_pnp.h')
    assert re.search(r'\bpnp_scf_cycle_fn\s*\(', src) and 'pnp_scf_cycle_fn' in _capi.SYMBOLS
    assert hasattr(C.CDLL(build_library()), 'pnp_scf_cycle_fn')
    assert not [s for s in _capi.SYMBOLS if 'catsk' in s or 'catkin' in s or 'microkinetic' in s]
    import inspect
    assert {'flux_fn', 'user'} <= set(inspect.signature(_capi.PnpSolver.scf_cycle).parameters)


def test_the_sources_are_not_part_of_the_other_libraries():
    from catint_amd import build
    others = (build.SOURCES + build.OBSERVE_SOURCES + build.BALANCE_SOURCES + build.REGRID_SOURCES + build.EQUIL_SOURCES + build.RESPONSE_SOURCES
              + build.KINETICS_SOURCES + build.COUPLE_SOURCES + build.SENS_SOURCES + build.DRC_SOURCES + build.MODES_SOURCES + build.UNITTEST_SOURCES)
    assert not any('catscfkin' in s or 'scfkin' in s for s in others)
    assert os.path.dirname(build.SCFKIN_LIB) == os.path.dirname(build.LIB)
    assert build.SCFKIN_SOURCES == ['catscfkin.hip'] and os.path.isdir(build.SCFKIN_DIR)
    assert callable(build.scfkin_needs_build)
    listed = {os.path.realpath(p) for p in build.SCFKIN_HEADERS}
    for h in ('catint_scfkin.h', 'catint_pnp.h'):
        assert os.path.realpath(os.path.join(ROOT, 'include', h)) in listed
    assert os.path.realpath(os.path.join(build.CSRC, 'pnp_kin.h')) in listed
    from tests.test_build_deps import reached
    sources = [os.path.join(build.SCFKIN_DIR, f) for f in build.SCFKIN_SOURCES]
    assert not reached(sources) - listed - {os.path.realpath(f) for f in sources}
    assert 'build_scfkin_library(' in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    # the main library's loop source is the parent's: the seam is host code in pnp_capi.hip
    assert 'pnp_scf_flux_fn' not in open(os.path.join(build.CSRC, 'pnp_scf.hip')).read()


def header_structs(name):
    out = {}
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
    structs = dict(header_structs('catint_scfkin.h'), pnp_scf_device=header_structs('catint_pnp.h')['pnp_scf_device'])
    assert set(PAIRS) <= set(structs)
    d = tmp_path_factory.mktemp('scfkin_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_scfkin.h"', 'int main(void) {']
    for s in list(PAIRS) + ['pnp_scf_device']:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (s, s))
        for f in structs[s]:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    for name, macro in MACROS.items():
        lines.append('  printf("%s n %%d\\n", %s);' % (name, macro))
    lines += ['  return 0;', '}']
    (d / 'abi.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(d / 'abi.c'), '-o', str(d / 'abi')])
    layout = {}
    for line in subprocess.check_output([str(d / 'abi')]).decode().splitlines():
        s, f, v = line.split()
        layout.setdefault(s, {})[f] = int(v)
    return layout


@pytest.mark.parametrize('cname', sorted(PAIRS) + ['pnp_scf_device'])
def test_ctypes_mirror_matches_the_compiler(cname, compiler_layout):
    from catint_amd import _capi, _scfkin
    cls = _capi.PnpScfDevice if cname == 'pnp_scf_device' else getattr(_scfkin, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_of_the_binding_are_the_header_s(compiler_layout):
    from catint_amd import _kinetics as k
    from catint_amd import _scfkin as s
    n = {name: compiler_layout[name]['n'] for name in MACROS}
    assert (s.MAX_SPECIES, s.MAX_ADSORBATES, s.MAX_STEPS) == (n['maxspecies'], n['maxads'], n['maxsteps']) == (k.MAX_SPECIES, k.MAX_ADSORBATES, k.MAX_STEPS)
    assert s.MIN_LOG == n['minlog'] == k.MIN_LOG and s.DROP == {'full': n['full'], 'stern': n['stern']}
    assert (s.CONVERGED, s.MAXIT, s.INPUT, s.PIVOT) == (n['converged'], n['maxit'], n['input'], n['pivot']) == (k.CONVERGED, k.MAXIT, k.INPUT, k.PIVOT)
    assert (s.EINVAL, s.ENOMEM, s.EDEVICE) == (n['einval'], n['enomem'], n['edevice'])
    assert (s.DEFAULT_TOL, s.DEFAULT_MAXIT) == (k.DEFAULT_TOL, k.DEFAULT_MAXIT)


@pytest.mark.parametrize('what, make, word', [
    ('struct_size of the parameters', lambda: (chain(), {'struct_size': 8}), 'catsk_params.struct_size'),
    ('nine species', lambda: (chain(N=9), {}), '9 species'),
    ('no adsorbate', lambda: (tables(np.zeros((1, 3), int), np.zeros((1, 3), int), [[1.0, 0.0]], [1.0], np.zeros((1, 4))), {}), '0 adsorbates'),
    ('nine adsorbates', lambda: (chain(S=9), {}), '9 adsorbates'),
    ('seventeen steps', lambda: (chain(R=17), {}), '17 steps'),
    ('an order of 4', lambda: (edit(chain(), f=poke('order_f', (0, 0), 4)), {}), 'order'),
    ('a step that does not conserve sites', lambda: (edit(chain(), f=poke('order_f', (0, 2), 2)), {}), 'conserve sites'),
    ('a zero cref', lambda: (edit(chain(), cref=np.array([1.0, 0.0])), {}), 'cref[1]'),
    ('a NaN site density', lambda: (edit(chain(), site_density=np.nan), {}), 'site_density'),
    ('a zero tolerance', lambda: (chain(), {'tol': 0.0}), 'tol'),
    ('a site count of 4', lambda: (edit(chain(), site_count=np.array([1.0, 4.0])), {}), 'site count 1'),
    ('maxit 0', lambda: (chain(), {'maxit': 0}), 'maxit'),
    ('potential_drop 2', lambda: (chain(), {'potential_drop': 2}), 'potential_drop'),
    ('negative max_waves', lambda: (chain(), {'max_waves': -1}), 'max_waves'),
    ('a NaN in dG', lambda: (edit(chain(), f=poke('dG', (1, 2), np.nan)), {}), 'step 1 has a non-finite'),
    ('e0 = +inf', lambda: (edit(chain(), f=poke('Ea', (0, 0), np.inf)), {}), 'step 0 has a non-finite'),
    ('a NaN nu', lambda: (edit(chain(), f=poke('nu', (0, 0), np.nan)), {}), 'nu of step 0'),
    ('an infinite capacitance', lambda: (chain(), {'stern_capacitance': np.inf}), 'surface charge'),
    ('a NaN phi_pzc', lambda: (chain(), {'phi_pzc': np.nan}), 'surface charge'),
    ('no lane', lambda: (chain(), {'phiM': np.zeros(0)}), 'batch < 1'),
])
def test_validation_errors_come_before_any_device_call(sk, what, make, word):
    from catint_amd import _scfkin
    tab, kw = make()
    args = dict(phiM=np.linspace(-0.1, -0.3, 2))
    args.update(kw)
    with pytest.raises(_scfkin.ScfKineticsError) as e:
        sk.begin(tab, **args)
    assert e.value.code == _scfkin.EINVAL, (what, str(e.value))
    assert word in str(e.value) and 'catsk_begin' in str(e.value), (what, str(e.value))
    assert sk.last_kernel == ''


def test_null_arguments_and_calls_before_begin(sk):
    from catint_amd import _capi, _scfkin
    lib = _scfkin.load_library()
    assert lib.catsk_begin(sk._h, None) == _scfkin.EINVAL and b'null' in lib.catsk_last_error(sk._h)
    assert lib.catsk_begin(None, None) == _scfkin.EINVAL and lib.catsk_create(0, None) == _scfkin.EINVAL
    o = _scfkin.CatskOutputs(struct_size=C.sizeof(_scfkin.CatskOutputs))
    assert lib.catsk_end(sk._h, C.byref(o)) == _scfkin.EINVAL and b'catsk_begin first' in lib.catsk_last_error(sk._h)
    assert lib.catsk_end(sk._h, None) == _scfkin.EINVAL and lib.catsk_end(None, C.byref(o)) == _scfkin.EINVAL
    o.struct_size = 8
    assert lib.catsk_end(sk._h, C.byref(o)) == _scfkin.EINVAL and b'catsk_outputs.struct_size' in lib.catsk_last_error(sk._h)
    z = np.zeros(4)
    zi = np.zeros(4, np.int32)
    assert lib.catsk_step_host(sk._h, _scfkin._dptr(z), _scfkin._dptr(z), _scfkin._iptr(zi), _scfkin._dptr(z)) == _scfkin.EINVAL
    assert b'catsk_begin first' in lib.catsk_last_error(sk._h)
    # the function of the seam refuses a context that has not begun, and a NULL one, without a device call
    fn = C.cast(sk.flux_fn, _capi.PnpScfFluxFn)
    d = _capi.PnpScfDevice(struct_size=C.sizeof(_capi.PnpScfDevice), nspecies=2, batch=2)
    assert fn(sk.user, C.byref(d)) == 1 and fn(None, C.byref(d)) == 1
    assert sk.last_kernel == ''


def test_the_library_holds_the_one_kernel(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)


def test_the_other_eleven_libraries_gained_no_kernel():
    from catint_amd import build as B
    libs = [(B.build_observe_library, B.OBSERVE_LIB), (B.build_balance_library, B.BALANCE_LIB), (B.build_regrid_library, B.REGRID_LIB),
            (B.build_equil_library, B.EQUIL_LIB), (B.build_response_library, B.RESPONSE_LIB), (B.build_kinetics_library, B.KINETICS_LIB),
            (B.build_couple_library, B.COUPLE_LIB), (B.build_sens_library, B.SENS_LIB), (B.build_drc_library, B.DRC_LIB),
            (B.build_modes_library, B.MODES_LIB)]
    B.build_library()
    try:
        compiled = set(K.compiled_kernels())
        per_lib = {}
        for build, lib in libs:
            build()
            per_lib[lib] = K.compiled_kernels(lib=lib)
            compiled |= per_lib[lib]
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert len(libs) == 10                                            # with the main library: eleven
    assert not [n for n in compiled if 'catsk' in n or 'flux_kernel' in n]
    assert per_lib[B.KINETICS_LIB] == {'catkin::steady_kernel'}       # the kernel whose iteration moved into the shared header


# ---- the calculator's opt-in path, with fakes --------------------------------------------------------------------------------------
class FakeSolver(object):
    """What run_scf_cycle asks of the transport handle; the device loop 'runs' three iterations and every lane leaves"""

    def __init__(self, transport_fn, log):
        self.transport_fn, self.log = transport_fn, log

    def solve_surface(self, flux):
        self.log.append(('solve_surface',))
        cs, vs, es = self.transport_fn(flux)
        return cs, vs, es, np.zeros(len(cs), np.int32)

    def scf_cycle(self, st, istep, max_iter, tau, faraday, nel, nprod, species_H=-1, species_OH=-1, flux_fn=None, user=None):
        self.log.append(('scf_cycle', istep, flux_fn, user, {k: np.array(v) for k, v in st.items()}))
        st['active'] = np.zeros_like(st['active'])
        return istep + 3

    def close(self):
        self.log.append(('close solver',))


class FakeScfKinetics(object):
    flux_fn, user = 0x1234, 0x5678

    def __init__(self, log):
        self.log = log

    def begin(self, tab, phiM, **kw):
        self.log.append(('begin', np.array(kw['theta_guess']), kw))
        self.B, self.T, self.N = len(phiM), len(tab['site_count']), np.asarray(tab['nu']).shape[1]

    def end(self):
        self.log.append(('end',))
        B, T, N = self.B, self.T, self.N
        return {'theta': np.full((B, T), 0.5), 'flux_scale': np.full((B, N), 2.0), 'flux_last': np.full((B, N), 3.0), 'status': np.zeros(B, np.int32),
                'iterations_last': np.full(B, 2, np.int32), 'iterations_total': np.full(B, 7, np.int32), 'calls': np.array([3] * (B - 1) + [0], np.int32)}

    def close(self):
        self.log.append(('close kinetics',))


def device_loop_calculator(monkeypatch, device_loop, log):
    from catint_amd.calculator import Calculator
    tp, model, transport_fn = scf_parts()
    calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-9)
    calc.set_microkinetics(model, site_density=2e-6, device_loop=device_loop)
    fake = FakeKinetics()
    solver = FakeSolver(transport_fn, log)

    def first(s, c0, phiM, flux, **kw):
        log.append(('solve_physical',))
        s.surface = transport_fn(flux)
        return np.zeros(len(phiM), np.int32)
    solver.get_surface = lambda: solver.surface
    monkeypatch.setattr(calc, '_kinetics_solver', lambda: fake)
    monkeypatch.setattr(calc, '_physical_solver', lambda B: solver)
    monkeypatch.setattr(calc, 'solve_physical', first)
    return calc, fake, tp


def test_device_loop_hands_over_after_the_host_iterations(monkeypatch):
    log = []
    calc, fake, tp = device_loop_calculator(monkeypatch, True, log)
    monkeypatch.setattr(calc, '_scf_kinetics', lambda: FakeScfKinetics(log))
    out = calc.run_scf_cycle(max_iter=200)
    assert [e[0] for e in log] == ['solve_physical', 'solve_surface', 'begin', 'scf_cycle', 'end', 'close kinetics', 'close solver']
    assert len(fake.calls) == 2 and len(out['history']) == 2 and out['iterations'] == 5
    begin, cycle = log[2], log[3]
    assert np.array_equal(begin[1], fake.calls[1]['theta'])                       # the coverages of the last host iteration are the guess
    assert begin[2]['potential_drop'] == 'stern' and begin[2]['stern_capacitance'] == 0.2 and begin[2]['phi_pzc'] == 0.16
    assert cycle[1:4] == (2, FakeScfKinetics.flux_fn, FakeScfKinetics.user) and cycle[4]['active'].all()
    # lanes the device called report its coverages, the lane it did not call keeps the host's
    assert (out['coverage'][:2] == 0.5).all() and np.array_equal(out['coverage'][2], fake.calls[1]['theta'][2])
    assert (out['flux_scale'][:2] == 2.0).all() and list(out['kinetic_calls']) == [3, 3, 0] and (out['kinetic_iterations'] == 7).all()
    assert out['converged'].all() and tp.alldata[0]['system']['coverage'][0] == 0.5


def test_without_device_loop_the_library_is_never_called(monkeypatch):
    log = []
    calc, fake, tp = device_loop_calculator(monkeypatch, False, log)

    def never():
        raise AssertionError('the context of the device loop was created without device_loop=True')
    monkeypatch.setattr(calc, '_scf_kinetics', never)
    out = calc.run_scf_cycle(max_iter=6)
    assert 'scf_cycle' not in [e[0] for e in log] and len(fake.calls) == out['iterations'] == len(out['history'])
    assert 'kinetic_calls' not in out and 'kinetic_iterations' not in out and 'device_loop' not in calc.microkinetics
    # with a transport_fn the loop stays on the host although the option is set
    log2 = []
    calc2, fake2, _ = device_loop_calculator(monkeypatch, True, log2)
    monkeypatch.setattr(calc2, '_scf_kinetics', never)
    _, _, transport_fn = scf_parts()
    out2 = calc2.run_scf_cycle(transport_fn=transport_fn, max_iter=6)
    assert len(fake2.calls) == out2['iterations'] and 'kinetic_calls' not in out2


def test_device_loop_needs_the_mixing_loop():
    from catint_amd.calculator import Calculator, CalculatorError
    tp, model, _ = scf_parts()
    with pytest.raises(CalculatorError, match="scf='mixing'"):
        Calculator(transport=tp, calc='comsol').set_microkinetics(model, scf='newton', device_loop=True)
