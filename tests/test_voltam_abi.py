"""libcatint_voltam without a GPU (the checks of tests/test_kintrans_abi.py, carried over): the library builds for gfx950 and exports
what include/catint_voltam.h declares, the ctypes mirrors have the compiler's layouts, every validation error is returned before any
device call, no point makes no device call, the library holds the one kernel, the build lists are complete, the transient and the
steady-state library gained nothing, and MeanFieldModel.electrons() is what parse_step reads."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import kernel_census as K
from tests import voltam_ref as VR
from tests.test_kinetics_abi import chain, edit, fake_view, poke

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {'catvm_params': 'CatvmParams', 'catvm_outputs': 'CatvmOutputs'}
INSTANCES = {'catvm::sweep_kernel'}


@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_voltam_library
    return build_voltam_library()


@pytest.fixture(scope='module')
def solver(libpath):
    from catint_amd import voltammetry
    with voltammetry.Voltammetry(0) as o:
        yield o


def header_source():
    src = open(os.path.join(ROOT, 'include', 'catint_voltam.h')).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    from catint_amd import voltammetry
    declared = sorted(set(re.findall(r'\b(catvm_[a-z0-9_]+)\s*\(', header_source())))
    assert declared == sorted(voltammetry.SYMBOLS) and len(declared) == 6
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(catvm_[a-z0-9_]+)\b', exported))) == declared
    assert not re.findall(r'\b(pnp|catkin|catkt)_[a-z0-9_]+\b', exported)          # and no symbol of another library


def test_the_sources_are_a_library_of_their_own():
    from catint_amd import build
    others = (build.SOURCES + build.OBSERVE_SOURCES + build.BALANCE_SOURCES + build.REGRID_SOURCES + build.EQUIL_SOURCES + build.RESPONSE_SOURCES
              + build.KINETICS_SOURCES + build.COUPLE_SOURCES + build.SENS_SOURCES + build.DRC_SOURCES + build.MODES_SOURCES + build.SCFKIN_SOURCES
              + build.KINTRANS_SOURCES + build.EIS_SOURCES + build.INTERACT_SOURCES)
    assert not any('catvm' in s or 'voltam' in s for s in others)
    assert os.path.dirname(build.VOLTAM_LIB) == os.path.dirname(build.LIB)
    assert build.VOLTAM_SOURCES == ['catvm.hip'] and os.path.isdir(build.VOLTAM_DIR) and callable(build.voltam_needs_build)
    # no name of this library carries one of the words the other libraries' tests forbid in foreign lists
    for name in build.VOLTAM_SOURCES + [os.path.basename(build.VOLTAM_DIR), os.path.basename(build.VOLTAM_LIB)]:
        assert not any(w in name for w in ('interact', 'catia', 'catkt', 'transient')), name
    listed = {os.path.realpath(p) for p in build.VOLTAM_HEADERS}
    for h in ('catint_voltam.h', 'catint_kinetics.h', 'catint_pnp.h'):
        assert os.path.realpath(os.path.join(ROOT, 'include', h)) in listed
    assert os.path.realpath(os.path.join(build.CSRC, 'pnp_kin.h')) in listed
    from tests.test_build_deps import reached
    sources = [os.path.join(build.VOLTAM_DIR, f) for f in build.VOLTAM_SOURCES]
    assert not reached(sources) - listed - {os.path.realpath(f) for f in sources}
    assert 'build_voltam_library(' in open(os.path.join(ROOT, '__graft_entry__.py')).read()


def header_structs():
    out = {}
    for body, struct in re.findall(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', header_source(), flags=re.S):
        fields = []
        for decl in body.split(';'):
            decl = decl.strip()
            if not decl:
                continue
            names = decl.split(None, 1)[1] if not decl.startswith('const') else decl.split(None, 2)[2]
            fields += [n.strip().lstrip('*').strip() for n in names.split(',')]
        out[struct] = fields
    return out


MACROS = {'done': 'CATVM_DONE', 'input': 'CATVM_INPUT', 'steps': 'CATVM_STEPS', 'maxsteps': 'CATVM_MAX_STEPS', 'maxseg': 'CATVM_MAX_SEGMENTS',
          'maxsamples': 'CATVM_MAX_SAMPLES', 'startmaxit': 'CATVM_START_MAXIT', 'einval': 'CATVM_EINVAL', 'enomem': 'CATVM_ENOMEM',
          'edevice': 'CATVM_EDEVICE'}


@pytest.fixture(scope='module')
def compiler_layout(tmp_path_factory):
    structs = header_structs()
    assert set(PAIRS) <= set(structs)
    d = tmp_path_factory.mktemp('voltam_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_voltam.h"', 'int main(void) {']
    for s in PAIRS:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (s, s))
        for f in structs[s]:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    for name, macro in MACROS.items():
        lines.append('  printf("%s n %%d\\n", %s);' % (name, macro))
    lines.append('  printf("faraday %.17g x\\n", CATVM_FARADAY);')
    lines += ['  return 0;', '}']
    (d / 'abi.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(d / 'abi.c'), '-o', str(d / 'abi')])
    layout = {}
    for line in subprocess.check_output([str(d / 'abi')]).decode().splitlines():
        s, f, v = line.split()
        layout.setdefault(s, {})[f] = float(f) if s == 'faraday' else int(v)
    return layout


@pytest.mark.parametrize('cname', sorted(PAIRS))
def test_ctypes_mirror_matches_the_compiler(cname, compiler_layout):
    from catint_amd import voltammetry
    cls = getattr(voltammetry, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_of_the_binding_are_the_header_s(compiler_layout):
    from catint_amd import voltammetry as v
    from catint_amd.units import unit_F
    n = {name: compiler_layout[name]['n'] for name in MACROS}
    assert (v.DONE, v.INPUT, v.STEPS) == (n['done'], n['input'], n['steps']) == (VR.DONE, VR.INPUT, VR.STEPS) == (0, 2, 3)
    assert (v.MAX_STEPS, v.MAX_SEGMENTS, v.MAX_SAMPLES) == (n['maxsteps'], n['maxseg'], n['maxsamples']) == (1000000, 64, 4096)
    assert n['startmaxit'] == VR.START_MAXIT == 100
    assert (v.EINVAL, v.ENOMEM, v.EDEVICE) == (n['einval'], n['enomem'], n['edevice'])
    (faraday,) = compiler_layout['faraday'].values()
    assert faraday == v.FARADAY == VR.FARADAY == unit_F
    d = VR.DEFAULTS
    assert (v.DEFAULT_RTOL, v.DEFAULT_ATOL, v.DEFAULT_NEWTON_TOL, v.DEFAULT_NEWTON_MAXIT, v.DEFAULT_MAX_STEPS) == (
        d['rtol'], d['atol'], d['newton_tol'], d['newton_maxit'], d['max_steps'])
    assert (v.DEFAULT_SEGMENTS, v.DEFAULT_SAMPLES) == (2, 200)
    from tests.voltam_cases import KT_EV, RATE_FLOOR
    assert v.default_rate_floor(KT_EV) == RATE_FLOOR


def sweep_args(n=2, N=2, R=2):
    return dict(electrons=np.ones(R), E_start=np.linspace(0.3, 0.2, n), E_vertex=np.full(n, -0.3), scan_rate=np.full(n, 0.1),
                csurf=np.full((n, N), 0.5), phi_surface=np.zeros(n), rate_floor=10.0, n_segments=2, samples=4)


VIEW = {'csurf': None, 'phi_surface': None}


@pytest.mark.parametrize('what, make, word', [
    # ---- what catkt_solve checks on the members the two structs share ----
    ('struct_size of the parameters', lambda: (None, chain(), {'struct_size': 8}), 'catvm_params.struct_size'),
    ('struct_size of the outputs', lambda: (None, chain(), {'out_struct_size': 8}), 'catvm_outputs.struct_size'),
    ('struct_size of the view', lambda: (fake_view(size=12), chain(), dict(VIEW)), 'pnp_device_view.struct_size'),
    ('nine species', lambda: (None, chain(N=9), {}), '9 species'),
    ('nine adsorbates', lambda: (None, chain(S=9), {}), '9 adsorbates'),
    ('seventeen steps', lambda: (None, chain(R=17), {}), '17 steps'),
    ('an order of 4', lambda: (None, edit(chain(), f=poke('order_f', (0, 0), 4)), {}), 'order'),
    ('a step that does not conserve sites', lambda: (None, edit(chain(), f=poke('order_f', (0, 2), 2)), {}), 'conserve sites'),
    ('an empty step', lambda: (None, edit(chain(S=2, R=4), f=lambda t: (t['order_f'].__setitem__(3, 0), t['order_b'].__setitem__(3, 0),
                                                                      t['nu'].__setitem__(3, 0.0))), {}), 'empty step'),
    ('a zero cref', lambda: (None, edit(chain(), cref=np.array([1.0, 0.0])), {}), 'cref[1]'),
    ('a zero site density', lambda: (None, edit(chain(), site_density=0.0), {}), 'site_density'),
    ('a site count of 4', lambda: (None, edit(chain(), site_count=np.array([1.0, 4.0])), {}), 'site count 1'),
    ('potential_drop 2', lambda: (None, chain(), {'potential_drop': 2}), 'potential_drop'),
    ('negative max_waves', lambda: (None, chain(), {'max_waves': -1}), 'max_waves'),
    ('a NaN in dG', lambda: (None, edit(chain(), f=poke('dG', (1, 2), np.nan)), {}), 'step 1 has a non-finite'),
    ('a NaN nu', lambda: (None, edit(chain(), f=poke('nu', (0, 0), np.nan)), {}), 'nu of step 0'),
    ('csurf without phi_surface', lambda: (None, chain(), {'phi_surface': None}), 'come together'),
    ('no view and no surface state', lambda: (None, chain(), dict(VIEW)), 'null view'),
    ('compat handle: no potential row', lambda: (fake_view(phi=None), chain(), dict(VIEW)), 'potential'),
    ('a lane outside the batch', lambda: (fake_view(), chain(), dict(VIEW, lanes=[0, 2])), 'lane index 2'),
    ('more points than lanes', lambda: (fake_view(B=1), chain(), dict(VIEW)), 'above the batch'),
    ('N different from the view', lambda: (fake_view(N=3), chain(), dict(VIEW)), 'the view has 3'),
    ('no sigma and an infinite capacitance', lambda: (None, chain(), {'stern_capacitance': np.inf}), 'surface charge'),
    ('a zero rtol', lambda: (None, chain(), {'rtol': 0.0}), 'rtol'),
    ('an infinite rtol', lambda: (None, chain(), {'rtol': np.inf}), 'rtol'),
    ('a NaN rtol', lambda: (None, chain(), {'rtol': np.nan}), 'rtol'),
    ('a zero newton_tol', lambda: (None, chain(), {'newton_tol': 0.0}), 'newton_tol'),
    ('a NaN newton_tol', lambda: (None, chain(), {'newton_tol': np.nan}), 'newton_tol'),
    ('a negative atol', lambda: (None, chain(), {'atol': -1e-12}), 'atol'),
    ('a NaN atol', lambda: (None, chain(), {'atol': np.nan}), 'atol'),
    ('newton_maxit 0', lambda: (None, chain(), {'newton_maxit': 0}), 'newton_maxit'),
    ('max_steps 0', lambda: (None, chain(), {'max_steps': 0}), 'max_steps outside [1, 1000000]'),
    ('max_steps above the cap', lambda: (None, chain(), {'max_steps': 1000001}), 'max_steps outside [1, 1000000]'),
    ('a NaN h0', lambda: (None, chain(), {'h0': np.nan}), 'h0'),
    # ---- what catvm_solve adds ----
    ('no electrons', lambda: (None, chain(), {'electrons': None}), 'electrons is required'),
    ('a NaN electron count', lambda: (None, chain(), {'electrons': [1.0, np.nan]}), 'electrons[1] is not finite'),
    ('an infinite electron count', lambda: (None, chain(), {'electrons': [-np.inf, 0.0]}), 'electrons[0] is not finite'),
    ('no E_vertex', lambda: (None, chain(), {'E_vertex': None}), 'E_start, E_vertex and scan_rate are required'),
    ('no scan_rate', lambda: (None, chain(), {'scan_rate': None}), 'E_start, E_vertex and scan_rate are required'),
    ('a zero scan rate', lambda: (None, chain(), {'scan_rate': [0.1, 0.0]}), 'scan_rate[1] must be positive and finite'),
    ('a negative scan rate', lambda: (None, chain(), {'scan_rate': [-1.0, 0.1]}), 'scan_rate[0] must be positive and finite'),
    ('an infinite scan rate', lambda: (None, chain(), {'scan_rate': [0.1, np.inf]}), 'scan_rate[1] must be positive and finite'),
    ('a NaN scan rate', lambda: (None, chain(), {'scan_rate': [np.nan, 0.1]}), 'scan_rate[0] must be positive and finite'),
    ('no segment', lambda: (None, chain(), {'n_segments': 0}), 'n_segments outside [1, 64]'),
    ('65 segments', lambda: (None, chain(), {'n_segments': 65}), 'n_segments outside [1, 64]'),
    ('no sample', lambda: (None, chain(), {'samples': 0}), 'samples outside [1, 4096]'),
    ('4097 samples', lambda: (None, chain(), {'samples': 4097}), 'samples outside [1, 4096]'),
    ('a negative rate_floor', lambda: (None, chain(), {'rate_floor': -1.0}), 'rate_floor'),
    ('an infinite rate_floor', lambda: (None, chain(), {'rate_floor': np.inf}), 'rate_floor'),
    ('a NaN rate_floor', lambda: (None, chain(), {'rate_floor': np.nan}), 'rate_floor'),
])
def test_validation_errors_come_before_any_device_call(solver, what, make, word):
    from catint_amd import voltammetry
    view, tab, kw = make()
    of = np.asarray(tab['order_f'])
    N = of.shape[1] - len(tab['site_count'])
    args = sweep_args(N=max(N, 0), R=of.shape[0])
    args.update(kw)
    with pytest.raises(voltammetry.VoltamError) as e:
        solver.sweep(view, tab, **args)
    assert e.value.code == voltammetry.EINVAL, (what, str(e.value))
    assert word in str(e.value), (what, str(e.value))
    assert solver.last_kernel == '' and solver.last_kernel_ms == -1.0


def test_a_bad_potential_of_one_point_is_no_error_of_the_call(solver):
    """a non-finite E_start or E_vertex is the point's CATVM_INPUT; with n = 0 behind it nothing is launched, so only the arguments
    of the call are judged here (the per-lane status is tests/test_gpu_voltam.py's)"""
    out = solver.sweep(None, chain(), np.ones(2), np.zeros(0), np.zeros(0), np.zeros(0), csurf=np.zeros((0, 2)), phi_surface=np.zeros(0),
                       rate_floor=10.0)
    assert out['status'].shape == (0,) and solver.last_kernel == ''


def test_the_python_layer_refuses_what_it_can_name(solver):
    from catint_amd import voltammetry
    args = sweep_args()
    with pytest.raises(ValueError, match='lateral interactions'):
        solver.sweep(None, dict(chain(), site_of=np.zeros(2, np.int32)), **args)
    with pytest.raises(ValueError, match='electrons has 3 values'):
        solver.sweep(None, chain(), **dict(args, electrons=np.ones(3)))
    with pytest.raises(ValueError, match='scan_rate has 3 values'):
        solver.sweep(None, chain(), **dict(args, scan_rate=np.ones(3)))
    with pytest.raises(ValueError, match='needs kT'):
        solver.sweep(None, chain(), **dict(args, rate_floor=None))
    with pytest.raises(ValueError, match='unknown field'):
        solver.sweep(None, chain(), fields=('drift',), **args)
    assert solver.last_kernel == ''
    import catint_amd
    assert catint_amd.Voltammetry is voltammetry.Voltammetry


def test_null_arguments_and_null_context(solver):
    from catint_amd import voltammetry
    lib = voltammetry.load_library()
    p = voltammetry.CatvmParams(struct_size=C.sizeof(voltammetry.CatvmParams))
    o = voltammetry.CatvmOutputs(struct_size=C.sizeof(voltammetry.CatvmOutputs))
    assert lib.catvm_solve(solver._h, None, None, C.byref(o)) == voltammetry.EINVAL
    assert b'null' in lib.catvm_last_error(solver._h)
    assert lib.catvm_solve(solver._h, None, C.byref(p), None) == voltammetry.EINVAL
    assert lib.catvm_solve(None, None, C.byref(p), C.byref(o)) == voltammetry.EINVAL
    assert lib.catvm_create(0, None) == voltammetry.EINVAL
    assert lib.catvm_last_kernel(solver._h) == b''


def test_no_point_makes_no_device_call(solver):
    """n == 0: valid, and done before the first device call (this machine may have no device at all); so is a call that asks for
    nothing"""
    from catint_amd import voltammetry
    out = solver.sweep(None, chain(S=2), np.ones(3), np.zeros(0), np.zeros(0), np.zeros(0), n_segments=3, samples=5, csurf=np.zeros((0, 2)),
                       phi_surface=np.zeros(0), rate_floor=10.0, fields=list(voltammetry.FIELDS))
    assert out['theta'].shape == (0, 15, 3) and out['flux'].shape == (0, 15, 2) and out['current'].shape == (0, 15)
    assert out['charge'].shape == (0, 15) and out['E_out'].shape == (0, 15) and out['t_reached'].shape == (0,) and out['mean_current'].shape == (0, 15)
    assert out['status'].shape == (0,) and out['steps'].shape == (0, 4) and out['steps'].dtype == np.int32
    out = solver.sweep(fake_view(), chain(), np.ones(2), np.zeros(0), np.zeros(0), np.zeros(0), lanes=[], samples=1, n_segments=1, rate_floor=0.0,
                       fields=('flux_scale',))
    assert out['flux_scale'].shape == (0, 1, 2)
    assert solver.last_kernel == ''
    lib = voltammetry.load_library()
    t = chain()
    keep = [np.ascontiguousarray(t[k], np.int32) for k in ('order_f', 'order_b')] + [np.ascontiguousarray(t[k], float) for k in
                                                                                      ('nu', 'cref', 'site_count', 'dG', 'Ea', 'lnA')]
    es, ev, sr, ne, cs, ps = np.ones(2), np.zeros(2), np.ones(2), np.ones(2), np.zeros((2, 2)), np.zeros(2)
    d = voltammetry._dptr
    p = voltammetry.CatvmParams(struct_size=C.sizeof(voltammetry.CatvmParams), nspecies=2, nadsorbates=1, nsteps=2, newton_maxit=8, max_steps=10, n=2,
                                site_density=1e-5, rtol=1e-3, newton_tol=1e-10, n_segments=1, samples=2, E_start=d(es), E_vertex=d(ev),
                                scan_rate=d(sr), electrons=d(ne), csurf=d(cs), phi_surface=d(ps))
    p.order_f, p.order_b = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in keep[:2])
    p.nu, p.cref, p.site_count, p.dG, p.Ea, p.lnA = (d(a) for a in keep[2:])
    o = voltammetry.CatvmOutputs(struct_size=C.sizeof(voltammetry.CatvmOutputs))
    assert lib.catvm_solve(solver._h, None, C.byref(p), C.byref(o)) == 0          # every output NULL: nothing to do
    assert lib.catvm_last_kernel(solver._h) == b''


def test_the_library_holds_the_one_kernel(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)


def test_the_transient_and_the_steady_library_gained_no_kernel_and_no_symbol():
    from catint_amd import build as B
    for f, lib, names, prefix in ((B.build_kinetics_library, B.KINETICS_LIB, {'catkin::steady_kernel'}, 'catkin_'),
                                  (B.build_kintrans_library, B.KINTRANS_LIB, {'catkt::transient_kernel'}, 'catkt_')):
        f()
        try:
            assert K.compiled_kernels(lib=lib) == names
        except K.CensusUnavailable as e:
            pytest.fail('kernel census unavailable: %s' % e)
        exported = subprocess.check_output(['nm', '-D', '--defined-only', lib]).decode()
        assert len(set(re.findall(r'\b(%s[a-z0-9_]+)\b' % prefix, exported))) == 6
        assert not re.findall(r'\bcatvm_[a-z0-9_]+\b', exported)
    from catint_amd import _capi
    assert not [s for s in _capi.SYMBOLS if 'catvm' in s or 'voltam' in s]
    assert hasattr(_capi.PnpSolver, 'get_voltammogram') and len(_capi.PnpSolver.SATELLITES) == 13


def test_the_model_s_electrons_are_those_of_its_steps():
    from catint_amd.interactions import InteractingModel
    from catint_amd.microkinetics import parse_step
    from tests.kinetics_cases import STEPS, co2r_model
    for variant in ('one_site', 'two_site'):
        m = co2r_model(variant)
        ne = m.electrons()
        assert ne.shape == (4,) and ne.dtype == np.float64
        assert ne.tolist() == [float(parse_step(s)['electrons']) for s in STEPS[variant]] == [0.0, 1.0, 1.0, 0.0]
        # the n_e tables() uses for dG
        assert np.array_equal(m.tables()['dG'][:, 1], ne / m.kT)
    from catint_amd.microkinetics import MeanFieldModel
    m = MeanFieldModel(['A'], {'X': 1}, ['X*_t <-> A_g + *_t + 2ele_g', {'reactants': {'A_g': 1, '*': 1}, 'products': {'X': 1}, 'electrons': 1.5}],
                       {'X': 0.1})
    assert m.electrons().tolist() == [-2.0, 1.5]
    assert InteractingModel.electrons is MeanFieldModel.electrons
