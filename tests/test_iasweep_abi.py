"""libcatint_iasweep without a GPU (the checks of tests/test_voltam_abi.py and tests/test_interact_abi.py, carried over): the library
builds for gfx950 and exports what include/catint_iasweep.h declares, the ctypes mirrors have the compiler's layouts, every validation
error of both parents is returned before any device call, no point makes no device call, the library holds the one kernel, the build
lists are complete, and PnpSolver.get_voltammogram sends an interacting model to the new class and a mean-field model to the old."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import iasweep_ref as SR
from tests import kernel_census as K
from tests.test_interact_abi import PIECEWISE, ia, two_types
from tests.test_kinetics_abi import chain, edit, fake_view, poke
from tests.test_voltam_abi import VIEW, sweep_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {'catis_params': 'CatisParams', 'catis_outputs': 'CatisOutputs'}
INSTANCES = {'catis::sweep_kernel'}


@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_iasweep_library
    return build_iasweep_library()


@pytest.fixture(scope='module')
def solver(libpath):
    from catint_amd import iasweep
    with iasweep.InteractingVoltammetry(0) as o:
        yield o


def header_source():
    src = open(os.path.join(ROOT, 'include', 'catint_iasweep.h')).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    from catint_amd import iasweep
    declared = sorted(set(re.findall(r'\b(catis_[a-z0-9_]+)\s*\(', header_source())))
    assert declared == sorted(iasweep.SYMBOLS) and len(declared) == 6
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(catis_[a-z0-9_]+)\b', exported))) == declared
    assert not re.findall(r'\b(pnp|catkin|catkt|catia|catvm)_[a-z0-9_]+\b', exported)          # and no symbol of another library


def test_the_sources_are_a_library_of_their_own():
    from catint_amd import build
    others = (build.SOURCES + build.OBSERVE_SOURCES + build.BALANCE_SOURCES + build.REGRID_SOURCES + build.EQUIL_SOURCES + build.RESPONSE_SOURCES
              + build.KINETICS_SOURCES + build.COUPLE_SOURCES + build.SENS_SOURCES + build.DRC_SOURCES + build.MODES_SOURCES + build.SCFKIN_SOURCES
              + build.KINTRANS_SOURCES + build.EIS_SOURCES + build.INTERACT_SOURCES + build.VOLTAM_SOURCES)
    assert not any('catis' in s or 'iasweep' in s for s in others)
    assert os.path.dirname(build.IASWEEP_LIB) == os.path.dirname(build.LIB)
    assert build.IASWEEP_SOURCES == ['catis.hip'] and os.path.isdir(build.IASWEEP_DIR) and callable(build.iasweep_needs_build)
    # no name of this library carries one of the words the other libraries' tests forbid in foreign lists
    for name in build.IASWEEP_SOURCES + [os.path.basename(build.IASWEEP_DIR), os.path.basename(build.IASWEEP_LIB)]:
        assert not any(w in name for w in ('interact', 'catia', 'catkt', 'transient', 'catvm', 'voltam')), name
    listed = {os.path.realpath(p) for p in build.IASWEEP_HEADERS}
    for h in ('catint_iasweep.h', 'catint_voltam.h', 'catint_interact.h', 'catint_kinetics.h', 'catint_pnp.h'):
        assert os.path.realpath(os.path.join(ROOT, 'include', h)) in listed
    assert os.path.realpath(os.path.join(build.CSRC, 'pnp_kin.h')) in listed
    from tests.test_build_deps import reached
    sources = [os.path.join(build.IASWEEP_DIR, f) for f in build.IASWEEP_SOURCES]
    assert not reached(sources) - listed - {os.path.realpath(f) for f in sources}
    assert 'build_iasweep_library(' in open(os.path.join(ROOT, '__graft_entry__.py')).read()


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


MACROS = {'done': 'CATIS_DONE', 'input': 'CATIS_INPUT', 'steps': 'CATIS_STEPS', 'maxsteps': 'CATIS_MAX_STEPS', 'maxseg': 'CATIS_MAX_SEGMENTS',
          'maxsamples': 'CATIS_MAX_SAMPLES', 'startmaxit': 'CATIS_START_MAXIT', 'einval': 'CATIS_EINVAL', 'enomem': 'CATIS_ENOMEM',
          'edevice': 'CATIS_EDEVICE'}


@pytest.fixture(scope='module')
def compiler_layout(tmp_path_factory):
    structs = header_structs()
    assert set(PAIRS) <= set(structs)
    d = tmp_path_factory.mktemp('iasweep_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_iasweep.h"', 'int main(void) {']
    for s in PAIRS:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (s, s))
        for f in structs[s]:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    for name, macro in MACROS.items():
        lines.append('  printf("%s n %%d\\n", %s);' % (name, macro))
    lines.append('  printf("faraday %.17g x\\n", CATIS_FARADAY);')
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
    from catint_amd import iasweep
    cls = getattr(iasweep, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_of_the_binding_are_the_header_s(compiler_layout):
    from catint_amd import iasweep as v
    from catint_amd import voltammetry
    n = {name: compiler_layout[name]['n'] for name in MACROS}
    assert (v.DONE, v.INPUT, v.STEPS) == (n['done'], n['input'], n['steps']) == (SR.DONE, SR.INPUT, SR.STEPS) == (0, 2, 3)
    assert (v.MAX_STEPS, v.MAX_SEGMENTS, v.MAX_SAMPLES) == (n['maxsteps'], n['maxseg'], n['maxsamples']) == (1000000, 64, 4096)
    assert n['startmaxit'] == SR.START_MAXIT == 100
    assert (v.EINVAL, v.ENOMEM, v.EDEVICE) == (n['einval'], n['enomem'], n['edevice'])
    (faraday,) = compiler_layout['faraday'].values()
    assert faraday == v.FARADAY == SR.FARADAY == voltammetry.FARADAY
    assert v.START_RAMP == 10 and (v.DEFAULT_RTOL, v.DEFAULT_SEGMENTS, v.DEFAULT_SAMPLES) == (voltammetry.DEFAULT_RTOL, 2, 200)
    assert set(v.FIELDS) == set(voltammetry.FIELDS) | {'energy_shift'} and v.DEFAULT_FIELDS == voltammetry.DEFAULT_FIELDS


def ias(t=None, **kw):
    return ia(chain() if t is None else t, **kw)


@pytest.mark.parametrize('what, make, word', [
    # ---- what catvm_solve reports on the members the structs share ----
    ('struct_size of the parameters', lambda: (None, ias(), {'struct_size': 8}), 'catis_params.struct_size'),
    ('struct_size of the outputs', lambda: (None, ias(), {'out_struct_size': 8}), 'catis_outputs.struct_size'),
    ('struct_size of the view', lambda: (fake_view(size=12), ias(), dict(VIEW)), 'pnp_device_view.struct_size'),
    ('nine species', lambda: (None, ias(chain(N=9)), {}), '9 species'),
    ('seventeen steps', lambda: (None, ias(chain(R=17)), {}), '17 steps'),
    ('an order of 4', lambda: (None, ias(edit(chain(), f=poke('order_f', (0, 0), 4))), {}), 'order'),
    ('a step that does not conserve sites', lambda: (None, ias(edit(chain(), f=poke('order_f', (0, 2), 2))), {}), 'conserve'),
    ('an empty step', lambda: (None, ias(edit(chain(S=2, R=4), f=lambda t: (t['order_f'].__setitem__(3, 0), t['order_b'].__setitem__(3, 0),
                                                                           t['nu'].__setitem__(3, 0.0)))), {}), 'empty step'),
    ('a zero cref', lambda: (None, ias(edit(chain(), cref=np.array([1.0, 0.0]))), {}), 'cref[1]'),
    ('a zero site density', lambda: (None, ias(edit(chain(), site_density=0.0)), {}), 'site_density'),
    ('a site count of 4', lambda: (None, ias(edit(chain(), site_count=np.array([1.0, 4.0]))), {}), 'site count 1'),
    ('potential_drop 2', lambda: (None, ias(), {'potential_drop': 2}), 'potential_drop'),
    ('negative max_waves', lambda: (None, ias(), {'max_waves': -1}), 'max_waves'),
    ('a NaN in dG', lambda: (None, ias(edit(chain(), f=poke('dG', (1, 2), np.nan))), {}), 'step 1 has a non-finite'),
    ('a NaN nu', lambda: (None, ias(edit(chain(), f=poke('nu', (0, 0), np.nan))), {}), 'nu of step 0'),
    ('csurf without phi_surface', lambda: (None, ias(), {'phi_surface': None}), 'come together'),
    ('no view and no surface state', lambda: (None, ias(), dict(VIEW)), 'null view'),
    ('compat handle: no potential row', lambda: (fake_view(phi=None), ias(), dict(VIEW)), 'potential'),
    ('a lane outside the batch', lambda: (fake_view(), ias(), dict(VIEW, lanes=[0, 2])), 'lane index 2'),
    ('more points than lanes', lambda: (fake_view(B=1), ias(), dict(VIEW)), 'above the batch'),
    ('N different from the view', lambda: (fake_view(N=3), ias(), dict(VIEW)), 'the view has 3'),
    ('no sigma and an infinite capacitance', lambda: (None, ias(), {'stern_capacitance': np.inf}), 'surface charge'),
    ('a zero rtol', lambda: (None, ias(), {'rtol': 0.0}), 'rtol'),
    ('a NaN rtol', lambda: (None, ias(), {'rtol': np.nan}), 'rtol'),
    ('a zero newton_tol', lambda: (None, ias(), {'newton_tol': 0.0}), 'newton_tol'),
    ('a negative atol', lambda: (None, ias(), {'atol': -1e-12}), 'atol'),
    ('newton_maxit 0', lambda: (None, ias(), {'newton_maxit': 0}), 'newton_maxit'),
    ('max_steps 0', lambda: (None, ias(), {'max_steps': 0}), 'max_steps outside [1, 1000000]'),
    ('max_steps above the cap', lambda: (None, ias(), {'max_steps': 1000001}), 'max_steps outside [1, 1000000]'),
    ('a NaN h0', lambda: (None, ias(), {'h0': np.nan}), 'h0'),
    ('no electrons', lambda: (None, ias(), {'electrons': None}), 'electrons is required'),
    ('a NaN electron count', lambda: (None, ias(), {'electrons': [1.0, np.nan]}), 'electrons[1] is not finite'),
    ('no E_vertex', lambda: (None, ias(), {'E_vertex': None}), 'E_start, E_vertex and scan_rate are required'),
    ('no scan_rate', lambda: (None, ias(), {'scan_rate': None}), 'E_start, E_vertex and scan_rate are required'),
    ('a zero scan rate', lambda: (None, ias(), {'scan_rate': [0.1, 0.0]}), 'scan_rate[1] must be positive and finite'),
    ('a NaN scan rate', lambda: (None, ias(), {'scan_rate': [np.nan, 0.1]}), 'scan_rate[0] must be positive and finite'),
    ('no segment', lambda: (None, ias(), {'n_segments': 0}), 'n_segments outside [1, 64]'),
    ('65 segments', lambda: (None, ias(), {'n_segments': 65}), 'n_segments outside [1, 64]'),
    ('no sample', lambda: (None, ias(), {'samples': 0}), 'samples outside [1, 4096]'),
    ('4097 samples', lambda: (None, ias(), {'samples': 4097}), 'samples outside [1, 4096]'),
    ('a negative rate_floor', lambda: (None, ias(), {'rate_floor': -1.0}), 'rate_floor'),
    ('a NaN rate_floor', lambda: (None, ias(), {'rate_floor': np.nan}), 'rate_floor'),
    # ---- what catia_solve reports on the members it brings ----
    ('no site type', lambda: (None, ias(site_fraction=np.zeros(0)), {}), '0 site types'),
    ('four site types', lambda: (None, ias(chain(S=4), site_fraction=np.full(4, 0.25)), {}), '4 site types'),
    ('no adsorbate', lambda: (None, ias(chain(S=1), site_fraction=np.array([0.5, 0.5]), site_of=np.array([0, 1], np.int32)), {}), '0 adsorbates'),
    ('ten columns', lambda: (None, ias(chain(S=9)), {}), 'at most 9 columns'),
    ('a free site that takes two sites', lambda: (None, ias(edit(chain(), site_count=np.array([2.0, 1.0]))), {}), 'its site count 1'),
    ('a site_of out of range', lambda: (None, ias(chain(S=2), site_of=np.array([0, 0, 5], np.int32)), {}), 'site_of[2] = 5 outside'),
    ('a negative site_of', lambda: (None, ias(chain(S=2), site_of=np.array([0, -1, 0], np.int32)), {}), 'site_of[1] = -1 outside'),
    ('a free-site column on another type', lambda: (None, dict(two_types(), site_of=np.array([1, 0, 0, 1], np.int32)), {'electrons': np.ones(3)}),
     'free site of type 0'),
    ('a zero fraction', lambda: (None, dict(two_types(), site_fraction=np.array([1.0, 0.0])), {'electrons': np.ones(3)}), 'site_fraction[1]'),
    ('a NaN fraction', lambda: (None, ias(site_fraction=np.array([np.nan])), {}), 'site_fraction[0]'),
    ('a step that breaks the balance of a type', lambda: (None, two_types(broken=True), {'electrons': np.ones(3)}), 'conserve the sites of type 0'),
    ('a NaN in eps', lambda: (None, ias(chain(S=2), eps=np.array([[0.0, np.nan], [0.0, 0.0]])), {}), 'eps has a non-finite'),
    ('an infinite eps_ts', lambda: (None, ias(chain(S=2), eps_ts=np.array([[0.0, 0.0], [np.inf, 0.0], [0.0, 0.0]])), {}), 'eps_ts has a non-finite'),
    ('an infinite strength', lambda: (None, ias(), {'strength': np.inf}), 'strength'),
    ('a NaN strength', lambda: (None, ias(strength=np.nan), {}), 'strength'),
    ('start_ramp 0', lambda: (None, ias(), {'start_ramp': 0}), 'start_ramp < 1'),
    ('a third response', lambda: (None, ias(response=2), {}), 'response is'),
    ('piecewise without parameters', lambda: (None, ias(response='piecewise'), {}), 'needs cutoff and smoothing'),
    ('a zero smoothing', lambda: (None, ias(**dict(PIECEWISE, smoothing=np.zeros(1))), {}), 'positive, finite smoothing'),
    ('a NaN cutoff', lambda: (None, ias(**dict(PIECEWISE, cutoff=np.full(1, np.nan))), {}), 'finite cutoff'),
])
def test_validation_errors_come_before_any_device_call(solver, what, make, word):
    from catint_amd import iasweep
    view, tab, kw = make()
    of = np.asarray(tab['order_f'])
    N = of.shape[1] - len(tab['site_count'])
    args = sweep_args(N=max(N, 0), R=of.shape[0])
    args.update(kw)
    with pytest.raises(iasweep.IasweepError) as e:
        solver.sweep(view, tab, **args)
    assert e.value.code == iasweep.EINVAL, (what, str(e.value))
    assert word in str(e.value), (what, str(e.value))
    assert solver.last_kernel == '' and solver.last_kernel_ms == -1.0


def test_a_bad_program_or_hold_of_one_point_is_no_error_of_the_call(solver):
    """a non-finite E_vertex or a hold_time that is not a time is the point's CATIS_INPUT; with n = 0 behind it nothing is launched, so
    only the arguments of the call are judged here (the per-lane status is tests/test_gpu_iasweep.py's)"""
    out = solver.sweep(None, ias(), np.ones(2), np.zeros(0), np.zeros(0), np.zeros(0), csurf=np.zeros((0, 2)), phi_surface=np.zeros(0),
                       rate_floor=10.0, hold_time=np.zeros(0))
    assert out['status'].shape == (0,) and solver.last_kernel == ''


def test_the_python_layer_refuses_what_it_can_name(solver):
    from catint_amd import iasweep, voltammetry
    args = sweep_args()
    with pytest.raises(ValueError, match='electrons has 3 values'):
        solver.sweep(None, ias(), **dict(args, electrons=np.ones(3)))
    with pytest.raises(ValueError, match='scan_rate has 3 values'):
        solver.sweep(None, ias(), **dict(args, scan_rate=np.ones(3)))
    with pytest.raises(ValueError, match='hold_time has 3 values'):
        solver.sweep(None, ias(), **dict(args, hold_time=np.ones(3)))
    with pytest.raises(ValueError, match='needs kT'):
        solver.sweep(None, ias(), **dict(args, rate_floor=None))
    with pytest.raises(ValueError, match='unknown field'):
        solver.sweep(None, ias(), fields=('drift',), **args)
    with pytest.raises(ValueError, match='site_of has 3 values'):
        solver.sweep(None, ias(site_of=np.zeros(3, np.int32)), **args)
    assert solver.last_kernel == ''
    import catint_amd
    assert catint_amd.InteractingVoltammetry is iasweep.InteractingVoltammetry
    # the mean-field class still refuses the model
    with voltammetry.Voltammetry(0) as vm:
        with pytest.raises(ValueError, match='lateral interactions'):
            vm.sweep(None, ias(), **args)


def test_null_arguments_and_null_context(solver):
    from catint_amd import iasweep
    lib = iasweep.load_library()
    p = iasweep.CatisParams(struct_size=C.sizeof(iasweep.CatisParams))
    o = iasweep.CatisOutputs(struct_size=C.sizeof(iasweep.CatisOutputs))
    assert lib.catis_solve(solver._h, None, None, C.byref(o)) == iasweep.EINVAL
    assert b'null' in lib.catis_last_error(solver._h)
    assert lib.catis_solve(solver._h, None, C.byref(p), None) == iasweep.EINVAL
    assert lib.catis_solve(None, None, C.byref(p), C.byref(o)) == iasweep.EINVAL
    assert lib.catis_create(0, None) == iasweep.EINVAL
    assert lib.catis_last_kernel(solver._h) == b''


def test_no_point_makes_no_device_call(solver):
    """n == 0: valid, and done before the first device call (this machine may have no device at all); so is a call that asks for
    nothing"""
    from catint_amd import iasweep
    out = solver.sweep(None, two_types(), np.ones(3), np.zeros(0), np.zeros(0), np.zeros(0), n_segments=3, samples=5, csurf=np.zeros((0, 2)),
                       phi_surface=np.zeros(0), rate_floor=10.0, fields=list(iasweep.FIELDS), theta0=np.zeros((0, 4)))
    assert out['theta'].shape == (0, 15, 4) and out['flux'].shape == (0, 15, 2) and out['current'].shape == (0, 15)
    assert out['energy_shift'].shape == (0, 15, 2) and out['t_reached'].shape == (0,) and out['mean_current'].shape == (0, 15)
    assert out['status'].shape == (0,) and out['steps'].shape == (0, 4) and out['steps'].dtype == np.int32
    out = solver.sweep(fake_view(), ias(), np.ones(2), np.zeros(0), np.zeros(0), np.zeros(0), lanes=[], samples=1, n_segments=1, rate_floor=0.0,
                       fields=('flux_scale',))
    assert out['flux_scale'].shape == (0, 1, 2)
    # the mean-field tables alone are one site type without interactions
    out = solver.sweep(None, chain(S=3), np.ones(4), np.zeros(0), np.zeros(0), np.zeros(0), csurf=np.zeros((0, 2)), phi_surface=np.zeros(0),
                       rate_floor=1.0, fields=('theta', 'energy_shift'))
    assert out['theta'].shape == (0, 400, 4) and out['energy_shift'].shape == (0, 400, 3)
    assert solver.last_kernel == ''
    # n = 2 and every output NULL: nothing to do, no device call
    lib = iasweep.load_library()
    t = ias()
    keep = [np.ascontiguousarray(t[k], np.int32) for k in ('order_f', 'order_b', 'site_of')] + \
        [np.ascontiguousarray(t[k], float) for k in ('nu', 'cref', 'site_count', 'dG', 'Ea', 'lnA', 'site_fraction', 'eps')]
    es, ev, sr, ne, cs, ps = np.ones(2), np.zeros(2), np.ones(2), np.ones(2), np.zeros((2, 2)), np.zeros(2)
    d = iasweep._dptr
    p = iasweep.CatisParams(struct_size=C.sizeof(iasweep.CatisParams), nspecies=2, nadsorbates=1, nsteps=2, newton_maxit=8, max_steps=10, n=2,
                            nsitetypes=1, start_ramp=1, strength=1.0, site_density=1e-5, rtol=1e-3, newton_tol=1e-10, n_segments=1, samples=2,
                            E_start=d(es), E_vertex=d(ev), scan_rate=d(sr), electrons=d(ne), csurf=d(cs), phi_surface=d(ps))
    p.order_f, p.order_b, p.site_of = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in keep[:3])
    p.nu, p.cref, p.site_count, p.dG, p.Ea, p.lnA, p.site_fraction, p.eps = (d(a) for a in keep[3:])
    o = iasweep.CatisOutputs(struct_size=C.sizeof(iasweep.CatisOutputs))
    assert lib.catis_solve(solver._h, None, C.byref(p), C.byref(o)) == 0
    assert lib.catis_last_kernel(solver._h) == b''


def test_the_library_holds_the_one_kernel(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)


# ---- the routing, with fakes ---------------------------------------------------------------------------------------------------------
class FakeSweeper(object):
    opened = []

    def __init__(self, device=0):
        self.device, self.calls, self.closed = device, [], False
        type(self).opened.append(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.closed = True

    def sweep(self, view, tables, electrons, E_start, E_vertex, scan_rate, **kw):
        self.calls.append(dict(kw, view=view, tables=tables, electrons=electrons, E_start=E_start, E_vertex=E_vertex, scan_rate=scan_rate))
        return {'status': np.zeros(len(E_start), np.int32)}


def test_the_solver_routes_an_interacting_model_to_the_new_class(monkeypatch):
    from catint_amd import _capi, iasweep, voltammetry
    from tests.interact_cases import co2r_model as interacting
    from tests.kinetics_cases import co2r_model as mean_field

    class FakeNew(FakeSweeper):
        opened = []

    class FakeOld(FakeSweeper):
        opened = []
    monkeypatch.setattr(iasweep, 'InteractingVoltammetry', FakeNew)
    monkeypatch.setattr(voltammetry, 'Voltammetry', FakeOld)
    s = object.__new__(_capi.PnpSolver)          # no handle: the host-surface path needs none
    s.B, s._obs = 2, dict(device=3, stern_capacitance=0.2, phi_pzc=0.1, phiM=None)
    host = dict(csurf=np.ones((2, 3)), phi_surface=np.zeros(2))
    ia_model, mf_model = interacting('one_site', 0.3, 0.15), mean_field('one_site')
    s.get_voltammogram(ia_model, [-0.6, -0.6], -1.0, [0.1, 1.0], hold_time=[1.0, 2.0], start_ramp=4, **host)
    assert len(FakeNew.opened) == 1 and not FakeOld.opened
    (ctx,) = FakeNew.opened
    (call,) = ctx.calls
    assert ctx.device == 3 and ctx.closed and call['view'] is None and call['hold_time'] == [1.0, 2.0] and call['start_ramp'] == 4
    assert 'eps' in call['tables'] and call['stern_capacitance'] == 0.2 and call['phi_pzc'] == 0.1
    assert np.array_equal(call['electrons'], ia_model.electrons()) and call['kT'] == ia_model.kT
    s.get_voltammogram(ia_model.tables(), [-0.6, -0.6], -1.0, [0.1, 1.0], electrons=ia_model.electrons(), kT=ia_model.kT, **host)
    assert len(FakeNew.opened) == 2 and FakeNew.opened[1].calls[0]['start_ramp'] is None and FakeNew.opened[1].closed
    s.get_voltammogram(mf_model, [-0.6, -0.6], -1.0, [0.1, 1.0], **host)
    assert len(FakeNew.opened) == 2 and len(FakeOld.opened) == 1 and FakeOld.opened[0].closed
    assert 'hold_time' not in FakeOld.opened[0].calls[0] and 'start_ramp' not in FakeOld.opened[0].calls[0]
    for more in (dict(hold_time=1.0), dict(start_ramp=3)):
        with pytest.raises(ValueError, match='hold_time and start_ramp belong'):
            s.get_voltammogram(mf_model, [-0.6, -0.6], -1.0, [0.1, 1.0], **host, **more)
    assert len(_capi.PnpSolver.SATELLITES) == 13 and not [k for k in _capi.PnpSolver.SATELLITES if 'iasweep' in k]
    assert not [k for k in _capi.SYMBOLS if 'catis' in k]
