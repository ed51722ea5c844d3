"""libcatint_kintrans without a GPU (the method of tests/test_kinetics_abi.py): the library builds for gfx950 and exports what
include/catint_kintrans.h declares, the ctypes mirrors have the compiler's layouts, every validation error is returned before any
device call, no point makes no device call, the library holds the one kernel.  The rescue of catint_amd._kintrans and the
calculator's opt-in are driven with the CPU restatements in the place of the two device contexts."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import kernel_census as K
from tests import kinetics_ref as KR
from tests import kintrans_cases as KC
from tests import kintrans_ref as KT
from tests.test_kinetics_abi import chain, edit, fake_view, host_args, poke

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {'catkt_params': 'CatktParams', 'catkt_outputs': 'CatktOutputs'}
INSTANCES = {'catkt::transient_kernel'}


@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_kintrans_library
    return build_kintrans_library()


@pytest.fixture(scope='module')
def solver(libpath):
    from catint_amd import _kintrans
    with _kintrans.TransientKinetics(0) as o:
        yield o


def header_source():
    src = open(os.path.join(ROOT, 'include', 'catint_kintrans.h')).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    from catint_amd import _kintrans
    declared = sorted(set(re.findall(r'\b(catkt_[a-z0-9_]+)\s*\(', header_source())))
    assert declared == sorted(_kintrans.SYMBOLS) and len(declared) == 6
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(catkt_[a-z0-9_]+)\b', exported))) == declared
    assert not re.findall(r'\b(pnp|catkin)_[a-z0-9_]+\b', exported)          # and no symbol of another library


def test_the_sources_are_a_library_of_their_own():
    from catint_amd import build
    others = (build.SOURCES + build.OBSERVE_SOURCES + build.BALANCE_SOURCES + build.REGRID_SOURCES + build.EQUIL_SOURCES + build.RESPONSE_SOURCES
              + build.KINETICS_SOURCES + build.COUPLE_SOURCES + build.SENS_SOURCES + build.DRC_SOURCES + build.MODES_SOURCES + build.SCFKIN_SOURCES)
    assert not any('catkt' in s or 'kintrans' in s for s in others)
    assert os.path.dirname(build.KINTRANS_LIB) == os.path.dirname(build.LIB)
    assert build.KINTRANS_SOURCES == ['catkt.hip'] and os.path.isdir(build.KINTRANS_DIR) and callable(build.kintrans_needs_build)
    listed = {os.path.realpath(p) for p in build.KINTRANS_HEADERS}
    for h in ('catint_kintrans.h', 'catint_kinetics.h', 'catint_pnp.h'):
        assert os.path.realpath(os.path.join(ROOT, 'include', h)) in listed
    assert os.path.realpath(os.path.join(build.CSRC, 'pnp_kin.h')) in listed
    from tests.test_build_deps import reached
    sources = [os.path.join(build.KINTRANS_DIR, f) for f in build.KINTRANS_SOURCES]
    assert not reached(sources) - listed - {os.path.realpath(f) for f in sources}
    assert 'build_kintrans_library(' in open(os.path.join(ROOT, '__graft_entry__.py')).read()


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


MACROS = {'done': 'CATKT_DONE', 'steady': 'CATKT_STEADY', 'input': 'CATKT_INPUT', 'steps': 'CATKT_STEPS', 'maxsteps': 'CATKT_MAX_STEPS',
          'einval': 'CATKT_EINVAL', 'enomem': 'CATKT_ENOMEM', 'edevice': 'CATKT_EDEVICE'}


@pytest.fixture(scope='module')
def compiler_layout(tmp_path_factory):
    structs = header_structs()
    assert set(PAIRS) <= set(structs)
    d = tmp_path_factory.mktemp('kintrans_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_kintrans.h"', 'int main(void) {']
    for s in PAIRS:
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


@pytest.mark.parametrize('cname', sorted(PAIRS))
def test_ctypes_mirror_matches_the_compiler(cname, compiler_layout):
    from catint_amd import _kintrans
    cls = getattr(_kintrans, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_of_the_binding_are_the_header_s(compiler_layout):
    from catint_amd import _kintrans as k
    n = {name: compiler_layout[name]['n'] for name in MACROS}
    assert (k.DONE, k.STEADY, k.INPUT, k.STEPS) == (n['done'], n['steady'], n['input'], n['steps']) == (KT.DONE, KT.STEADY, KT.INPUT, KT.STEPS)
    assert k.MAX_STEPS == n['maxsteps'] == 1000000
    assert (k.EINVAL, k.ENOMEM, k.EDEVICE) == (n['einval'], n['enomem'], n['edevice'])
    # the defaults the issue names, and those of the restatement
    assert (k.DEFAULT_MAX_STEPS, k.DEFAULT_NEWTON_MAXIT) == (20000, 8)
    d = KT.DEFAULTS
    assert (k.DEFAULT_RTOL, k.DEFAULT_ATOL, k.DEFAULT_NEWTON_TOL, k.DEFAULT_NEWTON_MAXIT, k.DEFAULT_MAX_STEPS) == (
        d['rtol'], d['atol'], d['newton_tol'], d['newton_maxit'], d['max_steps'])
    assert (k.RESCUE_T_OUT, k.RESCUE_RTOL, k.RESCUE_STEADY_TOL) == (KC.RESCUE_T_OUT[0], KC.RESCUE_OPTS['rtol'], KC.RESCUE_OPTS['steady_tol'])


VIEW = {'csurf': None, 'phi_surface': None}


@pytest.mark.parametrize('what, make, word', [
    # ---- what catkin_solve checks ----
    ('struct_size of the parameters', lambda: (None, chain(), {'struct_size': 8}), 'catkt_params.struct_size'),
    ('struct_size of the outputs', lambda: (None, chain(), {'out_struct_size': 8}), 'catkt_outputs.struct_size'),
    ('struct_size of the view', lambda: (fake_view(size=12), chain(), dict(VIEW)), 'pnp_device_view.struct_size'),
    ('nine species', lambda: (None, chain(N=9), host_args(N=9)), '9 species'),
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
    # ---- what catkt_solve adds ----
    ('no t_out', lambda: (None, chain(), {'t_out': None}), 'n_out < 1'),
    ('an empty t_out', lambda: (None, chain(), {'t_out': []}), 'n_out < 1'),
    ('a zero output time', lambda: (None, chain(), {'t_out': [0.0, 1.0]}), 't_out[0] must be positive'),
    ('a negative output time', lambda: (None, chain(), {'t_out': [-1.0]}), 't_out[0] must be positive'),
    ('an infinite output time', lambda: (None, chain(), {'t_out': [1.0, np.inf]}), 't_out[1] must be positive and finite'),
    ('a NaN output time', lambda: (None, chain(), {'t_out': [1.0, np.nan, 3.0]}), 't_out[1] must be positive and finite'),
    ('equal output times', lambda: (None, chain(), {'t_out': [1.0, 2.0, 2.0]}), 'not strictly increasing at index 2'),
    ('decreasing output times', lambda: (None, chain(), {'t_out': [2.0, 1.0]}), 'not strictly increasing at index 1'),
    ('a zero rtol', lambda: (None, chain(), {'rtol': 0.0}), 'rtol'),
    ('an infinite rtol', lambda: (None, chain(), {'rtol': np.inf}), 'rtol'),
    ('a NaN rtol', lambda: (None, chain(), {'rtol': np.nan}), 'rtol'),
    ('a zero newton_tol', lambda: (None, chain(), {'newton_tol': 0.0}), 'newton_tol'),
    ('a NaN newton_tol', lambda: (None, chain(), {'newton_tol': np.nan}), 'newton_tol'),
    ('a negative atol', lambda: (None, chain(), {'atol': -1e-12}), 'atol'),
    ('a NaN atol', lambda: (None, chain(), {'atol': np.nan}), 'atol'),
    ('a negative steady_tol', lambda: (None, chain(), {'steady_tol': -1.0}), 'steady_tol'),
    ('a NaN steady_tol', lambda: (None, chain(), {'steady_tol': np.nan}), 'steady_tol'),
    ('newton_maxit 0', lambda: (None, chain(), {'newton_maxit': 0}), 'newton_maxit'),
    ('max_steps 0', lambda: (None, chain(), {'max_steps': 0}), 'max_steps outside [1, 1000000]'),
    ('max_steps above the cap', lambda: (None, chain(), {'max_steps': 1000001}), 'max_steps outside [1, 1000000]'),
    ('a NaN h0', lambda: (None, chain(), {'h0': np.nan}), 'h0'),
])
def test_validation_errors_come_before_any_device_call(solver, what, make, word):
    from catint_amd import _kintrans
    view, tab, kw = make()
    N = np.asarray(tab['order_f']).shape[1] - len(tab['site_count'])
    args = dict(host_args(N=max(N, 0)), t_out=[1.0, 2.0])
    args.update(kw)
    with pytest.raises(_kintrans.KintransError) as e:
        solver.solve(view, tab, **args)
    assert e.value.code == _kintrans.EINVAL, (what, str(e.value))
    assert word in str(e.value), (what, str(e.value))
    assert solver.last_kernel == '' and solver.last_kernel_ms == -1.0


def test_null_arguments_and_null_context(solver):
    from catint_amd import _kintrans
    lib = _kintrans.load_library()
    p = _kintrans.CatktParams(struct_size=C.sizeof(_kintrans.CatktParams))
    o = _kintrans.CatktOutputs(struct_size=C.sizeof(_kintrans.CatktOutputs))
    assert lib.catkt_solve(solver._h, None, None, C.byref(o)) == _kintrans.EINVAL
    assert b'null' in lib.catkt_last_error(solver._h)
    assert lib.catkt_solve(solver._h, None, C.byref(p), None) == _kintrans.EINVAL
    assert lib.catkt_solve(None, None, C.byref(p), C.byref(o)) == _kintrans.EINVAL
    assert lib.catkt_create(0, None) == _kintrans.EINVAL
    assert lib.catkt_last_kernel(solver._h) == b''


def test_no_point_makes_no_device_call(solver):
    """n == 0: valid, and done before the first device call (this machine may have no device at all); so is a call that asks for
    nothing"""
    out = solver.solve(None, chain(S=2), np.zeros(0), [1.0, 2.0, 3.0], csurf=np.zeros((0, 2)), phi_surface=np.zeros(0))
    assert out['theta'].shape == (0, 3, 3) and out['flux'].shape == (0, 3, 2) and out['drift'].shape == (0, 3) and out['t_reached'].shape == (0,)
    assert out['status'].shape == (0,) and out['steps'].shape == (0, 3) and out['steps'].dtype == np.int32
    out = solver.solve(fake_view(), chain(), np.zeros(0), [1.0], lanes=[])
    assert out['flux_scale'].shape == (0, 1, 2)
    assert solver.last_kernel == ''
    from catint_amd import _kintrans
    lib = _kintrans.load_library()
    t = chain()
    keep = [np.ascontiguousarray(t[k], np.int32) for k in ('order_f', 'order_b')] + [np.ascontiguousarray(t[k], float) for k in
                                                                                      ('nu', 'cref', 'site_count', 'dG', 'Ea', 'lnA')]
    pm, cs, ps, tt = np.zeros(2), np.zeros((2, 2)), np.zeros(2), np.array([1.0])
    p = _kintrans.CatktParams(struct_size=C.sizeof(_kintrans.CatktParams), nspecies=2, nadsorbates=1, nsteps=2, newton_maxit=8, max_steps=10, n=2,
                              site_density=1e-5, rtol=1e-3, newton_tol=1e-10, n_out=1, t_out=_kintrans._dptr(tt), phiM=_kintrans._dptr(pm),
                              csurf=_kintrans._dptr(cs), phi_surface=_kintrans._dptr(ps))
    p.order_f, p.order_b = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in keep[:2])
    p.nu, p.cref, p.site_count, p.dG, p.Ea, p.lnA = (_kintrans._dptr(a) for a in keep[2:])
    o = _kintrans.CatktOutputs(struct_size=C.sizeof(_kintrans.CatktOutputs))
    assert lib.catkt_solve(solver._h, None, C.byref(p), C.byref(o)) == 0          # every output NULL: nothing to do
    assert lib.catkt_last_kernel(solver._h) == b''


def test_the_library_holds_the_one_kernel(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)


def test_the_kinetics_libraries_gained_no_kernel_and_no_symbol():
    from catint_amd import build as B
    for f, lib, names in ((B.build_kinetics_library, B.KINETICS_LIB, {'catkin::steady_kernel'}),):
        f()
        try:
            assert K.compiled_kernels(lib=lib) == names
        except K.CensusUnavailable as e:
            pytest.fail('kernel census unavailable: %s' % e)
    from catint_amd import _capi
    assert not [s for s in _capi.SYMBOLS if 'catkt' in s or 'transient' in s]
    assert hasattr(_capi.PnpSolver, 'get_kinetics_transient')


# ---- the rescue, with the CPU restatements in the place of the two device contexts ---------------------------------------------------
class FakeKinetics(object):
    def __init__(self):
        self.calls = []

    def solve(self, view, tab, phiM, csurf=None, phi_surface=None, potential_drop='stern', stern_capacitance=0.0, phi_pzc=0.0, theta_guess=None,
              fields=None, tol=1e-12, maxit=200, **kw):
        assert view is None and not {k for k, v in kw.items() if v is not None} - {'max_waves'}
        r = KR.solve_fp64(tab, phiM, csurf, phi_surface, w=1 if potential_drop == 'stern' else 0, CS=stern_capacitance, phi_pzc=phi_pzc,
                          theta_guess=theta_guess, tol=tol, maxit=maxit, sens=False)
        self.calls.append(dict(n=len(r['status']), guess=None if theta_guess is None else np.array(theta_guess), phiM=np.array(phiM)))
        return {k: np.array(r[k]) for k in tuple(fields) + ('status', 'iterations')}


class FakeTransient(object):
    def __init__(self):
        self.calls, self.closed = [], False

    def solve(self, view, tab, phiM, t_out, csurf=None, phi_surface=None, potential_drop='stern', stern_capacitance=0.0, phi_pzc=0.0, theta0=None,
              fields=None, max_waves=0, **opts):
        assert view is None and theta0 is None
        r = KT.solve(tab, phiM, csurf, phi_surface, t_out, w=1 if potential_drop == 'stern' else 0, CS=stern_capacitance, phi_pzc=phi_pzc, **opts)
        self.calls.append(dict(n=len(r['status']), t_out=list(t_out), opts=opts, phiM=np.array(phiM)))
        return {k: np.array(r[k]) for k in tuple(fields) + ('status', 'steps')}

    def close(self):
        self.closed = True


def kw_of(c):
    return dict(potential_drop='stern' if c.kw['w'] else 'full', stern_capacitance=c.kw['CS'], phi_pzc=c.kw['phi_pzc'])


@pytest.mark.parametrize('name', KC.RESCUE_NAMES)
def test_rescue_replaces_exactly_the_failed_rows(name):
    from catint_amd import _kintrans
    c = KC.case(name)
    kin, tr = FakeKinetics(), FakeTransient()
    kw = dict(kw_of(c), fields=('theta', 'flux', 'flux_scale'))
    first = kin.solve(None, c.tables, c.phiM, csurf=c.csurf, phi_surface=c.phi_surface, **kw)
    failed = first['status'] == 1
    assert failed.any()
    res = {k: v.copy() for k, v in first.items()}
    out = _kintrans.rescue(kin, tr, None, c.tables, c.phiM, res, per_point=dict(csurf=c.csurf, phi_surface=c.phi_surface, gamma=None), **kw)
    assert out is res and out['rescued'].dtype == bool and np.array_equal(out['rescued'], failed)
    assert (out['status'] == 0).all()
    # only the failed points were integrated, with the rescue's settings, and solved again from where they ended
    assert len(tr.calls) == 1 and tr.calls[0]['n'] == failed.sum() and tr.calls[0]['t_out'] == [1e12]
    assert tr.calls[0]['opts'] == dict(rtol=1e-2, steady_tol=1e-6) and np.array_equal(tr.calls[0]['phiM'], c.phiM[failed])
    assert len(kin.calls) == 2 and kin.calls[1]['n'] == failed.sum() and kin.calls[1]['guess'] is not None
    ref = KC.reference(name)
    assert np.array_equal(kin.calls[1]['guess'], ref['theta'][failed, 0])
    for k in ('theta', 'flux', 'flux_scale', 'iterations'):
        assert np.array_equal(out[k][~failed], first[k][~failed]), k
    assert (out['iterations'][failed] <= 3).all()
    assert np.abs((out['theta'] * c.tables['site_count']).sum(axis=1) - 1.0).max() <= 1e-14


def test_rescue_leaves_a_result_without_failures_alone():
    from catint_amd import _kintrans

    class Never(object):
        def solve(self, *a, **k):
            raise AssertionError('nothing failed: no integration')
    c = KC.case('random_S3')
    kin = FakeKinetics()
    kw = dict(kw_of(c), fields=('theta',))
    first = kin.solve(None, c.tables, c.phiM, csurf=c.csurf, phi_surface=c.phi_surface, **kw)
    res = {k: v.copy() for k, v in first.items()}
    _kintrans.rescue(kin, Never(), None, c.tables, c.phiM, res, per_point=dict(csurf=c.csurf, phi_surface=c.phi_surface), **kw)
    assert not res['rescued'].any() and len(kin.calls) == 1
    for k in first:
        assert np.array_equal(res[k], first[k])


def test_a_point_whose_second_solve_fails_keeps_its_first_rows():
    from catint_amd import _kintrans
    c = KC.case('rescue_S3')

    class Stubborn(FakeKinetics):
        def solve(self, *a, **k):
            out = FakeKinetics.solve(self, *a, **k)
            if len(self.calls) == 2:
                out['status'][0] = 3
                out['theta'][0] = -1.0
            return out
    kin, tr = Stubborn(), FakeTransient()
    kw = dict(kw_of(c), fields=('theta',))
    first = kin.solve(None, c.tables, c.phiM, csurf=c.csurf, phi_surface=c.phi_surface, **kw)
    res = {k: v.copy() for k, v in first.items()}
    _kintrans.rescue(kin, tr, None, c.tables, c.phiM, res, per_point=dict(csurf=c.csurf, phi_surface=c.phi_surface), **kw)
    assert list(res['rescued']) == [False, True, True, True] and list(res['status']) == [1, 0, 0, 0]
    assert np.array_equal(res['theta'][0], first['theta'][0]) and res['iterations'][0] == first['iterations'][0]


# ---- the calculator's opt-in -------------------------------------------------------------------------------------------------------
def test_the_calculator_passes_rescue_to_the_host_loops_only(monkeypatch):
    from catint_amd.calculator import Calculator, CalculatorError
    from tests.test_kinetics_abi import FakeKinetics as LoopKinetics, scf_parts
    tp, model, transport_fn = scf_parts()
    calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-9)
    with pytest.raises(CalculatorError, match='device loop'):
        calc.set_microkinetics(model, device_loop=True, rescue=True)
    calc.set_microkinetics(model, site_density=2e-6)
    assert 'rescue' not in calc.microkinetics
    calc.set_microkinetics(model, site_density=2e-6, rescue=True)
    assert calc.microkinetics['rescue'] is True
    # lane 1 fails in iteration 2: it is integrated and solved again instead of leaving the loop as failed
    fake, trans = LoopKinetics(), []

    def solve(view, tab, phiM, _fake=fake, **kw):
        out = LoopKinetics.solve(_fake, view, tab, phiM, **kw)
        if len(_fake.calls) == 2:
            out['status'] = out['status'].copy()
            out['status'][1] = 1
            out['flux'] = 1e3 * out['flux']
        return out
    fake.solve = solve

    def transient():
        trans.append(FakeTransient())
        return trans[-1]
    monkeypatch.setattr(calc, '_kinetics_solver', lambda: fake)
    monkeypatch.setattr(calc, '_transient_solver', transient)
    out = calc.run_scf_cycle(transport_fn=transport_fn, max_iter=200)
    assert out['converged'].all() and not out['failed'].any() and (out['kinetic_status'] == 0).all()
    assert len(trans) == 1 and trans[0].closed and trans[0].calls[0]['n'] == 1
    # without the option the same failure ends the lane
    tp, model, transport_fn = scf_parts()
    calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-9)
    calc.set_microkinetics(model, site_density=2e-6)
    fake2 = LoopKinetics()
    fake2.solve = lambda view, tab, phiM, **kw: solve(view, tab, phiM, _fake=fake2, **kw)
    monkeypatch.setattr(calc, '_kinetics_solver', lambda: fake2)
    monkeypatch.setattr(calc, '_transient_solver', lambda: pytest.fail('no rescue was asked for'))
    out = calc.run_scf_cycle(transport_fn=transport_fn, max_iter=200)
    assert list(out['failed']) == [False, True, False]
