"""libcatint_iacontrol without a GPU (the checks of tests/test_drc_abi.py and tests/test_interact_abi.py, carried over): the library
builds for gfx950 and exports what include/catint_iacontrol.h declares, the ctypes mirrors have the compiler's layouts, every validation
error of both parents is returned before any device call, no point makes no device call, the library holds the one kernel, the build
lists are complete, and PnpSolver.get_rate_control sends an interacting model to the new class and a mean-field model to its
satellite."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import kernel_census as K
from tests.test_interact_abi import PIECEWISE, ia, two_types
from tests.test_kinetics_abi import chain, edit, fake_view, poke

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {'catic_params': 'CaticParams', 'catic_outputs': 'CaticOutputs'}
INSTANCES = {'catic::control_kernel'}
VIEW = {'csurf': None, 'phi_surface': None}


@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_iacontrol_library
    return build_iacontrol_library()


@pytest.fixture(scope='module')
def solver(libpath):
    from catint_amd import iacontrol
    with iacontrol.InteractingRateControl(0) as o:
        yield o


def header_source():
    src = open(os.path.join(ROOT, 'include', 'catint_iacontrol.h')).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    from catint_amd import iacontrol
    declared = sorted(set(re.findall(r'\b(catic_[a-z0-9_]+)\s*\(', header_source())))
    assert declared == sorted(iacontrol.SYMBOLS) and len(declared) == 6
    assert declared == sorted('catic_' + s for s in ('create', 'destroy', 'last_error', 'last_kernel', 'last_kernel_ms', 'solve'))
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(catic_[a-z0-9_]+)\b', exported))) == declared
    assert not re.findall(r'\b(pnp|catkin|catdrc|catia|catis)_[a-z0-9_]+\b', exported)          # and no symbol of another library


def test_the_sources_are_a_library_of_their_own():
    from catint_amd import build
    others = (build.SOURCES + build.OBSERVE_SOURCES + build.BALANCE_SOURCES + build.REGRID_SOURCES + build.EQUIL_SOURCES + build.RESPONSE_SOURCES
              + build.KINETICS_SOURCES + build.COUPLE_SOURCES + build.SENS_SOURCES + build.DRC_SOURCES + build.MODES_SOURCES + build.SCFKIN_SOURCES
              + build.KINTRANS_SOURCES + build.EIS_SOURCES + build.INTERACT_SOURCES + build.VOLTAM_SOURCES + build.IASWEEP_SOURCES)
    assert not any('catic' in s or 'iacontrol' in s for s in others)
    assert os.path.dirname(build.IACONTROL_LIB) == os.path.dirname(build.LIB)
    assert build.IACONTROL_SOURCES == ['catic.hip'] and os.path.isdir(build.IACONTROL_DIR) and callable(build.iacontrol_needs_build)
    # no name of this library carries one of the words the other libraries' tests forbid in foreign lists
    for name in build.IACONTROL_SOURCES + [os.path.basename(build.IACONTROL_DIR), os.path.basename(build.IACONTROL_LIB)]:
        assert not any(w in name for w in ('interact', 'catia', 'catkt', 'transient', 'catvm', 'voltam', 'catis', 'iasweep', 'drc')), name
    listed = {os.path.realpath(p) for p in build.IACONTROL_HEADERS}
    for h in ('catint_iacontrol.h', 'catint_pnp.h'):
        assert os.path.realpath(os.path.join(ROOT, 'include', h)) in listed
    assert os.path.realpath(os.path.join(build.CSRC, 'pnp_kin.h')) in listed
    from tests.test_build_deps import reached
    sources = [os.path.join(build.IACONTROL_DIR, f) for f in build.IACONTROL_SOURCES]
    assert not reached(sources) - listed - {os.path.realpath(f) for f in sources}
    assert 'build_iacontrol_library(' in open(os.path.join(ROOT, '__graft_entry__.py')).read()


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


MACROS = {'ok': 'CATIC_OK_POINT', 'residual': 'CATIC_RESIDUAL', 'input': 'CATIC_INPUT', 'pivot': 'CATIC_PIVOT', 'einval': 'CATIC_EINVAL',
          'enomem': 'CATIC_ENOMEM', 'edevice': 'CATIC_EDEVICE', 'types': 'CATIC_MAX_SITE_TYPES', 'columns': 'CATIC_MAX_COLUMNS',
          'linear': 'CATIC_LINEAR', 'piecewise': 'CATIC_PIECEWISE'}


@pytest.fixture(scope='module')
def compiler_layout(tmp_path_factory):
    structs = header_structs()
    assert set(PAIRS) <= set(structs)
    d = tmp_path_factory.mktemp('iacontrol_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_iacontrol.h"', '#include "catint_drc.h"', '#include "catint_interact.h"',
             'int main(void) {']
    for s in PAIRS:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (s, s))
        for f in structs[s]:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    for name, macro in MACROS.items():
        lines.append('  printf("%s n %%d\\n", %s);' % (name, macro))
        for other in ('CATDRC_', 'CATIA_'):          # the values are the parents'
            lines.append('#ifdef %s\n  printf("%s same %%d\\n", %s == %s);\n#endif' % ((macro.replace('CATIC_', other),) + (name, macro, macro.replace('CATIC_', other))))
    lines += ['  return 0;', '}']
    (d / 'abi.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(d / 'abi.c'), '-o', str(d / 'abi')])
    layout = {}
    for line in subprocess.check_output([str(d / 'abi')]).decode().splitlines():
        s, f, v = line.split()
        if f == 'same':
            assert int(v) == 1, s
        else:
            layout.setdefault(s, {})[f] = int(v)
    return layout


@pytest.mark.parametrize('cname', sorted(PAIRS))
def test_ctypes_mirror_matches_the_compiler(cname, compiler_layout):
    from catint_amd import iacontrol
    cls = getattr(iacontrol, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_of_the_binding_are_the_header_s(compiler_layout):
    from catint_amd import _drc, iacontrol as v
    n = {name: compiler_layout[name]['n'] for name in MACROS}
    assert (v.OK_POINT, v.RESIDUAL, v.INPUT, v.PIVOT) == (n['ok'], n['residual'], n['input'], n['pivot']) == (0, 1, 2, 3)
    assert (v.EINVAL, v.ENOMEM, v.EDEVICE) == (n['einval'], n['enomem'], n['edevice'])
    assert (v.MAX_SITE_TYPES, v.MAX_COLUMNS) == (n['types'], n['columns']) and v.RESPONSE == {'linear': n['linear'], 'piecewise': n['piecewise']}
    assert set(v.FIELDS) == set(_drc.FIELDS) | {'dflux_dstrength', 'dy_dstrength', 'strength_control'}
    assert set(v.DEFAULT_FIELDS) == set(_drc.DEFAULT_FIELDS) | {'strength_control', 'dflux_dstrength'}
    assert v.DEFAULT_RESIDUAL_TOL == _drc.DEFAULT_RESIDUAL_TOL


def args_for(tab, n=2):
    of = np.asarray(tab['order_f'])
    T = len(tab['site_count'])
    N = max(of.shape[1] - T, 0)
    return dict(phiM=np.linspace(-0.1, -0.3, n), theta=np.full((n, T), 1.0 / max(T, 1)), csurf=np.full((n, N), 0.5), phi_surface=np.zeros(n))


def iac(t=None, **kw):
    return ia(chain() if t is None else t, **kw)


@pytest.mark.parametrize('what, make, word', [
    # ---- what catdrc_solve reports on the members the structs share, and for the state and the points ----
    ('struct_size of the parameters', lambda: (None, iac(), {'struct_size': 8}), 'catic_params.struct_size'),
    ('struct_size of the outputs', lambda: (None, iac(), {'out_struct_size': 8}), 'catic_outputs.struct_size'),
    ('struct_size of the view', lambda: (fake_view(size=12), iac(), dict(VIEW)), 'pnp_device_view.struct_size'),
    ('nine species', lambda: (None, iac(chain(N=9)), {}), '9 species'),
    ('no step', lambda: (None, iac(edit(chain(), order_f=np.zeros((0, 4), np.int32), order_b=np.zeros((0, 4), np.int32), nu=np.zeros((0, 2)),
                                        dG=np.zeros((0, 4)), Ea=np.zeros((0, 4)), lnA=np.zeros(0))), {}), '0 steps'),
    ('seventeen steps', lambda: (None, iac(chain(R=17)), {}), '17 steps'),
    ('an order of 4', lambda: (None, iac(edit(chain(), f=poke('order_f', (0, 0), 4))), {}), 'order'),
    ('a step that does not conserve sites', lambda: (None, iac(edit(chain(), f=poke('order_f', (0, 2), 2))), {}), 'conserve'),
    ('an empty step', lambda: (None, iac(edit(chain(S=2, R=4), f=lambda t: (t['order_f'].__setitem__(3, 0), t['order_b'].__setitem__(3, 0),
                                                                           t['nu'].__setitem__(3, 0.0)))), {}), 'empty step'),
    ('a zero cref', lambda: (None, iac(edit(chain(), cref=np.array([1.0, 0.0]))), {}), 'cref[1]'),
    ('a zero site density', lambda: (None, iac(edit(chain(), site_density=0.0)), {}), 'site_density'),
    ('a site count of 4', lambda: (None, iac(edit(chain(), site_count=np.array([1.0, 4.0]))), {}), 'site count 1'),
    ('potential_drop 2', lambda: (None, iac(), {'potential_drop': 2}), 'potential_drop'),
    ('negative max_waves', lambda: (None, iac(), {'max_waves': -1}), 'max_waves'),
    ('a NaN in dG', lambda: (None, iac(edit(chain(), f=poke('dG', (1, 2), np.nan))), {}), 'step 1 has a non-finite'),
    ('an infinite e1', lambda: (None, iac(edit(chain(), f=poke('Ea', (0, 1), -np.inf))), {}), 'step 0 has a non-finite'),
    ('a NaN nu', lambda: (None, iac(edit(chain(), f=poke('nu', (0, 0), np.nan))), {}), 'nu of step 0'),
    ('a zero residual_tol', lambda: (None, iac(), {'residual_tol': 0.0}), 'residual_tol'),
    ('a NaN residual_tol', lambda: (None, iac(), {'residual_tol': np.nan}), 'residual_tol'),
    ('an infinite residual_tol', lambda: (None, iac(), {'residual_tol': np.inf}), 'residual_tol'),
    ('no theta', lambda: (None, iac(), {'theta': None}), 'theta is required'),
    ('csurf without phi_surface', lambda: (None, iac(), {'phi_surface': None}), 'come together'),
    ('no view and no surface state', lambda: (None, iac(), dict(VIEW)), 'null view'),
    ('compat handle: no potential row', lambda: (fake_view(phi=None), iac(), dict(VIEW)), 'potential'),
    ('a lane outside the batch', lambda: (fake_view(), iac(), dict(VIEW, lanes=[0, 2])), 'lane index 2'),
    ('more points than lanes', lambda: (fake_view(B=1), iac(), dict(VIEW)), 'above the batch'),
    ('N different from the view', lambda: (fake_view(N=3), iac(), dict(VIEW)), 'the view has 3'),
    ('no sigma and an infinite capacitance', lambda: (None, iac(), {'stern_capacitance': np.inf}), 'surface charge'),
    # ---- what catia_solve reports on the members it brings ----
    ('no site type', lambda: (None, iac(site_fraction=np.zeros(0)), {}), '0 site types'),
    ('four site types', lambda: (None, iac(chain(S=4), site_fraction=np.full(4, 0.25)), {}), '4 site types'),
    ('no adsorbate', lambda: (None, iac(chain(S=1), site_fraction=np.array([0.5, 0.5]), site_of=np.array([0, 1], np.int32)), {}), '0 adsorbates'),
    ('ten columns', lambda: (None, iac(chain(S=9)), {}), 'at most 9 columns'),
    ('a free site that takes two sites', lambda: (None, iac(edit(chain(), site_count=np.array([2.0, 1.0]))), {}), 'its site count 1'),
    ('a site_of out of range', lambda: (None, iac(chain(S=2), site_of=np.array([0, 0, 5], np.int32)), {}), 'site_of[2] = 5 outside'),
    ('a negative site_of', lambda: (None, iac(chain(S=2), site_of=np.array([0, -1, 0], np.int32)), {}), 'site_of[1] = -1 outside'),
    ('a free-site column on another type', lambda: (None, dict(two_types(), site_of=np.array([1, 0, 0, 1], np.int32)), {}), 'free site of type 0'),
    ('a zero fraction', lambda: (None, dict(two_types(), site_fraction=np.array([1.0, 0.0])), {}), 'site_fraction[1]'),
    ('a NaN fraction', lambda: (None, iac(site_fraction=np.array([np.nan])), {}), 'site_fraction[0]'),
    ('a step that breaks the balance of a type', lambda: (None, two_types(broken=True), {}), 'conserve the sites of type 0'),
    ('a NaN in eps', lambda: (None, iac(chain(S=2), eps=np.array([[0.0, np.nan], [0.0, 0.0]])), {}), 'eps has a non-finite'),
    ('an infinite eps_ts', lambda: (None, iac(chain(S=2), eps_ts=np.array([[0.0, 0.0], [np.inf, 0.0], [0.0, 0.0]])), {}), 'eps_ts has a non-finite'),
    ('an infinite strength', lambda: (None, iac(), {'strength': np.inf}), 'strength'),
    ('a NaN strength', lambda: (None, iac(strength=np.nan), {}), 'strength'),
    ('a third response', lambda: (None, iac(response=2), {}), 'response is'),
    ('piecewise without parameters', lambda: (None, iac(response='piecewise'), {}), 'needs cutoff and smoothing'),
    ('a zero smoothing', lambda: (None, iac(**dict(PIECEWISE, smoothing=np.zeros(1))), {}), 'positive, finite smoothing'),
    ('a NaN cutoff', lambda: (None, iac(**dict(PIECEWISE, cutoff=np.full(1, np.nan))), {}), 'finite cutoff'),
])
def test_validation_errors_come_before_any_device_call(solver, what, make, word):
    from catint_amd import iacontrol
    view, tab, kw = make()
    args = args_for(tab)
    args.update(kw)
    with pytest.raises(iacontrol.IacontrolError) as e:
        solver.solve(view, tab, args.pop('phiM'), args.pop('theta'), **args)
    assert e.value.code == iacontrol.EINVAL, (what, str(e.value))
    assert word in str(e.value), (what, str(e.value))
    assert solver.last_kernel == '' and solver.last_kernel_ms == -1.0


def test_the_python_layer_refuses_what_it_can_name(solver):
    from catint_amd import iacontrol
    args = args_for(iac())
    pm, th = args.pop('phiM'), args.pop('theta')
    with pytest.raises(ValueError, match='theta has 6 values'):
        solver.solve(None, iac(), pm, np.ones((2, 3)), **args)
    with pytest.raises(ValueError, match='unknown field'):
        solver.solve(None, iac(), pm, th, fields=('drift',), **args)
    with pytest.raises(ValueError, match='site_of has 3 values'):
        solver.solve(None, iac(site_of=np.zeros(3, np.int32)), pm, th, **args)
    with pytest.raises(ValueError, match='eps has 4 values'):
        solver.solve(None, iac(eps=np.zeros((2, 2))), pm, th, **args)
    assert solver.last_kernel == ''
    import catint_amd
    assert catint_amd.InteractingRateControl is iacontrol.InteractingRateControl and catint_amd.iacontrol is iacontrol


def test_null_arguments_and_null_context(solver):
    from catint_amd import iacontrol
    lib = iacontrol.load_library()
    p = iacontrol.CaticParams(struct_size=C.sizeof(iacontrol.CaticParams))
    o = iacontrol.CaticOutputs(struct_size=C.sizeof(iacontrol.CaticOutputs))
    assert lib.catic_solve(solver._h, None, None, C.byref(o)) == iacontrol.EINVAL
    assert b'null' in lib.catic_last_error(solver._h)
    assert lib.catic_solve(solver._h, None, C.byref(p), None) == iacontrol.EINVAL
    assert lib.catic_solve(None, None, C.byref(p), C.byref(o)) == iacontrol.EINVAL
    assert lib.catic_create(0, None) == iacontrol.EINVAL
    assert lib.catic_last_kernel(solver._h) == b''


def test_no_point_makes_no_device_call(solver):
    """n == 0: valid, and done before the first device call (this machine may have no device at all); so is a call that asks for
    nothing"""
    from catint_amd import iacontrol
    out = solver.solve(None, two_types(), np.zeros(0), np.zeros((0, 4)), csurf=np.zeros((0, 2)), phi_surface=np.zeros(0),
                       fields=list(iacontrol.FIELDS))
    assert out['dflux_drc'].shape == (0, 3, 2) and out['dy_drc'].shape == (0, 3, 4) and out['dflux_dG'].shape == (0, 2, 2)
    assert out['tdrc'].shape == (0, 2, 2) and out['dflux_dstrength'].shape == (0, 2) and out['dy_dstrength'].shape == (0, 4)
    assert out['strength_control'].shape == (0, 2) and out['status'].shape == (0,) and out['status'].dtype == np.int32
    assert out['residual'].shape == (0,)
    out = solver.solve(fake_view(), iac(), np.zeros(0), np.zeros((0, 2)), lanes=[], fields=('flux_scale',))
    assert out['flux_scale'].shape == (0, 2)
    # the mean-field tables alone are one site type without interactions; a model object gives its own tables
    out = solver.solve(None, chain(S=3), np.zeros(0), np.zeros((0, 4)), csurf=np.zeros((0, 2)), phi_surface=np.zeros(0), fields=('tdrc', 'dy_dstrength'))
    assert out['tdrc'].shape == (0, 3, 2) and out['dy_dstrength'].shape == (0, 4)
    from tests.interact_cases import terrace_step_model
    out = solver.solve(None, terrace_step_model(), np.zeros(0), np.zeros((0, 7)), csurf=np.zeros((0, 3)), phi_surface=np.zeros(0))
    assert sorted(out) == sorted(iacontrol.DEFAULT_FIELDS + ('status', 'residual')) and out['tdrc'].shape == (0, 5, 3)
    assert solver.last_kernel == ''
    # n = 2 and every output NULL: nothing to do, no device call
    lib = iacontrol.load_library()
    t = iac()
    keep = [np.ascontiguousarray(t[k], np.int32) for k in ('order_f', 'order_b', 'site_of')] + \
        [np.ascontiguousarray(t[k], float) for k in ('nu', 'cref', 'site_count', 'dG', 'Ea', 'lnA', 'site_fraction', 'eps')]
    pm, th, cs, ps = np.zeros(2), np.full((2, 2), 0.5), np.zeros((2, 2)), np.zeros(2)
    d = iacontrol._dptr
    p = iacontrol.CaticParams(struct_size=C.sizeof(iacontrol.CaticParams), nspecies=2, nadsorbates=1, nsteps=2, n=2, nsitetypes=1, strength=1.0,
                              site_density=1e-5, residual_tol=1e-8, phiM=d(pm), theta=d(th), csurf=d(cs), phi_surface=d(ps))
    p.order_f, p.order_b, p.site_of = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in keep[:3])
    p.nu, p.cref, p.site_count, p.dG, p.Ea, p.lnA, p.site_fraction, p.eps = (d(a) for a in keep[3:])
    o = iacontrol.CaticOutputs(struct_size=C.sizeof(iacontrol.CaticOutputs))
    assert lib.catic_solve(solver._h, None, C.byref(p), C.byref(o)) == 0
    assert lib.catic_last_kernel(solver._h) == b''


def test_the_library_holds_the_one_kernel(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)


# ---- the routing, with fakes ---------------------------------------------------------------------------------------------------------
class FakeContext(object):
    opened = []

    def __init__(self, device=0):
        self.device, self.calls, self.closed = device, [], False
        type(self).opened.append(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.closed = True

    def solve(self, view, tables, phiM, theta, **kw):
        self.calls.append(dict(kw, view=view, tables=tables, phiM=phiM, theta=theta))
        n, N = len(phiM), np.asarray(tables['nu']).shape[1]
        R, T = np.asarray(tables['order_f']).shape[0], len(tables['site_count'])
        S = T - len(tables.get('site_fraction', [1.0]))
        shape = {'dflux_drc': (R, N), 'drc': (R, N), 'dflux_dG': (S, N), 'tdrc': (S, N), 'dflux_dstrength': (N,), 'strength_control': (N,),
                 'flux': (N,), 'flux_scale': (N,)}
        out = {k: np.ones((n,) + shape[k]) for k in kw['fields']}
        out.update(status=np.zeros(n, np.int32), residual=np.zeros(n))
        return out


def test_the_solver_routes_an_interacting_model_to_the_new_class(monkeypatch):
    from catint_amd import _capi, _drc, iacontrol
    from tests.interact_cases import co2r_model as interacting
    from tests.kinetics_cases import co2r_model as mean_field

    class FakeNew(FakeContext):
        opened = []

    class FakeOld(FakeContext):
        opened = []
    monkeypatch.setattr(iacontrol, 'InteractingRateControl', FakeNew)
    s = object.__new__(_capi.PnpSolver)          # no handle: the host-surface path needs none
    s.B, s._obs = 2, dict(device=3, stern_capacitance=0.2, phi_pzc=0.1, phiM=None)
    old = FakeOld()
    asked = []
    monkeypatch.setattr(_capi.PnpSolver, '_satellite', lambda self, attr: (asked.append(attr), old)[1])
    ia_model, mf_model = interacting('one_site', 0.3, 0.15), mean_field('one_site')
    host = dict(phiM=[-0.6, -0.7], csurf=np.ones((2, 3)), phi_surface=np.zeros(2))
    T = len(ia_model.tables()['site_count'])
    theta = np.full((2, T), 1.0 / T)
    out = s.get_rate_control(ia_model, theta=theta, residual_tol=1e-6, max_waves=2, **host)
    assert len(FakeNew.opened) == 1 and not old.calls and not asked
    (ctx,) = FakeNew.opened
    (call,) = ctx.calls
    assert ctx.device == 3 and ctx.closed and call['view'] is None and call['theta'] is theta and call['residual_tol'] == 1e-6
    assert 'eps' in call['tables'] and call['stern_capacitance'] == 0.2 and call['phi_pzc'] == 0.1 and call['max_waves'] == 2
    assert call['lanes'] is None and list(call['fields']) == list(iacontrol.DEFAULT_FIELDS)
    assert sorted(out) == sorted(iacontrol.DEFAULT_FIELDS + ('status', 'residual'))
    assert not [k for k, v in vars(s).items() if isinstance(v, FakeContext)]          # the context is not kept
    # the dict of tables routes the same way; kin and coupling give the apparent coefficients, the strength's among them
    N = 3
    kin = {'dflux_dc': np.zeros((2, N, N)), 'dflux_dphi': np.zeros((2, N, 2))}
    cp = {'T_c': np.zeros((2, N, N)), 'T_phi': np.zeros((2, N))}
    out = s.get_rate_control(ia_model.tables(), theta=theta, fields=('drc',), kin=kin, coupling=cp, rf=2.0, **host)
    assert len(FakeNew.opened) == 2 and FakeNew.opened[1].closed
    assert list(FakeNew.opened[1].calls[0]['fields']) == ['drc', 'dflux_drc', 'dflux_dG', 'flux', 'dflux_dstrength']
    assert sorted(out) == sorted(['drc', 'status', 'residual', 'dflux_drc_apparent', 'drc_apparent', 'dflux_dG_apparent', 'tdrc_apparent',
                                  'dflux_dstrength_apparent', 'strength_control_apparent'])
    # M = I: the apparent derivative is rf times the intrinsic one, the normalised one divides by rf flux and carries the strength
    lam = ia_model.tables()['strength']
    assert np.array_equal(out['dflux_dstrength_apparent'], np.full((2, N), 2.0))
    want = lam * _drc.normalised(np.full((2, 1, N), 2.0), 2.0 * np.ones((2, N)), ia_model.tables()['nu'])[:, 0, :]
    assert np.array_equal(out['strength_control_apparent'], want) and out['strength_control_apparent'].shape == (2, N)
    # a mean-field model keeps its satellite and its fields
    out = s.get_rate_control(mf_model, theta=theta, **host)
    assert len(FakeNew.opened) == 2 and asked == ['_rate_control'] and len(old.calls) == 1 and not old.closed
    assert list(old.calls[0]['fields']) == list(_drc.DEFAULT_FIELDS)
    out = s.get_rate_control(mf_model, theta=theta, fields=('drc',), kin=kin, coupling=cp, **host)
    assert list(old.calls[1]['fields']) == ['drc', 'dflux_drc', 'dflux_dG', 'flux'] and 'strength_control_apparent' not in out
    assert len(_capi.PnpSolver.SATELLITES) == 13 and not [k for k in _capi.PnpSolver.SATELLITES if 'iacontrol' in k]
    assert not [k for k in _capi.SYMBOLS if 'catic' in k]


def test_theta_none_takes_the_coverages_of_get_kinetics(monkeypatch):
    from catint_amd import _capi, iacontrol
    from tests.interact_cases import co2r_model as interacting

    class FakeNew(FakeContext):
        opened = []
    monkeypatch.setattr(iacontrol, 'InteractingRateControl', FakeNew)
    s = object.__new__(_capi.PnpSolver)
    s.B, s._obs = 2, dict(device=0, stern_capacitance=0.2, phi_pzc=0.1, phiM=None)
    model = interacting('one_site', 0.3, 0.15)
    T = len(model.tables()['site_count'])
    theta = np.full((2, T), 0.25)
    seen = []
    monkeypatch.setattr(_capi.PnpSolver, 'get_kinetics', lambda self, tables, **kw: (seen.append((tables, kw)), {'theta': theta})[1])
    s.get_rate_control(model, phiM=[-0.6, -0.7], csurf=np.ones((2, 3)), phi_surface=np.zeros(2), fields=('strength_control',))
    ((tables, kw),) = seen
    assert 'eps' in tables and kw['fields'] == ('theta',)
    assert FakeNew.opened[0].calls[0]['theta'] is theta


def test_the_calculator_still_refuses_rate_control_of_an_interacting_model():
    """out of scope on purpose: tests/test_interact_abi.py pins the refusal and its message"""
    from catint_amd.calculator import Calculator, CalculatorError
    from tests.test_interact_abi import interacting_scf_parts
    tp, model, _ = interacting_scf_parts()
    with pytest.raises(CalculatorError, match='rate_control works on the mean-field model'):
        Calculator(transport=tp, calc='comsol').set_microkinetics(model, rate_control=True)
