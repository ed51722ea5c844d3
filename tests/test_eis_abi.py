"""libcatint_eis without a GPU (the method of tests/test_kintrans_abi.py): the library builds for gfx950 and exports what
include/catint_eis.h declares, the ctypes mirrors have the compiler's layouts, every validation error of both entry points is returned
before any device call, no point and no output make no device call, the dependency list of the build is complete, and the library holds
the kinetic kernel and the eight instances of the electrode kernel."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import kernel_census as K
from tests.test_kinetics_abi import chain, edit, fake_view, host_args, poke

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {'cateis_params': 'CateisParams', 'cateis_outputs': 'CateisOutputs'}
INSTANCES = {'cateis::kinetic_kernel'} | {'cateis::electrode_kernel<%d>' % nb for nb in range(2, 10)}


@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_eis_library
    return build_eis_library()


@pytest.fixture(scope='module')
def handle(libpath):
    from catint_amd import _eis
    with _eis.Impedance(0) as o:
        yield o


def header_source():
    src = open(os.path.join(ROOT, 'include', 'catint_eis.h')).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    from catint_amd import _eis
    declared = sorted(set(re.findall(r'\b(cateis_[a-z0-9_]+)\s*\(', header_source())))
    assert declared == sorted(_eis.SYMBOLS) and len(declared) == 7
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(cateis_[a-z0-9_]+)\b', exported))) == declared
    assert not re.findall(r'\b(pnp|catkin|catresp|catcpl|catdrc|catkt)_[a-z0-9_]+\b', exported)          # and no symbol of another library
    from catint_amd import _capi
    assert not [s for s in _capi.SYMBOLS if 'cateis' in s]
    assert hasattr(_capi.PnpSolver, 'get_impedance') and hasattr(_capi.PnpSolver, 'get_kinetic_admittance')


def test_the_sources_are_a_library_of_their_own_with_a_complete_dependency_list():
    from catint_amd import build
    others = (build.SOURCES + build.OBSERVE_SOURCES + build.BALANCE_SOURCES + build.REGRID_SOURCES + build.EQUIL_SOURCES + build.RESPONSE_SOURCES
              + build.KINETICS_SOURCES + build.COUPLE_SOURCES + build.SENS_SOURCES + build.DRC_SOURCES + build.MODES_SOURCES + build.SCFKIN_SOURCES
              + build.KINTRANS_SOURCES)
    assert not any('eis' in s for s in others)
    assert os.path.dirname(build.EIS_LIB) == os.path.dirname(build.LIB)
    assert build.EIS_SOURCES == ['cateis.hip'] and os.path.isdir(build.EIS_DIR) and callable(build.eis_needs_build)
    listed = {os.path.realpath(p) for p in build.EIS_HEADERS}
    for h in ('catint_eis.h', 'catint_pnp.h'):
        assert os.path.realpath(os.path.join(ROOT, 'include', h)) in listed
    for h in ('pnp_team.h', 'pnp_kin.h', 'pnp_post.h'):
        assert os.path.realpath(os.path.join(build.CSRC, h)) in listed
    from tests.test_build_deps import reached
    sources = [os.path.join(build.EIS_DIR, f) for f in build.EIS_SOURCES]
    assert not reached(sources) - listed - {os.path.realpath(f) for f in sources}
    assert 'build_eis_library(' in open(os.path.join(ROOT, '__graft_entry__.py')).read()


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


MACROS = {'ok': 'CATEIS_STATUS_OK', 'pivot': 'CATEIS_STATUS_PIVOT', 'input': 'CATEIS_STATUS_INPUT', 'singular': 'CATEIS_STATUS_SINGULAR',
          'residual': 'CATEIS_STATUS_RESIDUAL', 'maxfreq': 'CATEIS_MAX_FREQ', 'maxnx': 'CATEIS_MAX_NX', 'stern': 'CATEIS_WALL_STERN',
          'einval': 'CATEIS_EINVAL', 'enomem': 'CATEIS_ENOMEM', 'edevice': 'CATEIS_EDEVICE'}


@pytest.fixture(scope='module')
def compiler_layout(tmp_path_factory):
    structs = header_structs()
    assert set(PAIRS) <= set(structs)
    d = tmp_path_factory.mktemp('eis_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_eis.h"', 'int main(void) {']
    for s in PAIRS:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (s, s))
        for f in structs[s]:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    for name, macro in MACROS.items():
        lines.append('  printf("%s n %%d\\n", %s);' % (name, macro))
    lines.append('  printf("growth x %g\\n", CATEIS_PIVOT_GROWTH_LIMIT);')
    lines.append('  printf("tiny x %g\\n", CATEIS_SINGULAR);')
    lines += ['  return 0;', '}']
    (d / 'abi.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(d / 'abi.c'), '-o', str(d / 'abi')])
    layout = {}
    for line in subprocess.check_output([str(d / 'abi')]).decode().splitlines():
        s, f, v = line.split()
        layout.setdefault(s, {})[f] = float(v) if f == 'x' else int(v)
    return layout


@pytest.mark.parametrize('cname', sorted(PAIRS))
def test_ctypes_mirror_matches_the_compiler(cname, compiler_layout):
    from catint_amd import _eis
    cls = getattr(_eis, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_of_the_binding_are_the_header_s(compiler_layout):
    from catint_amd import _eis as e
    n = {name: compiler_layout[name]['n'] for name in MACROS}
    assert (e.OK, e.PIVOT, e.INPUT, e.SINGULAR_A, e.RESIDUAL) == (n['ok'], n['pivot'], n['input'], n['singular'], n['residual']) == (0, 1, 2, 3, 4)
    assert (e.MAX_FREQ, e.MAX_NX, e.WALL['stern']) == (n['maxfreq'], n['maxnx'], n['stern'])
    assert (e.EINVAL, e.ENOMEM, e.EDEVICE) == (n['einval'], n['enomem'], n['edevice'])
    assert e.PIVOT_GROWTH_LIMIT == compiler_layout['growth']['x'] == 1e8 and e.SINGULAR == compiler_layout['tiny']['x'] == 1e-12
    from tests import couple_ref as CR
    assert (CR.SINGULAR, CR.GROWTH) == (e.SINGULAR, e.PIVOT_GROWTH_LIMIT)


VIEW = {'csurf': None, 'phi_surface': None}


def theta_of(tab, n=2):
    return np.full((n, len(tab['site_count'])), 1.0 / len(tab['site_count']))


# what catkin_solve checks, and what cateis_kinetic adds
KINETIC_ERRORS = [
    ('struct_size of the parameters', lambda: (None, chain(), {'struct_size': 8}), 'cateis_params.struct_size'),
    ('struct_size of the outputs', lambda: (None, chain(), {'out_struct_size': 8}), 'cateis_outputs.struct_size'),
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
    ('no theta', lambda: (None, chain(), {'theta': None}), 'theta is required'),
    ('no omega', lambda: (None, chain(), {'omega': None}), 'nfreq = 0'),
    ('an empty omega', lambda: (None, chain(), {'omega': []}), 'nfreq = 0'),
    ('257 frequencies', lambda: (None, chain(), {'omega': np.arange(257.0)}), 'nfreq = 257'),
    ('a negative omega', lambda: (None, chain(), {'omega': [0.0, -1.0]}), 'omega[1]'),
    ('an infinite omega', lambda: (None, chain(), {'omega': [np.inf]}), 'omega[0]'),
    ('a NaN omega', lambda: (None, chain(), {'omega': [1.0, 2.0, np.nan]}), 'omega[2]'),
    ('a negative residual_tol', lambda: (None, chain(), {'residual_tol': -1e-8}), 'residual_tol'),
    ('a NaN residual_tol', lambda: (None, chain(), {'residual_tol': np.nan}), 'residual_tol'),
    ('an infinite residual_tol', lambda: (None, chain(), {'residual_tol': np.inf}), 'residual_tol'),
]


@pytest.mark.parametrize('what, make, word', KINETIC_ERRORS)
def test_kinetic_validation_errors_come_before_any_device_call(handle, what, make, word):
    from catint_amd import _eis
    view, tab, kw = make()
    N = np.asarray(tab['order_f']).shape[1] - len(tab['site_count'])
    args = dict(host_args(N=max(N, 0)), theta=theta_of(tab), omega=[0.0, 1.0])
    args.update(kw)
    with pytest.raises(_eis.EisError) as e:
        handle.kinetic(view, tab, **args)
    assert e.value.code == _eis.EINVAL, (what, str(e.value))
    assert word in str(e.value), (what, str(e.value))
    assert str(e.value).split(': ')[1].startswith('cateis_kinetic')
    assert handle.last_kernel == '' and handle.last_kernel_ms == -1.0


def medium(N=2, nx=16, **kw):
    m = dict(D=np.full(N, 1e-9), charges=np.array([96485.0, -96485.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])[:N], x=np.linspace(0.0, 1e-8, nx),
             beta=40.0, eps=7e-10, dx=1e-8 / (nx - 1), stern_capacitance=0.2, wall_bc='stern')
    m.update(kw)
    return m


def bent(x, i):
    x = np.array(x)
    x[i] = x[i - 1]
    return x


# what catcpl_solve checks of the medium, and what cateis_solve adds
SOLVE_ERRORS = [
    ('struct_size of the view', lambda: (fake_view(size=12), {}), 'pnp_device_view.struct_size'),
    ('struct_size of the parameters', lambda: (fake_view(), {'struct_size': 8}), 'cateis_params.struct_size'),
    ('struct_size of the outputs', lambda: (fake_view(), {'out_struct_size': 8}), 'cateis_outputs.struct_size'),
    ('compat handle: no potential row', lambda: (fake_view(phi=None), {}), 'potential'),
    ('two grid points', lambda: (fake_view(nx=2), medium(nx=2)), 'nx = 2'),
    ('x not increasing', lambda: (fake_view(), medium(x=bent(np.linspace(0.0, 1e-8, 16), 5))), 'not strictly increasing at index 5'),
    ('a zero D', lambda: (fake_view(), medium(D=np.array([1e-9, 0.0]))), 'species 1'),
    ('a NaN charge', lambda: (fake_view(), medium(charges=np.array([np.nan, 1.0]))), 'species 0'),
    ('a negative radius', lambda: (fake_view(), medium(mpb_radius=np.array([1e-10, -1e-10]))), 'species 1'),
    ('a zero beta', lambda: (fake_view(), medium(beta=0.0)), 'beta'),
    ('an infinite eps', lambda: (fake_view(), medium(eps=np.inf)), 'eps'),
    ('a NaN velocity', lambda: (fake_view(), medium(velocity=np.nan)), 'velocity'),
    ('a Dirichlet wall', lambda: (fake_view(), medium(wall_bc='dirichlet')), 'Stern wall'),
    ('an unknown wall', lambda: (fake_view(), medium(wall_bc=2)), 'unknown wall_bc'),
    ('a Stern wall without a capacitance', lambda: (fake_view(), medium(stern_capacitance=0.0)), 'capacitance'),
    ('a reaction with a species outside', lambda: (fake_view(), medium(reactions=[([0], [2], 1.0, 1.0)])), 'species index 2'),
    ('a reaction with five reactants', lambda: (fake_view(), medium(reactions=[([0] * 5, [1], 1.0, 1.0)])), None),
    ('a negative rf', lambda: (fake_view(), medium(rf=-1.0)), 'rf must be >= 0'),
    ('a NaN rf', lambda: (fake_view(), medium(rf=np.nan)), 'rf must be >= 0'),
    ('an infinite rf', lambda: (fake_view(), medium(rf=np.inf)), 'rf must be >= 0'),
    ('negative max_waves', lambda: (fake_view(), medium(max_waves=-1)), 'max_waves'),
    ('a lane outside the batch', lambda: (fake_view(), medium(lanes=[0, 2])), 'lane index 2'),
    ('N different from the view', lambda: (fake_view(N=3), medium(N=3)), 'the view has 3'),
    ('no theta', lambda: (fake_view(), medium(theta=None)), 'theta is required'),
    ('an empty omega', lambda: (fake_view(), medium(omega=[])), 'nfreq = 0'),
    ('a negative omega', lambda: (fake_view(), medium(omega=[-1.0])), 'omega[0]'),
    ('a NaN residual_tol', lambda: (fake_view(), medium(residual_tol=np.nan)), 'residual_tol'),
    ('an order of 4', lambda: (fake_view(), medium(tables=edit(chain(), f=poke('order_f', (0, 0), 4)))), 'order'),
]


@pytest.mark.parametrize('what, make, word', SOLVE_ERRORS)
def test_solve_validation_errors_come_before_any_device_call(handle, what, make, word):
    from catint_amd import _eis
    view, kw = make()
    kw = dict(medium(), **kw)
    tab = kw.pop('tables', chain())
    args = dict(phiM=np.array([-0.1, -0.2]), theta=theta_of(tab), omega=[0.0, 1.0])
    for k in ('theta', 'omega'):
        if k in kw:
            args[k] = kw.pop(k)
    try:
        with pytest.raises(_eis.EisError) as e:
            handle.solve(view, tab, args['phiM'], args['theta'], args['omega'], kw.pop('D'), kw.pop('charges'), kw.pop('x'), kw.pop('beta'),
                         kw.pop('eps'), kw.pop('dx'), **kw)
    except ValueError as err:           # (the marshalling of the reaction table refuses five reactants itself)
        assert word is None, (what, err)
        return
    assert e.value.code == _eis.EINVAL, (what, str(e.value))
    assert word is None or word in str(e.value), (what, str(e.value))
    assert str(e.value).split(': ')[1].startswith('cateis_solve')
    assert handle.last_kernel == '' and handle.last_kernel_ms == -1.0


def test_a_host_surface_state_is_refused_by_solve(handle):
    from catint_amd import _eis
    lib = _eis.load_library()
    tab = chain()
    keep = [np.ascontiguousarray(tab[k], np.int32) for k in ('order_f', 'order_b')] + [np.ascontiguousarray(tab[k], float) for k in
                                                                                        ('nu', 'cref', 'site_count', 'dG', 'Ea', 'lnA')]
    m = medium()
    arr = [np.ascontiguousarray(m[k], float) for k in ('D', 'charges', 'x')]
    pm, cs, ps, th, om = np.zeros(2), np.ones((2, 2)), np.zeros(2), theta_of(tab), np.array([0.0])
    p = _eis.CateisParams(struct_size=C.sizeof(_eis.CateisParams), nspecies=2, nadsorbates=1, nsteps=2, potential_drop=1, nfreq=1, wall_bc=1,
                          n=2, site_density=1e-5, stern_capacitance=0.2, residual_tol=1e-8, beta=40.0, eps=7e-10, dx=m['dx'], rf=1.0,
                          phiM=_eis._dptr(pm), csurf=_eis._dptr(cs), phi_surface=_eis._dptr(ps), theta=_eis._dptr(th), omega=_eis._dptr(om),
                          D=_eis._dptr(arr[0]), charges=_eis._dptr(arr[1]), x=_eis._dptr(arr[2]))
    p.order_f, p.order_b = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in keep[:2])
    p.nu, p.cref, p.site_count, p.dG, p.Ea, p.lnA = (_eis._dptr(a) for a in keep[2:])
    o = _eis.CateisOutputs(struct_size=C.sizeof(_eis.CateisOutputs))
    view = fake_view()
    assert lib.cateis_solve(handle._h, C.byref(view), C.byref(p), C.byref(o)) == _eis.EINVAL
    assert b'csurf and phi_surface must be NULL' in lib.cateis_last_error(handle._h)
    # ... and with the view's surface state the same call, which asks for nothing, is done before any device call
    p.csurf, p.phi_surface = None, None
    assert lib.cateis_solve(handle._h, C.byref(view), C.byref(p), C.byref(o)) == 0
    assert lib.cateis_kinetic(handle._h, C.byref(view), C.byref(p), C.byref(o)) == 0
    p.csurf, p.phi_surface = _eis._dptr(cs), _eis._dptr(ps)
    assert lib.cateis_kinetic(handle._h, None, C.byref(p), C.byref(o)) == 0
    assert lib.cateis_last_kernel(handle._h) == b'' and lib.cateis_last_kernel_ms(handle._h) == -1.0


def test_null_arguments_and_null_context(handle):
    from catint_amd import _eis
    lib = _eis.load_library()
    p = _eis.CateisParams(struct_size=C.sizeof(_eis.CateisParams))
    o = _eis.CateisOutputs(struct_size=C.sizeof(_eis.CateisOutputs))
    view = fake_view()
    for f in (lib.cateis_kinetic, lib.cateis_solve):
        assert f(handle._h, C.byref(view), None, C.byref(o)) == _eis.EINVAL
        assert b'null' in lib.cateis_last_error(handle._h)
        assert f(handle._h, C.byref(view), C.byref(p), None) == _eis.EINVAL
        assert f(None, C.byref(view), C.byref(p), C.byref(o)) == _eis.EINVAL
    assert lib.cateis_solve(handle._h, None, C.byref(p), C.byref(o)) == _eis.EINVAL
    assert lib.cateis_create(0, None) == _eis.EINVAL
    assert lib.cateis_last_kernel(handle._h) == b''


def test_no_point_makes_no_device_call(handle):
    """n == 0: valid, and done before the first device call (this machine may have no device at all)"""
    out = handle.kinetic(None, chain(S=2), np.zeros(0), np.zeros((0, 3)), [0.0, 1.0, 2.0], csurf=np.zeros((0, 2)), phi_surface=np.zeros(0),
                         fields=('Kc', 'Kphi', 'dy', 'residual'))
    assert out['Kc'].shape == (0, 3, 2, 2) and out['Kphi'].shape == (0, 3, 2, 2) and out['dy'].shape == (0, 3, 3, 4)
    assert out['Kc'].dtype == np.complex128 and out['residual'].shape == (0,) and out['status'].shape == (0, 3) and out['status'].dtype == np.int32
    m = medium()
    out = handle.solve(fake_view(), chain(), np.zeros(0), np.zeros((0, 2)), [0.0], m['D'], m['charges'], m['x'], m['beta'], m['eps'], m['dx'],
                       lanes=[], stern_capacitance=0.2, fields=('admittance', 'Tc', 'tphi'))
    assert out['admittance'].shape == (0, 1) and out['Tc'].shape == (0, 1, 2, 2) and out['tphi'].shape == (0, 1)
    assert handle.last_kernel == '' and handle.last_kernel_ms == -1.0


def test_the_library_holds_the_kinetic_kernel_and_eight_electrode_instances(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)
    assert len(compiled) == 9


def test_the_calculator_option_is_off_by_default_and_validated():
    from catint_amd.calculator import Calculator, CalculatorError
    from tests.test_kinetics_abi import scf_parts
    tp, model, transport_fn = scf_parts()
    calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-9)
    calc.set_microkinetics(model, site_density=2e-6)
    assert 'impedance' not in calc.microkinetics
    calc.set_microkinetics(model, site_density=2e-6, impedance=[0.0, 10.0])
    assert np.array_equal(calc.microkinetics['impedance'], [0.0, 10.0])
    for bad in ([], [-1.0], [np.nan], [1.0, np.inf]):
        with pytest.raises(CalculatorError, match='impedance'):
            calc.set_microkinetics(model, site_density=2e-6, impedance=bad)
    # the impedance is formed at the state a device transport holds: a host transport_fn has none
    with pytest.raises(CalculatorError, match='transport_fn'):
        calc.run_scf_cycle(transport_fn=transport_fn, max_iter=3)
