"""libcatint_drc without a GPU (the method of tests/test_kinetics_abi.py).  The library builds for gfx950 and exports what the header
declares, the header is plain C, the ctypes mirrors have the compiler's layouts, every validation error is returned before any device
call, the dependency list is complete, the library holds the one kernel.  The NumPy restatement of include/catint_drc.h
(tests/drc_ref.py, which tests/test_gpu_drc.py compares the device with) is checked on all ten cases of tests/kinetics_cases.py against
the same formulas at 60 digits, for the identities
  I1  sum_r dflux_drc[r][k] = flux_k            (lowering every transition state by one kT multiplies every rate by e)
  I2  dflux_drc = dflux_dlnkf + dflux_dlnkb
  I3  dflux_dphi[:, q] = sum_r dflux_dlnkf[r] dlf_r + dflux_dlnkb[r] dlb_r     (the chain rule through ln kf, ln kb; KR.slopes)
each in units of the term sums, and against central differences of re-solved steady states: through off[n][R][2] for the rate
constants, through shifted dG / Ea tables for the transition states and the adsorbate energies.  The apparent algebra against
numpy.linalg.solve; the calculator's opt-in with fakes.

Worst errors of control_fp64 against 60 digits over all cases, in units of drc_scale (printed by
test_fp64_restatement_against_60_digits): raw derivatives 9.2e-15, dy_drc 1.0e-14, normalised 8.1e-15, flux 7.2e-15 of flux_scale, all
on the four-step mechanism, where |y| reaches 134; the random networks stay below 2.0e-15.  Residual of the states <= 1.2e-14.
Without the header's refinement step the same figures were 1.3e-13 and, for dy_drc, 1.3e-11 (random_S3: the entries of J are
themselves sums that cancel)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from catint_amd import _drc          # fails without the feature
from tests import drc_ref as DR
from tests import kernel_census as K
from tests import kinetics_cases as KC
from tests import kinetics_ref as KR
from tests.test_kinetics_abi import chain, edit, fake_view, host_args, poke, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {'catdrc_params': 'CatdrcParams', 'catdrc_outputs': 'CatdrcOutputs'}
INSTANCES = {'catdrc::control_kernel'}
ALL = list(_drc.FIELDS)


# ---- the library -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_drc_library
    return build_drc_library()


@pytest.fixture(scope='module')
def solver(libpath):
    with _drc.RateControl(0) as o:
        yield o


def header_source():
    src = open(os.path.join(ROOT, 'include', 'catint_drc.h')).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    declared = sorted(set(re.findall(r'\b(catdrc_[a-z0-9_]+)\s*\(', header_source())))
    assert declared == sorted(_drc.SYMBOLS) and len(declared) == 6
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(catdrc_[a-z0-9_]+)\b', exported))) == declared
    # and no symbol with another library's prefix
    assert not re.findall(r'\b(?:pnp|catobs|catbal|catgrid|cateq|catresp|catkin|catcpl|catsens)_[a-z0-9_]+\b', exported)


def test_the_build_lists_and_the_dependency_walk():
    from catint_amd import build
    from tests.test_build_deps import reached
    others = (build.SOURCES + build.OBSERVE_SOURCES + build.BALANCE_SOURCES + build.REGRID_SOURCES + build.EQUIL_SOURCES + build.RESPONSE_SOURCES
              + build.KINETICS_SOURCES + build.COUPLE_SOURCES + build.SENS_SOURCES)
    assert not any('catdrc' in s or 'drc' in s for s in others)
    assert os.path.basename(build.DRC_LIB) == 'libcatint_drc.so' and os.path.dirname(build.DRC_LIB) == os.path.dirname(build.LIB)
    assert build.DRC_SOURCES == ['catdrc.hip'] and os.path.isdir(build.DRC_DIR) and callable(build.drc_needs_build)
    sources = [os.path.join(build.DRC_DIR, f) for f in build.DRC_SOURCES]
    listed = {os.path.realpath(p) for p in sources + build.DRC_HEADERS}
    assert len(listed) == len(sources + build.DRC_HEADERS), 'a file is listed twice'
    found = reached(sources)
    for h in ('catint_drc.h', 'catint_pnp.h'):
        assert os.path.realpath(os.path.join(ROOT, 'include', h)) in found
    assert not found - listed, 'included but not in DRC_HEADERS: %s' % sorted(found - listed)
    assert not listed - found, 'listed but not included: %s' % sorted(listed - found)
    assert 'build_drc_library(' in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    assert '--offload-arch=gfx950' in build.FLAGS and build.build_drc_library() == build.DRC_LIB and not build.drc_needs_build()


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


MACROS = {'maxspecies': 'CATDRC_MAX_SPECIES', 'maxads': 'CATDRC_MAX_ADSORBATES', 'maxsteps': 'CATDRC_MAX_STEPS', 'maxorder': 'CATDRC_MAX_ORDER',
          'maxsites': 'CATDRC_MAX_SITES', 'minlog': '(int)CATDRC_MIN_LOG', 'full': 'CATDRC_DROP_FULL', 'stern': 'CATDRC_DROP_STERN',
          'okpoint': 'CATDRC_OK_POINT', 'residual': 'CATDRC_RESIDUAL', 'input': 'CATDRC_INPUT', 'pivot': 'CATDRC_PIVOT', 'einval': 'CATDRC_EINVAL',
          'enomem': 'CATDRC_ENOMEM', 'edevice': 'CATDRC_EDEVICE'}


@pytest.fixture(scope='module')
def compiler_layout(tmp_path_factory):
    """The header compiles as plain C (c99, -Wall -Werror); sizes, offsets and constants as the compiler sees them"""
    structs = header_structs()
    assert set(PAIRS) <= set(structs)
    d = tmp_path_factory.mktemp('drc_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_drc.h"', 'int main(void) {']
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
    cls = getattr(_drc, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_and_fields_of_the_binding_are_the_header_s(compiler_layout):
    from catint_amd import _kinetics as k
    n = {name: compiler_layout[name]['n'] for name in MACROS}
    assert (_drc.MAX_SPECIES, _drc.MAX_ADSORBATES, _drc.MAX_STEPS, _drc.MAX_ORDER, _drc.MAX_SITES) == (
        n['maxspecies'], n['maxads'], n['maxsteps'], n['maxorder'], n['maxsites']) == (k.MAX_SPECIES, k.MAX_ADSORBATES, k.MAX_STEPS, k.MAX_ORDER, k.MAX_SITES)
    assert _drc.MIN_LOG == n['minlog'] == k.MIN_LOG and _drc.DROP == {'full': n['full'], 'stern': n['stern']} == k.DROP
    assert (_drc.OK_POINT, _drc.RESIDUAL, _drc.INPUT, _drc.PIVOT) == (n['okpoint'], n['residual'], n['input'], n['pivot']) == (0, 1, 2, 3)
    assert (_drc.EINVAL, _drc.ENOMEM, _drc.EDEVICE) == (n['einval'], n['enomem'], n['edevice'])
    # the parameters are catkin_params without maxit, tol, theta_guess (and the padding word), plus theta and residual_tol
    kin = [f for f, _ in k.CatkinParams._fields_ if f not in ('maxit', 'tol', 'theta_guess', 'reserved')]
    mine = [f for f, _ in _drc.CatdrcParams._fields_ if f not in ('theta', 'residual_tol')]
    assert mine == kin
    assert sorted(f for f, _ in _drc.CatdrcOutputs._fields_) == sorted(ALL + ['struct_size', 'reserved', 'residual', 'status'])
    assert set(_drc.DEFAULT_FIELDS) <= set(ALL) and _drc.DEFAULT_RESIDUAL_TOL == 1e-8


def drc_args(n=2, N=2, T=2):
    return dict(host_args(n=n, N=N), theta=np.full((n, T), 1.0 / T))


@pytest.mark.parametrize('what, make, word', [
    ('struct_size of the parameters', lambda: (None, chain(), {'struct_size': 8}), 'catdrc_params.struct_size'),
    ('struct_size of the outputs', lambda: (None, chain(), {'out_struct_size': 8}), 'catdrc_outputs.struct_size'),
    ('struct_size of the view', lambda: (fake_view(size=12), chain(), {'csurf': None, 'phi_surface': None}), 'pnp_device_view.struct_size'),
    ('nine species', lambda: (None, chain(N=9), {}), '9 species'),
    ('no adsorbate', lambda: (None, tables(np.zeros((1, 3), int), np.zeros((1, 3), int), [[1.0, 0.0]], [1.0], np.zeros((1, 4))), {}), '0 adsorbates'),
    ('nine adsorbates', lambda: (None, chain(S=9), {}), '9 adsorbates'),
    ('no step', lambda: (None, tables(np.zeros((0, 4), int), np.zeros((0, 4), int), np.zeros((0, 2)), [1.0, 1.0], np.zeros((0, 4))), {}), '0 steps'),
    ('seventeen steps', lambda: (None, chain(R=17), {}), '17 steps'),
    ('an order of 4', lambda: (None, edit(chain(), f=poke('order_f', (0, 0), 4)), {}), 'order'),
    ('a negative order', lambda: (None, edit(chain(), f=poke('order_b', (1, 1), -1)), {}), 'order'),
    ('a step that does not conserve sites', lambda: (None, edit(chain(), f=poke('order_f', (0, 2), 2)), {}), 'conserve sites'),
    ('a step that does not conserve sites (two-site adsorbate)', lambda: (None, edit(chain(), site_count=np.array([1.0, 2.0])), {}), 'conserve sites'),
    ('an empty step', lambda: (None, edit(chain(S=2, R=4), f=lambda t: (t['order_f'].__setitem__(3, 0), t['order_b'].__setitem__(3, 0),
                                                                      t['nu'].__setitem__(3, 0.0))), {}), 'empty step'),
    ('a zero cref', lambda: (None, edit(chain(), cref=np.array([1.0, 0.0])), {}), 'cref[1]'),
    ('an infinite cref', lambda: (None, edit(chain(), cref=np.array([np.inf, 1.0])), {}), 'cref[0]'),
    ('a zero site density', lambda: (None, edit(chain(), site_density=0.0), {}), 'site_density'),
    ('a NaN site density', lambda: (None, edit(chain(), site_density=np.nan), {}), 'site_density'),
    ('a zero residual tolerance', lambda: (None, chain(), {'residual_tol': 0.0}), 'residual_tol'),
    ('a negative residual tolerance', lambda: (None, chain(), {'residual_tol': -1e-8}), 'residual_tol'),
    ('an infinite residual tolerance', lambda: (None, chain(), {'residual_tol': np.inf}), 'residual_tol'),
    ('a NaN residual tolerance', lambda: (None, chain(), {'residual_tol': np.nan}), 'residual_tol'),
    ('no theta', lambda: (None, chain(), {'theta': None}), 'theta is required'),
    ('a site count of 4', lambda: (None, edit(chain(), site_count=np.array([1.0, 4.0])), {}), 'site count 1'),
    ('a site count of 0', lambda: (None, edit(chain(), site_count=np.array([1.0, 0.0])), {}), 'site count 1'),
    ('a free site that takes two sites', lambda: (None, edit(chain(), site_count=np.array([2.0, 1.0])), {}), 'site count 0'),
    ('a NaN site count', lambda: (None, edit(chain(), site_count=np.array([1.0, np.nan])), {}), 'site count 1'),
    ('potential_drop 2', lambda: (None, chain(), {'potential_drop': 2}), 'potential_drop'),
    ('negative max_waves', lambda: (None, chain(), {'max_waves': -1}), 'max_waves'),
    ('a NaN in dG', lambda: (None, edit(chain(), f=poke('dG', (1, 2), np.nan)), {}), 'step 1 has a non-finite'),
    ('an infinite dG', lambda: (None, edit(chain(), f=poke('dG', (0, 0), -np.inf)), {}), 'step 0 has a non-finite'),
    ('e0 = +inf', lambda: (None, edit(chain(), f=poke('Ea', (0, 0), np.inf)), {}), 'step 0 has a non-finite'),
    ('e1 = -inf', lambda: (None, edit(chain(), f=poke('Ea', (1, 1), -np.inf)), {}), 'step 1 has a non-finite'),
    ('a NaN lnA', lambda: (None, edit(chain(), f=poke('lnA', 1, np.nan)), {}), 'step 1 has a non-finite'),
    ('a NaN nu', lambda: (None, edit(chain(), f=poke('nu', (0, 0), np.nan)), {}), 'nu of step 0'),
    ('csurf without phi_surface', lambda: (None, chain(), {'phi_surface': None}), 'come together'),
    ('no view and no surface state', lambda: (None, chain(), {'csurf': None, 'phi_surface': None}), 'null view'),
    ('compat handle: no potential row', lambda: (fake_view(phi=None), chain(), {'csurf': None, 'phi_surface': None}), 'potential'),
    ('a lane outside the batch', lambda: (fake_view(), chain(), {'csurf': None, 'phi_surface': None, 'lanes': [0, 2]}), 'lane index 2'),
    ('a negative lane', lambda: (fake_view(), chain(), {'csurf': None, 'phi_surface': None, 'lanes': [-1, 0]}), 'lane index -1'),
    ('more points than lanes', lambda: (fake_view(B=1), chain(), {'csurf': None, 'phi_surface': None}), 'above the batch'),
    ('N different from the view', lambda: (fake_view(N=3), chain(), {'csurf': None, 'phi_surface': None}), 'the view has 3'),
    ('no sigma and an infinite capacitance', lambda: (None, chain(), {'stern_capacitance': np.inf}), 'surface charge'),
    ('no sigma and a NaN phi_pzc', lambda: (None, chain(), {'phi_pzc': np.nan}), 'surface charge'),
])
def test_validation_errors_come_before_any_device_call(solver, what, make, word):
    view, tab, kw = make()
    of = np.asarray(tab['order_f'])
    T = len(tab['site_count'])
    N = of.shape[1] - T if of.ndim == 2 else 2
    args = drc_args(N=max(N, 0), T=T)
    args.update(kw)
    with pytest.raises(_drc.DrcError) as e:
        solver.solve(view, tab, **args)
    assert e.value.code == _drc.EINVAL, (what, str(e.value))
    assert word in str(e.value), (what, str(e.value))
    assert solver.last_kernel == '' and solver.last_kernel_ms == -1.0


def test_null_arguments_no_point_and_no_output_make_no_device_call(solver):
    lib = _drc.load_library()
    p = _drc.CatdrcParams(struct_size=C.sizeof(_drc.CatdrcParams))
    o = _drc.CatdrcOutputs(struct_size=C.sizeof(_drc.CatdrcOutputs))
    assert lib.catdrc_solve(solver._h, None, None, C.byref(o)) == _drc.EINVAL and b'null' in lib.catdrc_last_error(solver._h)
    assert lib.catdrc_solve(solver._h, None, C.byref(p), None) == _drc.EINVAL
    assert lib.catdrc_solve(None, None, C.byref(p), C.byref(o)) == _drc.EINVAL
    assert lib.catdrc_create(0, None) == _drc.EINVAL and lib.catdrc_create(-1, C.byref(C.c_void_p())) == _drc.EINVAL
    p.nspecies, p.nadsorbates, p.nsteps, p.residual_tol, p.site_density = 2, 1, 2, 1e-8, 1e-5
    assert lib.catdrc_solve(solver._h, None, C.byref(p), C.byref(o)) == _drc.EINVAL and b'are required' in lib.catdrc_last_error(solver._h)
    # n = 0 is valid, with host arrays and with a view no device stands behind; a given sigma needs no capacitance
    out = solver.solve(None, chain(S=2), np.zeros(0), np.zeros((0, 3)), csurf=np.zeros((0, 2)), phi_surface=np.zeros(0), fields=ALL,
                       sigma=np.zeros(0), stern_capacitance=np.nan)
    assert out['drc'].shape == (0, 3, 2) and out['tdrc'].shape == (0, 2, 2) and out['dy_drc'].shape == (0, 3, 3) and out['dflux_dG'].shape == (0, 2, 2)
    assert out['status'].shape == (0,) and out['status'].dtype == np.int32 and out['residual'].shape == (0,)
    out = solver.solve(fake_view(), chain(), np.zeros(0), np.zeros((0, 2)), lanes=[])
    assert out['flux'].shape == (0, 2)
    with pytest.raises(ValueError, match='unknown field'):
        solver.solve(None, chain(), np.zeros(0), np.zeros((0, 2)), csurf=np.zeros((0, 2)), phi_surface=np.zeros(0), fields=['theta'])
    assert solver.last_kernel == '' and solver.last_kernel_ms == -1.0


def test_the_library_holds_the_one_kernel_and_the_others_gained_none(libpath):
    from catint_amd import _capi, build as B
    try:
        assert K.compiled_kernels(lib=libpath) == INSTANCES
        for f, lib in ((B.build_kinetics_library, B.KINETICS_LIB), (B.build_couple_library, B.COUPLE_LIB), (B.build_sens_library, B.SENS_LIB)):
            f()
            assert not [n for n in K.compiled_kernels(lib=lib) if 'catdrc' in n or 'control_kernel' in n]
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert not [s for s in _capi.SYMBOLS if 'drc' in s or 'rate_control' in s]          # no pnp_* symbol was added for it
    assert hasattr(_capi.PnpSolver, 'get_rate_control')


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def restated(name):
    """(case, fp64 kinetics, fp64 rate control at its coverages), computed once per case"""
    if name not in restated.cache:
        c = KC.case(name)
        fp = KC.references(name)[0]
        restated.cache[name] = (c, fp, DR.control_fp64(c.tables, c.phiM, c.csurf, c.phi_surface, fp['theta'], **c.kw))
    return restated.cache[name]


restated.cache = {}


@pytest.mark.parametrize('name', KC.CASE_NAMES)
def test_fp64_restatement_against_60_digits(name):
    """Every point is a converged state well inside the clamp (status 0, residual at rounding); the fp64 restatement agrees with the same
    formulas at 60 digits to 1e-12 of drc_scale in every field, the bound tests/test_kinetics_abi.py sets its sensitivities: four
    orders above the 1e-16 of the format for sums of up to R T terms behind a solve of order T."""
    c, fp, r = restated(name)
    ref = DR.control_mp(c.tables, c.phiM, c.csurf, c.phi_surface, fp['theta'], **c.kw)
    err = DR.errors(r, ref, r)
    print(name, 'residual %.1e' % r['residual'].max(), {k: '%.1e' % v.max() for k, v in err.items()})
    assert (r['status'] == 0).all() and r['residual'].max() <= 1e-12
    assert (np.log(fp['theta']) > KR.MIN_LOG + 1.0).all()          # no coverage sits at the clamp
    assert float(max(abs(v) for v in ref['residual'])) <= 1e-12
    for k, v in err.items():
        assert v.max() <= 1e-12, (k, v.max())


@pytest.mark.parametrize('name', KC.CASE_NAMES)
def test_sum_rule_split_and_chain_rule(name):
    c, fp, r = restated(name)
    t = KR._arrays(c.tables)
    N, R = t['N'], t['R']
    sc = r['drc_scale']
    # I1: in units of the sum of the terms of the left-hand side and of the flux
    i1 = np.abs(r['dflux_drc'].sum(axis=1) - r['flux']) / (sc['dflux_drc'].sum(axis=1) + r['flux_scale'] + 1e-300)
    # I2
    i2 = np.abs(r['dflux_drc'] - r['dflux_dlnkf'] - r['dflux_dlnkb']) / (sc['dflux_drc'] + sc['dflux_dlnkf'] + sc['dflux_dlnkb'] + 1e-300)
    # I3: the kinetics reference's own dflux_dphi against the chain rule through ln kf, ln kb
    i3 = np.zeros((len(c.phiM), N, 2))
    for i in range(len(c.phiM)):
        V, sg = KR.potential_and_charge(c.phiM[i], c.phi_surface[i], c.kw['w'], c.kw['CS'], c.kw['phi_pzc'], None)
        _, _, br = KR.rate_constants(t, V, sg, np.zeros((R, 2)))
        for q, (dV, ds) in enumerate(((1.0, c.kw['CS']), (-1.0 if c.kw['w'] else 0.0, -c.kw['CS']))):
            dlf, dlb = KR.slopes(t, sg, br, dV, ds)
            chain_rule = dlf @ r['dflux_dlnkf'][i] + dlb @ r['dflux_dlnkb'][i]
            terms = np.abs(dlf) @ sc['dflux_dlnkf'][i] + np.abs(dlb) @ sc['dflux_dlnkb'][i] + fp['dflux_scale'][i][:, N + q]
            i3[i, :, q] = np.abs(chain_rule - fp['dflux_dphi'][i][:, q]) / (terms + 1e-300)
    print(name, 'I1 %.1e  I2 %.1e  I3 %.1e (units of the term sums)' % (i1.max(), i2.max(), i3.max()))
    # Each identity is linear in fields whose error against 60 digits is bounded by 1e-12 of their scales
    # (test_fp64_restatement_against_60_digits, tests/test_kinetics_abi.py for dflux_dphi), and the units here are the sums of those
    # scales: 1e-12.  I1 holds at F = 0 only: the state's residual enters it once
    assert i1.max() <= 1e-12 + r['residual'].max() and i2.max() <= 1e-12 and i3.max() <= 1e-12


def shifted(tab, r=None, s=None, h=0.0):
    """The tables with the transition state of step r lowered by h kT (Ea of a step that has one), or the free energy of adsorbate s
    lowered by h kT at fixed transition states"""
    t = {k: np.array(v) if isinstance(v, np.ndarray) else v for k, v in tab.items()}
    if r is not None:
        t['Ea'][r, 0] -= h
    else:
        N = t['order_f'].shape[1] - len(t['site_count'])
        m = (t['order_b'] - t['order_f'])[:, N + s]
        t['dG'][:, 0] += -m * h
        t['Ea'][:, 0] += t['order_f'][:, N + s] * h          # (-inf stays -inf: no transition state)
    return t


@pytest.mark.parametrize('name', KC.CASE_NAMES)
def test_central_differences_of_resolved_steady_states(name):
    """d flux / d off[r][0], d off[r][1] through solve_fp64(off=...); the transition-state and adsorbate columns through shifted Ea / dG
    tables (a transition-state column only where Ea is the branch of Ga at the point: elsewhere the table does not move the rate
    constants, and the column is covered by I2).  h = 1e-5 and h / 2; per point and species the tolerance is 10 x the largest
    |FD(h) - FD(h/2)| over the columns (the differences' own truncation and rounding), printed in units of flux_scale."""
    c, fp, r = restated(name)
    t = KR._arrays(c.tables)
    N, R, S = t['N'], t['R'], t['S']
    n = len(c.phiM)

    def flux(tab, off):
        return KR.solve_fp64(tab, c.phiM, c.csurf, c.phi_surface, off=off, theta_guess=fp['theta'], sens=False, **c.kw)['flux']

    def fd(make, h):
        plus, minus = make(h), make(-h)
        return (flux(*plus) - flux(*minus)) / (2 * h)

    def off_col(rr, side):
        def make(h):
            off = np.zeros((n, R, 2))
            off[:, rr, side] = h
            return c.tables, off
        return make
    columns = [(off_col(rr, 0), r['dflux_dlnkf'][:, rr], None) for rr in range(R)] + [(off_col(rr, 1), r['dflux_dlnkb'][:, rr], None) for rr in range(R)]
    branch = np.zeros((n, R), int)
    for i in range(n):
        V, sg = KR.potential_and_charge(c.phiM[i], c.phi_surface[i], c.kw['w'], c.kw['CS'], c.kw['phi_pzc'], None)
        branch[i] = KR.rate_constants(t, V, sg, np.zeros((R, 2)))[2]
    for rr in range(R):
        if (branch[:, rr] == 0).any():
            columns.append((lambda h, rr=rr: (shifted(c.tables, r=rr, h=h), None), r['dflux_drc'][:, rr], branch[:, rr] == 0))
    for s in range(1, S + 1):
        columns.append((lambda h, s=s: (shifted(c.tables, s=s, h=h), None), r['dflux_dG'][:, s - 1], None))
    assert len(columns) > 2 * R + S or not (branch == 0).any()
    h = 1e-5
    err, spread = np.zeros((n, N)), np.zeros((n, N))
    for make, analytic, where in columns:
        a, b = fd(make, h), fd(make, h / 2)
        use = np.ones(n, bool) if where is None else where
        err = np.maximum(err, np.where(use[:, None], np.abs(b - analytic), 0.0))
        spread = np.maximum(spread, np.where(use[:, None], np.abs(a - b), 0.0))
    scale = np.where(fp['flux_scale'] > 0, fp['flux_scale'], 1.0)
    print(name, '%d columns: worst |FD(h/2) - analytic| %.1e, worst tolerance 10 |FD(h) - FD(h/2)| %.1e (units of flux_scale); worst ratio %.2f'
          % (len(columns), (err / scale).max(), (10 * spread / scale).max(), (err / np.where(spread > 0, 10 * spread, 1.0))[spread > 0].max(initial=0.0)))
    assert (err <= 10.0 * spread).all(), (err / scale).max()


def test_apparent_algebra_against_numpy():
    rng = np.random.RandomState(3)
    n, P, N = 5, 7, 4
    raw = rng.randn(n, P, N)
    kin = {'dflux_dc': 0.3 * rng.randn(n, N, N), 'dflux_dphi': rng.randn(n, N, 2)}
    cp = {'T_c': 0.5 * rng.randn(n, N, N), 'T_phi': 0.2 * rng.randn(n, N)}
    # point 3: a singular Newton matrix (K_c T_c = I, no potential part)
    kin['dflux_dc'][3], kin['dflux_dphi'][3], cp['T_c'][3] = np.eye(N), 0.0, np.eye(N) / 1.7
    got = _drc.apparent(raw, kin, cp, rf=1.7)
    for i in range(n):
        if i == 3:
            assert np.isnan(got[i]).all()
            continue
        want = DR.apparent(raw[i], kin['dflux_dc'][i], kin['dflux_dphi'][i][:, 1], cp['T_c'][i], cp['T_phi'][i], rf=1.7)
        assert np.allclose(got[i], want, rtol=1e-13, atol=0)
        # the defining relation: g' = rf (raw + K_c T_c g' + K_phi T_phi . g')
        M = kin['dflux_dc'][i] @ cp['T_c'][i] + np.outer(kin['dflux_dphi'][i][:, 1], cp['T_phi'][i])
        assert np.allclose(got[i], 1.7 * (raw[i] + got[i] @ M.T), rtol=1e-10, atol=1e-12)
    # no transport answer: the apparent derivative is rf times the intrinsic one
    flat = _drc.apparent(raw, kin, {'T_c': np.zeros((n, N, N)), 'T_phi': np.zeros((n, N))}, rf=2.0)
    assert np.array_equal(flat, 2.0 * raw)
    nu = np.array([[1.0, 0.0, 0.0, -1.0], [0.0, 0.0, 2.0, 0.0]])
    flux = rng.randn(n, N)
    q = _drc.normalised(raw, flux, nu)
    assert (q[:, :, 1] == 0.0).all() and np.array_equal(q[:, :, [0, 2, 3]], (raw / flux[:, None, :])[:, :, [0, 2, 3]])


# ---- the calculator's opt-in, with fakes -------------------------------------------------------------------------------------------
class FakeRateControl(object):
    """RateControl's solve on the CPU restatement; records every call"""
    made = []

    def __init__(self):
        self.calls, self.closed = [], False
        FakeRateControl.made.append(self)

    def solve(self, view, tab, phiM, theta, csurf=None, phi_surface=None, potential_drop='stern', stern_capacitance=0.0, phi_pzc=0.0, gamma=None,
              fields=None, **kw):
        assert view is None
        r = DR.control_fp64(tab, phiM, csurf, phi_surface, theta, w=1 if potential_drop == 'stern' else 0, CS=stern_capacitance, phi_pzc=phi_pzc,
                            gamma=gamma)
        self.calls.append({'theta': np.array(theta), 'csurf': np.array(csurf), 'fields': tuple(fields)})
        return {k: r[k] for k in tuple(fields) + ('status', 'residual')}

    def close(self):
        self.closed = True


def test_the_calculator_option_adds_the_keys_and_its_absence_nothing(monkeypatch):
    from catint_amd.calculator import Calculator
    from tests.test_kinetics_abi import FakeKinetics, scf_parts
    results = {}
    for option in (False, True):
        tp, model, transport_fn = scf_parts()
        calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-9)
        calc.set_microkinetics(model, site_density=2e-6, **({'rate_control': True} if option else {}))
        fake = FakeKinetics()
        monkeypatch.setattr(calc, '_kinetics_solver', lambda _f=fake: _f)
        FakeRateControl.made = []
        if option:
            monkeypatch.setattr(calc, '_rate_control_solver', FakeRateControl)
        else:
            def never():
                raise AssertionError('a rate-control context was created without the option')
            monkeypatch.setattr(calc, '_rate_control_solver', never)
        results[option] = (calc.run_scf_cycle(transport_fn=transport_fn, max_iter=200), tp, fake, list(FakeRateControl.made), model)
    off, tp0, fake0, _, _ = results[False]
    on, tp1, fake1, made, model = results[True]
    assert 'rate_control' not in off and all('rate_control' not in tp0.alldata[i]['system'] for i in range(3))
    # the loop itself is unchanged: same iterates, one more kinetics call (at the final surface state), one rate-control call
    assert len(fake0.calls) == off['iterations'] and len(fake1.calls) == on['iterations'] + 1 and on['iterations'] == off['iterations']
    for k in ('flux', 'surface_concentration', 'coverage'):
        assert np.array_equal(on[k], off[k]), k
    assert len(made) == 1 and made[0].closed and len(made[0].calls) == 1 and fake1.closed
    assert np.array_equal(made[0].calls[0]['csurf'], on['surface_concentration']) and np.array_equal(made[0].calls[0]['theta'], fake1.calls[-1]['theta'])
    rc = on['rate_control']
    assert set(rc) == {'drc', 'tdrc', 'status', 'residual', 'kinetic_status'}
    R, S, N = 2, 1, 3
    assert rc['drc'].shape == (3, R, N) and rc['tdrc'].shape == (3, S, N) and (rc['status'] == 0).all() and rc['residual'].max() <= 1e-12
    # the sum rule on the normalised coefficients of the species the mechanism touches; exactly 0 for the one it does not (K+)
    assert np.allclose(rc['drc'][:, :, 1:].sum(axis=1), 1.0, rtol=0, atol=1e-9) and (rc['drc'][:, :, 0] == 0.0).all()
    for i in range(3):
        got = tp1.alldata[i]['system']['rate_control']
        assert set(got) == set(rc) and np.array_equal(got['drc'], rc['drc'][i]) and np.array_equal(got['tdrc'], rc['tdrc'][i])
    # they are the restatement's at the final state
    tab = dict(model.tables(), site_density=2e-6)
    ref = DR.control_fp64(tab, np.array([-0.3, -0.4, -0.5]), on['surface_concentration'], 0.1 * np.array([-0.3, -0.4, -0.5]), made[0].calls[0]['theta'],
                          w=1, CS=0.2, phi_pzc=0.16)
    assert np.array_equal(ref['drc'], rc['drc'])
