"""libcatint_interact without a GPU (the method of tests/test_kinetics_abi.py, whose table helpers it uses): the library builds for
gfx950 and exports what include/catint_interact.h declares, the ctypes mirrors have the compiler's layouts, every validation error is
returned before any device call, n = 0 makes none, the library holds the one kernel.  Every parity case of tests/interact_cases.py
converges in the fp64 reference at every point.  InteractingModel: the parser that keeps the site suffix, the column layout, the
geometric-mean rule, the transition-state rows, units and errors; MeanFieldModel still refuses two site types.  The routing of
PnpSolver.get_kinetics and Calculator.set_microkinetics is driven with fakes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import interact_cases as IC
from tests import interact_ref as IR
from tests import kernel_census as K
from tests import kinetics_cases as KC
from tests.test_kinetics_abi import chain, edit, fake_view, header_source, host_args, poke, scf_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {'catia_params': 'CatiaParams', 'catia_outputs': 'CatiaOutputs'}
INSTANCES = {'catia::interact_kernel'}


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', IC.CASE_NAMES)
def test_every_point_of_every_parity_case_converges_in_the_reference(name):
    c = IC.case(name)
    fp = IC.fp64(name)
    assert (fp['status'] == 0).all() and (fp['ramp_reached'] == c.ramp - 1).all() and fp['iterations'].max() <= c.ramp * 200
    N, G, S, R = IR.shape(c.tables)
    assert 1 <= G <= 3 and G + S <= 9
    # the interaction is visible: some binding energy moves by more than a tenth of kT
    assert np.abs(fp['energy_shift']).max() > 0.1, np.abs(fp['energy_shift']).max()
    x = np.asarray(c.tables['site_fraction'])
    for g in range(G):
        on = np.asarray(c.tables['site_of']) == g
        assert np.allclose((fp['theta'] * c.tables['site_count'])[:, on].sum(axis=1), x[g], rtol=1e-12, atol=0)


def test_the_interaction_lowers_the_coverages_of_the_four_step_mechanism():
    """The largest adsorbate coverage over the lattice: 0.91 in the mean-field model, 0.21 with 0.3 / 0.15 eV, 0.08 with 1.0 / 0.5 eV"""
    from tests import kinetics_ref as KR
    c = KC.case('co2r_one_site')
    top = [KR.solve_fp64(c.tables, c.phiM, c.csurf, c.phi_surface, sens=False, **c.kw)['theta'][:, 1:].max()]
    top += [IC.fp64('co2r_one_site_' + tag)['theta'][:, 1:].max() for tag in ('weak', 'strong')]
    assert abs(top[0] - 0.91) < 0.01 and abs(top[1] - 0.21) < 0.01 and abs(top[2] - 0.08) < 0.01, top


def test_a_point_that_fails_without_the_ramp_converges_with_it():
    """... found on the CPU for tests/test_gpu_interact.py: the two-site variant with the strong interaction at one stage stops at maxit
    at 9 of the 39 points; in five stages every point converges"""
    c = IC.case('co2r_two_site_strong')
    one = IR.solve_fp64(c.tables, c.phiM, c.csurf, c.phi_surface, ramp=1, sens=False, **c.kw)
    assert (one['status'] == 1).sum() == 9 and (one['status'] == 0).sum() == 30
    assert (IC.fp64('co2r_two_site_strong')['status'] == 0).all()


# ---- InteractingModel ----------------------------------------------------------------------------------------------------------------
def test_the_parser_keeps_the_site_suffix():
    from catint_amd.interactions import parse_step
    st = parse_step('H*_s + CO*_t <-> HCO-TS_t <-> CHO*_t + *_s; beta=0.4')
    assert st['reactants'] == {('H', 's'): 1, ('CO', 't'): 1} and st['products'] == {('CHO', 't'): 1, ('*', 's'): 1}
    assert st['ts'] == ('HCO-TS', 't') and st['beta'] == 0.4 and st['electrons'] == 0
    st = parse_step('CO2_g + 2*_t + ele_g <-> CO2*_t')
    assert st['reactants'] == {'CO2_g': 1, ('*', 't'): 2} and st['electrons'] == 1 and st['ts'] is None


def test_one_site_type_gives_the_mean_field_tables_plus_the_new_keys():
    from catint_amd.interactions import INTERACTION_KEYS, has_interactions
    for variant in ('one_site', 'two_site'):
        a = KC.co2r_model(variant).tables()
        b = IC.co2r_model(variant, 0.3, 0.15).tables()
        assert set(b) == set(a) | set(INTERACTION_KEYS) and has_interactions(b) and not has_interactions(a)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
        kT = KC.co2r_model(variant).kT
        assert list(b['site_of']) == [0, 0, 0, 0] and list(b['site_fraction']) == [1.0] and b['strength'] == 1.0 and b['response'] == 'linear'
        assert np.allclose(b['eps'], (0.15 + 0.15 * np.eye(3)) / kT, rtol=1e-14)
        # the row of the one transition state (step 2: COOH* -> CO*) is the mean of the rows of its initial and final state
        of, ob = b['order_f'][:, 4:].astype(float), b['order_b'][:, 4:].astype(float)
        assert np.allclose(b['eps_ts'][2], 0.5 * (of[2] + ob[2]) @ b['eps'], rtol=1e-14) and (b['eps_ts'][[0, 1, 3]] == 0.0).all()


def test_two_site_types_columns_cross_terms_and_ts_rows():
    m = IC.terrace_step_model()
    t = m.tables()
    kT = m.kT
    assert list(t['site_of']) == [0, 1, 0, 0, 0, 1, 1] and list(t['site_fraction']) == [0.9, 0.1] and list(t['site_count']) == [1.0] * 7
    N = 3
    # 'CO*_t + *_s <-> CO*_s + *_t':   columns *_t *_s CO2 COOH CO_t CO_s H
    assert t['order_f'][4, N:].tolist() == [0, 1, 0, 0, 1, 0, 0] and t['order_b'][4, N:].tolist() == [1, 0, 0, 0, 0, 1, 0]
    assert t['order_f'][6, N:].tolist() == [0, 1, 0, 0, 0, 0, 0] and t['order_b'][6].tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0, 1]
    e = t['eps'] * kT
    assert np.isclose(e[2, 3], np.sqrt(0.3 * 0.5)) and np.isclose(e[3, 2], e[2, 3])          # CO_t x CO_s: the geometric mean
    assert np.isclose(e[0, 1], 0.2) and np.isclose(e[4, 3], 0.1) and e[4, 4] == 0.0 and e[4, 0] == 0.0          # H has no self term: no mean
    assert np.array_equal(t['eps'], t['eps'].T)
    # explicit transition-state rows
    m2 = IC.terrace_step_model(ts_interactions={'COOH-ele': {'CO_t': 0.25}})
    row = m2.tables()['eps_ts'][2] * kT
    assert np.allclose(row, [0.0, 0.0, 0.25, 0.0, 0.0])
    # the piecewise response with per-type parameters
    m3 = IC.terrace_step_model(response='piecewise', cutoff={'t': 0.25, 's': 0.5}, smoothing=0.05, strength=0.5)
    t3 = m3.tables()
    assert t3['response'] == 'piecewise' and list(t3['cutoff']) == [0.25, 0.5] and list(t3['smoothing']) == [0.05, 0.05] and t3['strength'] == 0.5


def test_string_and_dict_forms_give_identical_tables():
    from catint_amd.interactions import InteractingModel
    dicts = [{'reactants': {'X_g': 1, '*_t': 1}, 'products': {'A': 1}}, {'reactants': {'A': 1, '*_s': 1}, 'products': {'B': 1, '*_t': 1}, 'ts': 'TS'},
             {'reactants': {'B': 1}, 'products': {'Y_g': 1, '*_s': 1}, 'electrons': -1}]
    strings = ['X_g + *_t <-> A*_t', 'A*_t + *_s <-> TS_t <-> B*_s + *_t', 'B*_s <-> Y_g + *_s + ele_g']
    kw = dict(interactions={('A', 'A'): 0.2, ('B', 'B'): 0.4}, site_fractions={'t': 0.7, 's': 0.3})
    a, b = (InteractingModel(['X', 'Y'], {'A': ('t', 1), 'B': ('s', 1)}, s, {'A': 0.1, 'B': 0.2, 'TS': 0.9}, **kw).tables() for s in (dicts, strings))
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_model_errors_are_clear():
    from catint_amd.interactions import InteractingModel
    from catint_amd.microkinetics import MeanFieldModel, MicrokineticsError

    def make(steps, ads={'A': ('t', 1), 'B': ('s', 1)}, fr={'t': 0.5, 's': 0.5}, **kw):
        return InteractingModel(['X', 'Y'], ads, steps, {'A': 0.1, 'B': 0.2, 'TS': 0.9}, site_fractions=fr, **kw)
    ok = ['X_g + *_t <-> A*_t', 'A*_t + *_s <-> B*_s + *_t', 'B*_s <-> Y_g + *_s']
    make(ok)
    with pytest.raises(MicrokineticsError, match="conserve the sites of type 't'"):
        make(['X_g + *_t <-> A*_t', 'A*_t <-> B*_s'])
    with pytest.raises(MicrokineticsError, match="puts 'A' on the site type 's'"):
        make(['X_g + *_s <-> A*_s'])
    with pytest.raises(MicrokineticsError, match="unknown site type 'q'"):
        make(['X_g + *_q <-> A*_t'])
    with pytest.raises(MicrokineticsError, match='has no fraction'):
        make(ok, ads={'A': ('t', 1), 'B': ('u', 1)})
    with pytest.raises(MicrokineticsError, match='site types: 1 .. 3'):
        make(ok, fr={'t': 0.25, 's': 0.25, 'u': 0.25, 'v': 0.25})
    with pytest.raises(MicrokineticsError, match='positive and finite'):
        make(ok, fr={'t': 1.0, 's': 0.0})
    with pytest.raises(MicrokineticsError, match='site_fractions is needed'):
        make(ok, fr=None)
    with pytest.raises(MicrokineticsError, match="names 'C', which is no adsorbate"):
        make(ok, interactions={('A', 'C'): 0.1})
    with pytest.raises(MicrokineticsError, match='not finite'):
        make(ok, interactions={('A', 'A'): np.inf})
    with pytest.raises(MicrokineticsError, match='given twice'):
        make(ok, interactions={('A', 'B'): 0.1, ('B', 'A'): 0.2})
    with pytest.raises(MicrokineticsError, match='response'):
        make(ok, response='cubic')
    with pytest.raises(MicrokineticsError, match='smoothing must be positive'):
        make(ok, response='piecewise', smoothing=0.0)
    with pytest.raises(MicrokineticsError, match="names no site type"):
        make([{'reactants': {'X_g': 1, '*': 1}, 'products': {'A': 1}}])
    with pytest.raises(MicrokineticsError, match='at most 9 columns'):
        InteractingModel(['X'], {'A%d' % i: ('t', 1) for i in range(8)}, [], {}, site_fractions={'t': 0.5, 's': 0.5})
    with pytest.raises(MicrokineticsError, match='occupies 4 sites'):
        make(ok, ads={'A': ('t', 4), 'B': ('s', 1)})
    # the mean-field model still refuses a step that names two sites
    with pytest.raises(MicrokineticsError, match='one site type'):
        MeanFieldModel(['X', 'Y'], {'A': 1, 'B': 2}, ['X_g + *_t <-> A*_s'], {'A': 0.1, 'B': 0.2})


# ---- the library -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_interact_library
    return build_interact_library()


@pytest.fixture(scope='module')
def solver(libpath):
    from catint_amd import _interact
    with _interact.InteractingKinetics(0) as o:
        yield o


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    from catint_amd import _interact
    declared = sorted(set(re.findall(r'\b(catia_[a-z0-9_]+)\s*\(', header_source('catint_interact.h'))))
    assert declared == sorted(_interact.SYMBOLS) and len(declared) == 6
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(catia_[a-z0-9_]+)\b', exported))) == declared
    assert not re.findall(r'\b(pnp|catkin)_[a-z0-9_]+\b', exported)


def test_a_library_of_its_own_that_leaves_the_shared_header_alone():
    from catint_amd import build
    assert build.INTERACT_SOURCES == ['catia.hip'] and os.path.isdir(build.INTERACT_DIR) and callable(build.interact_needs_build)
    assert os.path.dirname(build.INTERACT_LIB) == os.path.dirname(build.LIB)
    listed = {os.path.realpath(p) for p in build.INTERACT_HEADERS}
    for h in ('catint_interact.h', 'catint_pnp.h'):
        assert os.path.realpath(os.path.join(ROOT, 'include', h)) in listed
    assert os.path.realpath(os.path.join(build.CSRC, 'pnp_kin.h')) in listed
    from tests.test_build_deps import reached
    sources = [os.path.join(build.INTERACT_DIR, f) for f in build.INTERACT_SOURCES]
    assert not reached(sources) - listed - {os.path.realpath(f) for f in sources}
    assert 'build_interact_library(' in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    others = build.SOURCES + build.KINETICS_SOURCES + build.DRC_SOURCES + build.SCFKIN_SOURCES + build.KINTRANS_SOURCES + build.EIS_SOURCES
    assert not any('catia' in s or 'interact' in s for s in others)


def test_the_library_holds_the_one_kernel(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)


def header_structs():
    out = {}
    for body, struct in re.findall(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', header_source('catint_interact.h'), flags=re.S):
        fields = []
        for decl in body.split(';'):
            decl = decl.strip()
            if not decl:
                continue
            names = decl.split(None, 1)[1] if not decl.startswith('const') else decl.split(None, 2)[2]
            fields += [n.strip().lstrip('*').strip() for n in names.split(',')]
        out[struct] = fields
    return out


MACROS = {'maxspecies': 'CATIA_MAX_SPECIES', 'maxtypes': 'CATIA_MAX_SITE_TYPES', 'maxcols': 'CATIA_MAX_COLUMNS', 'maxsteps': 'CATIA_MAX_STEPS',
          'maxorder': 'CATIA_MAX_ORDER', 'maxsites': 'CATIA_MAX_SITES', 'minlog': '(int)CATIA_MIN_LOG', 'full': 'CATIA_DROP_FULL',
          'stern': 'CATIA_DROP_STERN', 'linear': 'CATIA_LINEAR', 'piecewise': 'CATIA_PIECEWISE', 'converged': 'CATIA_CONVERGED',
          'maxit': 'CATIA_MAXIT', 'input': 'CATIA_INPUT', 'pivot': 'CATIA_PIVOT', 'einval': 'CATIA_EINVAL', 'enomem': 'CATIA_ENOMEM',
          'edevice': 'CATIA_EDEVICE'}


@pytest.fixture(scope='module')
def compiler_layout(tmp_path_factory):
    structs = header_structs()
    assert set(PAIRS) <= set(structs)
    d = tmp_path_factory.mktemp('interact_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_interact.h"', 'int main(void) {']
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
    from catint_amd import _interact
    cls = getattr(_interact, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_of_the_binding_are_the_header_s(compiler_layout):
    from catint_amd import _interact as k
    from catint_amd import interactions as m
    n = {name: compiler_layout[name]['n'] for name in MACROS}
    assert (k.MAX_SPECIES, k.MAX_SITE_TYPES, k.MAX_COLUMNS, k.MAX_STEPS, k.MAX_ORDER, k.MAX_SITES) == \
        (n['maxspecies'], n['maxtypes'], n['maxcols'], n['maxsteps'], n['maxorder'], n['maxsites']) == (8, 3, 9, 16, 3, 3)
    assert k.MIN_LOG == n['minlog'] == -700 == IR.MIN_LOG
    assert k.DROP == {'full': n['full'], 'stern': n['stern']} and k.RESPONSE == {'linear': n['linear'], 'piecewise': n['piecewise']}
    assert (k.CONVERGED, k.MAXIT, k.INPUT, k.PIVOT) == (n['converged'], n['maxit'], n['input'], n['pivot']) == (0, 1, 2, 3)
    assert (k.EINVAL, k.ENOMEM, k.EDEVICE) == (n['einval'], n['enomem'], n['edevice'])
    assert (k.DEFAULT_TOL, k.DEFAULT_MAXIT, k.DEFAULT_RAMP, k.SCF_RAMP) == (1e-12, 200, 1, 10)
    assert (m.MAX_SITE_TYPES, m.MAX_COLUMNS) == (k.MAX_SITE_TYPES, k.MAX_COLUMNS)


def ia(t, **kw):
    """the mean-field tables `t` with the new keys: one site type without interactions, or what kw says"""
    T = len(t['site_count'])
    G = len(kw.get('site_fraction', np.ones(1)))
    S = max(T - G, 0)
    out = dict(t, site_of=np.zeros(T, np.int32), site_fraction=np.ones(1), eps=np.zeros((S, S)), strength=1.0)
    out.update(kw)
    return out


def two_types(broken=False):
    """X + *_0 <-> A;  A + *_1 <-> B + *_0;  B <-> Y + *_1   (columns X Y | *_0 *_1 A B);  broken: the second step is A <-> B"""
    of = np.array([[1, 0, 1, 0, 0, 0], [0, 0, 0, 0 if broken else 1, 1, 0], [0, 0, 0, 0, 0, 1]], np.int32)
    ob = np.array([[0, 0, 0, 0, 1, 0], [0, 0, 0 if broken else 1, 0, 0, 1], [0, 1, 0, 1, 0, 0]], np.int32)
    from tests.test_kinetics_abi import tables
    t = tables(of, ob, [[-1.0, 0.0], [0.0, 0.0], [0.0, 1.0]], np.ones(4), np.zeros((3, 4)))
    return dict(t, site_of=np.array([0, 1, 0, 1], np.int32), site_fraction=np.array([0.6, 0.4]), eps=np.zeros((2, 2)), strength=1.0)


PIECEWISE = dict(response='piecewise', cutoff=np.array([0.25]), smoothing=np.array([0.05]))


@pytest.mark.parametrize('what, make, word', [
    # what catkin_solve reports
    ('struct_size of the parameters', lambda: (None, ia(chain()), {'struct_size': 8}), 'catia_params.struct_size'),
    ('struct_size of the outputs', lambda: (None, ia(chain()), {'out_struct_size': 8}), 'catia_outputs.struct_size'),
    ('struct_size of the view', lambda: (fake_view(size=12), ia(chain()), {'csurf': None, 'phi_surface': None}), 'pnp_device_view.struct_size'),
    ('nine species', lambda: (None, ia(chain(N=9)), host_args(N=9)), '9 species'),
    ('no step', lambda: (None, ia(edit(chain(), order_f=np.zeros((0, 4), np.int32), order_b=np.zeros((0, 4), np.int32), nu=np.zeros((0, 2)),
                                       dG=np.zeros((0, 4)), Ea=np.zeros((0, 4)), lnA=np.zeros(0))), {}), '0 steps'),
    ('seventeen steps', lambda: (None, ia(chain(R=17)), {}), '17 steps'),
    ('an order of 4', lambda: (None, ia(edit(chain(), f=poke('order_f', (0, 0), 4))), {}), 'order'),
    ('a step that does not conserve sites', lambda: (None, ia(edit(chain(), f=poke('order_f', (0, 2), 2))), {}), 'conserve'),
    ('an empty step', lambda: (None, ia(edit(chain(S=2, R=4), f=lambda t: (t['order_f'].__setitem__(3, 0), t['order_b'].__setitem__(3, 0),
                                                                          t['nu'].__setitem__(3, 0.0)))), {}), 'empty step'),
    ('a zero cref', lambda: (None, ia(edit(chain(), cref=np.array([1.0, 0.0]))), {}), 'cref[1]'),
    ('a NaN site density', lambda: (None, ia(edit(chain(), site_density=np.nan)), {}), 'site_density'),
    ('a zero tolerance', lambda: (None, ia(chain()), {'tol': 0.0}), 'tol'),
    ('a site count of 4', lambda: (None, ia(edit(chain(), site_count=np.array([1.0, 4.0]))), {}), 'site count 1'),
    ('a free site that takes two sites', lambda: (None, ia(edit(chain(), site_count=np.array([2.0, 1.0]))), {}), 'its site count 1'),
    ('maxit 0', lambda: (None, ia(chain()), {'maxit': 0}), 'maxit'),
    ('potential_drop 2', lambda: (None, ia(chain()), {'potential_drop': 2}), 'potential_drop'),
    ('negative max_waves', lambda: (None, ia(chain()), {'max_waves': -1}), 'max_waves'),
    ('a NaN in dG', lambda: (None, ia(edit(chain(), f=poke('dG', (1, 2), np.nan))), {}), 'step 1 has a non-finite'),
    ('e0 = +inf', lambda: (None, ia(edit(chain(), f=poke('Ea', (0, 0), np.inf))), {}), 'step 0 has a non-finite'),
    ('a NaN nu', lambda: (None, ia(edit(chain(), f=poke('nu', (0, 0), np.nan))), {}), 'nu of step 0'),
    ('csurf without phi_surface', lambda: (None, ia(chain()), {'phi_surface': None}), 'come together'),
    ('no view and no surface state', lambda: (None, ia(chain()), {'csurf': None, 'phi_surface': None}), 'null view'),
    ('compat handle: no potential row', lambda: (fake_view(phi=None), ia(chain()), {'csurf': None, 'phi_surface': None}), 'potential'),
    ('a lane outside the batch', lambda: (fake_view(), ia(chain()), {'csurf': None, 'phi_surface': None, 'lanes': [0, 2]}), 'lane index 2'),
    ('more points than lanes', lambda: (fake_view(B=1), ia(chain()), {'csurf': None, 'phi_surface': None}), 'above the batch'),
    ('N different from the view', lambda: (fake_view(N=3), ia(chain()), {'csurf': None, 'phi_surface': None}), 'the view has 3'),
    ('no sigma and an infinite capacitance', lambda: (None, ia(chain()), {'stern_capacitance': np.inf}), 'surface charge'),
    # what this library adds
    ('no site type', lambda: (None, ia(chain(), site_fraction=np.zeros(0)), {}), '0 site types'),
    ('four site types', lambda: (None, ia(chain(S=4), site_fraction=np.full(4, 0.25)), {}), '4 site types'),
    ('no adsorbate', lambda: (None, ia(chain(S=1), site_fraction=np.array([0.5, 0.5]), site_of=np.array([0, 1], np.int32)), {}), '0 adsorbates'),
    ('ten columns', lambda: (None, ia(chain(S=9)), {}), 'at most 9 columns'),
    ('a site_of out of range', lambda: (None, ia(chain(S=2), site_of=np.array([0, 0, 5], np.int32)), {}), 'site_of[2] = 5 outside'),
    ('a negative site_of', lambda: (None, ia(chain(S=2), site_of=np.array([0, -1, 0], np.int32)), {}), 'site_of[1] = -1 outside'),
    ('a free-site column on another type', lambda: (None, dict(two_types(), site_of=np.array([1, 0, 0, 1], np.int32)), {}), 'free site of type 0'),
    ('a zero fraction', lambda: (None, dict(two_types(), site_fraction=np.array([1.0, 0.0])), {}), 'site_fraction[1]'),
    ('a NaN fraction', lambda: (None, ia(chain(), site_fraction=np.array([np.nan])), {}), 'site_fraction[0]'),
    ('a step that breaks the balance of a type', lambda: (None, two_types(broken=True), {}), 'conserve the sites of type 0'),
    ('a NaN in eps', lambda: (None, ia(chain(S=2), eps=np.array([[0.0, np.nan], [0.0, 0.0]])), {}), 'eps has a non-finite'),
    ('an infinite eps_ts', lambda: (None, ia(chain(S=2), eps_ts=np.array([[0.0, 0.0], [np.inf, 0.0], [0.0, 0.0]])), {}), 'eps_ts has a non-finite'),
    ('an infinite strength', lambda: (None, ia(chain()), {'strength': np.inf}), 'strength'),
    ('a NaN strength', lambda: (None, ia(chain(), strength=np.nan), {}), 'strength'),
    ('ramp 0', lambda: (None, ia(chain()), {'ramp': 0}), 'ramp < 1'),
    ('a third response', lambda: (None, ia(chain(), response=2), {}), 'response is'),
    ('piecewise without parameters', lambda: (None, ia(chain(), response='piecewise'), {}), 'needs cutoff and smoothing'),
    ('a zero smoothing', lambda: (None, ia(chain(), **dict(PIECEWISE, smoothing=np.zeros(1))), {}), 'positive, finite smoothing'),
    ('a negative smoothing', lambda: (None, ia(chain(), **dict(PIECEWISE, smoothing=-np.ones(1))), {}), 'positive, finite smoothing'),
    ('a NaN cutoff', lambda: (None, ia(chain(), **dict(PIECEWISE, cutoff=np.full(1, np.nan))), {}), 'finite cutoff'),
])
def test_validation_errors_come_before_any_device_call(solver, what, make, word):
    from catint_amd import _interact
    view, tab, kw = make()
    N = np.asarray(tab['order_f']).shape[1] - len(tab['site_count'])
    args = host_args(N=max(N, 0))
    args.update(kw)
    with pytest.raises(_interact.InteractError) as e:
        solver.solve(view, tab, **args)
    assert e.value.code == _interact.EINVAL, (what, str(e.value))
    assert word in str(e.value), (what, str(e.value))
    assert solver.last_kernel == '' and solver.last_kernel_ms == -1.0


def test_null_arguments_and_null_context(solver):
    from catint_amd import _interact
    lib = _interact.load_library()
    p = _interact.CatiaParams(struct_size=C.sizeof(_interact.CatiaParams))
    o = _interact.CatiaOutputs(struct_size=C.sizeof(_interact.CatiaOutputs))
    assert lib.catia_solve(solver._h, None, None, C.byref(o)) == _interact.EINVAL
    assert b'null' in lib.catia_last_error(solver._h)
    assert lib.catia_solve(solver._h, None, C.byref(p), None) == _interact.EINVAL
    assert lib.catia_solve(None, None, C.byref(p), C.byref(o)) == _interact.EINVAL
    assert lib.catia_create(0, None) == _interact.EINVAL
    p.nspecies, p.nadsorbates, p.nsteps, p.maxit, p.tol, p.site_density, p.nsitetypes, p.ramp, p.strength = 2, 1, 2, 10, 1e-12, 1e-5, 1, 1, 1.0
    assert lib.catia_solve(solver._h, None, C.byref(p), C.byref(o)) == _interact.EINVAL
    assert b'site_of, site_fraction and eps are required' in lib.catia_last_error(solver._h)
    assert lib.catia_last_kernel(solver._h) == b''


def test_no_point_makes_no_device_call(solver):
    from catint_amd import _interact
    out = solver.solve(None, two_types(), np.zeros(0), csurf=np.zeros((0, 2)), phi_surface=np.zeros(0), fields=list(_interact.FIELDS), ramp=3)
    assert out['theta'].shape == (0, 4) and out['energy_shift'].shape == (0, 2) and out['rate'].shape == (0, 3) and out['dflux_dc'].shape == (0, 2, 2)
    assert out['status'].shape == (0,) and out['ramp_reached'].dtype == np.int32 and out['iterations'].dtype == np.int32
    out = solver.solve(fake_view(), ia(chain()), np.zeros(0), lanes=[])
    assert out['flux_scale'].shape == (0, 2) and solver.last_kernel == ''
    # the mean-field tables alone are one site type without interactions
    out = solver.solve(None, chain(S=3), np.zeros(0), csurf=np.zeros((0, 2)), phi_surface=np.zeros(0))
    assert out['theta'].shape == (0, 4) and out['energy_shift'].shape == (0, 3)


# ---- the routing, with fakes ---------------------------------------------------------------------------------------------------------
class FakeInteract(object):
    """InteractingKinetics.solve on the CPU reference; records every call"""

    def __init__(self, fail_warm=()):
        self.calls, self.closed, self.fail_warm = [], False, set(fail_warm)

    def _h(self):
        return None

    def solve(self, view, tab, phiM, csurf=None, phi_surface=None, potential_drop='stern', stern_capacitance=0.0, phi_pzc=0.0, gamma=None,
              theta_guess=None, fields=None, ramp=1, lanes=None, **kw):
        assert view is None
        r = IR.solve_fp64(tab, phiM, csurf, phi_surface, w=1 if potential_drop == 'stern' else 0, CS=stern_capacitance, phi_pzc=phi_pzc,
                          gamma=gamma, theta_guess=theta_guess, sens=False, ramp=ramp)
        if theta_guess is not None and len(self.calls) in self.fail_warm:
            r['status'][1] = 1
        self.calls.append({'guess': None if theta_guess is None else np.array(theta_guess), 'ramp': ramp, 'n': len(np.atleast_1d(phiM)),
                           'iterations': r['iterations'].copy(), 'theta': r['theta'].copy()})
        return {k: r[k] for k in ('theta', 'flux', 'flux_scale', 'energy_shift', 'status', 'iterations', 'ramp_reached')}

    def close(self):
        self.closed = True


def interacting_scf_parts(self_eV=0.3):
    from catint_amd.interactions import InteractingModel
    tp, _, transport_fn = scf_parts()
    model = InteractingModel(list(tp.species.keys()), {'CO2': ('t', 1)}, ['CO2_g + *_t <-> CO2*_t', 'CO2*_t + ele_g <-> TS_t <-> HCO3_g + *_t; beta=0.5'],
                             {'CO2': 0.1, 'TS': 0.6}, interactions={('CO2', 'CO2'): self_eV}, solution={'HCO3_g': 'HCO3-'}, site_density=1e-6)
    return tp, model, transport_fn


def ramped(fake, ramp):
    """catint_amd._interact.RampedKinetics over the fake: its solve with InteractingKinetics.solve replaced"""
    from catint_amd import _interact

    class Ramped(_interact.RampedKinetics):
        def __init__(self):
            self.ramp, self.retried = ramp, 0

        def close(self):
            fake.close()
    return Ramped()


def test_the_calculator_routes_an_interacting_model_to_the_new_library(monkeypatch):
    from catint_amd import _interact
    from catint_amd.calculator import Calculator
    tp, model, transport_fn = interacting_scf_parts()
    calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-9)
    calc.set_microkinetics(model, site_density=2e-6, ramp=4)
    assert calc.microkinetics['ramp'] == 4 and 'eps' in calc.microkinetics['tables']
    made = []
    monkeypatch.setattr(_interact.RampedKinetics, '__init__', lambda self, device=0, ramp=10: made.append((device, ramp)))
    calc._kinetics_solver()
    assert made == [(calc.device, 4)]
    # a mean-field model keeps the kinetics library
    tp2, mf, _ = scf_parts()
    calc2 = Calculator(transport=tp2, calc='comsol')
    calc2.set_microkinetics(mf)
    assert 'ramp' not in calc2.microkinetics
    from catint_amd import _kinetics
    monkeypatch.setattr(_kinetics.KineticsSolver, '__init__', lambda self, device=0: made.append('mean-field'))
    calc2._kinetics_solver()
    assert made[-1] == 'mean-field'


@pytest.mark.parametrize('fail_at', [(), (2,)])
def test_the_first_iteration_ramps_later_ones_warm_start_and_a_failed_lane_is_retried(monkeypatch, fail_at):
    from catint_amd import _interact
    from catint_amd.calculator import Calculator
    tp, model, transport_fn = interacting_scf_parts()
    calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-9)
    calc.set_microkinetics(model, site_density=2e-6, ramp=4)
    fake = FakeInteract(fail_warm=fail_at)
    monkeypatch.setattr(_interact.InteractingKinetics, 'solve', lambda self, *a, **kw: fake.solve(*a, **kw))
    solver = ramped(fake, 4)
    monkeypatch.setattr(calc, '_kinetics_solver', lambda: solver)
    out = calc.run_scf_cycle(transport_fn=transport_fn, max_iter=200)
    assert fake.closed and out['converged'].all() and not out['failed'].any()
    calls = fake.calls
    assert calls[0]['guess'] is None and calls[0]['ramp'] == 4 and calls[0]['n'] == 3
    warm = [c for c in calls[1:] if c['guess'] is not None]
    assert all(c['ramp'] == 1 and c['n'] == 3 for c in warm) and warm[-1]['iterations'].max() <= 3
    retries = [c for c in calls[1:] if c['guess'] is None]
    if fail_at:
        assert len(retries) == 1 and retries[0]['ramp'] == 4 and retries[0]['n'] == 1 and solver.retried == 1
        assert len(calls) == out['iterations'] + 1
    else:
        assert not retries and solver.retried == 0 and len(calls) == out['iterations']
    # the fluxes are the interacting model's at the final surface state
    tab = dict(model.tables(), site_density=2e-6)
    phis = np.array([-0.3, -0.4, -0.5])
    ref = IR.solve_fp64(tab, phis, out['surface_concentration'], 0.1 * phis, w=1, CS=0.2, phi_pzc=0.16, sens=False, ramp=4)
    assert np.allclose(ref['flux'], out['flux'], rtol=1e-6, atol=1e-30) and np.allclose(ref['theta'], out['coverage'], rtol=1e-6)


def test_with_zero_interactions_the_history_is_the_mean_field_run_s(monkeypatch):
    from catint_amd import _interact
    from catint_amd.calculator import Calculator
    from tests.test_kinetics_abi import FakeKinetics
    results = []
    for interacting in (False, True):
        tp, model, transport_fn = interacting_scf_parts(0.0) if interacting else scf_parts()
        calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-9)
        calc.set_microkinetics(model, site_density=2e-6)
        if interacting:
            fake = FakeInteract()
            monkeypatch.setattr(_interact.InteractingKinetics, 'solve', lambda self, *a, _f=fake, **kw: _f.solve(*a, **kw))
            solver = ramped(fake, 1)
        else:
            solver = FakeKinetics()
        monkeypatch.setattr(calc, '_kinetics_solver', lambda _s=solver: _s)
        results.append(calc.run_scf_cycle(transport_fn=transport_fn, max_iter=200))
    a, b = results
    assert a['iterations'] == b['iterations'] and np.array_equal(a['converged'], b['converged'])
    assert np.allclose(a['flux'], b['flux'], rtol=1e-12, atol=0) and np.allclose(a['coverage'], b['coverage'], rtol=1e-12, atol=0)
    assert np.allclose(a['accuracy'], b['accuracy'], rtol=1e-6, atol=1e-15)


@pytest.mark.parametrize('kw, word', [({'rate_control': True}, 'rate_control'), ({'device_loop': True}, 'device_loop'), ({'rescue': True}, 'rescue'),
                                      ({'impedance': [0.0, 10.0]}, 'impedance')])
def test_the_mean_field_libraries_refuse_an_interacting_model(kw, word):
    from catint_amd.calculator import Calculator, CalculatorError
    tp, model, _ = interacting_scf_parts()
    calc = Calculator(transport=tp, calc='comsol')
    with pytest.raises(CalculatorError, match='%s works on the mean-field model' % word):
        calc.set_microkinetics(model, **kw)
    with pytest.raises(CalculatorError, match='ramp'):
        calc.set_microkinetics(model, ramp=0)
    tp2, mf, _ = scf_parts()
    Calculator(transport=tp2, calc='comsol').set_microkinetics(mf, **({} if 'impedance' in kw else kw))          # the mean-field model: as before
