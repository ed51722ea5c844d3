"""libcatint_kinetics without a GPU (the method of tests/test_equil_abi.py).  The NumPy restatement of include/catint_kinetics.h
(tests/kinetics_ref.py, which tests/test_gpu_kinetics.py compares the device with) is checked against known answers -- the Langmuir
isotherm, the closed form of the reversible two-step cycle, detailed balance, kf / kb = exp(-dG) in the three branches of Ga -- and
against 60-digit solves on every case of tests/kinetics_cases.py.  MeanFieldModel: string and dict forms, bookkeeping, units, errors.
The library builds for gfx950 and exports what the header declares, the ctypes mirrors have the compiler's layouts, every validation
error is returned before any device call, the library holds the one kernel and the other six libraries gained none.  The calculator's
opt-in path is driven with fakes.

Worst errors of solve_fp64 against the 60-digit solves over all cases (tests/kinetics_cases.py: references;
printed by test_fp64_reference_against_60_digits): log-coverages 3.8e-14 (the CO2-free points of the four-step mechanism, where |y|
reaches 134 and exp / log of the comparison alone cost |y| eps), rates and fluxes 3.3e-14 of rate_gross / flux_scale, sensitivities
4.9e-14 of the sum of the absolute terms of an entry with the part from the linear solve counted as |J^-1| |J| |dy| (2.5e-8 of the
plain term sum with |dy| itself: an entry of size 1e-35 beside terms of 1e-25)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import kernel_census as K
from tests import kinetics_cases as KC
from tests import kinetics_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {'catkin_params': 'CatkinParams', 'catkin_outputs': 'CatkinOutputs'}
INSTANCES = {'catkin::steady_kernel'}


# ---- the reference against known answers -------------------------------------------------------------------------------------------
def tables(of, ob, nu, ns, dG, Ea=None, lnA=None, cref=None, sd=1e-5):
    of, ob = np.asarray(of, np.int32), np.asarray(ob, np.int32)
    R, N = of.shape[0], of.shape[1] - len(ns)
    dG = np.asarray(dG, float).reshape(R, 4)
    return {'order_f': of, 'order_b': ob, 'nu': np.asarray(nu, float).reshape(R, N), 'cref': np.ones(N) if cref is None else np.asarray(cref, float),
            'site_count': np.asarray(ns, float), 'dG': dG, 'Ea': np.tile([-np.inf, 0.0, 0.0, 0.0], (R, 1)) if Ea is None else np.asarray(Ea, float),
            'lnA': np.zeros(R) if lnA is None else np.asarray(lnA, float), 'site_density': sd}


def langmuir(lnK):
    # A + * <-> A*; columns: A | *, A*
    return tables([[1, 1, 0]], [[0, 0, 1]], [[-1.0]], [1.0, 1.0], [[-lnK, 0.0, 0.0, 0.0]])


def test_langmuir_isotherm():
    for lnK, a in ((2.0, 0.3), (-5.0, 4.0), (20.0, 1e-3), (0.0, 1.0)):
        r = KR.solve_fp64(langmuir(lnK), [0.0], [[a]], [0.0], sens=False)
        Ka = np.exp(lnK) * a
        assert r['status'][0] == 0
        assert abs(r['theta'][0, 1] - Ka / (1.0 + Ka)) <= 1e-13 * Ka / (1.0 + Ka)
        assert abs(r['theta'][0, 0] - 1.0 / (1.0 + Ka)) <= 1e-13 / (1.0 + Ka)
        assert abs(r['rate'][0, 0]) <= 1e-12 * r['rate_gross'][0, 0] or r['rate_gross'][0, 0] == 0.0


def two_step(dG1, dG2, lnA=(1.0, 0.5)):
    # A + * <-> A* <-> B + *; columns: A, B | *, A*
    return tables([[1, 0, 1, 0], [0, 0, 0, 1]], [[0, 0, 0, 1], [0, 1, 1, 0]], [[-1.0, 0.0], [0.0, 1.0]], [1.0, 1.0],
                  [[dG1, 0, 0, 0], [dG2, 0, 0, 0]], lnA=lnA)


def test_two_step_cycle_against_its_closed_form():
    for dG1, dG2, aA, aB in ((-1.0, -2.0, 0.5, 0.1), (3.0, -4.0, 2.0, 1e-3), (-6.0, 5.0, 1e-2, 3.0), (0.5, 0.5, 1.0, 0.0)):
        t = two_step(dG1, dG2)
        r = KR.solve_fp64(t, [0.0], [[aA, aB]], [0.0], sens=False)
        kf1, kf2 = np.exp(t['lnA'] - np.maximum([dG1, dG2], 0.0))
        kb1, kb2 = kf1 * np.exp(dG1), kf2 * np.exp(dG2)
        den = kf1 * aA + kb1 + kf2 + kb2 * aB
        theta, tof = (kf1 * aA + kb2 * aB) / den, (kf1 * kf2 * aA - kb1 * kb2 * aB) / den
        assert r['status'][0] == 0
        assert abs(r['theta'][0, 1] - theta) <= 1e-13 * theta
        assert abs(r['rate'][0, 0] - tof) <= 1e-13 * abs(tof) and abs(r['rate'][0, 1] - tof) <= 1e-13 * abs(tof)
        assert abs(r['flux'][0, 1] - 1e-5 * tof) <= 1e-13 * abs(1e-5 * tof)


def test_detailed_balance_at_the_overall_equilibrium():
    for dG1, dG2 in ((-1.0, -2.0), (4.0, -7.0), (-9.0, 3.0)):
        aA = 0.37
        aB = aA * np.exp(-(dG1 + dG2))          # a_B / a_A = K1 K2
        r = KR.solve_fp64(two_step(dG1, dG2), [0.0], [[aA, aB]], [0.0], sens=False)
        assert r['status'][0] == 0
        assert (np.abs(r['rate'][0]) <= 1e-12 * r['rate_gross'][0]).all(), r['rate'][0] / r['rate_gross'][0]


def test_kf_over_kb_is_exp_minus_dG_in_every_branch_of_Ga():
    t = KR._arrays(tables(np.zeros((3, 3), int) + [0, 1, 0], np.zeros((3, 3), int) + [0, 0, 1], np.zeros((3, 1)), [1.0, 1.0],
                          [[1.0, 2.0, 0.5, 0.1], [3.0, 2.0, 0.5, 0.1], [-3.0, 2.0, 0.5, 0.1]],
                          Ea=[[6.0, 1.0, 0.2, 0.0], [0.5, 1.0, 0.2, 0.0], [-np.inf, 0.0, 0.0, 0.0]], lnA=[1.0, 2.0, 3.0]))
    V, sg = 0.3, -0.2
    lf, lb, br = KR.rate_constants(t, V, sg, np.zeros((3, 2)))
    assert list(br) == [0, 1, 2]
    dG = t['dG'][:, 0] + t['dG'][:, 1] * V + t['dG'][:, 2] * sg + t['dG'][:, 3] * sg * sg
    assert np.allclose(lf - lb, -dG, rtol=0, atol=1e-15)
    Ea0 = 6.0 + 1.0 * V + 0.2 * sg
    assert np.isclose(lf[0], 1.0 - Ea0, atol=1e-15) and np.isclose(lf[1], 2.0 - dG[1], atol=1e-15) and lf[2] == 3.0
    # a tie takes the first of (Ea, dG, 0): the derivative of that branch
    t2 = KR._arrays(tables([[0, 1, 0]], [[0, 0, 1]], np.zeros((1, 1)), [1.0, 1.0], [[2.0, 1.0, 0.0, 0.0]], Ea=[[2.0, 0.5, 0.0, 0.0]]))
    _, _, br = KR.rate_constants(t2, 0.0, 0.0, np.zeros((1, 2)))
    assert br[0] == 0
    dlf, dlb = KR.slopes(t2, 0.0, br, 1.0, 0.0)
    assert dlf[0] == -0.5 and dlb[0] == 0.5


@pytest.mark.parametrize('name', KC.CASE_NAMES)
def test_fp64_reference_against_60_digits(name):
    """The fp64 reference converges on every point within 200 iterations (the four-step mechanism within 140 from the uniform surface)
    and agrees with the 60-digit root: log-coverages to 1e-13, rates and fluxes to 1e-13 of their gross scales, the sensitivities to
    1e-12 of the sum of the absolute terms of an entry (tests/kinetics_ref.py: for the part that comes out of the linear solve these are
    the terms of J^-1 (J dy), the componentwise bound of Gaussian elimination)."""
    fp, ref, err = KC.references(name)
    assert (fp['status'] == 0).all() and fp['iterations'].max() <= (140 if name.startswith('co2r') else 200)
    print(name, 'iterations %d .. %d' % (fp['iterations'].min(), fp['iterations'].max()), {k: '%.1e' % v.max() for k, v in err.items()})
    assert err['y'].max() <= 1e-13 and err['rate'].max() <= 1e-13 and err['flux'].max() <= 1e-13
    assert err['dflux_dc'].max() <= 1e-12 and err['dflux_dphi'].max() <= 1e-12


def test_sensitivities_are_the_derivatives_of_the_fluxes():
    """... also in fp64 alone: central differences of solve_fp64 on a well-conditioned point"""
    c = KC.case('co2r_two_site')
    i = 3          # -0.5 V, 30 mol/m^3
    base = KR.solve_fp64(c.tables, c.phiM[i:i + 1], c.csurf[i:i + 1], c.phi_surface[i:i + 1], **c.kw)
    for p in range(5):
        h = 1e-6
        out = []
        for sign in (1, -1):
            pm, cs, p0 = c.phiM[i:i + 1].copy(), c.csurf[i:i + 1].copy(), c.phi_surface[i:i + 1].copy()
            if p < 3:
                h = 1e-6 * cs[0, p]
                cs[0, p] += sign * h
            elif p == 3:
                pm += sign * h
            else:
                p0 += sign * h
            out.append(KR.solve_fp64(c.tables, pm, cs, p0, sens=False, **c.kw)['flux'][0])
        fd = (out[0] - out[1]) / (2 * h)
        an = base['dflux_dc'][0][:, p] if p < 3 else base['dflux_dphi'][0][:, p - 3]
        assert np.allclose(fd, an, rtol=1e-5, atol=1e-5 * np.abs(an).max()), (p, fd, an)


def test_clamped_and_zero_concentrations():
    t = two_step(-1.0, -2.0)
    neg = KR.solve_fp64(t, [0.0], [[-0.5, 0.2]], [0.0])
    zero = KR.solve_fp64(t, [0.0], [[0.0, 0.2]], [0.0])
    assert np.array_equal(neg['theta'], zero['theta']) and np.array_equal(neg['flux'], zero['flux'])
    assert (neg['dflux_dc'][0][:, 0] == 0.0).all() and (zero['dflux_dc'][0][:, 0] != 0.0).any() and np.isfinite(zero['dflux_dc']).all()
    nan = KR.solve_fp64(t, [0.0, 0.0], [[np.nan, 0.2], [0.1, 0.2]], [0.0, 0.0])
    assert list(nan['status']) == [2, 0] and np.isnan(nan['theta'][0]).all() and np.isfinite(nan['theta'][1]).all()
    # an adsorbate nothing produces or consumes sits at CATKIN_MIN_LOG
    dead = tables([[1, 1, 0, 0]], [[0, 0, 1, 0]], [[-1.0]], [1.0, 1.0, 1.0], [[-1.0, 0, 0, 0]])
    r = KR.solve_fp64(dead, [0.0], [[0.5]], [0.0])
    assert r['status'][0] == 0 and r['y'][0, 2] == KR.MIN_LOG


# ---- MeanFieldModel ----------------------------------------------------------------------------------------------------------------
def test_string_and_dict_forms_give_identical_tables():
    from catint_amd.microkinetics import MeanFieldModel
    dicts = [{'reactants': {'CO2_g': 1, '*': 1}, 'products': {'CO2': 1}},
             {'reactants': {'CO2': 1, '*': 1, 'H2O_g': 1}, 'products': {'COOH': 1, 'OH_g': 1}, 'electrons': 1},
             {'reactants': {'COOH': 1}, 'products': {'CO': 1, '*': 1, 'OH_g': 1}, 'ts': 'COOH-ele', 'electrons': 1, 'beta': 0.5},
             {'reactants': {'CO': 1}, 'products': {'CO_g': 1, '*': 1}}]
    a = KC.co2r_model('two_site').tables()
    b = MeanFieldModel(KC.SPECIES, KC.SITES['two_site'], dicts, KC.ENERGIES, solution=KC.SOLUTION, solution_energies=KC.SOLUTION_ENERGIES,
                       cref=1000.0, site_density=1.6e-5).tables()
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_site_count_and_electron_bookkeeping():
    t = KC.co2r_model('two_site').tables()
    N = 3
    assert list(t['site_count']) == [1.0, 1.0, 2.0, 1.0]
    #                         CO2 CO OH- |  * CO2* COOH CO*
    assert t['order_f'].tolist() == [[1, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 1, 0, 0], [0, 0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0, 1]]
    assert t['order_b'].tolist() == [[0, 0, 0, 0, 1, 0, 0], [0, 0, 1, 0, 0, 1, 0], [0, 0, 1, 1, 0, 0, 1], [0, 1, 0, 1, 0, 0, 0]]
    assert t['nu'].tolist() == [[-1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]]
    assert (t['site_count'] @ (t['order_b'] - t['order_f'])[:, N:].T == 0).all()
    kT = KC.co2r_model('two_site').kT
    assert np.allclose(t['dG'][:, 1], np.array([0.0, 1.0, 1.0, 0.0]) / kT) and np.allclose(t['Ea'][2, 1], 0.5 / kT)
    assert np.isneginf(t['Ea'][[0, 1, 3], 0]).all() and np.isfinite(t['Ea'][2]).all()
    # electrons on the product side count negative
    from catint_amd.microkinetics import parse_step
    assert parse_step('A*_t <-> B*_t + 2ele_g')['electrons'] == -2
    assert parse_step('2*_t + A_g <-> A*_t; beta=0.3; prefactor=1e12') == {'reactants': {'*': 2, 'A_g': 1}, 'products': {'A': 1}, 'ts': None,
                                                                          'electrons': 0, 'beta': 0.3, 'prefactor': 1e12}


def test_unit_conversion_of_one_hand_computed_step():
    """COOH* + e- <-> [COOH-ele] <-> CO* + OH-  at 298.15 K: kT = 0.0256925704 eV.  dG0 = 0.15 - 0.55 = -0.40 eV -> -15.568703 kT;
    the sigma slope (0.002 - 0.010) eV per micro C/cm^2 = -0.8 eV per C/m^2 -> -31.137406 kT m^2/C; Ea0 = 1.05 - 0.55 = 0.50 eV ->
    19.460879 kT, sigma slope 0; prefactor kT/h = 6.21244e12 1/s -> ln 29.457574"""
    t = KC.co2r_model('one_site').tables()
    kT = 1.38064852e-23 * 298.15 / 1.6021766208e-19
    assert abs(kT - 0.0256925704) < 1e-10
    assert np.allclose(t['dG'][2], [-0.40 / kT, 1.0 / kT, -0.8 / kT, 0.0], rtol=1e-12)
    assert abs(t['dG'][2, 0] + 15.568703) < 1e-6 and abs(t['dG'][2, 2] + 31.137406) < 1e-6
    assert np.allclose(t['Ea'][2], [0.50 / kT, 0.5 / kT, 0.0, 0.0], rtol=1e-12, atol=1e-12) and abs(t['Ea'][2, 0] - 19.460879) < 1e-6
    assert abs(t['lnA'][2] - 29.457574) < 1e-6
    # the quadratic term: 1e-4 eV per (micro C/cm^2)^2 = 1 eV per (C/m^2)^2
    assert np.isclose(t['dG'][0, 3], 1.0 / kT, rtol=1e-12) and np.isclose(t['dG'][0, 2], 1.5 / kT, rtol=1e-12)
    assert np.isclose(t['dG'][3, 0], (0.30 - 0.15) / kT, rtol=1e-12)          # the solution energy of CO


def test_model_errors_are_clear():
    from catint_amd.microkinetics import MeanFieldModel, MicrokineticsError

    def make(steps, ads={'A': 1, 'B': 2}):
        return MeanFieldModel(['X', 'Y'], ads, steps, {'A': 0.1, 'B': 0.2, 'TS': 0.9})
    with pytest.raises(MicrokineticsError, match='one site type'):
        make(['X_g + *_t <-> A*_s'])
    with pytest.raises(MicrokineticsError, match='conserve sites'):
        make(['A*_t <-> B*_t'])
    with pytest.raises(MicrokineticsError, match="unknown name 'Z_g'"):
        make(['Z_g + *_t <-> A*_t'])
    with pytest.raises(MicrokineticsError, match="unknown name 'C'"):
        make(['X_g + *_t <-> C*_t'])
    with pytest.raises(MicrokineticsError, match='transition state'):
        make(['X_g + *_t <-> QQ_t <-> A*_t'])
    with pytest.raises(MicrokineticsError, match='sites'):
        make(['X_g + *_t <-> A*_t'], ads={'A': 4})
    with pytest.raises(MicrokineticsError, match='unknown option'):
        make(['X_g + *_t <-> A*_t; gamma=2'])
    make(['X_g + *_t <-> A*_t', 'A*_t + *_t <-> TS_t <-> B*_t', 'B*_t <-> Y_g + 2*_t'])


# ---- the library -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def libpath():
    from catint_amd.build import build_kinetics_library
    return build_kinetics_library()


@pytest.fixture(scope='module')
def solver(libpath):
    from catint_amd import _kinetics
    with _kinetics.KineticsSolver(0) as o:
        yield o


def header_source(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_the_library_exports_exactly_the_declared_symbols(libpath):
    from catint_amd import _kinetics
    declared = sorted(set(re.findall(r'\b(catkin_[a-z0-9_]+)\s*\(', header_source('catint_kinetics.h'))))
    assert declared == sorted(_kinetics.SYMBOLS) and len(declared) == 6
    lib = C.CDLL(libpath)
    for s in declared:
        assert hasattr(lib, s), s
    exported = subprocess.check_output(['nm', '-D', '--defined-only', libpath]).decode()
    assert sorted(set(re.findall(r'\b(catkin_[a-z0-9_]+)\b', exported))) == declared
    assert not re.findall(r'\bpnp_[a-z0-9_]+\b', exported)          # and no pnp_* symbol


def test_the_sources_are_not_part_of_the_other_libraries():
    from catint_amd import build
    others = build.SOURCES + build.OBSERVE_SOURCES + build.BALANCE_SOURCES + build.REGRID_SOURCES + build.EQUIL_SOURCES + build.RESPONSE_SOURCES
    assert not any('catkin' in s or 'kinetics' in s for s in others)
    assert os.path.dirname(build.KINETICS_LIB) == os.path.dirname(build.LIB)
    assert build.KINETICS_SOURCES == ['catkin.hip'] and os.path.isdir(build.KINETICS_DIR)
    assert callable(build.kinetics_needs_build)
    listed = {os.path.realpath(p) for p in build.KINETICS_HEADERS}
    for h in ('catint_kinetics.h', 'catint_pnp.h'):
        assert os.path.realpath(os.path.join(ROOT, 'include', h)) in listed
    assert os.path.realpath(os.path.join(build.CSRC, 'pnp_post.h')) in listed
    from tests.test_build_deps import reached
    sources = [os.path.join(build.KINETICS_DIR, f) for f in build.KINETICS_SOURCES]
    assert not reached(sources) - listed - {os.path.realpath(f) for f in sources}
    assert 'build_kinetics_library(' in open(os.path.join(ROOT, '__graft_entry__.py')).read()


def header_structs():
    out = {}
    for body, struct in re.findall(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', header_source('catint_kinetics.h'), flags=re.S):
        fields = []
        for decl in body.split(';'):
            decl = decl.strip()
            if not decl:
                continue
            names = decl.split(None, 1)[1] if not decl.startswith('const') else decl.split(None, 2)[2]
            fields += [n.strip().lstrip('*').strip() for n in names.split(',')]
        out[struct] = fields
    return out


MACROS = {'maxspecies': 'CATKIN_MAX_SPECIES', 'maxads': 'CATKIN_MAX_ADSORBATES', 'maxsteps': 'CATKIN_MAX_STEPS', 'maxorder': 'CATKIN_MAX_ORDER',
          'maxsites': 'CATKIN_MAX_SITES', 'minlog': '(int)CATKIN_MIN_LOG', 'full': 'CATKIN_DROP_FULL', 'stern': 'CATKIN_DROP_STERN',
          'converged': 'CATKIN_CONVERGED', 'maxit': 'CATKIN_MAXIT', 'input': 'CATKIN_INPUT', 'pivot': 'CATKIN_PIVOT', 'einval': 'CATKIN_EINVAL',
          'enomem': 'CATKIN_ENOMEM', 'edevice': 'CATKIN_EDEVICE'}


@pytest.fixture(scope='module')
def compiler_layout(tmp_path_factory):
    structs = header_structs()
    assert set(PAIRS) <= set(structs)
    d = tmp_path_factory.mktemp('kinetics_abi')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "catint_kinetics.h"', 'int main(void) {']
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
    from catint_amd import _kinetics
    cls = getattr(_kinetics, PAIRS[cname])
    want = dict(compiler_layout[cname])
    assert C.sizeof(cls) == want.pop('sizeof')
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == want


def test_constants_of_the_binding_are_the_header_s(compiler_layout):
    from catint_amd import _kinetics as k
    n = {name: compiler_layout[name]['n'] for name in MACROS}
    assert (k.MAX_SPECIES, k.MAX_ADSORBATES, k.MAX_STEPS, k.MAX_ORDER, k.MAX_SITES) == (n['maxspecies'], n['maxads'], n['maxsteps'], n['maxorder'],
                                                                                      n['maxsites']) == (8, 8, 16, 3, 3)
    assert k.MIN_LOG == n['minlog'] == -700 == KR.MIN_LOG
    assert k.DROP == {'full': n['full'], 'stern': n['stern']}
    assert (k.CONVERGED, k.MAXIT, k.INPUT, k.PIVOT) == (n['converged'], n['maxit'], n['input'], n['pivot']) == (0, 1, 2, 3)
    assert (k.EINVAL, k.ENOMEM, k.EDEVICE) == (n['einval'], n['enomem'], n['edevice'])
    assert (k.DEFAULT_TOL, k.DEFAULT_MAXIT) == (1e-12, 200)
    from catint_amd import microkinetics as m
    assert (m.MAX_ORDER, m.MAX_SITES) == (k.MAX_ORDER, k.MAX_SITES)


def fake_view(N=2, B=2, phi=0x1000, size=None, nx=16):
    """A view no device stands behind: validation must reject the call without reading it."""
    from catint_amd import _kinetics
    return _kinetics.PnpDeviceView(C.sizeof(_kinetics.PnpDeviceView) if size is None else size, 2, N, nx, (nx + 15) // 16 * 16, 0, B, 0x1000, phi,
                                   0x1000, None)


def host_args(n=2, N=2):
    return dict(phiM=np.linspace(-0.1, -0.3, n), csurf=np.full((n, N), 0.5), phi_surface=np.zeros(n))


def chain(N=2, S=1, R=None):
    """A + * <-> X_1 <-> ... <-> X_S <-> B + * padded to R steps with copies of the first"""
    T = S + 1
    of, ob, nu = [], [], []
    for r in range(S + 1):
        f, b, v = np.zeros(N + T, int), np.zeros(N + T, int), np.zeros(N)
        if r == 0:
            f[N] = 1
            if N:
                f[0], v[0] = 1, -1.0
        else:
            f[N + r] = 1
        if r == S:
            b[N] = 1
            if N > 1:
                b[1], v[1] = 1, 1.0
        else:
            b[N + r + 1] = 1
        of.append(f); ob.append(b); nu.append(v)
    while R is not None and len(of) < R:
        of.append(of[0]); ob.append(ob[0]); nu.append(nu[0])
    return tables(of, ob, np.array(nu).reshape(len(of), N), np.ones(T), np.zeros((len(of), 4)))


def edit(t, **kw):
    t = {k: np.array(v) if isinstance(v, np.ndarray) else v for k, v in t.items()}
    for k, v in kw.items():
        if callable(v):
            v(t)
        else:
            t[k] = v
    return t


def poke(key, idx, value):
    def f(t):
        t[key] = np.array(t[key], float if key not in ('order_f', 'order_b') else np.int32)
        t[key][idx] = value
    return f


@pytest.mark.parametrize('what, make, word', [
    ('struct_size of the parameters', lambda: (None, chain(), {'struct_size': 8}), 'catkin_params.struct_size'),
    ('struct_size of the outputs', lambda: (None, chain(), {'out_struct_size': 8}), 'catkin_outputs.struct_size'),
    ('struct_size of the view', lambda: (fake_view(size=12), chain(), {'csurf': None, 'phi_surface': None}), 'pnp_device_view.struct_size'),
    ('nine species', lambda: (None, chain(N=9), host_args(N=9)), '9 species'),
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
    ('a zero tolerance', lambda: (None, chain(), {'tol': 0.0}), 'tol'),
    ('an infinite tolerance', lambda: (None, chain(), {'tol': np.inf}), 'tol'),
    ('a site count of 4', lambda: (None, edit(chain(), site_count=np.array([1.0, 4.0])), {}), 'site count 1'),
    ('a site count of 0', lambda: (None, edit(chain(), site_count=np.array([1.0, 0.0])), {}), 'site count 1'),
    ('a free site that takes two sites', lambda: (None, edit(chain(), site_count=np.array([2.0, 1.0])), {}), 'site count 0'),
    ('a NaN site count', lambda: (None, edit(chain(), site_count=np.array([1.0, np.nan])), {}), 'site count 1'),
    ('maxit 0', lambda: (None, chain(), {'maxit': 0}), 'maxit'),
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
    from catint_amd import _kinetics
    view, tab, kw = make()
    N = np.asarray(tab['order_f']).shape[1] - len(tab['site_count']) if np.asarray(tab['order_f']).ndim == 2 else 2
    args = host_args(N=max(N, 0))
    args.update(kw)
    with pytest.raises(_kinetics.KineticsError) as e:
        solver.solve(view, tab, **args)
    assert e.value.code == _kinetics.EINVAL, (what, str(e.value))
    assert word in str(e.value), (what, str(e.value))
    assert solver.last_kernel == '' and solver.last_kernel_ms == -1.0


def test_a_given_sigma_needs_no_capacitance(solver):
    """... validation passes it on: with n = 0 the call then succeeds without a device"""
    out = solver.solve(None, chain(), np.zeros(0), csurf=np.zeros((0, 2)), phi_surface=np.zeros(0), sigma=np.zeros(0), stern_capacitance=np.nan)
    assert out['theta'].shape == (0, 2)


def test_null_arguments_and_null_context(solver, libpath):
    from catint_amd import _kinetics
    lib = _kinetics.load_library()
    p = _kinetics.CatkinParams(struct_size=C.sizeof(_kinetics.CatkinParams))
    o = _kinetics.CatkinOutputs(struct_size=C.sizeof(_kinetics.CatkinOutputs))
    assert lib.catkin_solve(solver._h, None, None, C.byref(o)) == _kinetics.EINVAL
    assert b'null' in lib.catkin_last_error(solver._h)
    assert lib.catkin_solve(solver._h, None, C.byref(p), None) == _kinetics.EINVAL
    assert lib.catkin_solve(None, None, C.byref(p), C.byref(o)) == _kinetics.EINVAL
    assert lib.catkin_create(0, None) == _kinetics.EINVAL
    assert lib.catkin_last_kernel(solver._h) == b''
    # the tables NULL
    p.nspecies, p.nadsorbates, p.nsteps, p.maxit, p.tol, p.site_density = 2, 1, 2, 10, 1e-12, 1e-5
    assert lib.catkin_solve(solver._h, None, C.byref(p), C.byref(o)) == _kinetics.EINVAL
    assert b'are required' in lib.catkin_last_error(solver._h)
    t = chain()
    keep = [np.ascontiguousarray(t[k], np.int32) for k in ('order_f', 'order_b')] + [np.ascontiguousarray(t[k], float) for k in
                                                                                      ('nu', 'cref', 'site_count', 'dG', 'Ea', 'lnA')]
    p.order_f, p.order_b = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in keep[:2])
    p.nu, p.cref, p.site_count, p.dG, p.Ea, p.lnA = (_kinetics._dptr(a) for a in keep[2:])
    assert lib.catkin_solve(solver._h, None, C.byref(p), C.byref(o)) == _kinetics.EINVAL
    assert b'phiM is required' in lib.catkin_last_error(solver._h)
    pm, cs, ps = np.zeros(2), np.zeros((2, 2)), np.zeros(2)
    p.phiM, p.csurf, p.phi_surface = _kinetics._dptr(pm), _kinetics._dptr(cs), _kinetics._dptr(ps)
    p.n = -1
    assert lib.catkin_solve(solver._h, None, C.byref(p), C.byref(o)) == _kinetics.EINVAL
    assert b'n < 0' in lib.catkin_last_error(solver._h)
    # every output NULL: nothing to do, and no device call
    p.n = 2
    assert lib.catkin_solve(solver._h, None, C.byref(p), C.byref(o)) == 0
    assert lib.catkin_last_kernel(solver._h) == b''


def test_no_point_makes_no_device_call(solver):
    """n == 0: valid, and done before the first device call (this machine may have no device at all)."""
    out = solver.solve(None, chain(S=2), np.zeros(0), csurf=np.zeros((0, 2)), phi_surface=np.zeros(0), fields=['theta', 'rate', 'rate_gross', 'flux', 'flux_scale', 'dflux_dc', 'dflux_dphi'])
    assert out['theta'].shape == (0, 3) and out['rate'].shape == (0, 3) and out['flux'].shape == (0, 2) and out['dflux_dc'].shape == (0, 2, 2)
    assert out['dflux_dphi'].shape == (0, 2, 2) and out['status'].shape == (0,) and out['iterations'].dtype == np.int32
    v = fake_view()
    out = solver.solve(v, chain(), np.zeros(0), lanes=[])
    assert out['flux_scale'].shape == (0, 2)
    assert solver.last_kernel == ''


def test_the_library_holds_the_one_kernel(libpath):
    try:
        compiled = K.compiled_kernels(lib=libpath)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert compiled == INSTANCES, sorted(compiled ^ INSTANCES)


def test_the_other_libraries_gained_no_kernel():
    from catint_amd import build as B
    for f in (B.build_library, B.build_observe_library, B.build_balance_library, B.build_regrid_library, B.build_equil_library,
              B.build_response_library):
        f()
    try:
        compiled = set(K.compiled_kernels())
        for lib in (B.OBSERVE_LIB, B.BALANCE_LIB, B.REGRID_LIB, B.EQUIL_LIB, B.RESPONSE_LIB):
            compiled |= K.compiled_kernels(lib=lib)
    except K.CensusUnavailable as e:
        pytest.fail('kernel census unavailable: %s' % e)
    assert not [n for n in compiled if 'catkin' in n or 'steady_kernel' in n]
    from catint_amd import _capi
    assert not [s for s in _capi.SYMBOLS if 'catkin' in s or 'microkinetic' in s]        # no pnp_* symbol was added for it
    assert hasattr(_capi.PnpSolver, 'get_kinetics')


# ---- the calculator's opt-in path, with fakes --------------------------------------------------------------------------------------
class FakeKinetics(object):
    """KineticsSolver's solve on the CPU reference; records every call"""

    def __init__(self):
        self.calls, self.closed = [], False

    def solve(self, view, tab, phiM, csurf=None, phi_surface=None, potential_drop='stern', stern_capacitance=0.0, phi_pzc=0.0, gamma=None,
              theta_guess=None, fields=None, **kw):
        assert view is None
        r = KR.solve_fp64(tab, phiM, csurf, phi_surface, w=1 if potential_drop == 'stern' else 0, CS=stern_capacitance, phi_pzc=phi_pzc,
                          gamma=gamma, theta_guess=theta_guess, sens=False)
        self.calls.append({'guess': None if theta_guess is None else np.array(theta_guess), 'iterations': r['iterations'].copy(),
                           'theta': r['theta'].copy(), 'args': (potential_drop, stern_capacitance, phi_pzc), 'fields': fields})
        return {k: r[k] for k in ('theta', 'flux', 'flux_scale', 'status', 'iterations')}

    def close(self):
        self.closed = True


def scf_parts():
    from catint_amd.microkinetics import MeanFieldModel
    from tests.test_host_physical import make_tp
    phis = np.array([-0.3, -0.4, -0.5])
    tp = make_tp(phis)                      # species K+, HCO3-, CO2
    names = list(tp.species.keys())
    model = MeanFieldModel(names, {'CO2': 1}, ['CO2_g + *_t <-> CO2*_t', 'CO2*_t + ele_g <-> TS_t <-> HCO3_g + *_t; beta=0.5'], {'CO2': 0.1, 'TS': 0.6},
                           solution={'HCO3_g': 'HCO3-'}, site_density=1e-6)
    cb = np.array([float(tp.species[s]['bulk_concentration']) for s in names])

    def transport_fn(flux):
        return cb[None, :] + flux * 4e-8 / 1e-9, 0.1 * phis, np.zeros(len(phis))
    return tp, model, transport_fn


def test_without_the_option_the_call_sequence_is_unchanged(monkeypatch):
    from catint_amd.calculator import Calculator, CalculatorError
    from tests.test_response_abi import run_with
    calc, tp, s = run_with(monkeypatch, {})
    assert [c[0] for c in s.calls] == ['set_batch', 'solve'] and getattr(calc, 'microkinetics', None) is None
    tp, model, transport_fn = scf_parts()
    calc = Calculator(transport=tp, calc='comsol')

    def never():
        raise AssertionError('a kinetics context was created without set_microkinetics')
    monkeypatch.setattr(calc, '_kinetics_solver', never)
    seen = []

    def flux_cb(state):
        seen.append(set(state))
        return np.zeros((3, 3))
    out = calc.run_scf_cycle(flux_cb, transport_fn=transport_fn, max_iter=3)
    assert seen[0] == {'istep', 'phiM', 'surface_pH', 'surface_concentration', 'surface_efield', 'surface_potential'}
    assert 'coverage' not in out and 'flux_scale' not in out and 'coverage' not in tp.alldata[0]['system']
    with pytest.raises(CalculatorError, match='needs the physical mode'):
        calc.run_scf_cycle()


def test_with_the_option_the_loop_runs_the_device_kinetics_warm_started(monkeypatch):
    from catint_amd.calculator import Calculator
    tp, model, transport_fn = scf_parts()
    calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-9)
    calc.set_microkinetics(model, site_density=2e-6, potential_drop='stern')
    fake = FakeKinetics()
    monkeypatch.setattr(calc, '_kinetics_solver', lambda: fake)
    out = calc.run_scf_cycle(transport_fn=transport_fn, max_iter=200)      # (transport_fn stands in for the GPU solve)
    assert fake.closed and len(fake.calls) == out['iterations'] >= 3
    assert out['converged'].all() and not out['failed'].any()
    assert fake.calls[0]['guess'] is None
    for k in range(1, len(fake.calls)):
        # warm start from the previous iterate (a lane that has left the loop keeps the coverages of its last active iteration)
        assert np.allclose(fake.calls[k]['guess'], fake.calls[k - 1]['theta'], rtol=1e-6, atol=0)
    assert np.array_equal(fake.calls[1]['guess'], fake.calls[0]['theta']) and np.array_equal(fake.calls[2]['guess'], fake.calls[1]['theta'])
    assert fake.calls[-1]['iterations'].max() <= 3 < fake.calls[0]['iterations'].min()
    assert fake.calls[0]['args'] == ('stern', 0.2, 0.16) and tuple(fake.calls[0]['fields']) == ('theta', 'flux', 'flux_scale')
    assert out['coverage'].shape == (3, 2) and out['flux_scale'].shape == (3, 3)
    assert np.allclose(out['coverage'].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    for i in range(3):
        assert np.array_equal(tp.alldata[i]['system']['coverage'], out['coverage'][i])
    # the fluxes are the model's at the final surface state, with the site density of set_microkinetics
    tab = dict(model.tables(), site_density=2e-6)
    phis = np.array([-0.3, -0.4, -0.5])
    ref = KR.solve_fp64(tab, phis, out['surface_concentration'], 0.1 * phis, w=1, CS=0.2, phi_pzc=0.16,
                        sens=False)
    assert np.allclose(ref['flux'], out['flux'], rtol=1e-6, atol=1e-30)
    assert (out['flux'][:, 2] < 0).all() and (out['flux'][:, 1] > 0).all() and (out['flux'][:, 0] == 0).all()


@pytest.mark.parametrize('code, at', [(1, 1), (3, 1), (3, 4), (2, 2)])
def test_a_lane_whose_kinetics_fail_leaves_the_loop_as_failed(monkeypatch, code, at):
    """Lane 1 returns kinetic status `code` in SCF iteration `at` (with the numbers as computed, or NaN for status 2): its fluxes are not
    handed to the transport, the lane ends failed and not converged with the status in the result, the other lanes converge as before"""
    from catint_amd.calculator import Calculator
    results = []
    for poison in (False, True):
        tp, model, transport_fn = scf_parts()
        calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-9)
        calc.set_microkinetics(model, site_density=2e-6)
        fake = FakeKinetics()
        handed = []

        def solve(view, tab, phiM, _fake=fake, **kw):
            out = FakeKinetics.solve(_fake, view, tab, phiM, **kw)
            if poison and len(_fake.calls) == at:
                out['status'] = out['status'].copy()
                out['status'][1] = code
                out['flux'] = out['flux'].copy()
                out['flux'][1] = np.nan if code == 2 else 1e3 * out['flux'][1]
            return out
        fake.solve = solve

        def recording(flux, _t=transport_fn):
            handed.append(np.array(flux))
            return _t(flux)
        monkeypatch.setattr(calc, '_kinetics_solver', lambda _f=fake: _f)
        results.append((calc.run_scf_cycle(transport_fn=recording, max_iter=200), handed, tp))
    (clean, h0, _), (out, h1, tp) = results
    assert clean['converged'].all() and (clean['kinetic_status'] == 0).all()
    assert list(out['failed']) == [False, True, False] and list(out['converged']) == [True, False, True]
    assert list(out['kinetic_status']) == [0, code, 0] and tp.alldata[1]['system']['kinetic_status'] == code
    assert [tp.alldata[i]['system']['kinetic_status'] for i in (0, 2)] == [0, 0]
    assert np.isfinite(np.array(h1)).all()
    # what the transport saw for the lane in that iteration is its previous flux, never the failed solve's
    assert np.array_equal(h1[at - 1][1], h1[at - 2][1] if at > 1 else np.asarray(tp.flux_bound[:, 0], float))
    assert not np.array_equal(h1[at - 1][1], h0[at - 1][1])
    for i in (0, 2):
        assert np.array_equal(out['flux'][i], clean['flux'][i]) and np.array_equal(out['coverage'][i], clean['coverage'][i])


def test_the_two_kinetic_models_exclude_each_other():
    from catint_amd.calculator import Calculator, CalculatorError
    tp, model, _ = scf_parts()
    calc = Calculator(transport=tp, calc='comsol')
    calc.set_microkinetics(model)
    with pytest.raises(CalculatorError, match='exclude each other'):
        calc.set_surface_kinetics([{'species': 'CO2', 'rate': 1e-6, 'stoichiometry': {'CO2': -1.0}}])
    calc.set_microkinetics(None)
    calc.set_surface_kinetics([{'species': 'CO2', 'rate': 1e-6, 'stoichiometry': {'CO2': -1.0}}])
    with pytest.raises(CalculatorError, match='exclude each other'):
        calc.set_microkinetics(model)
    tp2, model2, _ = scf_parts()
    with pytest.raises(CalculatorError, match='physical mode'):
        Calculator(transport=tp2, calc='Crank-Nicolson', dt=1e-9, tmax=1e-8).set_microkinetics(model2)
    with pytest.raises(CalculatorError, match='potential_drop'):
        Calculator(transport=tp2, calc='comsol').set_microkinetics(model2, potential_drop='half')
    # a model over other species than the transport's: the calculator's own error, for the orders and for nu alike
    with pytest.raises(CalculatorError, match='3 species'):
        Calculator(transport=tp2, calc='comsol').set_microkinetics(KC.co2r_model('one_site').tables() | {'nu': np.zeros((4, 2))})
    with pytest.raises(CalculatorError, match='3 species'):
        Calculator(transport=tp2, calc='comsol').set_microkinetics(chain(N=2, S=1))
