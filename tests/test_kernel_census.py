"""The kernel census (tests/kernel_census.py) against the built library, without a GPU: the compiled kernels are exactly the census
instances and the kernels covered elsewhere, every named test exists and dispatched its kernels when traced on its own
(profiles/kernel_census_covered.txt), and every census instance was dispatched by the traced run of tests/test_gpu_kernel_census.py
recorded in profiles/kernel_census_dispatched.txt."""
import ast
import os

import pytest

from tests import kernel_census as K


@pytest.fixture(scope='module')
def compiled():
    try:
        return K.compiled_kernels()
    except K.CensusUnavailable as e:
        pytest.skip('kernel census unavailable: %s' % e)


def test_compiled_kernels_are_the_census_and_the_covered_kernels(compiled):
    known = set(K.CENSUS) | set(K.COVERED_ELSEWHERE)
    missing, stale = sorted(compiled - known), sorted(known - compiled)
    assert not missing, 'compiled kernels without a census case or a covering test: %s' % missing
    assert not stale, 'census / covered entries the library does not compile: %s' % stale


def test_every_instance_of_the_solver_families_has_a_census_case(compiled):
    assert not set(K.CENSUS) & set(K.COVERED_ELSEWHERE)
    assert all(K.family(n) in K.FAMILIES for n in K.CENSUS)
    in_scope = {n for n in compiled if K.family(n) in K.FAMILIES}
    assert in_scope == set(K.CENSUS), sorted(in_scope ^ set(K.CENSUS))


def test_census_cases_fit_their_instances():
    """What the case's shape decides, it must decide for the instance: the block size N + 1 of the physical-mode families, the points
    per lane of the compat families (nx - 2 <= 64 P, up to 1026 points in one wave, then WY waves)."""
    def points_per_lane(nx):
        return next(P for P in (1, 2, 4, 8, 16) if nx - 2 <= 64 * P) if nx <= 1026 else 16
    for name, case in K.CENSUS.items():
        args = [a.strip() for a in name[name.index('<') + 1:-1].split(',')]
        if case.path == 'newton':
            assert int(args[0]) == case.N + 1, name
        else:
            assert int(args[0]) == points_per_lane(case.nx), name
            if K.family(name) in ('step_kernel_mw', 'poisson_kernel_mw'):
                assert int(args[1]) == (2 if case.nx - 2 <= 2048 else 4), name


def test_every_covering_test_exists():
    for name, ref in K.COVERED_ELSEWHERE.items():
        path, func = ref.split('::')
        with open(os.path.join(K.ROOT, path)) as f:
            tree = ast.parse(f.read())
        defs = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
        assert func in defs, '%s: %s does not exist' % (name, ref)


def test_every_covering_test_dispatched_its_kernels():
    covered = K.read_covered()
    wrong = sorted('%s: %s' % kv for kv in K.COVERED_ELSEWHERE.items() if kv not in covered)
    assert not wrong, 'covering tests that did not dispatch their kernel when traced (%s): %s' % (os.path.relpath(K.COVERED, K.ROOT), wrong)


def test_every_census_instance_was_dispatched():
    dispatched = K.read_dispatched()
    missing = sorted(set(K.CENSUS) - dispatched)
    assert not missing, 'census instances absent from %s: %s' % (os.path.relpath(K.DISPATCHED, K.ROOT), missing)


def test_census_names_of_demangled_and_traced_kernels():
    assert K.census_name('void pnp::newton_lane_kernel<3, 0, true, false>(pnp::NewtonArgs) [clone .kd]') == 'newton_lane_kernel<3, 0, true, false>'
    assert K.census_name('void pnp::step_kernel<8, 3, 1>(pnp::DevArgs)') == 'step_kernel<8, 3, 1>'
    assert K.census_name('bdf2_accumulate_kernel.kd') == 'bdf2_accumulate_kernel'
    assert K.census_name('pnp::rates_kernel(pnp::DevArgs, pnp::ReactionTable, double*) [clone .kd]') == 'rates_kernel'
