"""The table of driven Newton cases (tests/newton_regimes.py) checked without a GPU, with the oracle alone.

Per case, on its compared lanes (NR.conditions and the second solver):
  * every lane converges within the case's maxit (50), on every step;
  * the free-volume backtrack fires in at least three compared lanes, the floor at a tenth and the dphi_max scaling in at least one
    each, and at least one compared lane stays mild (no backtrack);
  * the oracle's two linear solvers, the banded LU and the cyclic reduction that mirrors the device, give equal iteration counts and
    states within 1e-10 of the profile scale (per species 5e-8 relative): twenty times below the 2e-9 / 1e-6 bar the device is held
    to, because the device differs from the oracle as the two solvers differ from each other -- in elimination order and rounding --
    and the reason why the device test may demand identical iteration counts;
  * the '/estimate' cases leave through the error estimate in a compared lane, the '/predictor' cases fire both clips of the predictor;
  * the single-precision record cases stay, with the arithmetic of tools/probe/f32_records_oracle.py (block Thomas whose
    back-substitution sees float32 records) on the whole batch, inside the bar of assert_close_f32_records: counts at most one apart in
    at most a tenth of the operating points.  Both chosen batches give identical counts in every operating point.
These are conditions on the table, not measurements: a case that misses one gets another seed, recipe or timestep factor
(tests/newton_regimes.py says which were tried), the bars stay.

The table rule and the dispatch record (profiles/newton_regimes_dispatched.txt) are checked here too.  Measured: the 63 cases take 52 s
on one core (the two single-precision cases, 37 operating points with three solvers, 8 s of it).
"""
import numpy as np
import pytest

from oracle import pnp_physical as PH
from tests import newton_regimes as NR
from tests.kernel_census import CENSUS, family, read_dispatched
from tests.newton_regimes import REGIMES


def mode_arg(instance):
    return int(NR.template_args(instance)[NR.MODE_ARG[family(instance)]])


def test_table_covers_every_family():
    """The rule of the table: steric instances only (MODE >= 1), the physics class compiles to the instance's MODE, and per family every
    block size it compiles, both modes, stationary and transient; the lane family with separate passes, the fused update and
    single-precision record columns; the lane pair and quad with both values of the BDF flag; a 256-thread build of the row-per-thread
    kernel; one team case that exchanges rows through device memory."""
    seen = {}
    for key, r in REGIMES.items():
        assert key.split('/')[0] == r.instance and r.instance in CENSUS and r.recipe in NR.RECIPES, key
        fam = family(r.instance)
        assert fam in NR.MODE_ARG, key
        assert mode_arg(r.instance) >= 1 and mode_arg(r.instance) == NR.mode_of(r.instance, r.physics), key
        case = CENSUS[r.instance]
        lanes = NR.compared_lanes(key)
        assert len(set(lanes)) == len(lanes) and all(0 <= b < case.B for b in lanes), key
        assert NR.is_f32(r) or 4 <= len(lanes) <= 6, key
        seen.setdefault(fam, []).append(r)
    assert set(seen) == set(NR.MODE_ARG)
    for fam, rs in seen.items():
        args = [NR.template_args(r.instance) for r in rs]
        compiled = {int(NR.template_args(n)[0]) for n in CENSUS if family(n) == fam and mode_arg(n) >= 1}
        assert {int(a[0]) for a in args} == compiled, (fam, 'block sizes')
        assert {mode_arg(r.instance) for r in rs} == {1, 2}, (fam, 'modes')
        assert {r.factor is None for r in rs} == {True, False}, (fam, 'stationary and transient')
        if fam == 'newton_lane_kernel':
            assert {a[2] for a in args} == {'true', 'false'} and 'true' in {a[3] for a in args}, 'lane: fused, separate passes, f32 records'
        if fam in ('newton_lane2_kernel', 'newton_lane4_kernel'):
            assert {a[2] for a in args} == {'true', 'false'}, (fam, 'BDF flag')
        if fam == 'newton_kernel':
            assert '256' in {a[1] for a in args}, 'row-per-thread: 256-thread build'
        if fam == 'newton_team_kernel':
            assert any(dict(CENSUS[r.instance].env).get('NEWTON_EXCHANGE') == 'global' for r in rs), 'team: exchange through device memory'
    groups = {'lane': NR.LANE_FAMILIES, 'workgroup': NR.WORKGROUP_FAMILIES}
    for name, fams in groups.items():
        mine = [(k, r) for k, r in REGIMES.items() if family(r.instance) in fams]
        assert sum(1 for k, r in mine if dict(r.extra).get('error_estimate')) >= 2, (name, 'error estimate')
        assert any('predictor' in k.split('/')[1:] and 'pred' in CENSUS[r.instance].stepper for k, r in mine), (name, 'predictor')


def test_every_table_instance_was_dispatched():
    """profiles/newton_regimes_dispatched.txt: the kernels a traced run of tests/test_gpu_newton_regimes.py dispatched
    (tools/kernel_census_dispatched.py)."""
    dispatched = read_dispatched(NR.DISPATCHED)
    missing = sorted({r.instance for r in REGIMES.values()} - dispatched)
    assert not missing, 'table instances absent from the dispatch record: %s' % missing


def close(a, b, rtol):
    """assert_close of tests/test_gpu_newton.py at another bar: the states within rtol of the profile scale, equal iteration counts."""
    (c, phi, it), (rc, rphi, rit) = a, b
    cscale = np.abs(rc).max(axis=2, keepdims=True)
    assert np.abs(c - rc).max() <= rtol * cscale.max() and (np.abs(c - rc) / (np.abs(rc) + 1e-3 * cscale)).max() < 500 * rtol
    assert np.abs(phi - rphi).max() <= rtol * max(np.abs(rphi).max(), 0.025)
    assert np.array_equal(it, rit), (it, rit)


@pytest.mark.parametrize('key', sorted(REGIMES))
def test_case_reaches_the_branches_and_both_solvers_agree(key):
    r = REGIMES[key]
    branches = []
    ref = NR.oracle(key, branches=branches)
    NR.conditions(key, branches, ref[2])
    pcr = NR.oracle(key, solver=PH.solve_block_pcr)
    close(pcr, ref, 1e-10)
    if NR.is_f32(r):
        # the bar of tests/test_gpu_kernel_census.py: assert_close_f32_records, with the arithmetic of tools/probe/f32_records_oracle.py
        f32 = NR.oracle(key, solver=NR.thomas_f32)
        d = np.abs(f32[2] - ref[2])
        assert d.max() <= 1 and (d != 0).mean() <= 0.1, (f32[2], ref[2])
        assert np.abs(f32[0] - ref[0]).max() <= 2e-9 * np.abs(ref[0]).max()
