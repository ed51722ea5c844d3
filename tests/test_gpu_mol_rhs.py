"""GPU: the method-of-lines right-hand side kernels (pnp_mol_rhs: rates_kernel, mol_rhs_kernel<P>, the charge row / multi-wave Poisson /
mol_rhs_pointwise_kernel chain beyond one wave) called directly, against a reference that is not the device.

Every case (tests/mol_cases.py) is a batch of 5 lanes on a handle of capacity 8; every lane has its own state, Poisson boundary values,
vzeta and wall fluxes (mixed signs, one zero), and the state uploaded with set_batch is NOT the argument of mol_rhs (twice as large, not
neutral): a rate or a charge row taken from the handle's state, from lane 0, from the neighbouring species or grid point is off by
a visible factor.  Every lane is compared, per species row, scaled by that row's largest reference value.

Bars (tests/mol_cases.py bar_short / bar_long): on grids up to 259 points the reference is the multiprecision restatement
(tests/mol_ref.py) and the device is held to 16 x E_oracle, the error the fp64 oracle itself makes on that case -- device and oracle are
both fp64 and differ in summation order and FMA contraction only (tree scans of depth log2(nx) against left-to-right sums).  On longer
grids the reference is the fp64 oracle (Thomas) and the bar 16 x the largest E_oracle of the short grids x nx/259.  Neither is looser
than the 1e-9 of the older tests.  Measured values: profiles/mol_rhs_unit.md."""
import numpy as np
import pytest

from oracle import pnp_ref as R
from catint_amd.host import solver_from_problem
from tests import mol_cases as MC
from tests import mol_ref as M

pytestmark = pytest.mark.gpu


def device_rhs(inp, y=None, reactions=True):
    p = inp.problems[0]
    if not reactions:
        p = R.Problem(**dict(p.__dict__, reactions=[]))
    with solver_from_problem(p, 'FTCS', batch_capacity=MC.CAPACITY) as s:
        s.set_batch(inp.upload, inp.pb, inp.vzeta, inp.flux)
        return s.mol_rhs(inp.y if y is None else y)


@pytest.mark.parametrize('case', MC.ALL, ids=MC.case_id)
def test_every_lane_against_the_reference(case):
    inp = MC.make_case(case)
    f = device_rhs(inp)
    assert f.shape == (MC.B, case.N * case.nx) and np.isfinite(f).all()
    if case.nx <= MC.MP_MAX_NX:
        ref, bar, e = MC.mp_rhs(case), MC.bar_short(case), '%.2e' % MC.e_oracle(case)
    else:
        ref, bar, e = MC.oracle_rhs(inp), MC.bar_long(case), '-'
    err = max(float(M.row_errors(f[b], ref[b], case.N).max()) for b in range(MC.B))
    print('MOLRHS | %s | %s | %.2e | %.2e |' % (MC.case_id(case), e, err, bar))
    M.assert_rows_within(f, ref, case.N, bar, MC.case_id(case))
    for b in range(MC.B):      # the bulk point is exactly zero, and nothing of a row is left unwritten
        assert (f[b].reshape(case.N, case.nx)[:, -1] == 0.0).all()


ISOLATED = [c for c in MC.SPECIES + MC.TABLES + MC.NOMIG + [g for g in MC.GRIDS if g.nx in (5, 259, 1026, 2050) and not g.lf] if c.table != 'none']


@pytest.mark.parametrize('case', ISOLATED, ids=MC.case_id)
def test_rate_term_isolated(case):
    """mol_rhs with the table minus mol_rhs of a second handle without it is the rate term alone: R.get_rates of the ARGUMENT on the
    interior points, exactly zero at the wall cell and at the bulk point.  Scaled per species row by max |rates|, so that an index error
    shows where the rates are a few percent of the right-hand side.  Bar per row: the kernels add the rate last, f = fl(g + rate), so
    the difference carries one rounding of f (and one of g when the subtraction is not exact), 2^-52 max |f|, plus the rate's own
    rounding, at most 8 x 2^-53 of the two products it is the difference of (up to four factors and a constant each, contracted or not)."""
    inp = MC.make_case(case)
    N, nx = case.N, case.nx
    with_table, without = device_rhs(inp), device_rhs(inp, reactions=False)
    worst = 0.0
    for b, p in enumerate(inp.problems):
        C = inp.y[b].reshape(N, nx)
        rates, mag = R.get_rates(C, p), MC.rate_magnitudes(C, p)
        diff = (with_table[b] - without[b]).reshape(N, nx)
        assert (diff[:, 0] == 0.0).all() and (diff[:, -1] == 0.0).all()
        assert np.abs(rates[:, 0]).max() > 0 and np.abs(rates[:, -1]).max() > 0          # ... where the rates themselves are not
        for k in range(N):
            scale = np.abs(rates[k, 1:-1]).max()
            if scale == 0.0:                                                            # a species no reaction names
                assert (diff[k] == 0.0).all()
                continue
            bar = (2.0 ** -52 * np.abs(with_table[b].reshape(N, nx)[k]).max() + 8 * 2.0 ** -53 * mag[k].max()) / scale
            err = np.abs(diff[k, 1:-1] - rates[k, 1:-1]).max() / scale
            assert bar < 1e-9
            assert err <= bar, (MC.case_id(case), b, k, err, bar)
            worst = max(worst, err / bar)
    print('MOLRATE | %s | largest error / bar %.3f |' % (MC.case_id(case), worst))


@pytest.mark.parametrize('case', [MC.GRIDS[4], MC.TABLES[0], MC.GRIDS[20], MC.NOMIG[3]], ids=MC.case_id)
def test_a_second_call_gives_the_bits_of_a_fresh_handle(case):
    """rates, ytmp / ftmp and the gradient row are scratch of the handle: a call with another argument carries nothing over"""
    inp, other = MC.make_case(case), MC.make_case(case, seed=1)
    assert not np.array_equal(inp.y, other.y)
    p = inp.problems[0]
    with solver_from_problem(p, 'FTCS', batch_capacity=MC.CAPACITY) as s:
        s.set_batch(inp.upload, inp.pb, inp.vzeta, inp.flux)
        first = s.mol_rhs(3.0 * other.y)
        second = s.mol_rhs(inp.y)
        third = s.mol_rhs(inp.y)
    fresh = device_rhs(inp)
    assert not np.array_equal(first, fresh)
    assert np.array_equal(second, fresh) and np.array_equal(third, fresh)
