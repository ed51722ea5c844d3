"""CPU: the multiprecision restatement of ode_func (tests/mol_ref.py) pinned to the fp64 oracle (oracle/pnp_ref.py mol_rhs, itself
pinned bit for bit to the reference's samples), the oracle's own error E_oracle on every short-grid case of the matrix of
tests/test_gpu_mol_rhs.py, and the assertion of that file shown to work: it passes an fp64 evaluation that sums in another order and
rejects seven ways of getting the right-hand side subtly wrong."""
import glob
import os

import numpy as np
import pytest

from oracle import pnp_ref as R
from tests import mol_cases as MC
from tests import mol_ref as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MOL = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, 'odeint_*.npz')))
PIN = 1e-12      # the bar of the oracle's own banded-against-dense pin (tests/test_oracle_golden.py)


@pytest.mark.parametrize('name', MOL)
def test_restatement_agrees_with_the_reference_samples(name):
    """the reference's own right-hand-side samples (reactions, migration off, Lax-Friedrichs, wall flux among them)"""
    d = np.load(os.path.join(GOLDEN, name + '.npz'))
    p = R.problem_from_golden(d)[0]
    assert len(d['rhs_states']) == 3
    for s, val in zip(d['rhs_states'], d['rhs_values']):
        ref = M.mol_rhs(s, p, use_reactions=bool(p.reactions))
        assert M.row_errors(val, ref, p.N).max() < PIN
        assert ref.reshape(p.N, -1)[:, -1].tolist() == [0] * p.N
        if p.reactions:
            rr = M.rates_array(s, p)
            assert M.row_errors(R.get_rates(s.reshape(p.N, -1), p), rr, p.N).max() < PIN
            # the wall cell carries no rate term: the restatement with and without the table agree there exactly
            plain = M.mol_rhs(s, p, use_reactions=False).reshape(p.N, -1)
            assert (ref.reshape(p.N, -1)[:, 0] == plain[:, 0]).all() and (ref.reshape(p.N, -1)[:, 1] != plain[:, 1]).any()


def test_the_matrix_is_the_one_the_issue_lists():
    assert MC.B == 5 and MC.CAPACITY == 8
    assert {c.nx for c in MC.GRIDS} == {5, 66, 67, 130, 131, 258, 259, 514, 515, 1026, 1027, 2050}
    assert all(c.table != 'none' for c in MC.GRIDS) and {c.pb for c in MC.GRIDS} == set(MC.MOL_PB)
    for nx in MC.GRID_NX:
        assert {c.lf for c in MC.GRIDS if c.nx == nx} == {False, True}
    assert {(c.N, c.nx) for c in MC.SPECIES} == {(N, nx) for N in (1, 2, 7, 16) for nx in (67, 1027)}
    assert all(c.mig == (c.N > 1) for c in MC.SPECIES)
    assert {c.table for c in MC.TABLES} == {'buffer', 'overwrite', 'max'}
    assert {(c.nx, c.table != 'none') for c in MC.NOMIG} == {(nx, r) for nx in (67, 1027) for r in (False, True)} and not any(c.mig for c in MC.NOMIG)
    t = MC.table('max', 16)
    assert len(t) == 16 and max(len(l) for l, r, _, _ in t) == 4 == max(len(r) for l, r, _, _ in t)
    for c in MC.ALL:
        inp = MC.make_case(c)
        assert len({tuple(np.nan_to_num(r, nan=7.0)) for r in inp.pb}) == MC.B and len(set(inp.vzeta)) == MC.B      # per-lane values
        assert len({R.pb_mode_from_bound(r) for r in inp.pb}) == 1
        assert len({tuple(r) for r in inp.flux}) == MC.B and ((inp.flux == 0).sum(axis=1) >= (c.N > 1)).all() and (inp.flux == 0).any()
        assert c.N < 3 or ((inp.flux > 0).any(axis=1) | (inp.flux < 0).any(axis=1)).all()
        assert (inp.flux > 0).any() and (inp.flux < 0).any() and (inp.y > 0).all()
        assert len({r.tobytes() for r in inp.y}) == MC.B and not np.array_equal(inp.upload, inp.y)


@pytest.mark.parametrize('case', MC.SHORT, ids=MC.case_id)
def test_oracle_error_against_the_restatement(case):
    """E_oracle: what rounding costs the fp64 oracle on this case -- the pin of the restatement on all five Poisson branches, every
    species count and rate table, and the number the device bar is a multiple of."""
    e = MC.e_oracle(case)
    inp = MC.make_case(case)
    dense = MC.oracle_rhs(inp, solver='dense')
    e_dense = max(M.row_errors(dense[b], MC.mp_rhs(case)[b], case.N).max() for b in range(MC.B))
    print('E_oracle %s: banded %.3e dense %.3e bar %.3e' % (MC.case_id(case), e, e_dense, MC.bar_short(case)))
    assert MC.FLOOR <= e < PIN and e_dense < PIN
    assert MC.bar_short(case) <= 1e-9


# ---- an fp64 evaluation in another order, and the seven defects --------------------------------------------------------------------------
MUTANTS = ['rates_from_the_uploaded_state', 'flux_of_lane_0', 'rate_at_the_wall_cell', 'rate_at_the_bulk_point', 'rates_of_neighbour_species_swapped',
           'migration_kept_when_off', 'rates_accumulated']


def gradient_other_order(C, p):
    """grad_v with the charge row summed in reverse species order, the Dirichlet-Dirichlet system eliminated from the bulk end, and
    the prefix sums taken by cumsum"""
    nx, dx = p.nx, p.dx
    lapl = np.zeros(nx)
    for k in reversed(range(p.N)):
        lapl = lapl - C[k] * (p.charges[k] / p.eps)
    vw, vb, gw, gb = p.pb
    g = np.zeros(nx)
    if not np.isnan(vw) and not np.isnan(vb):
        m = nx - 2
        b = lapl[1:nx - 1] * (dx * dx)
        b[0] -= vw
        b[-1] -= vb
        x = R._thomas(np.ones(m), -2.0 * np.ones(m), np.ones(m), b[::-1].copy())[::-1]
        v = np.concatenate([[vw], x, [vb]])
        g[1:nx - 1] = (v[2:] - v[:-2]) * (0.5 / dx)
        g[0], g[-1] = 2.0 * g[1] - g[2], 2.0 * g[-2] - g[-3]
    elif not np.isnan(gw):
        g[1:nx - 1] = gw + np.cumsum(lapl[1:nx - 1] * dx)
        g[0], g[-1] = gw, 2.0 * g[-2] - g[-3]
    else:
        g[1:nx - 1] = (gb - np.cumsum((lapl[1:nx - 1] * dx)[::-1]))[::-1]
        g[0], g[-1] = 2.0 * g[1] - g[2], gb
    return g


def rates_accumulated(C, p):
    rates = np.zeros_like(C)
    for lhs, rhs, kf, kr in p.reactions:
        pl = np.prod([C[k] for k in lhs], axis=0) if lhs else np.ones(C.shape[1])
        pr = np.prod([C[k] for k in rhs], axis=0) if rhs else np.ones(C.shape[1])
        for k in lhs:
            rates[k] += pr * kr - pl * kf
        for k in rhs:
            rates[k] += pl * kf - pr * kr
    return rates


def emulate(inp, mutant=None):
    """what a correct fp64 kernel may return (mutant None): the same formulas, associated differently; or one of the defects"""
    out = []
    for b, p in enumerate(inp.problems):
        N, nx, dx, dt = p.N, p.nx, p.dx, p.dt
        C = inp.y[b].reshape(N, nx)
        flux = inp.flux[0] if mutant == 'flux_of_lane_0' else inp.flux[b]
        mig = p.use_migration or mutant == 'migration_kept_when_off'
        g = gradient_other_order(C, p) if mig else np.zeros(nx)
        Cr = inp.upload[b].reshape(N, nx) if mutant == 'rates_from_the_uploaded_state' else C
        rates = np.zeros_like(C)
        if p.reactions:
            rates = rates_accumulated(Cr, p) if mutant == 'rates_accumulated' else R.get_rates(Cr, p)
        if mutant == 'rates_of_neighbour_species_swapped' and N > 1:
            for k in range(0, N - 1, 2):
                rates[[k, k + 1]] = rates[[k + 1, k]]
        f = np.zeros((N, nx))
        for k in range(N):
            bq = p.beta * p.charges[k]
            d2 = ((C[k, 2:] - C[k, 1:-1]) - (C[k, 1:-1] - C[k, :-2])) / (dx * dx)
            dcg = (C[k, 2:] * g[2:] - C[k, :-2] * g[:-2]) * (0.5 / dx)
            f[k, 1:-1] = p.D[k] * d2 + p.D[k] * bq * dcg + rates[k, 1:-1]
            if p.lax_friedrich:
                f[k, 1:-1] += d2 * (dx * dx) / (2.0 * dt)
            f[k, 0] = (p.D[k] * (C[k, 2] - C[k, 0]) / (2.0 * dx) + p.D[k] * bq * C[k, 1] * g[1] - flux[k]) / dx
            if p.lax_friedrich:
                f[k, 0] += (C[k, 1] - C[k, 0]) / dt
            if mutant == 'rate_at_the_wall_cell':
                f[k, 0] += rates[k, 0]
            if mutant == 'rate_at_the_bulk_point':
                f[k, -1] = rates[k, -1]
        out.append(f.reshape(-1))
    return np.stack(out)


def check(case, f):
    """the assertion of tests/test_gpu_mol_rhs.py on the result f[B][N*nx] of one case"""
    inp = MC.make_case(case)
    if case.nx <= MC.MP_MAX_NX:
        return M.assert_rows_within(f, MC.mp_rhs(case), case.N, MC.bar_short(case), MC.case_id(case))
    return M.assert_rows_within(f, MC.oracle_rhs(inp), case.N, MC.bar_long(case), MC.case_id(case))


@pytest.mark.parametrize('case', MC.ALL, ids=MC.case_id)
def test_the_assertion_passes_an_fp64_evaluation_in_another_order(case):
    f = emulate(MC.make_case(case))
    assert not np.array_equal(f, MC.oracle_rhs(MC.make_case(case)))
    check(case, f)


@pytest.mark.parametrize('mutant', MUTANTS)
def test_the_assertion_rejects(mutant):
    """every case of the matrix that the defect can touch rejects it (at least one short-grid and one long-grid case each)"""
    def touched(c):
        if mutant == 'migration_kept_when_off':
            return not c.mig and c.N > 1
        if mutant == 'flux_of_lane_0':
            return True
        if mutant == 'rates_of_neighbour_species_swapped':
            return c.table != 'none' and c.N > 1
        return c.table != 'none'
    cases = [c for c in MC.ALL if touched(c)]
    if mutant == 'rates_accumulated':      # tables in which a species is written more than once
        cases = [c for c in cases if c.table in ('overwrite', 'buffer', 'max', 'single')]
    assert any(c.nx <= MC.MP_MAX_NX for c in cases) and any(c.nx > MC.MP_MAX_NX for c in cases)
    for c in cases:
        f = emulate(MC.make_case(c), mutant)
        with pytest.raises(AssertionError, match='error'):
            check(c, f)
            print('not rejected:', mutant, MC.case_id(c))
