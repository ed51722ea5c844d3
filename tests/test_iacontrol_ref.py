"""tests/iacontrol_ref.py, the restatements of include/catint_iacontrol.h, on the CPU (no device, no library).

The mathematics: control_mp at the 60-digit steady state of every case of tests/interact_cases.py against central differences of
interact_ref's 60-digit solves with the parameter of the column shifted by +-1e-20 -- off[r][0], off[r][1] or both (the rate constants
and the transition state of step r), the a0 and e0 entries of the tables (the formation energy of an adsorbate: a0_r by -m[r][G+a],
e0_r by +order_f[r][N+G+a]) and the strength.  Nothing of the code under test is on the reference side: the re-solves know the model
through interact_ref._mp_rates alone.  Then control_fp64 against control_mp, the reduction to drc_ref.control_fp64 bit for bit, and the
sum rule."""
import mpmath as mp
import numpy as np
import pytest

from tests import drc_ref as DR
from tests import iacontrol_ref as CR
from tests import interact_cases as IC
from tests import interact_ref as IR
from tests import kinetics_cases as KC
from tests import kinetics_ref as KR

H = mp.mpf(10) ** -20


def columns(t):
    """(field, row, d off [R][2], d a0 [R], d e0 [R], d strength) of every column, in the order of iacontrol_ref"""
    R, S, G = t['R'], t['S'], t['G']
    zero, out = np.zeros(R), []
    for fam, (kf, kb) in (('dflux_dlnkf', (1, 0)), ('dflux_dlnkb', (0, 1)), ('dflux_drc', (1, 1))):
        for r in range(R):
            d = np.zeros((R, 2))
            d[r] = (kf, kb)
            out.append((fam, r, d, zero, zero, 0))
    for a in range(S):
        out.append(('dflux_dG', a, np.zeros((R, 2)), -t['m'][:, G + a], t['ofc'][:, G + a], 0))
    out.append(('dflux_dstrength', None, np.zeros((R, 2)), zero, zero, 1))
    return out


def shifted(t, off, lam, col, sign):
    """the tables, the off row and the strength with the column's parameter moved by sign * H"""
    _, _, d_off, d_a0, d_e0, d_lam = col
    f = mp.mpf
    R = t['R']
    dG, Ea = np.array(t['dG'], dtype=object), np.array(t['Ea'], dtype=object)
    o = np.empty((R, 2), dtype=object)
    for r in range(R):
        dG[r, 0] = f(t['dG'][r, 0]) + sign * H * int(d_a0[r])
        if t['ts'][r]:
            Ea[r, 0] = f(t['Ea'][r, 0]) + sign * H * int(d_e0[r])
        for q in range(2):
            o[r, q] = f(off[r, q]) + sign * H * int(d_off[r, q])
    return dict(t, dG=dG, Ea=Ea), o, lam + sign * H * d_lam


@pytest.mark.parametrize('name', IC.CASE_NAMES)
def test_control_mp_agrees_with_central_differences_of_60_digit_solves(name):
    c = IC.case(name)
    fp = IC.fp64(name)
    assert (fp['status'] == 0).all()
    t = IR._arrays(c.tables)
    N, T, R, G = t['N'], t['T'], t['R'], t['G']
    w, CS, pzc = c.kw['w'], c.kw['CS'], c.kw['phi_pzc']
    cols = columns(t)
    worst = {k: 0.0 for k in CR.RAW + CR.DY}
    with mp.workdps(IR.DPS):
        f = mp.mpf
        off = np.zeros((R, 2))
        g = np.ones(N)
        ys = []
        states = []
        for i in range(len(c.phiM)):
            lam = f(float(fp['strength_reached'][i]))
            assert lam == f(t['strength'])
            V, sg, a = IR._mp_inputs(t, c.phiM[i], c.csurf[i], c.phi_surface[i], w, CS, pzc, None, g)
            rf, rb, _ = IR._mp_rates(t, [f(v) for v in fp['y'][i]], V, sg, a, off, lam)
            dead = {s for s in range(G, T) if sum(abs(int(t['m'][r, s])) * (rf[r] + rb[r]) for r in range(R)) == 0}
            point = (f(c.phiM[i]), [f(v) for v in c.csurf[i]], f(c.phi_surface[i]), w, CS, pzc, None)
            y, _, _, flux, _, frozen = IR._mp_solve(t, fp['y'][i], dead, *point, off, g, lam, want_frozen=True)
            ys.append(y)
            states.append((dead, point, lam, frozen))
        ref = CR.control_mp(c.tables, c.phiM, c.csurf, c.phi_surface, None, w=w, CS=CS, phi_pzc=pzc, y_mp=ys)
        for i, (dead, point, lam, frozen) in enumerate(states):
            assert ref['residual'][i] < mp.mpf(10) ** -40
            scale = ref['flux_scale'][i]
            for p, col in enumerate(cols):
                (tp, op, lp), (tm, om, lm) = shifted(t, off, lam, col, +1), shifted(t, off, lam, col, -1)
                yp, _, _, fluxp, _, _ = IR._mp_solve(tp, ys[i], dead, *point, op, g, lp, frozen=frozen)
                ym, _, _, fluxm, _, _ = IR._mp_solve(tm, ys[i], dead, *point, om, g, lm, frozen=frozen)
                fam, row = col[0], col[1]
                want = ref[fam][i] if row is None else ref[fam][i][row]
                for k in range(N):
                    d = abs((fluxp[k] - fluxm[k]) / (2 * H) - want[k])
                    if scale[k] == 0:
                        assert d == 0
                    else:
                        worst[fam] = max(worst[fam], float(d / scale[k]))
                for k in range(T):
                    d = abs((yp[k] - ym[k]) / (2 * H) - ref['dy'][i][p][k])
                    key = 'dy_drc' if fam == 'dflux_drc' else ('dy_dstrength' if fam == 'dflux_dstrength' else None)
                    if key:
                        worst[key] = max(worst[key], float(d))
                    assert d < mp.mpf(10) ** -15, (i, fam, row, k)
    print(name, 'control_mp against central differences, in units of flux_scale (dy: absolute):',
          '; '.join('%s %.1e' % kv for kv in worst.items()))
    for k, v in worst.items():
        assert v <= 1e-15, (k, v)


@pytest.mark.parametrize('name', IC.CASE_NAMES)
def test_control_fp64_agrees_with_control_mp_and_keeps_the_sum_rule(name):
    c = IC.case(name)
    theta = IC.fp64(name)['theta']
    fp = CR.control_fp64(c.tables, c.phiM, c.csurf, c.phi_surface, theta, **c.kw)
    ref = CR.control_mp(c.tables, c.phiM, c.csurf, c.phi_surface, theta, **c.kw)
    assert (fp['status'] == 0).all() and fp['residual'].max() <= 1e-12
    # The fluxes and their derivatives in units of drc_scale, entry by entry.  dy in units of the largest drc_scale of its column:
    # elimination with partial pivoting is backward stable in the norm, and componentwise only as far as |J^-1| is known -- an entry of
    # J^-1 that is itself a difference of equal terms (two rows of a quasi-equilibrated step) makes drc_scale of a dy entry of 1e-29
    # too small, as at one point of the terrace-and-step case.
    scales = dict(fp, drc_scale=dict(fp['drc_scale'], **{k: np.broadcast_to(fp['drc_scale'][k].max(axis=-1, keepdims=True),
                                                                            fp['drc_scale'][k].shape) for k in CR.DY}))
    err = CR.errors(fp, ref, scales)
    print(name, 'control_fp64 against control_mp, in units of drc_scale:', '; '.join('%s %.1e' % (k, v.max()) for k, v in err.items()))
    # one solve and one refinement step of a T <= 9 system, every sum of at most 16 terms: a few hundred roundings of the term sums
    for k, v in err.items():
        assert v.max() <= 1e-13, (k, v.max())
    assert np.allclose(KR.mp_err(ref['flux_scale'], fp['flux_scale'], fp['flux_scale']), 0.0, atol=1e-14)
    # scaling every rate constant by one factor leaves the coverages unchanged, shifts included: sum_r dflux_drc[r][k] = flux_k
    gap = np.abs(fp['dflux_drc'].sum(axis=1) - fp['flux'])
    bound = 1e-13 * (fp['drc_scale']['dflux_drc'].sum(axis=1) + fp['flux_scale'])
    print(name, 'sum rule: worst gap / bound %.2e' % (gap / np.where(bound > 0, bound, 1.0)).max())
    assert (gap <= bound).all()
    with mp.workdps(IR.DPS):
        for i in range(len(c.phiM)):
            for k in range(len(ref['flux'][i])):
                total = sum(ref['dflux_drc'][i][r][k] for r in range(len(ref['dflux_drc'][i])))
                # (at the fp64 coverages the state is a root to rounding only: the rule holds to the residual times the term sum)
                assert abs(total - ref['flux'][i][k]) <= mp.mpf(1e-11) * abs(ref['flux_scale'][i][k]) + mp.mpf(10) ** -300
    # the normalised fields are the quotients of the raw ones
    idle = ~(np.asarray(c.tables['nu']) != 0.0).any(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        want = fp['dflux_dstrength'] / fp['flux']
        want = np.where(idle[None, :], 0.0, float(c.tables['strength']) * want)
    assert np.array_equal(fp['strength_control'], want, equal_nan=True)


def mean_field_as_interacting(tables, **more):
    T = len(tables['site_count'])
    return dict(tables, site_of=np.zeros(T, np.int32), site_fraction=np.ones(1), eps=np.zeros((T - 1, T - 1)), strength=0.0, **more)


@pytest.mark.parametrize('name', KC.CASE_NAMES)
def test_one_site_type_at_strength_0_has_the_bits_of_the_mean_field_restatement(name):
    c = KC.case(name)
    theta = KR.solve_fp64(c.tables, c.phiM, c.csurf, c.phi_surface, sens=False, **c.kw)['theta']
    want = DR.control_fp64(c.tables, c.phiM, c.csurf, c.phi_surface, theta, **c.kw)
    for tab in (mean_field_as_interacting(c.tables), mean_field_as_interacting(c.tables, response='piecewise', cutoff=[0.25], smoothing=[0.05])):
        got = CR.control_fp64(tab, c.phiM, c.csurf, c.phi_surface, theta, **c.kw)
        for k in CR.OLD + ('residual', 'status'):
            assert np.array_equal(want[k], got[k], equal_nan=True), k
        for k in want['drc_scale']:
            assert np.array_equal(want['drc_scale'][k], got['drc_scale'][k], equal_nan=True), k
        assert (got['dflux_dstrength'] == 0.0).all() and (got['strength_control'] == 0.0).all()
    # an interaction table that is there but switched off by the strength changes the old families by nothing either
    S = len(c.tables['site_count']) - 1
    on = dict(mean_field_as_interacting(c.tables), eps=np.full((S, S), 2.0))
    got = CR.control_fp64(on, c.phiM, c.csurf, c.phi_surface, theta, **c.kw)
    for k in CR.OLD:
        assert np.array_equal(want[k], got[k], equal_nan=True), k
    assert np.isfinite(got['dflux_dstrength']).all() and (got['dflux_dstrength'] != 0.0).any()
    assert (got['strength_control'] == 0.0).all()
