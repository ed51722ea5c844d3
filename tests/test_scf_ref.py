"""The restatement of the device SCF loop (tests/scf_ref.py) and the case table of tests/scf_cases.py, on the CPU.

(a) With the analytic kinetics / transport pair of tests/test_host_scf.py as its transport, scf_ref.scf_lane walks the iterates of the
    REFERENCE's own loop (tests/golden/scf_cycle.json, written by tests/golden/make_scf_golden.py) -- heads, tails, iterations 41/42,
    final mix and pH, the lane that never leaves the fallback -- to the tolerances of test_host_scf.py.  That ties the reference of
    tests/test_gpu_scf.py to catint/calculator.py:294-406 without going through catint_amd/calculator.py.
(b) The case table on the reference alone: every branch a case names fires in the lane meant for it, stuck lanes are stuck with a finite
    state, every other solve converges within half of maxit, and no accuracy of any lane at any iteration lies within a factor 1.5 of the
    case's tau -- the integer bookkeeping the device is compared on (exit iteration, active, mix, step_to_check) cannot flip on rounding.
"""
import json
import os

import numpy as np
import pytest

from tests import scf_cases, scf_ref

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scf_cycle.json')))
F = 96485.33289        # (any value: the accuracy is a ratio of current densities)


@pytest.mark.parametrize('entry', GOLDEN, ids=[e['input']['name'] for e in GOLDEN])
def test_restatement_walks_the_reference_loops_iterates(entry):
    case, ref = entry['input'], entry['reference']
    cb, D, L, kin = np.array(ref['bulk']), np.array(case['D']), case['system']['boundary thickness'], case['kinetics']
    wall = {'species': [kin['educt']], 'nu': [kin['nu']]}
    nel = [1.0, 1.0, 1.0, 2.0]           # CO2 + H2O + 2 e- -> CO + 2 OH-: nel = 2 for CO (calculator.py:389-400)
    iOH = ref['species_order'].index('OH-')
    assert 'H+' not in ref['species_order']
    for phiM, lane in zip(case['phis'], ref['lanes']):
        K = [kin['k0'] * np.exp(-kin['alpha'] * (phiM - kin['phi0']))]

        def transport(flux):
            return cb + flux * L / D, phiM, 0.0, 'ok'
        # the reference's start: istep = 0, step_to_check = 0, accuracy = inf, surface = bulk (calculator.py:296-298)
        state = {'surface_concentration': cb.copy(), 'surface_concentration_old': np.zeros(4), 'flux': np.zeros(4),
                 'current_density_old': np.zeros(4), 'mix': case['mix_scf'], 'accuracy': np.inf, 'surface_pH': np.nan,
                 'surface_potential': phiM, 'surface_efield': 0.0, 'step_to_check': 0, 'active': 1, 'failed': 0}
        n = lane['iterations']
        out, last, trace = scf_ref.scf_lane(state, wall, K, phiM, transport, 0, n if not lane['converged'] else case['max_iter'],
                                            case['tau_scf'], F, nel=nel, species_OH=iOH)
        assert last == n == len(trace)
        for it, t in enumerate(lane['trace_head']):
            assert np.allclose(trace[it]['sc'], t['sc_in'], rtol=1e-13, atol=0), (phiM, it)
            assert np.allclose(trace[it]['flux'], t['flux'], rtol=1e-13, atol=0)
            assert np.allclose(trace[it]['sc_out'], t['sc_out'], rtol=1e-13, atol=1e-300)
            assert np.isclose(trace[it]['surface_pH'], t['surface_pH'], rtol=1e-13)
            assert trace[it]['mix'] == t['mix']
        for k, t in enumerate(lane['trace_tail']):
            it = n - len(lane['trace_tail']) + k
            assert np.allclose(trace[it]['sc'], t['sc_in'], rtol=1e-12, atol=0), (phiM, it)
            assert np.allclose(trace[it]['sc_out'], t['sc_out'], rtol=1e-12, atol=1e-300)
        for k, t in enumerate(lane['trace_41_42']):
            assert np.allclose(trace[40 + k]['sc'], t['sc_in'], rtol=1e-12, atol=0)
        assert [[t['iteration'], t['mix']] for i, t in enumerate(trace) if i == 0 or t['mix'] != trace[i - 1]['mix']] == lane['mix_changes']
        assert [t['iteration'] for t in trace if t['sc_out'].min() < 0] == lane['negative_iterations']
        assert np.allclose(out['surface_concentration'], lane['final_sc'], rtol=1e-12, atol=0)
        assert np.allclose(out['flux'], lane['final_flux'], rtol=1e-12, atol=0)
        assert np.isclose(out['surface_pH'], lane['final_surface_pH'], rtol=1e-12)
        assert out['mix'] == lane['final_mix'] and out['failed'] == 0
        assert out['active'] == (0 if lane['converged'] else 1)
        if not lane['converged']:
            assert all('fallback' in t['fired'] for t in trace[3:])        # (iteration 2 answered positive: the fallback starts at 4)
    names = [e['input']['name'] for e in GOLDEN]
    assert {'slow_mixing_decay', 'stuck_on_the_negative_fallback', 'negative_surface_concentration'} <= set(names)


@pytest.mark.parametrize('name', list(scf_cases.CASES))
def test_case_table_reaches_its_branches_and_keeps_clear_of_tau(name):
    case = scf_cases.get(name)
    ref = case.reference()
    maxit = scf_cases.MAXIT
    for j, lane in enumerate(case.lanes):
        trace, tr = ref.traces[j], ref.transports[j]
        fired = set().union(*[t['fired'] for t in trace]) if trace else set()
        assert set(lane.get('fires', ())) <= fired, (name, j, lane.get('fires'), fired)
        for spec in lane.get('fires_at', ()):                      # (branch, iteration)
            at = [t for t in trace if t['iteration'] == spec[1]]
            assert at and spec[0] in at[0]['fired'], (name, j, spec)
        stuck = [t['iteration'] for t in trace if t['stuck']]
        if 'stuck_from' in lane:
            assert stuck == list(range(lane['stuck_from'], case.max_iter + 1)), (name, j, stuck)
            assert np.isfinite(tr.c).all() and np.isfinite(tr.phi).all()
            assert ref.out['active'][j] == 1 and (ref.out['surface_concentration'][j] == -1.0).all()
        else:
            assert not stuck, (name, j, stuck)
        for it, t in zip(tr.iterations, trace):
            if t['status'] == 'ok':
                assert it <= maxit // 2, (name, j, t['iteration'], it)
            elif t['status'] == 'stuck':
                assert it == maxit + 1
        if lane.get('inactive'):
            assert not trace
        if lane.get('fails'):
            assert ref.out['failed'][j] == 1 and ref.out['active'][j] == 0
        else:
            assert ref.out['failed'][j] == 0
            for t in trace:                                        # the guard band (a condition on the inputs, not a tolerance)
                a = t['accuracy']
                assert not (case.tau / 1.5 <= a <= 1.5 * case.tau), (name, j, t['iteration'], a)
        if 'exits_at' in lane:
            assert ref.last[j] == lane['exits_at'], (name, j, ref.last[j])
    if case.distinct_exits:
        assert len({ref.last[j] for j, l in enumerate(case.lanes) if not l.get('fails') and 'stuck_from' not in l}) >= case.distinct_exits
    assert ref.iterations == max(ref.last)
    if case.wall.get('alpha') is not None:          # the Butler-Volmer factor is live: the reaction plane is not at the electrode potential
        ok = np.array([not l.get('fails') for l in case.lanes])
        assert (np.abs(case.phiM - ref.out['surface_potential'])[ok] > 1e-3).all()
