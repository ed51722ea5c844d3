"""tests/scfkin_ref.py -- the restatement tests/test_gpu_scfkin.py compares pnp_scf_cycle_fn with -- against the host loop it restates,
and the case table of tests/scfkin_cases.py against what its entries say.  No device.

The reference of the restatement is Calculator.run_scf_cycle itself: on the end-to-end case of tests/test_gpu_kinetics.py (N = 4,
nx = 64, Stern wall, eight potentials) the host loop runs with the CPU kinetics (tests.test_kinetics_abi.FakeKinetics) and the oracle's
transport, once for two iterations and once to the end; the restatement entered with the arrays of the first run must end with the
arrays and the iteration count of the second, exactly -- both sides are NumPy over the same functions."""
import numpy as np
import pytest

from catint_amd.units import unit_F
from oracle import pnp_physical as PH
from tests import scfkin_cases as SC
from tests import scfkin_ref
from tests.scf_cases import MAXIT
from tests.test_kinetics_abi import FakeKinetics


class Recording(FakeKinetics):
    def solve(self, view, tab, phiM, csurf=None, **kw):
        out = FakeKinetics.solve(self, view, tab, phiM, csurf=csurf, **kw)
        self.calls[-1]['csurf'] = np.array(csurf)
        return out


def host_loop(max_iter):
    """The end-to-end case on the CPU, as tests.test_gpu_kinetics.scf_on_the_cpu runs it: (result, kinetics, transports, tp)"""
    from catint_amd.calculator import Calculator
    from tests.test_gpu_kinetics import E2E_PHIS, e2e_model, e2e_transport
    tp = e2e_transport()
    calc = Calculator(transport=tp, calc='comsol', tau_scf=1e-8)
    calc.set_microkinetics(e2e_model(tp), site_density=2e-6)
    fake = Recording()
    calc._kinetics_solver = lambda: fake
    cb = [tp.species[sp]['bulk_concentration'] for sp in tp.species]
    c0 = tp.c0.reshape(tp.nspecies, tp.nx)
    transports = [scfkin_ref.OracleTransport(PH.PhysicalProblem(D=tp.D, charges=tp.charges, beta=tp.beta, eps=tp.eps, dx=tp.dx, nx=tp.nx, c_bulk=cb,
                                                                phiM=phiM, flux=np.zeros(tp.nspecies), stern_capacitance=0.2, phi_pzc=0.1),
                                             c0, np.zeros(tp.nx), tol=1e-8, maxit=50) for phiM in E2E_PHIS]

    def transport_fn(flux):
        res = [t(flux[i]) for i, t in enumerate(transports)]
        return np.array([r[0] for r in res]), np.array([r[1] for r in res]), np.array([r[2] for r in res])
    return calc.run_scf_cycle(transport_fn=transport_fn, max_iter=max_iter), fake, transports, tp, calc


def test_the_restatement_entered_after_iteration_2_ends_where_the_host_loop_ends():
    from tests.test_gpu_kinetics import E2E_PHIS
    two, fake, transports, tp, calc = host_loop(2)
    full, _, _, tp_full, _ = host_loop(200)
    assert full['converged'].all() and 10 < full['iterations'] < 60 and len(fake.calls) == 2
    B = len(E2E_PHIS)
    system = [tp.alldata[i]['system'] for i in range(B)]
    live = ~(two['converged'] | two['failed'])
    assert live.all()
    state = {'surface_concentration': two['surface_concentration'], 'surface_concentration_old': fake.calls[1]['csurf'], 'flux': two['flux'],
             'current_density_old': two['current_density'], 'mix': two['mix'], 'accuracy': two['accuracy'], 'surface_pH': two['surface_pH'],
             'surface_potential': np.array([s['surface_potential'] for s in system]), 'surface_efield': np.array([s['surface_efield'] for s in system]),
             'step_to_check': np.zeros(B, np.int32), 'active': live.astype(np.int32), 'failed': two['failed'].astype(np.int32)}
    micro = calc.microkinetics
    kin = scfkin_ref.Kinetics(micro['tables'], micro['potential_drop'], 0.2, 0.1)
    kstates = [kin.begin(two['coverage'][b]) for b in range(B)]
    out, kout, iterations, traces = scfkin_ref.scfkin_batch(state, kin, kstates, np.array(E2E_PHIS), transports, 2, 200, 1e-8, unit_F)
    assert iterations == full['iterations']
    for mine, theirs in (('surface_concentration', 'surface_concentration'), ('flux', 'flux'), ('current_density_old', 'current_density'),
                         ('mix', 'mix'), ('accuracy', 'accuracy'), ('surface_pH', 'surface_pH')):
        assert np.array_equal(out[mine], full[theirs]), mine
    assert not out['active'].any() and not out['failed'].any()
    assert np.array_equal(kout['theta'], full['coverage']) and np.array_equal(kout['flux_scale'], full['flux_scale'])
    assert np.array_equal(kout['status'], full['kinetic_status']) and np.array_equal(kout['flux_last'], full['flux'])
    for b in range(B):
        s = tp_full.alldata[b]['system']
        assert out['surface_potential'][b] == s['surface_potential'] and out['surface_efield'][b] == s['surface_efield']
        assert kout['calls'][b] == len(traces[b]) == kout['calls'][b] and traces[b][-1]['iteration'] <= iterations


@pytest.mark.parametrize('name', sorted(SC.CASES))
def test_every_lane_of_the_case_table_does_what_its_entry_says(name):
    case = SC.get(name)
    ref = case.reference()
    assert case.istep < ref.iterations < case.max_iter                      # the loop ends because every lane has left
    assert not ref.out['active'].any()
    passed_decay = False
    for j, lane in enumerate(case.lanes):
        trace = ref.traces[j]
        if lane.get('inactive'):
            assert not trace and ref.kin['calls'][j] == 0 and np.isnan(ref.kin['theta'][j]).all()
            for k in scfkin_ref.ROWS + scfkin_ref.SCALARS + scfkin_ref.FLAGS:
                assert np.array_equal(ref.out[k][j], ref.entry_state[k][j], equal_nan=True), (j, k)
            continue
        if lane.get('fails'):
            assert len(trace) == 1 and trace[0]['kinetic_status'] == lane['fails'] == ref.kin['status'][j] and trace[0]['status'] == 'nan'
            assert ref.out['failed'][j] == 1 and np.isnan(ref.out['flux'][j]).all() and (ref.kin['flux_last'][j] == 0).all()
            continue
        assert ref.out['failed'][j] == 0 and ref.kin['status'][j] == 0 and ref.kin['calls'][j] == len(trace) >= 3
        assert all(t['status'] == 'ok' and t['kinetic_status'] == 0 for t in trace)
        # every transport solve well inside its iteration limit, every accuracy a factor 1.5 away from tau
        assert max(ref.transports[j].iterations) <= MAXIT // 2, (j, ref.transports[j].iterations)
        acc = np.array([t['accuracy'] for t in trace])
        assert np.isfinite(acc).all()
        ratio = np.abs(acc) / case.tau
        assert np.minimum(ratio, 1.0 / ratio).max() <= 1.0 / 1.5, (j, acc)
        assert (acc[:-1] > case.tau).all() and acc[-1] <= case.tau
        decays = [t['iteration'] for t in trace if t['decay']]
        assert decays == ([lane['decays_at']] if 'decays_at' in lane else []), (j, decays)
        passed_decay = passed_decay or any(d > 41 and trace[-1]['iteration'] > d for d in decays)
        # the kinetics are warm-started: the first call starts from the uniform surface, the last ones are a few iterations
        its = [t['kinetic_iterations'] for t in trace]
        assert its[0] > 8 and its[-1] <= 4, (j, its)
    if name == 'B':
        assert passed_decay and case.species_OH == 1 and case.x is not None and case.nx == 33
        assert (ref.out['surface_pH'][[0, 1, 3, 5]] != 7.0).all() and ref.out['surface_pH'][4] == 7.0
        assert case.kin.S == 3 and list(case.kin.tables['site_count']) == [1.0, 1.0, 2.0, 1.0]
    else:
        assert case.nx == 65 and case.N == 4 and case.P == 8 and (ref.out['surface_pH'] == 7.0).all()      # (Transport(nx=64): 64 cells)
