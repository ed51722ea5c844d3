"""One context of every satellite library across calls whose device buffer has to grow (the method of tests/test_gpu_handle_reuse.py,
which covers the solver handle only).

A context keeps one device buffer that only grows: a call that needs more frees it and allocates a larger one, and every address the
kernel is given has to be formed after that.  Each test makes three calls on one context -- 3 operating points, then 70 (more than one
wavefront of the one-point-per-lane kernels, more than one group of every team width, and more outputs, frequencies, parameters or
output times than the first call asked for), then the 3 again -- and each result must equal, to the bit and including the status and
iteration rows, what a context that did nothing before returns for the same call.  Both runs execute the same kernel on the same
inputs, so no tolerance is involved.

The electrolyte is tests/response_cases.py: small(2, nx, stern=True) (N = 2, block size 3) at nx = 33, the smallest single-wave grid
whose interior does not fill the wave, and nx = 66, where the last thread stores the bulk point; the states are the device's own from
the bulk state.  The surface mechanism is tests/eis_cases.py: chain_tables(2); its coverages and the kinetic inputs of the coupling
come from one solve of libcatint_kinetics per batch, shared by the tests and left unchanged."""
import numpy as np
import pytest

from catint_amd import (_balance, _couple, _drc, _eis, _equil, _kinetics, _kintrans, _modes, _observe, _regrid, _response,  # noqa: F401
                        _sens)          # fails without the features
from tests import eis_cases as EC
from tests import response_cases as RC
from tests.reuse_cases import differing
from tests.test_gpu_couple import load, open_solver

pytestmark = pytest.mark.gpu

SMALL, LARGE = 3, 70
GRIDS = (33, 66)
_cache = {}


class Batch(object):
    """A solver that holds n converged operating points, and what the calls on its view share"""

    def __init__(self, case, n):
        self.case, self.n = case, n
        self.phis = case.phiM * np.linspace(1.0, 0.05, n)
        self.s = open_solver(case, n)
        load(self.s, case, self.phis, [case.bulk_state()] * n)
        status = self.s.solve_stationary()
        assert (status == 0).all(), (case.name, n, status)
        self.view = self.s.device_view()
        self.o = self.s._obs
        self.lanes = np.arange(n, dtype=np.int64)
        self.flux = np.zeros((n, case.N))
        self.tables = EC.chain_tables(case.N)
        with _kinetics.KineticsSolver(0) as k:
            self.kin = k.solve(self.view, self.tables, self.phis, lanes=self.lanes, fields=('theta', 'flux', 'dflux_dc', 'dflux_dphi'),
                               **self.surface())
        assert (self.kin['status'] == 0).all(), self.kin['status']

    def surface(self):
        return dict(stern_capacitance=self.o['stern_capacitance'], phi_pzc=self.o['phi_pzc'])

    def medium(self, *names):
        """D, charges, x, beta, eps, dx in the order of `names`"""
        return [self.o[k] for k in names]

    def wall(self):
        return dict(mpb_radius=self.o['mpb_radius'], wall_bc=self.o['wall_bc'], stern_capacitance=self.o['stern_capacitance'])


def batches(nx):
    """(the small batch, the large batch) on a grid of nx points, solved once per session"""
    if nx not in _cache:
        case = RC.small(2, nx, stern=True)
        _cache[nx] = (Batch(case, SMALL), Batch(case, LARGE))
    return _cache[nx]


@pytest.fixture(scope='module', autouse=True)
def close_all():
    yield
    for pair in _cache.values():
        for b in pair:
            b.s.close()
    _cache.clear()


def omegas(b, big):
    return b.case.omegas()[:3] if big else (0.0,)


# library -> (context class, call(ctx, batch, big) -> dict of arrays).  big: the call that grows the buffer asks for more of everything
def observe(ctx, b, big):
    fields = [f for f in _observe.FIELDS if f != 'pH'] if big else ['charge_density']
    return ctx.electrolyte(b.view, *b.medium('D', 'charges', 'x', 'beta'), mpb_radius=b.o['mpb_radius'], fields=fields, scalars=big)


def balance(ctx, b, big):
    return ctx.species(b.view, *b.medium('D', 'charges', 'x', 'beta'), b.flux, b.phis, mpb_radius=b.o['mpb_radius'],
                       fields=None if big else ['flux'], scalars=big)


def regrid(ctx, b, big):
    x = b.o['x']
    return ctx.resample(b.view, *b.medium('D', 'charges', 'x', 'beta'), np.linspace(x[0], x[-1], 41 if big else 17), mpb_radius=b.o['mpb_radius'])


def equil(ctx, b, big):
    return ctx.solve(b.view, *b.medium('charges', 'x', 'beta', 'eps', 'dx'), b.phis, 0.0, b.case.cb, **b.wall())


def response(ctx, b, big):
    return ctx.solve(b.view, *b.medium('D', 'charges', 'x', 'beta', 'eps', 'dx'), b.phis, omega=omegas(b, big), lanes=b.lanes,
                     fields=None if big else ['admittance'], profiles=big, **b.wall())


def kinetics(ctx, b, big):
    return ctx.solve(b.view, b.tables, b.phis, lanes=b.lanes, fields=list(_kinetics.FIELDS) if big else ['theta'], **b.surface())


def drc(ctx, b, big):
    return ctx.solve(b.view, b.tables, b.phis, b.kin['theta'], lanes=b.lanes, fields=list(_drc.FIELDS) if big else ['drc'], **b.surface())


def kintrans(ctx, b, big):
    return ctx.solve(b.view, b.tables, b.phis, (1e-9, 1e-7, 1e-5) if big else (1e-9,), lanes=b.lanes, theta0=b.kin['theta'],
                     fields=None if big else ['theta'], **b.surface())


def couple(ctx, b, big):
    kphi = np.ascontiguousarray(b.kin['dflux_dphi'][:, :, 1])
    return ctx.solve(b.view, *b.medium('D', 'charges', 'x', 'beta', 'eps', 'dx'), b.flux, b.kin['flux'], b.kin['dflux_dc'], kphi, lanes=b.lanes,
                     fields=None if big else ['dflux'], **b.wall())


def sens(ctx, b, big):
    parameters = ['phiM', ('flux', 0), ('D', 1), 'stern_capacitance'] if big else ['phiM']
    return ctx.solve(b.view, *b.medium('D', 'charges', 'x', 'beta', 'eps', 'dx'), b.phis, b.flux, parameters, lanes=b.lanes,
                     fields=None if big else ['dsigma'], **b.wall())


def modes(ctx, b, big):
    m = 4 if big else 2
    return ctx.solve(b.view, *b.medium('D', 'charges', 'x', 'beta', 'eps', 'dx'), b.phis, _modes.default_start(m, b.case.N, b.case.nx),
                     iterations=3, lanes=b.lanes, fields=list(_modes.FIELDS) if big else ['ritz'], **b.wall())


def eis_kinetic(ctx, b, big, F=None):
    om = omegas(b, big) if F is None else omegas(b, True)[:F]
    return ctx.kinetic(b.view, b.tables, b.phis, b.kin['theta'], om, lanes=b.lanes, fields=['Kc', 'Kphi', 'dy', 'residual'] if big else ['Kc'],
                       **b.surface())


def eis_solve(ctx, b, big, F=None):
    om = omegas(b, big) if F is None else omegas(b, True)[:F]
    return ctx.solve(b.view, b.tables, b.phis, b.kin['theta'], om, *b.medium('D', 'charges', 'x', 'beta', 'eps', 'dx'), rf=1.0, lanes=b.lanes,
                     mpb_radius=b.o['mpb_radius'], wall_bc=b.o['wall_bc'], stern_capacitance=b.o['stern_capacitance'], phi_pzc=b.o['phi_pzc'],
                     fields=list(_eis.FIELDS) if big else ['admittance'])


LIBRARIES = {
    'observe': (_observe.Observer, observe), 'balance': (_balance.Balancer, balance), 'regrid': (_regrid.Regridder, regrid),
    'equil': (_equil.Equilibrator, equil), 'response': (_response.Responder, response), 'kinetics': (_kinetics.KineticsSolver, kinetics),
    'couple': (_couple.Coupler, couple), 'sens': (_sens.Sensitizer, sens), 'drc': (_drc.RateControl, drc), 'modes': (_modes.ModeSolver, modes),
    'kintrans': (_kintrans.TransientKinetics, kintrans), 'eis_kinetic': (_eis.Impedance, eis_kinetic), 'eis_solve': (_eis.Impedance, eis_solve),
}


def rows(res):
    """the arrays of a result in the order of their names"""
    return [res[k] for k in sorted(res)]


def regrow(handle, call, nx):
    """small, large, small on one context against each on a context of its own"""
    small, large = batches(nx)
    fresh = []
    for b, big in ((small, False), (large, True)):
        with handle(0) as ctx:
            fresh.append(call(ctx, b, big))
    for res in fresh:          # rows of NaN alone would compare equal whatever the kernel was given
        assert all(np.isfinite(a).any() for a in rows(res) if a.dtype.kind in 'fc' and a.size), sorted(res)
    with handle(0) as ctx:
        for step, (b, big, want) in enumerate(((small, False, fresh[0]), (large, True, fresh[1]), (small, False, fresh[0]))):
            got = call(ctx, b, big)
            assert sorted(got) == sorted(want)
            bad = differing(rows(got), rows(want))
            assert not bad, (step, [sorted(want)[i] for i in bad])


@pytest.mark.parametrize('nx', GRIDS)
@pytest.mark.parametrize('name', sorted(LIBRARIES))
def test_a_context_that_grew_computes_what_a_fresh_one_computes(name, nx):
    handle, call = LIBRARIES[name]
    regrow(handle, call, nx)


@pytest.mark.parametrize('name', ['eis_kinetic', 'eis_solve'])
def test_the_turn_loop_of_a_context_that_grew(name, monkeypatch):
    """the grow step in two turns: one frequency, 70 pairs, 64 pairs per turn"""
    handle, call = LIBRARIES[name]
    monkeypatch.setenv('CATEIS_WORKSPACE_BYTES', '1')
    regrow(handle, lambda ctx, b, big: call(ctx, b, big, F=1), 33)
