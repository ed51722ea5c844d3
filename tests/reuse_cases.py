"""The cases of tests/test_gpu_handle_reuse.py (test infrastructure, no tests of its own): small compat-mode and physical-mode problems,
the calls a handle can be given, and the snapshot of everything a caller can read back.

A pnp_handle keeps much that outlives a call -- the charge-row ping-pong and the step parity, per-lane BDF2 / predictor history, the
lane order, the caller's mask, workspaces that are zeroed when they are allocated and assumed clean afterwards.  The property the tests
check is one sentence: whatever a handle did before, after an upload it computes what a handle that did nothing before computes, to the
bit.  Both runs execute the same kernels on the same rows, so no tolerance is involved."""
import numpy as np

from catint_amd import _capi
from catint_amd.host import solver_from_problem
from catint_amd.synthetic import make_batch
from tests.test_gpu_lane_mask import FAMILIES, Case
from tests.test_gpu_newton import BETA, EPS

# ---- compat mode ------------------------------------------------------------------------------------------------------------------------
# method -> (N, nx, B, capacity, dt in units of the explicit limit dx^2 / (2 D_max)).  nx is no multiple of the row pitch (16 doubles):
# rows have pad columns.  B * 10 per-lane reals of the explicit integrators reach past the first row of a state-sized buffer (nx = 66,
# B = 33), capacity > B leaves rows behind the batch.  FTCS must stay below its limit; on the Crank-Nicolson handle the integrators get
# intervals of three times the limit, so that DOPRI5 / DOP853 take several steps per interval and RKC more than two stages.
COMPAT = {
    'FTCS': (2, 66, 33, 40, 0.4),
    'Crank-Nicolson': (3, 130, 5, 6, 3.0),
}
TWO_WAVES = (2, 1030, 3, 6, 3.0)       # two waves per system (grids beyond 1026 points), on a Crank-Nicolson handle


def compat_problem(N, nx, B, ratio, seed):
    """make_batch with the timestep given in units of the explicit stability limit, a perturbed start and wall fluxes"""
    dt_factor = ratio * 40.0 / (2.0 * (nx - 1) ** 2)       # make_batch: dt = dt_factor * debye * L / D_max, dx = 40 debye / (nx - 1)
    p, c0, pb, vz, fl = make_batch(B, N, nx, seed=seed, phi_max=0.02, dt_factor=dt_factor)
    rng = np.random.default_rng(seed + 1)
    c0 = c0 * (1 + 0.05 * rng.uniform(-1, 1, c0.shape))
    fl = rng.uniform(-1e-4, 1e-4, fl.shape)
    return p, np.ascontiguousarray(c0), pb, vz, fl


def compat_solver(p, method, capacity):
    return solver_from_problem(p, method, batch_capacity=capacity)


def rhs_argument(s, seed=7):
    """The argument of the mol_rhs op: positive, not the state"""
    return np.random.default_rng(seed).uniform(0.5, 30.0, (s.B, s.N * s.nx))


ODE_KW = dict(nsteps=10000)
# name -> call on a solver with a batch; returns a tuple of arrays (what the call itself hands back)
OPS = {
    'step1': lambda s: (s.step(3, 1), ())[1],                                   # odd number of steps, one launch each
    'fused': lambda s: (s.step(5, 0), ())[1],                                   # odd number of steps, one launch
    'integrate': lambda s: s.integrate(4, [1, 3]),
    'mol_rhs': lambda s: (s.mol_rhs(rhs_argument(s)),),
    'rkc': lambda s: s.integrate_rkc(2, [0, 1]),
    'dop853': lambda s: s.integrate_dop853(2, [0, 1], **ODE_KW),
    'dopri5': lambda s: s.integrate_dopri5(2, [0, 1], **ODE_KW),
}
# the read-backs and parameter updates of the long chain: they must leave nothing behind either
SIDE_CALLS = {
    'get_state': lambda s: s.get_state(),
    'get_surface': lambda s: s.get_surface(),
    'set_pb': lambda s: s.set_pb(np.nan_to_num(np.tile([0.013, -0.002, 0.0, 0.0], (s.B, 1))), np.full(s.B, 0.013)),
    'set_flux': lambda s: s.set_flux(np.full((s.B, s.N), 3e-5)),
}
LONG_CHAIN = ['step1', 'get_state', 'fused', 'integrate', 'set_flux', 'mol_rhs', 'rkc', 'get_surface', 'dop853', 'dopri5', 'set_pb', 'dop853',
              'scf_cycle', 'get_state', 'step1']


def scf_state(B, N):
    """A well-formed state dictionary of PnpSolver.scf_cycle"""
    st = {k: np.zeros((B, N)) for k in ('surface_concentration', 'surface_concentration_old', 'flux', 'current_density_old')}
    st.update({k: np.zeros(B) for k in ('mix', 'accuracy', 'surface_pH', 'surface_potential', 'surface_efield')})
    st.update({k: np.zeros(B, np.int32) for k in ('step_to_check', 'active', 'failed')})
    return st


def call(s, name):
    if name == 'scf_cycle':      # a compat handle refuses the device SCF loop (physical mode only) -- and the refusal leaves nothing behind
        try:
            s.scf_cycle(scf_state(s.B, s.N), istep=1, max_iter=1, tau_scf=1e-12, faraday=96485.0)
        except _capi.PnpError as e:
            assert e.code == -1 and 'PNP_METHOD_NEWTON' in str(e), e
        else:
            raise AssertionError('pnp_scf_cycle accepted a compat handle')
        return ()
    if name in SIDE_CALLS:
        SIDE_CALLS[name](s)
        return ()
    return tuple(OPS[name](s))


def snapshot(s):
    """Everything a caller can read back from a handle: state, derived potential rows, surface values, status (and, physical mode, the
    Newton iteration counts)"""
    out = tuple(s.get_state()) + tuple(s.get_surface()) + (s.get_status(),)
    if s.method == 'Newton':
        out = out + (s.newton_iterations(),)
    return out


def differing(a, b):
    """Indices of the arrays of two results that are not equal to the bit (NaN equals NaN: a poisoned lane is compared too)"""
    assert len(a) == len(b), (len(a), len(b))
    return [i for i, (x, y) in enumerate(zip(a, b))
            if np.shape(x) != np.shape(y) or not np.array_equal(np.asarray(x), np.asarray(y), equal_nan=np.asarray(x).dtype.kind == 'f')]


# ---- physical mode ----------------------------------------------------------------------------------------------------------------------
# the families NEWTON_KERNEL can force, at the shapes tests/test_gpu_lane_mask.py drives them with ('lane': 70 operating points, so that
# the lane kernels deal them to their slots by the previous call's iteration counts)
NEWTON_FAMILIES = {k: FAMILIES[k] for k in ('generic', 'team', 'sweep', 'lane', 'lane2', 'lane4')}


class NewtonCase(Case):
    """tests/test_gpu_lane_mask.py's Case with a handle capacity of its own, a second batch of the same problem (other bulk
    concentrations and electrode potentials) and handles that start without a batch."""

    def __init__(self, family, seed, kw=None, B=None, capacity=None, nx=None):
        N, nx0, B0, options = NEWTON_FAMILIES[family]
        Case.__init__(self, N, nx0 if nx is None else nx, B0 if B is None else B, seed, options, kw or {})
        self.family = family
        self.capacity = self.B if capacity is None else capacity

    def other(self, B=None, seed=1000):
        """Another batch for the same handle: same species, grid and timestep"""
        o = NewtonCase(self.family, seed, self.kw, B=self.B if B is None else B, capacity=self.capacity, nx=self.nx)
        assert o.dx == self.dx and np.array_equal(o.D, self.D)
        o.dt = self.dt
        return o

    def handle(self, kw=None):
        s = _capi.PnpSolver(self.N, self.nx, self.dx, self.dt, BETA, EPS, self.D, self.q, method='Newton', batch_capacity=self.capacity)
        s.set_option('NEWTON_KERNEL', '')
        for k, v in self.options.items():
            s.set_option(k, v)
        s.set_newton(**(self.kw if kw is None else kw))
        return s

    def upload(self, s, c=None, phi=None, lanes=None):
        """set_batch of this case's operating points (lanes: a subset / permutation) with the state c (None: the bulk state) and, when
        given, the potential rows phi"""
        idx = np.arange(self.B) if lanes is None else np.asarray(lanes)
        s.set_batch(self.c0[idx] if c is None else c, self.pb[idx], np.zeros(len(idx)), np.zeros((len(idx), self.N)))
        if phi is not None:
            s.set_potential(phi)

