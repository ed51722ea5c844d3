"""GPU: the two bodies of step_kernel<P, W, G> (catint_amd/csrc/pnp_kernels.hip).

A fused Crank-Nicolson launch on the Dirichlet/Dirichlet Poisson branch whose species all stay staged (N <= W G, P >= 2, no rate
terms) runs the kernel's fast body: launch constants read once, rows resident in LDS, three barriers per step.  Every other launch,
and every launch with CATINT_PNP_STEP_GENERIC=1, runs the general body.  The two share their arithmetic statements, so they must
agree BIT FOR BIT: np.array_equal on the four arrays of get_state() and on get_status().

Instances are forced as the census forces them (PNP_KERNEL = 2, PNP_WAVES_PER_GRID, PNP_SPECIES_PER_WAVE); the inputs are
compat_inputs of tests/test_gpu_kernel_census.py on its 'dd' branch: per-lane Poisson boundary values, vzeta and wall fluxes and a
perturbed initial state, so every lane and every species carries constants of its own and a wrongly indexed hoisted constant shows.
"""
import functools

import numpy as np
import pytest

from catint_amd.host import solver_from_problem
from oracle import c_oracle as CO
from tests.kernel_census import compat
from tests.test_gpu_kernel_census import OPTIONS, compat_inputs

pytestmark = pytest.mark.gpu

B = 5
STATUS_NEGATIVE = 3          # PNP_STATUS_NEGATIVE (include/catint_pnp.h)
LDS_BYTES = 64 * 1024        # dynamic LDS a launch gets without asking for more

# (W, G, N): the headline instance; one idle wave; two and three species per wave; a short last group that recomputes species N-1; ...
CONFIGS = [(3, 1, 3), (3, 1, 2), (1, 2, 2), (1, 3, 3), (2, 2, 4), (2, 2, 3), (4, 1, 4), (1, 1, 1)]
# nx (points per lane P): 130 (2, every slot real), 131 (4, ragged: the last real row sits mid-wave), 258 (4, full), 259 (8, ragged),
# 512 (8, the headline's), 515 (16, ragged)
GRIDS = [130, 131, 258, 259, 512, 515]
# launches: first-step path only; resident steps; an odd count (charge-row ping-pong); the state re-entering from device memory
LAUNCHES = [(1,), (2,), (7,), (3, 3)]


def points_per_lane(nx):
    return next(P for P in (1, 2, 4, 8, 16) if nx - 2 <= 64 * P)


def step_lds_bytes(P, W, G):
    """step_lds_bytes of pnp_kernels.hip: (2 + W G) padded rows of rowbuf_doubles<P>() doubles."""
    cap = 128 * (P // 2 + 1)
    need = max(cap + cap // P + 4, 388)
    return (2 + W * G) * ((need + 1) & ~1) * 8


def shapes():
    out = [(W, G, N, nx) for (W, G, N) in CONFIGS for nx in (131, 512)] + [(3, 1, 3, nx) for nx in GRIDS if nx not in (131, 512)]
    return [s for s in out if step_lds_bytes(points_per_lane(s[3]), s[0], s[1]) <= LDS_BYTES]


@functools.lru_cache(maxsize=None)
def inputs(N, nx, method='CN', pb_name='dd'):
    """(problem, c0, pb, vzeta, flux) of B lanes; computed once per shape and never written to."""
    seed = 1000 * nx + N
    p, c0, pb, vz, fl = compat_inputs(compat(max(N, 2), nx, B, method, pb_name, 'fused'), pb_name, seed)
    if N == 1:
        # the synthetic batches start at two species: keep the first one, diluted so that the unbalanced charge leaves the potential
        # at the few millivolts of the neutral batches
        c0 = np.ascontiguousarray(c0.reshape(B, 2, nx)[:, 0, :]) * 1e-3
        fl = np.ascontiguousarray(fl[:, :1]) * 1e-3
        p.D, p.charges, p.flux_bound, p.species = p.D[:1], p.charges[:1], p.flux_bound[:1], p.species[:1]
    for a in (c0, pb, vz, fl):
        a.setflags(write=False)
    return p, c0, pb, vz, fl


def run(monkeypatch, W, G, N, nx, launches, generic, method='CN', pb_name='dd', flux=None):
    """State and status after the launches step(n, 0) of `launches`, on step_kernel<P, W, G> with the option set or unset."""
    for k in OPTIONS + ('PNP_STEP_GENERIC',):
        monkeypatch.delenv('CATINT_' + k, raising=False)
    monkeypatch.setenv('CATINT_PNP_KERNEL', '2')
    monkeypatch.setenv('CATINT_PNP_WAVES_PER_GRID', str(W))
    monkeypatch.setenv('CATINT_PNP_SPECIES_PER_WAVE', str(G))
    if generic:
        monkeypatch.setenv('CATINT_PNP_STEP_GENERIC', '1')
    p, c0, pb, vz, fl = inputs(N, nx, method, pb_name)
    with solver_from_problem(p, {'CN': 'Crank-Nicolson', 'FTCS': 'FTCS'}[method], batch_capacity=B) as s:
        s.set_batch(c0, pb, vz, fl if flux is None else flux)
        for n in launches:
            s.step(n, 0)
        state = s.get_state()
        status = s.get_status()
    return tuple(np.array(a) for a in state), np.array(status)


def assert_identical(got, ref, what):
    (gs, gst), (rs, rst) = got, ref
    for name, a, b in zip(('c', 'phi', 'grad', 'lapl'), gs, rs):
        assert np.array_equal(a, b), (what, name, float(np.abs(a - b).max()))
    assert np.array_equal(gst, rst), (what, gst, rst)


@pytest.mark.parametrize('W,G,N,nx', shapes())
def test_fast_body_equals_general_body_bit_for_bit(W, G, N, nx, monkeypatch):
    fast = {}
    for launches in LAUNCHES:
        fast[launches] = run(monkeypatch, W, G, N, nx, launches, generic=False)
        general = run(monkeypatch, W, G, N, nx, launches, generic=True)
        assert np.all(general[1] == 0), (launches, general[1])
        assert_identical(fast[launches], general, launches)
    # two launches of three steps against one of six: the state written back and read again is the state that stayed in LDS
    assert_identical(fast[(3, 3)], run(monkeypatch, W, G, N, nx, (6,), generic=False), 'step(3) twice against step(6)')


def test_status_of_a_lane_driven_negative(monkeypatch):
    """A wall flux that empties lane 2's wall cells: the general body reports PNP_STATUS_NEGATIVE for that lane, and so must the fast."""
    W, G, N, nx = 3, 1, 3, 131
    p, c0, pb, vz, fl = inputs(N, nx)
    flux = fl.copy()
    flux[2] = -3.0 * c0.reshape(B, N, nx)[2, :, 1] * p.D / p.dx      # c[0] = c[1] + flux dx / D (+ migration) = -2 c[1]
    general = run(monkeypatch, W, G, N, nx, (2,), generic=True, flux=flux)
    assert general[1][2] == STATUS_NEGATIVE and np.all(np.delete(general[1], 2) == 0), general[1]
    assert_identical(run(monkeypatch, W, G, N, nx, (2,), generic=False, flux=flux), general, 'negative lane')


@pytest.mark.parametrize('W,G,N', [(3, 1, 3), (1, 2, 2)])
@pytest.mark.parametrize('nx', [131, 512])
def test_fast_body_matches_the_c_oracle(W, G, N, nx, monkeypatch):
    """Four fused steps on three lanes: state, potential, gradient and Laplacian to rtol 1e-9 (run_compat_case's bar)."""
    p, c0, pb, vz, fl = inputs(N, nx)
    (c, v, g, l), st = run(monkeypatch, W, G, N, nx, (4,), generic=False)
    assert np.all(st == 0), st
    sub = [0, B // 2, B - 1]
    oc = np.ascontiguousarray(c0[sub].reshape(len(sub), N, nx).copy())
    ov, og, ol = CO.steps(p, 'Crank-Nicolson', oc, pb[sub], vz[sub], fl[sub], 4)
    for name, a, b in (('c', c[sub], oc), ('phi', v[sub], ov), ('grad', g[sub], og), ('lapl', l[sub], ol)):
        err = np.abs(np.asarray(a).reshape(np.shape(b)) - b).max() / max(np.abs(b).max(), 1e-300)
        print(name, err)
        assert err < 1e-9, (name, err)


@pytest.mark.parametrize('W,G,N,method,pb_name', [(3, 1, 3, 'FTCS', 'dd'), (3, 1, 3, 'CN', 'vwall_gbulk'), (2, 2, 5, 'CN', 'dd')],
                         ids=['ftcs', 'not-dd', 'multi-round'])
def test_option_makes_no_difference_where_the_fast_body_does_not_apply(W, G, N, method, pb_name, monkeypatch):
    for launches in ((1,), (4,)):
        a = run(monkeypatch, W, G, N, 131, launches, generic=False, method=method, pb_name=pb_name)
        b = run(monkeypatch, W, G, N, 131, launches, generic=True, method=method, pb_name=pb_name)
        assert np.all(a[1] == 0), a[1]
        assert_identical(a, b, (method, pb_name, launches))
