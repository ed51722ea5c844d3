"""GPU: the instructions taken out of step_kernel<P, W, G>'s fused Crank-Nicolson step leave every bit where it was.

catint_amd/csrc/pnp_kernels.hip forms the stencil coefficients of a point once (hsr + e4r grad_v and hsr - e4r grad_v; the matrix's
off-diagonals are their negatives), takes the lane status behind the time loop from the rows staged in LDS and reads a chunk of the
staged rows together, ahead of its stores.  A division by the launch constant nx - 1 through a reciprocal formed once per launch,
bit-identical while the numerator's exponent lies in a window, was built and measured too; it is not in the kernel
(profiles/step_diet_bench.md holds the measurements), its cases stay: whatever divides there next has to pass them.  Checked here, on
the shapes at which each of these can go wrong:
  1. every position of the last real row within its lane -- (nx - 3) % P takes every value for P = 2, 4, 8 and 16: the fast body
     equals the general body (CATINT_PNP_STEP_GENERIC=1) byte for byte, and both reproduce the SHA-256 digests recorded from the commit
     before the change on an MI355X (tests/golden/step_diet_parent.json, written by tools/probe/step_diet_digests.py);
  2. the status evaluated behind the loop: a lane driven negative and a lane that starts with a NaN, launches of one and of seven steps;
  3. the division: a numerator of exactly zero, a tiny one (1e-300), and two huge ones (1e+250, 1e+190) -- below, above and in the upper
     end of the exponent range in which the hardware's division step leaves its operands unscaled for 2 <= nx - 1 <= 4097:
     fast equals general byte for byte, both equal the C oracle to 1e-9.
Bytes are compared (tobytes), not values, so that a flipped sign of a zero shows.  One thing is not part of the bytes: the sign and the
payload of a NaN.  IEEE 754 leaves them to the implementation, the fast and the general body of the commit before the change already
differ in them (the lane that starts with a NaN: sign bits), and a negated operand moves them; every NaN is compared as the one
canonical quiet NaN, so what is pinned is where the NaNs are.
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from catint_amd.synthetic import make_batch
from oracle import c_oracle as CO
from tests import test_gpu_step_fast as F
from tests.test_gpu_step_fast import B, LDS_BYTES, STATUS_NEGATIVE, inputs, points_per_lane, run, step_lds_bytes

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'step_diet_parent.json')
STATUS_NAN = 2               # PNP_STATUS_NAN (include/catint_pnp.h)
NAMES = ('c', 'phi', 'grad', 'lapl', 'status')
LAUNCHES = [(1,), (3,)]
# nx by points per lane: 129, 130 (P = 2), 255 ... 258 (4), 507 ... 514 (8, with the headline's 512), 515 ... 530 (16)
ROW_GRIDS = [129, 130] + list(range(255, 259)) + list(range(507, 515)) + list(range(515, 531))
# (W, G, N, nx)
ROW_SHAPES = [(3, 1, 3, nx) for nx in ROW_GRIDS] + [(W, G, N, nx) for (W, G, N) in ((1, 2, 2), (2, 2, 4)) for nx in range(507, 515)]
STATUS_LAUNCHES = [(1,), (7,)]
NAN_LANE, NAN_SPECIES = 3, 1


def key(case, W, G, N, nx, launches, generic):
    return '%s W%d G%d N%d nx%d steps%s %s' % (case, W, G, N, nx, '+'.join(str(n) for n in launches), 'general' if generic else 'default')


def as_bytes(result):
    state, status = result
    out = []
    for a in state:
        u = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).copy()
        u[np.isnan(a).reshape(u.shape)] = 0x7ff8000000000000      # (see the docstring)
        out.append(u.tobytes())
    return out + [np.ascontiguousarray(status).tobytes()]


def digests(result):
    return {name: hashlib.sha256(b).hexdigest() for name, b in zip(NAMES, as_bytes(result))}


def assert_same_bytes(got, ref, what):
    for name, a, b in zip(NAMES, as_bytes(got), as_bytes(ref)):
        assert a == b, (what, name)


# ---- the cases beside the plain ones: inputs computed once, never written to ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def negative_flux():
    """The wall flux of tests/test_gpu_step_fast.py's negative-lane case: it empties lane 2's wall cells."""
    p, c0, pb, vz, fl = inputs(3, 131)
    flux = fl.copy()
    flux[2] = -3.0 * c0.reshape(B, 3, 131)[2, :, 1] * p.D / p.dx
    flux.setflags(write=False)
    return flux


@functools.lru_cache(maxsize=None)
def nan_inputs(N, nx):
    """inputs(N, nx) with a NaN in the middle of one row of lane NAN_LANE."""
    p, c0, pb, vz, fl = inputs(N, nx)
    c = c0.reshape(B, N, nx).copy()
    c[NAN_LANE, NAN_SPECIES, nx // 2] = np.nan
    c = np.ascontiguousarray(c.reshape(c0.shape))
    c.setflags(write=False)
    return p, c, pb, vz, fl


def status_cases():
    """(case, (W, G, N, nx), expected status)"""
    neg = np.zeros(B, int)
    neg[2] = STATUS_NEGATIVE
    nan = np.zeros(B, int)
    nan[NAN_LANE] = STATUS_NAN
    return [('negative', (3, 1, 3, 131), neg), ('nan', (3, 1, 3, 512), nan)]


def run_status(monkeypatch, case, shape, launches, generic):
    if case == 'nan':
        monkeypatch.setattr(F, 'inputs', lambda N_, nx_, method='CN', pb_name='dd': nan_inputs(N_, nx_))
        return run(monkeypatch, *shape, launches, generic=generic)
    return run(monkeypatch, *shape, launches, generic=generic, flux=negative_flux())


# Division: two species of charge +1 and -1 at equal concentrations, a power of two per lane, so that the products with the charge
# constant are exact and the charge row is exactly zero: the numerator vb - vw - G of the first step is vb - vw itself.  Wall fluxes of
# opposite sign (three tenths of what would empty the wall cell) separate the charges, so that after the step the potential, its
# gradient and its Laplacian are far above rounding and can be compared with the oracle.
DIV_SHAPES = [(3, 1, 2, 512), (1, 2, 2, 131)]
# vb - vw: exactly zero; biased exponent 26, below the range v_div_scale_f64 leaves unscaled for these divisors ([54, 1791]); above it
# (1853); in its upper end (1654)
DIV_DELTA = {'zero': 0.0, 'tiny': 1e-300, 'large': 1e250, 'high': 1e190}


@functools.lru_cache(maxsize=None)
def div_inputs(nx, delta):
    p, c0, pb, vz, fl = make_batch(B, 2, nx, seed=nx, phi_max=0.02, dt_factor=min(1e-4, 0.5 * 40.0 / (nx - 1) ** 2))
    assert list(p.charges / abs(p.charges[0])) == [1.0, -1.0]
    conc = 2.0 ** np.arange(-2, B - 2)
    c = np.ascontiguousarray(np.broadcast_to(conc[:, None, None], (B, 2, nx)).reshape(B, 2 * nx))
    pb = np.full((B, 4), np.nan)
    # (a wall potential of zero where the difference has to survive the subtraction; one per lane where it is zero)
    pb[:, 0] = np.linspace(-0.02, 0.02, B) if delta == 0.0 else 0.0
    pb[:, 1] = pb[:, 0] + delta
    vz = pb[:, 0].copy()
    fl = 0.3 * conc[:, None] * p.D[None, :] / p.dx * np.array([1.0, -1.0])
    p.pb = pb[0].copy()
    if delta > 1.0:
        # the timestep shrinks as the potential grows, so that the migration number e4r grad_v stays what it is at 20 mV and the
        # step stays the well-conditioned problem on which an rtol of 1e-9 against the oracle means something
        p.dt *= 0.02 / delta
    for a in (c, pb, vz, fl):
        a.setflags(write=False)
    return p, c, pb, vz, fl


@functools.lru_cache(maxsize=None)
def div_oracle(nx, delta, nsteps):
    """(c, phi, grad, lapl) of the C oracle after nsteps steps."""
    p, c0, pb, vz, fl = div_inputs(nx, delta)
    oc = np.ascontiguousarray(c0.reshape(B, 2, nx).copy())
    with np.errstate(all='ignore'):
        ov, og, ol = CO.steps(p, 'Crank-Nicolson', oc, pb, vz, fl, nsteps)
    return oc.reshape(B, 2 * nx), ov, og, ol


def run_div(monkeypatch, shape, delta, launches, generic):
    monkeypatch.setattr(F, 'inputs', lambda N_, nx_, method='CN', pb_name='dd': div_inputs(nx_, delta))
    return run(monkeypatch, *shape, launches, generic=generic)


def all_digests(monkeypatch):
    """{key: {array name: digest}} of every case compared with the golden file; tools/probe/step_diet_digests.py writes this."""
    out = {}
    for shape in ROW_SHAPES:
        for launches in LAUNCHES:
            for generic in (False, True):
                out[key('row', *shape, launches, generic)] = digests(run(monkeypatch, *shape, launches, generic=generic))
    for case, shape, _ in status_cases():
        for launches in STATUS_LAUNCHES:
            for generic in (False, True):
                with pytest.MonkeyPatch.context() as mp:
                    out[key(case, *shape, launches, generic)] = digests(run_status(mp, case, shape, launches, generic))
    return out


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_shape_fits_the_lds():
    for (W, G, N, nx) in ROW_SHAPES + DIV_SHAPES:
        assert step_lds_bytes(points_per_lane(nx), W, G) <= LDS_BYTES, (W, G, N, nx)
    for P, grids in ((2, (129, 130)), (4, range(255, 259)), (8, range(507, 515)), (16, range(515, 531))):
        assert all(points_per_lane(nx) == P for nx in grids)
        assert {(nx - 3) % P for nx in grids} == set(range(P))


@pytest.mark.parametrize('W,G,N,nx', ROW_SHAPES)
def test_last_real_row_anywhere_in_its_lane(W, G, N, nx, monkeypatch):
    for launches in LAUNCHES:
        fast = run(monkeypatch, W, G, N, nx, launches, generic=False)
        general = run(monkeypatch, W, G, N, nx, launches, generic=True)
        assert np.all(general[1] == 0), (launches, general[1])
        assert_same_bytes(fast, general, launches)
        for generic, got in ((False, fast), (True, general)):
            k = key('row', W, G, N, nx, launches, generic)
            d = digests(got)
            assert d == golden()[k], (k, [n for n in NAMES if d[n] != golden()[k][n]])


@pytest.mark.parametrize('case,shape,expected', status_cases(), ids=[c[0] for c in status_cases()])
def test_status_taken_behind_the_time_loop(case, shape, expected, monkeypatch):
    for launches in STATUS_LAUNCHES:
        general = run_status(monkeypatch, case, shape, launches, True)
        assert np.array_equal(general[1], expected), (launches, general[1])
        fast = run_status(monkeypatch, case, shape, launches, False)
        assert np.array_equal(fast[1], expected), (launches, fast[1])
        assert_same_bytes(fast, general, (case, launches))
        for generic, got in ((False, fast), (True, general)):
            k = key(case, *shape, launches, generic)
            d = digests(got)
            assert d == golden()[k], (k, [n for n in NAMES if d[n] != golden()[k][n]])


def test_oracle_stays_finite_at_the_large_differences():
    """No GPU work: one step at vb - vw = 1e+250 (and 1e+190) leaves the oracle's state finite, so the issue's value is the one tested."""
    for nx in sorted({s[3] for s in DIV_SHAPES}):
        for which in ('large', 'high'):
            assert all(np.isfinite(a).all() for a in div_oracle(nx, DIV_DELTA[which], 1)), (nx, which)


@pytest.mark.parametrize('W,G,N,nx', DIV_SHAPES)
@pytest.mark.parametrize('which', list(DIV_DELTA))
def test_division_by_the_number_of_intervals(which, W, G, N, nx, monkeypatch):
    delta = DIV_DELTA[which]
    for launches in ((1,), (3,)) if delta < 1.0 else ((1,),):
        fast = run_div(monkeypatch, (W, G, N, nx), delta, launches, False)
        general = run_div(monkeypatch, (W, G, N, nx), delta, launches, True)
        assert_same_bytes(fast, general, (which, launches))
        ref = div_oracle(nx, delta, sum(launches))
        dx = div_inputs(nx, delta)[0].dx
        phi_max = float(np.abs(ref[1][np.isfinite(ref[1])]).max())
        # The error is taken relative to the largest entry of the oracle's array, as in tests/test_gpu_step_fast.py.  The gradient and
        # the Laplacian are first and second differences of the potential, so fp64 gives them no better than eps max|phi| / dx and
        # eps max|phi| / dx^2: where the true array is zero (vw = vb, first step) the oracle's own entries are that rounding, and the
        # scale is the one the differences were formed at.
        floor = {'c': 0.0, 'phi': 0.0, 'grad': phi_max / dx, 'lapl': phi_max / dx ** 2}
        for name, a, b in zip(NAMES, fast[0], ref):
            a = np.asarray(a).reshape(np.shape(b))
            ok = np.isfinite(a) & np.isfinite(b)
            with np.errstate(all='ignore'):
                scale = max(np.abs(b[ok]).max(), floor[name], 1e-300) if ok.any() else 1.0
                err = (np.abs(a[ok] / scale - b[ok] / scale)).max() if ok.any() else 0.0
            print(which, launches, name, 'finite %d of %d' % (ok.sum(), ok.size), 'err', err)
            assert err < 1e-9, (which, launches, name, err)
