"""GPU: the cooperative epilogue of step_kernel<P, W, G>'s fast body, on the shapes that decide who owns which chunk of a row.

Behind the species section every thread of the workgroup reads its 16-byte chunks of the staged rows back from LDS, stores them, folds
them into the next charge row and, on a launch's last step, takes the status from them (catint_amd/csrc/pnp_kernels.hip, section 3).
Which thread owns which chunk follows from W, from the pitch and from the number of staged rows in use; a change to that epilogue -- who
reads, when the stores go out, where the status is taken -- has to leave every bit where it is.  profiles/step_epilogue_bench.md holds
the measurements of one such change (the epilogue split into a critical and a deferred half); this file is what it was checked with,
and it checks the `bound_ctrl` wave shifts of tridiag_wave<P, G, DPP1> (catint_amd/csrc/pnp_wave.h) on these shapes:
  1. the fast body equals the general body (CATINT_PNP_STEP_GENERIC=1) bit for bit in c, phi, grad, lapl and the status;
  2. the bytes are those of the commit before the `bound_ctrl` shifts: SHA-256 digests recorded from that commit on an MI355X
     (tests/golden/step_epilogue_parent.json, written by tools/probe/step_epilogue_digests.py), fast and general;
  3. a lane that holds a negative value reports PNP_STATUS_NEGATIVE from the fast body as from the general one, wherever in the row
     -- and so in whichever thread's chunk -- the value sits.

Shapes (W, G, N, nx) the golden file of tests/test_gpu_step_poisson.py does not hold:
  (4,1,3,259)   a wave without a species that still owns chunks
  (4,1,4,131)   P = 4: a third of the threads that own chunks have a row position
  (4,1,4,1026)  P = 16, 58.9 KB of LDS
  (3,1,2,512)   N < W G on the headline instance
  (3,1,3,514)   ldx = 528: a partial third chunk if two of the three waves owned every chunk
  (2,1,2,67)    P = 2, W = 2
  (2,2,3,514)   two species per wave, a short last group
  (1,2,2,259)   a single wave
Launches: (1,) is a last step only, (2,), (7,) and (3, 3) as in tests/test_gpu_step_fast.py.
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import c_oracle as CO
from tests import test_gpu_step_fast as F
from tests.test_gpu_step_fast import B, LDS_BYTES, STATUS_NEGATIVE, assert_identical, inputs, points_per_lane, run, step_lds_bytes

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'step_epilogue_parent.json')
# (W, G, N, nx)
SHAPES = [(4, 1, 3, 259), (4, 1, 4, 131), (4, 1, 4, 1026), (3, 1, 2, 512), (3, 1, 3, 514), (2, 1, 2, 67), (2, 2, 3, 514), (1, 2, 2, 259)]
LAUNCHES = [(1,), (2,), (7,), (3, 3)]
NAMES = ('c', 'phi', 'grad', 'lapl', 'status')


def shapes():
    """Every shape of SHAPES fits the 64 KB of LDS a launch gets (the largest, <16, 4, 1> at nx = 1026, takes 58 944 bytes): none is dropped."""
    return [s for s in SHAPES if step_lds_bytes(points_per_lane(s[3]), s[0], s[1]) <= LDS_BYTES]


def key(W, G, N, nx, launches, generic):
    return 'W%d G%d N%d nx%d steps%s %s' % (W, G, N, nx, '+'.join(str(n) for n in launches), 'general' if generic else 'default')


def digests(result):
    state, status = result
    arrays = [np.ascontiguousarray(a) for a in state] + [np.ascontiguousarray(status)]
    return {name: hashlib.sha256(a.tobytes()).hexdigest() for name, a in zip(NAMES, arrays)}


_RESULTS = {}


def result(monkeypatch, W, G, N, nx, launches, generic):
    """run() of tests/test_gpu_step_fast.py, once per case for the whole module; the arrays are never written to."""
    k = (W, G, N, nx, launches, generic)
    if k not in _RESULTS:
        _RESULTS[k] = run(monkeypatch, W, G, N, nx, launches, generic=generic)
    return _RESULTS[k]


def all_digests(monkeypatch):
    """{key: {array name: digest}} of every case; tools/probe/step_epilogue_digests.py writes this as the golden file."""
    return {key(W, G, N, nx, launches, generic): digests(result(monkeypatch, W, G, N, nx, launches, generic))
            for (W, G, N, nx) in shapes() for launches in LAUNCHES for generic in (False, True)}


def test_every_shape_fits_the_lds():
    assert shapes() == SHAPES


@pytest.mark.parametrize('W,G,N,nx', SHAPES)
def test_fast_body_equals_general_body_bit_for_bit(W, G, N, nx, monkeypatch):
    for launches in LAUNCHES:
        general = result(monkeypatch, W, G, N, nx, launches, True)
        assert np.all(general[1] == 0), (launches, general[1])
        assert_identical(result(monkeypatch, W, G, N, nx, launches, False), general, launches)


@pytest.mark.parametrize('W,G,N,nx', SHAPES)
def test_bytes_are_those_of_the_parent_commit(W, G, N, nx, monkeypatch):
    with open(GOLDEN) as f:
        golden = json.load(f)
    for launches in LAUNCHES:
        for generic in (False, True):
            k = key(W, G, N, nx, launches, generic)
            got = digests(result(monkeypatch, W, G, N, nx, launches, generic))
            assert got == golden[k], (k, [n for n in NAMES if got[n] != golden[k][n]])


# ---- status: one negative value, wherever in the row it sits ---------------------------------------------------------------------
# The value is planted in the slowest species of one lane, at a point next to the wall, in the middle of the row and next to the bulk:
# at W = 3, nx = 512 these are chunks of thread 1 (wave 0), thread 128 (wave 2) and thread 63's second chunk (wave 0); at W = 4,
# nx = 259 of threads 1, 64 and 128 (waves 0, 1, 2).  Crank-Nicolson spreads a spike of -1 over its neighbours within a step or
# two (at nx = 512 the batch runs at D dt / dx^2 up to 0.5), and at grid point 1 the Robin wall condition copies the sign into the wall value,
# so that neither keeps "one negative value" for three steps.  What does, by the C oracle
# (test_oracle_keeps_the_value_negative_and_the_rest_positive): grid point 2 instead of 1, and the point's own value times
# -2.5 (next to the bulk, whose Dirichlet value pulls harder: -3.5).
NEG_LANE, NEG_SPECIES = 2, 2
NEG_SHAPES = [(3, 1, 3, 512), (4, 1, 3, 259)]
NEG_STEPS = (1, 3)


def neg_points(nx):
    """(grid point, factor): the planted value is -factor times the value it replaces."""
    return ((2, 2.5), (nx // 2, 2.5), (nx - 2, 3.5))


@functools.lru_cache(maxsize=None)
def negative_inputs(N, nx, point, factor):
    """inputs(N, nx) with the value at `point` of species NEG_SPECIES of lane NEG_LANE times -factor; computed once and never written to."""
    p, c0, pb, vz, fl = inputs(N, nx)
    c = c0.reshape(B, N, nx).copy()
    c[NEG_LANE, NEG_SPECIES, point] *= -factor
    c = np.ascontiguousarray(c.reshape(c0.shape))
    c.setflags(write=False)
    return p, c, pb, vz, fl


@functools.lru_cache(maxsize=None)
def oracle_rows(N, nx, point, factor, nsteps):
    """Lane NEG_LANE of negative_inputs after nsteps steps of the C oracle, [N][nx]."""
    p, c0, pb, vz, fl = negative_inputs(N, nx, point, factor)
    sub = [NEG_LANE]
    oc = np.ascontiguousarray(c0.reshape(B, N, nx)[sub].copy())
    CO.steps(p, 'Crank-Nicolson', oc, pb[sub], vz[sub], fl[sub], nsteps, want_potential=False)
    return oc[0]


@pytest.mark.parametrize('N,nx', sorted({(s[2], s[3]) for s in NEG_SHAPES}))
def test_oracle_keeps_the_value_negative_and_the_rest_positive(N, nx):
    """No GPU work: the inputs of the status test do what it relies on -- after the steps the planted value is still the one negative value."""
    for point, factor in neg_points(nx):
        for nsteps in NEG_STEPS:
            rows = oracle_rows(N, nx, point, factor, nsteps)
            assert rows[NEG_SPECIES, point] < 0.0, (point, nsteps, rows[NEG_SPECIES, point])
            rest = np.delete(rows.reshape(-1), NEG_SPECIES * nx + point)
            assert np.all(rest > 0.0), (point, nsteps, float(rest.min()))


@pytest.mark.parametrize('W,G,N,nx', NEG_SHAPES)
def test_status_of_a_negative_value_anywhere_in_the_row(W, G, N, nx, monkeypatch):
    for point, factor in neg_points(nx):
        monkeypatch.setattr(F, 'inputs', lambda N_, nx_, method='CN', pb_name='dd', at=(point, factor): negative_inputs(N_, nx_, *at))
        for nsteps in NEG_STEPS:
            general = run(monkeypatch, W, G, N, nx, (nsteps,), generic=True)
            assert general[1][NEG_LANE] == STATUS_NEGATIVE and np.all(np.delete(general[1], NEG_LANE) == 0), (point, nsteps, general[1])
            fast = run(monkeypatch, W, G, N, nx, (nsteps,), generic=False)
            assert np.array_equal(fast[1], general[1]), (point, nsteps, fast[1], general[1])
            assert_identical(fast, general, (point, nsteps))
