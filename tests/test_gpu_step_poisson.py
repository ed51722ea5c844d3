"""GPU: the Poisson section of step_kernel<P, W, G> after its register branch lost the work the result does not need.

The Dirichlet/Dirichlet register branch of poisson_wave (catint_amd/csrc/pnp_kernels.hip) now reads the four end values h at grid points
1, 2, m-1 and m straight from the charge row in LDS and blanks the bulk slot of that row once per step instead of selecting in every lane.
The change is meant to move values along other paths and to leave every bit where it was, so:
  1. the bytes of c, phi, grad, lapl and the status are those of the commit before the change: SHA-256 digests recorded from that
     commit on an MI355X (tests/golden/step_poisson_parent.json, written by tools/probe/step_poisson_digests.py), with the fast body
     and with CATINT_PNP_STEP_GENERIC=1;
  2. the fast body equals the general body bit for bit on the grids this file adds;
  3. the fast body matches the C oracle, which catches an error made identically in both bodies.

Grids: to those of tests/test_gpu_step_fast.py (m mod P in {0, 1, 6}) this file adds 132, 133, 261, 513, 514 and 1026, which put m mod P
at 2, 3, 3, 7, 0 and 0 of P = 4, 4, 8, 8, 8 and 16: grid points m and m-1 then fall into one lane, into two neighbouring lanes, or on either
side of a pad slot of the LDS row.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import c_oracle as CO
from tests.test_gpu_step_fast import B, LDS_BYTES, assert_identical, inputs, points_per_lane, run, step_lds_bytes

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'step_poisson_parent.json')
# (W, G, N, nx)
SHAPES = [(3, 1, 3, 512), (3, 1, 3, 131), (1, 2, 2, 131), (1, 3, 3, 132), (2, 2, 4, 133), (3, 1, 3, 261), (3, 1, 3, 513), (3, 1, 3, 514),
          (3, 1, 3, 1026)]
LAUNCHES = [(1,), (7,), (3, 3)]
NAMES = ('c', 'phi', 'grad', 'lapl', 'status')


def shapes():
    """Every shape of SHAPES fits the 64 KB of LDS a launch gets (the largest, <16, 3, 1> at nx = 1026, takes 49 120 bytes): none is dropped."""
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
    """{key: {array name: digest}} of every case; tools/probe/step_poisson_digests.py writes this as the golden file."""
    return {key(W, G, N, nx, launches, generic): digests(result(monkeypatch, W, G, N, nx, launches, generic))
            for (W, G, N, nx) in shapes() for launches in LAUNCHES for generic in (False, True)}


def test_every_shape_fits_the_lds():
    assert shapes() == SHAPES


@pytest.mark.parametrize('W,G,N,nx', shapes())
def test_bytes_are_those_of_the_parent_commit(W, G, N, nx, monkeypatch):
    with open(GOLDEN) as f:
        golden = json.load(f)
    for launches in LAUNCHES:
        for generic in (False, True):
            k = key(W, G, N, nx, launches, generic)
            got = digests(result(monkeypatch, W, G, N, nx, launches, generic))
            assert got == golden[k], (k, [n for n in NAMES if got[n] != golden[k][n]])


@pytest.mark.parametrize('W,G,N,nx', shapes())
def test_fast_body_equals_general_body_bit_for_bit(W, G, N, nx, monkeypatch):
    for launches in LAUNCHES:
        general = result(monkeypatch, W, G, N, nx, launches, True)
        assert np.all(general[1] == 0), (launches, general[1])
        assert_identical(result(monkeypatch, W, G, N, nx, launches, False), general, launches)


@pytest.mark.parametrize('nx', [133, 513])
def test_fast_body_matches_the_c_oracle(nx, monkeypatch):
    """Four fused steps on three lanes: state, potential, gradient and Laplacian to rtol 1e-9 (run_compat_case's bar)."""
    W, G, N = 3, 1, 3
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
