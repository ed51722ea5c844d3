"""GPU: every Newton kernel family's damping clips driven against the oracle (the table of tests/newton_regimes.py).

One parametrised test over the table, with the census's own mechanism (tests/test_gpu_kernel_census.py): the option environment is
cleared, the case's options force its kernel instance, and run_both of tests/test_gpu_newton.py solves the census's batch with the
case's inputs on the device and the compared lanes on the oracle.  Every lane of the batch must end with status 0; the compared lanes
pass assert_close unchanged (2e-9 of the profile scale, 1e-6 per species relative, identical iteration counts), the single-precision
record cases assert_close_f32_records on the whole batch.  The oracle run of the same call fills the branch counters, and the
conditions of tests/test_newton_regimes.py are asserted on them again: a case cannot fall back into the mild regime unnoticed.

Recipes, what was tried and left out, and the oracle's branch counts per family: tests/newton_regimes.py.

Measured on an MI355X (one run, all 63 cases passed, 7 s in all): the worst state error of any case was 5.9e-7 of the bar
(newton_kernel<5, 512, 2>; about 1e-15 of the profile scale), iteration counts equal in every compared lane, the single-precision
record cases included.  No lane of any case was handed back by the lane families' pivot-growth monitor (status 1), so no case had to
move to a milder recipe for it.

That the cases bite was checked once with a scratch build of the library (not committed) in which theta of the free-volume backtrack is
negated in all nine copies: all 63 cases fail, on the status of the batch or the iteration counts of the compared lanes.  The same
change in a scratch copy of the oracle, compared with the unchanged oracle through assert_close, fails all 63 as well and nothing in
the census's regime, where the backtrack never fires.
"""
import numpy as np
import pytest

from tests import newton_regimes as NR
from tests.kernel_census import CENSUS
from tests.newton_regimes import REGIMES
from tests.test_gpu_kernel_census import OPTIONS, assert_close_f32_records
from tests.test_gpu_newton import assert_close, run_both

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('key', sorted(REGIMES))
def test_driven_case_matches_the_oracle(key, monkeypatch):
    r = REGIMES[key]
    case = CENSUS[r.instance]
    for k in OPTIONS:
        monkeypatch.delenv('CATINT_' + k, raising=False)
    monkeypatch.setenv('CATINT_NEWTON_KERNEL', case.kernel)
    for k, v in case.env:
        monkeypatch.setenv('CATINT_' + k, str(v))
    lanes = NR.compared_lanes(key)
    branches = []
    (c, phi, its, st), ref = run_both(lanes=lanes, branches=branches, **NR.regime_args(key))
    NR.conditions(key, branches, ref[2])                  # the case is still in the driven regime
    rc, rphi, rit = ref
    ratio = max(np.abs(c[lanes] - rc).max() / (2e-9 * np.abs(rc).max()), np.abs(phi[lanes] - rphi).max() / (2e-9 * max(np.abs(rphi).max(), 0.025)))
    fired = {name: sum(1 for b in branches if b[name] > 0) for name in ('damped', 'floor', 'free_volume', 'free_min', 'estimate')}
    print('%s: worst state error %.3g of the bar, status %s, iterations %s (oracle %s), lanes with each branch %s'
          % (key, ratio, sorted(set(st.tolist())), its[lanes].tolist(), rit.tolist(), fired))
    assert np.all(st == 0), st                            # every lane of the batch converged
    got = (c[lanes], phi[lanes], its[lanes], st)
    (assert_close_f32_records if NR.is_f32(r) else assert_close)(got, ref)
