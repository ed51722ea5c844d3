"""GPU parity of the lane-quad kernel (pnp_lane4.hip, W = 4): the cases of tests/lane_cols_cases.py with this kernel forced."""
import pytest

pytest.register_assert_rewrite('tests.lane_cols_cases')
from tests.lane_cols_cases import *  # noqa: E402,F401,F403  (the test functions and pytestmark: collected here, under this module's ids)


@pytest.fixture(autouse=True)
def kernel(monkeypatch):
    monkeypatch.setenv('CATINT_NEWTON_KERNEL', 'lane4')
    return 'lane4'
