"""The inputs of the nonstop kernel's step-by-step test (tests/nonstop_cases.py) are what they claim, on the host replay."""
import pytest

from tests import nonstop_cases as ncs


@pytest.mark.parametrize("H,scenario,rand,draws", ncs.CONFIGS)
def test_batches_hold_their_events_away_from_rounding(H, scenario, rand, draws):
    met = ncs.census(ncs.build(H, scenario, rand, draws))
    assert met["margin"] >= 1e-9
    assert met["finished"] >= 10 and met["rejected"] >= 10 and met["place"] >= 1
    assert all(met["arrivals"].get(n, 0) >= 20 for n in range(min(H, 3) + 1))
    if draws:
        assert met["policy"] >= 10
    if rand:
        assert met["attributes"] >= 5
