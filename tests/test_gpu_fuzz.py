"""Randomised parity sweep: seeded random scene configurations (image size incl. odd / sub-tile sizes, Gaussian count,
footprint scale, SH degree / precomputed colours, precomputed covariance, scale modifier, background, camera pose on
the reference's circle path) rendered by the HIP library and by the reference build (oracle/_ref, the reference's own
kernels compiled for gfx950): integer outputs and forward floats must be bit-identical, gradients within tolerance.
Each case is tiny, so the sweep also hits the degenerate ends (P = 1, 1x1 tile grids, lists shorter than a round,
lists of several rounds, everything culled)."""
import os

import pytest

from grad_ladder import (MAX_CASE_FRACTION, MAX_CASE_FRACTION_REF_TOO, MAX_ROW_FRACTION, MAX_ROW_FRACTION_REF_TOO, assert_exits_stay_rare,
                         new_tally)
from sweep_support import check_random_case

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("GSR_FUZZ_CASES", "512"))
# the exits of the gradient comparison (tests/grad_ladder.py) over the sweep, capped by test_fuzz_escape_hatches_stay_rare
TALLY = new_tally()


@pytest.mark.parametrize("i", range(N_CASES))
def test_random_case_matches_reference_build(i, gpu_device):
    check_random_case(i, gpu_device, TALLY)


def test_fuzz_escape_hatches_stay_rare():
    """Runs after the sweep (same process): how many cases / rows needed a fallback of the gradient comparison."""
    if TALLY["cases"] == 0:
        pytest.skip("no fuzz case ran in this process")
    print("fuzz tally:", TALLY)
    assert_exits_stay_rare(TALLY, MAX_CASE_FRACTION, MAX_ROW_FRACTION, MAX_CASE_FRACTION_REF_TOO, MAX_ROW_FRACTION_REF_TOO)
