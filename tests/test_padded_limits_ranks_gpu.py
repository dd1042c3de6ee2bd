"""`-m gpu`: the SpMM kernels over padded slices across ranks -- their OFFD instantiations --, on two crafted matrices of
tests/padded_cases.py cut into three equal row ranges whose sizes are no multiples of 64. Spawned ranks share the one GPU through the
host-staged transport (worker: tests/mp_padded_workers.py, on the spawn and report helpers of tests/mp_workers.py). Every rank's
SpMM of 17 shifted vectors is the oracle's rows for that rank in its bytes under all three forms, and the integer residual norms
are exact after the sum over the ranks.

clusters4_odd  four clusters on both sides of the diagonal: the middle rank has halo on both sides; 256-row tiles
lengths_x3     three blocks of `lengths` below each other (rows of 0 .. 33 entries to the right of the diagonal), one per rank: the
               first two ranks have halo. (`lengths` itself cut in three leaves the padded layout: padded_cases.RANK_CASES.)"""
import pytest

import mp_padded_workers as W
import mp_workers
import padded_cases as K

pytestmark = pytest.mark.gpu
WALL_LIMIT = 240.0      # seconds per case


@pytest.mark.parametrize("name", K.RANK_CASES)
def test_three_ranks(name):
    skips = mp_workers.run_ranks(W.padded_worker, 3, name, WALL_LIMIT)
    assert not skips, skips
