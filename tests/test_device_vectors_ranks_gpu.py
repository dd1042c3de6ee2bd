"""`-m gpu`: the device-resident vector calls across ranks. Spawned ranks share the one GPU through the
host-staged transport (workers: tests/mp_device_vector_workers.py, on the spawn and report helpers of tests/mp_workers.py). Every rank
compares, as bytes against the same call on numpy arrays: the collective spmv, a bicgstab and a pipe_bicgstab solve (k, x, r, result
fields, traces), load / run / warm-started load / run / fetch, and a five-column solve_multi; every call on tensors moves
bicg_comm_counts by what its host variant moves them.

synth.transport_like(40000) over 3 ranks; mp_multi_workers.matrix("six") over 7 ranks, where the seventh rank has no rows, passes
empty tensors (the library gets NULL) and takes part in every collective."""
import pytest

import mp_device_vector_workers as W
import mp_workers

pytestmark = pytest.mark.gpu
WALL_LIMIT = 240.0      # seconds per case


def _run(name, world):
    skips = mp_workers.run_ranks(W.device_worker, world, name, WALL_LIMIT)
    assert not skips, skips


def test_three_ranks_on_tensors_equal_three_ranks_on_numpy():
    _run("transport", 3)


def test_a_rank_without_rows_passes_no_arrays():
    _run("six", 7)
