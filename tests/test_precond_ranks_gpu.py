"""`-m gpu`: the diagonal preconditioner and BICG_BICGSTAB_DIAG across ranks. Spawned ranks share the one
GPU through the host-staged transport (workers: tests/mp_precond_workers.py, on the spawn and report helpers of tests/mp_workers.py).
On every rank, as bytes: method 4 with d = 1 equals method 0 at the same partition; method 4 with d = powers of two equals method 0
on the matrix whose diag and offd columns are scaled by their owner's 1 / d (the hat vectors' halo exchange); method 4 moves
bicg_comm_counts by exactly what method 0 moves it, the install by nothing; without a preconditioner every rank is refused.

synth.transport_like(40000) over 3 ranks; mp_multi_workers.matrix("six") over 7 ranks, where the seventh rank has no rows and
passes NULL for its part of the diagonal."""
import pytest

import mp_precond_workers as W
import mp_workers

pytestmark = pytest.mark.gpu
WALL_LIMIT = 240.0      # seconds per case


def _run(name, world):
    skips = mp_workers.run_ranks(W.precond_worker, world, name, WALL_LIMIT)
    assert not skips, skips


def test_three_ranks():
    _run("transport", 3)


def test_a_rank_without_rows_passes_null():
    _run("six", 7)
