"""`-m gpu`: the block-Jacobi preconditioner and BICG_BICGSTAB_BLOCK across ranks. Spawned ranks share the
one GPU through the host-staged transport (workers: tests/mp_block_precond_workers.py, on the spawn and report helpers of
tests/mp_workers.py). On every rank, as bytes: method 5 with blocks that hold d = powers of two on their diagonals and zeros
elsewhere (bs = 4) equals method 4 with that d at the same partition; method 5 moves bicg_comm_counts by exactly what method 4 moves
it, the install by nothing; without a block preconditioner every rank is refused with -2.

synth.transport_like(40000) over 3 ranks (13334 / 13333 / 13333 local rows: partial last blocks at bs = 4, blocks local to the rank);
mp_multi_workers.matrix("six") over 7 ranks, where the seventh rank has no rows and passes NULL for its blocks."""
import pytest

import mp_block_precond_workers as W
import mp_workers

pytestmark = pytest.mark.gpu
WALL_LIMIT = 240.0      # seconds per case


def _run(name, world):
    skips = mp_workers.run_ranks(W.block_worker, world, name, WALL_LIMIT)
    assert not skips, skips


def test_three_ranks():
    _run("transport", 3)


def test_a_rank_without_rows_passes_null():
    _run("six", 7)
