"""`-m gpu`: the right-preconditioned methods 4 and 5 of bicg_solve_multi across ranks (csrc/bicg_multi.cpp):
3 and 7 spawned ranks -- at most 7 processes hold the GPU at a time -- share the one GPU through the host-staged transport. The
workers: tests/mp_multi_precond_workers.py. Partitions: transport_like(40000) over 3 ranks; the 6-row matrix of mp_multi_workers over
7 ranks, whose seventh rank has no rows and passes None for its diagonal and its blocks. Block sizes differ between ranks (4 on
even ranks, 3 on odd ones): blocks are a rank's own.

Everything is compared as bytes. E: k, dot_r, dot_zero, the breakdown iteration and the four traces of every column are the same
on every rank. D: a column of the set equals the collective one-column call at the same partition, and check_every = 7 changes
nothing. B: method 4 with d = powers of two equals the plain collective call on A D^-1 at the same partition, x up to the scaling.
A rank whose preconditioner was cleared returns -2 and the others -1; x, r and the allocation count stay as they were everywhere, and
the next correct call gives the bytes of the one before."""
import pytest

import mp_multi_precond_workers as W
import mp_workers

pytestmark = pytest.mark.gpu
WALL_LIMIT = 240.0      # seconds per case
PARTITIONS = [("transport40000", 3), ("six", 7)]


@pytest.mark.parametrize("name,world", PARTITIONS)
def test_same_scalars_on_every_rank_columns_alone_and_powers_of_two(name, world):
    assert not mp_workers.run_ranks(W.precond_worker, world, f"props:{name}", WALL_LIMIT)


@pytest.mark.parametrize("name,world", PARTITIONS)
def test_a_rank_without_its_preconditioner_refuses_for_all(name, world):
    assert not mp_workers.run_ranks(W.precond_worker, world, f"cleared:{name}", WALL_LIMIT)
