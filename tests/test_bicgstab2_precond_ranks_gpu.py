"""`-m gpu`: the right-preconditioned BiCGStab(2), methods 7 and 8, across ranks. Three spawned ranks
share the one GPU through the host-staged transport (worker: tests/mp_bicgstab2_precond_workers.py, on the spawn and report helpers
of tests/mp_workers.py). Three sweeps at tol = 0: the same scalar bytes on every rank, x and r within the computed tolerance of the
numpy restatement on the whole system, four halo exchanges and five all-reduces per sweep, none for an install or an application;
a rank without rows; a rank whose preconditioner was cleared is refused on its own, without a collective; and the issue's S3 with
its 4 x 4 blocks converges over three ranks as on one."""
import pytest

import mp_bicgstab2_precond_workers as W
import mp_workers

pytestmark = pytest.mark.gpu
WALL_LIMIT = 240.0      # seconds per case


def _run(name):
    skips = mp_workers.run_ranks(W.stab2_precond_worker, 3, name, WALL_LIMIT)
    assert not skips, skips


def test_three_ranks():
    _run("transport")


def test_a_rank_without_rows():
    _run("empty")


def test_a_rank_whose_preconditioner_was_cleared_is_refused_on_its_own():
    _run("cleared")


def test_block_coupled_convection_converges_over_three_ranks():
    _run("convection")
