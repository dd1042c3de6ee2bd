"""`-m gpu`: BiCGStab(2), method 6, across ranks. Spawned ranks share the one GPU through the host-staged
transport (worker: tests/mp_bicgstab2_workers.py, on the spawn and report helpers of tests/mp_workers.py). Three sweeps at tol = 0:
the same scalar bytes on every rank, x and r within the computed tolerance of the numpy restatement on the whole system, four halo
exchanges and five all-reduces per sweep; and one solve to tol 1e-10 on the (16, 20) convection stencil over three ranks.

synth.transport_like(40000) over 3 ranks; mp_multi_workers.matrix("six") over 7 ranks, where the seventh rank has no rows."""
import pytest

import mp_bicgstab2_workers as W
import mp_workers

pytestmark = pytest.mark.gpu
WALL_LIMIT = 240.0      # seconds per case


def _run(name, world):
    skips = mp_workers.run_ranks(W.stab2_worker, world, name, WALL_LIMIT)
    assert not skips, skips


def test_three_ranks():
    _run("transport", 3)


def test_a_rank_without_rows():
    _run("six", 7)


def test_convection_converges_over_three_ranks():
    _run("convection", 3)
