"""`-m gpu`: bicg_update_values across ranks (csrc/bicg_refresh.cpp). Spawned ranks share the one GPU through
the host-staged transport (workers: tests/mp_update_workers.py, on the spawn and report helpers of tests/mp_workers.py); every rank
updates the diag and offd values of its own blocks to its share of revalued(A, 21). Then, as bytes against fresh contexts created on
the new values on every rank: the collective spmv, a bicgstab solve and a pipe_bicgstab solve (k, x, r, traces). The update itself
moves no transport counter (bicg_comm_counts) and no allocation count.

Matrix: synth.transport_like(40000) over 3 ranks. Under the host-staged transport a context is never persistent (the persistent
iteration across ranks needs the peer-to-peer data path: persist_build, csrc/bicg_create.cpp), so the persistent plan's refill through
its source map -- offd entries included -- is checked by a second case that enables the peer-to-peer path first and asserts the
`persist` flag (a peer-to-peer path that does not come up between ranks sharing one device is a failure). One more case runs 7 ranks on the 6-row matrix of mp_multi_workers.matrix("six"): the seventh rank has no rows and calls
with empty arrays."""
import pytest

import mp_update_workers as W
import mp_workers

pytestmark = pytest.mark.gpu
WALL_LIMIT = 240.0      # seconds per case


def _run(case, name, world):
    skips = mp_workers.run_ranks(W.update_worker, world, f"{case}:{name}", WALL_LIMIT)
    if skips:
        pytest.skip(skips[0])


def test_three_ranks_update_their_blocks():
    _run("host", "transport", 3)


def test_three_ranks_with_the_persistent_plan():
    _run("p2p", "transport", 3)


def test_a_rank_without_rows_calls_with_empty_arrays():
    _run("host", "six", 7)
