"""`-m gpu`: the products of csrc/bicg_spmv_csr.hip across ranks, on two crafted matrices of tests/csr_cases.py cut into three equal
row ranges. Spawned ranks share the one GPU through the host-staged transport (worker: tests/mp_csr_workers.py, on the spawn and
report helpers of tests/mp_workers.py): on the middle rank some row blocks touch the halo (the launch with the offd part in its
epilogue) and some do not; every rank's product is the reference's in its bytes; six iterations of bicgstab follow the oracle over
three virtual ranks.

odd_rows    rows over lanes: row blocks of 1, 256 / T -+ 1 and 255 rows; the rows of 8192 entries reach across all three ranks
all_blocks  row-block stream: the middle rank holds the end of the short-row stretch, the single long rows and the exact-2044 block"""
import pytest

import mp_csr_workers as W
import mp_workers

pytestmark = pytest.mark.gpu
WALL_LIMIT = 240.0      # seconds per case


@pytest.mark.parametrize("name", ["odd_rows", "all_blocks"])
def test_three_ranks(name):
    skips = mp_workers.run_ranks(W.csr_worker, 3, name, WALL_LIMIT)
    assert not skips, skips
