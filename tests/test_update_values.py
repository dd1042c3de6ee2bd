"""bicg_update_values, the parts that need no GPU.

1. bicg_persist_plan_sources: the map through which the persistent plan's pval is refilled decodes back to the values.
2. The claim the whole feature stands on: the sliced-ELL plan depends on the PATTERN only. A matrix and the same pattern with other
   values (`revalued`) give the same summary and the same digest of every array of the plan except the values themselves (sval).
   Where the plan holds values in lists (constant / masked slices) that is not so by design -- those contexts verify, never
   rewrite -- so the matrices whose plan has such slices are left out here. A later plan decision that reads values is caught.

`revalued(A, seed)`: val * s with s from default_rng(seed), in [1.0, 1.2] on the diagonal and in [0.9, 1.1] elsewhere, so row
dominance survives; zeros=3 additionally sets three off-diagonal values to exactly 0.0 (a stored zero is a value, not a pattern
change)."""
import numpy as np
import pytest

from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import synth
from test_sell_plan import MATRICES, _fixture

NONE = 0xFFFFFFFF


def revalued(A, seed, zeros=0, lo=0):
    """the pattern of A with other values; lo: global number of A's first row (a rank's diag block: the diagonal is col == lo + row)"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(A.rows, dtype=np.int64), np.diff(A.ptr.astype(np.int64)))
    on_diag = A.col.astype(np.int64) == rows + lo
    s = np.where(on_diag, 1.0 + 0.2 * rng.random(A.nnz), 0.9 + 0.2 * rng.random(A.nnz))
    val = np.asarray(A.val, dtype=np.float64) * s
    if zeros:
        val[rng.choice(np.flatnonzero(~on_diag), size=zeros, replace=False)] = 0.0
    return synth.CSR(A.rows, A.cols, A.ptr.copy(), A.col.copy(), val)


def _persist_cases():
    A = synth.transport_like(40000)
    yield "transport/P1", H.single_rank_blocks(A), 1, A, None
    diag, offd, counts, displs = synth.split_blocks(A, 2, 1)
    yield "transport/P2r1", H.HostBlocks(diag, offd, A.rows, counts, displs), 2, diag, offd
    R = _fixture("ragged_n400")
    yield "ragged_n400", H.single_rank_blocks(R), 1, R, None


def test_persist_plan_sources_decode_back_to_the_values():
    for name, blk, world, diag, offd in _persist_cases():
        P = H.persist_plan(blk, world, 60)
        assert P is not None, name
        psrc = H.persist_plan_sources(blk, world, 60, P["entries"])
        assert psrc is not None and psrc.shape == P["pval"].shape, name
        values = diag.val if offd is None else np.concatenate((diag.val, offd.val))
        pad = psrc == NONE
        assert np.array_equal(P["pval"][~pad].view(np.uint64), np.asarray(values, dtype=np.float64)[psrc[~pad]].view(np.uint64)), name
        assert np.all(P["pval"][pad].view(np.uint64) == 0), name
        # every source index exactly once
        assert np.array_equal(np.sort(psrc[~pad]), np.arange(len(values), dtype=np.uint32)), name
        # diag entries first: within a row the first rdiag entries come from the diag block
        nnz_d = diag.nnz
        r = 5 % diag.rows
        e = int(P["pbase"][r // 64]) + 64 * np.arange(int(P["rlen"][r])) + r % 64
        assert np.all(psrc[e][:int(P["rdiag"][r])] < nnz_d) and np.all(psrc[e][int(P["rdiag"][r]):] >= nnz_d), name


@pytest.mark.parametrize("name", list(MATRICES))
def test_the_plan_depends_on_the_pattern_only(name):
    A = MATRICES[name]()
    s0, d0 = H.sell_plan_digest(H.single_rank_blocks(A))
    if s0["constant_entries"] or s0["masked_rows"]:
        return      # the plan of this matrix holds values in lists (constant / masked slices): verified, never rewritten
    s1, d1 = H.sell_plan_digest(H.single_rank_blocks(revalued(A, 21)))
    assert s1 == s0, {k: (s0[k], s1[k]) for k in s0 if s0[k] != s1[k]}
    assert H.SELL_ARRAYS[3] == "sval"
    differ = [a for a in H.SELL_ARRAYS if a != "sval" and d0[a] != d1[a]]
    assert not differ, differ
    if s0["sell_entries"]:
        assert d0["sval"] != d1["sval"]


def test_the_list_driven_window_depends_on_the_pattern_only():
    """the list-driven window is a plan of large blocks: random_rows_n3000 with the shared facts of a large matrix, as
    tests/test_sell_plan.py's "inflated" cases pass them"""
    A = MATRICES["random_rows_n3000"]()
    f = -(-6500000 // A.nnz)
    s0, d0 = H.sell_plan_digest(H.single_rank_blocks(A), 1, A.rows * f, A.nnz * f)
    assert s0["jag"] and s0["window"] == 2
    s1, d1 = H.sell_plan_digest(H.single_rank_blocks(revalued(A, 21)), 1, A.rows * f, A.nnz * f)
    assert s1 == s0
    assert [a for a in H.SELL_ARRAYS if a != "sval" and d0[a] != d1[a]] == [] and d0["sval"] != d1["sval"]


def test_enough_matrices_take_part():
    """the early return above must not empty the test: every layout is among the matrices that take part"""
    seen = []
    for name, make in MATRICES.items():
        s, _ = H.sell_plan_digest(H.single_rank_blocks(make()))
        if not (s["constant_entries"] or s["masked_rows"]):
            seen.append(s)
    assert any(not s["jag"] and s["c16"] and s["sell_entries"] for s in seen), "padded, 16-bit"
    assert any(s["jag"] and s["window"] == 1 for s in seen), "jagged, run windows"
    assert any(s["jag"] and s["window"] == 0 and s["sell_entries"] for s in seen), "jagged without a window (the list-driven one: the test above)"
    assert any(s["rowsplit"] for s in seen), "rows over lanes"
    assert any(s["nblk"] and s["sell_entries"] for s in seen), "row blocks beside slices"
