"""BICG_PLAN="reorder=1|2" on the host (csrc/bicg_reorder.cpp; no GPU): the ordering bicg_reorder_plan returns, the block
bicg_permute_block builds from it, what the sliced-ELL plan makes of that block, and the token.

The ordering is reverse Cuthill-McKee on the symmetrised pattern; what is asked of it here are the conditions the product kernels
impose on a numbering, not measurements: at most 2048 distinct columns per 256-row group (kJagwMaxSlots, csrc/bicg_device.h: the
list-driven x window of k_spmv_jagl), columns within 16 bits of their rows (16-bit offsets). The block keeps the stored order of
every row's entries -- the reason products on it stay bit-identical to the reference's mult() (src/matrix.c:498-516) on the
caller's matrix -- which is checked array for array against a numpy construction that sorts nothing."""
import numpy as np
import pytest

from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import mesh, synth

_built = {}


def _mesh(m, kind):
    key = (m, kind)
    if key not in _built:
        _built[key] = mesh.fem_unstructured(m, kind, scale_decades=2.0)
    return _built[key]


def _block_diagonal(A, B, seed=4):
    """A and B side by side on the diagonal, then a random symmetric permutation (entry order of the rows kept)"""
    n = A.rows + B.rows
    ptr = np.concatenate([A.ptr.astype(np.int64), A.nnz + B.ptr[1:].astype(np.int64)])
    col = np.concatenate([A.col.astype(np.int64), A.rows + B.col.astype(np.int64)])
    val = np.concatenate([A.val, B.val])
    C = synth.CSR(n, n, ptr.astype(np.uint32), col.astype(np.uint32), val)
    return _permuted_numpy(C, np.random.default_rng(seed).permutation(n))


def _permuted_numpy(A, perm):
    """P A P^T for perm[new] = old: a stable sort of the entries by new row, columns renamed, nothing else"""
    n = A.rows
    perm = np.asarray(perm, dtype=np.int64)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n, dtype=np.int64)
    row, col, val = A.to_coo()
    new_row = inv[row.astype(np.int64)]
    order = np.argsort(new_row, kind="stable")
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(new_row, minlength=n), out=ptr[1:])
    return synth.CSR(n, n, ptr.astype(np.uint32), inv[col.astype(np.int64)][order].astype(np.uint32), val[order])


CASES = {
    "mesh16_random": lambda: _mesh(16, "random"),
    # unsymmetric pattern, empty rows, long rows
    "random_rows": lambda: synth.random_rows(8000, 12, seed=3, empty_frac=0.1, long_rows={100: 3000, 2500: 2000}),
    "two_meshes": lambda: _block_diagonal(_mesh(10, "generator"), _mesh(12, "generator")),
    "diagonal_300": lambda: synth.CSR(300, 300, np.arange(301, dtype=np.uint32), np.arange(300, dtype=np.uint32), np.ones(300)),
    "one_row": lambda: synth.CSR(1, 1, np.array([0, 1], dtype=np.uint32), np.zeros(1, dtype=np.uint32), np.ones(1)),
}


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    A = CASES[request.param]()
    return request.param, A, H.single_rank_blocks(A)


def test_valid_permutation(case):
    name, A, blocks = case
    perm, stats = H.reorder_plan(blocks)
    assert perm.shape == (A.rows,) and np.array_equal(np.sort(perm), np.arange(A.rows)), name
    assert stats["rows"] == A.rows and stats["reserved"] == 0
    if name == "two_meshes":
        assert stats["components"] == 2 and stats["isolated_rows"] == 0
    if name in ("diagonal_300", "one_row"):
        assert stats["isolated_rows"] == A.rows and stats["components"] == 0
        assert np.array_equal(perm, np.arange(A.rows))          # rows without neighbours: original order
    if name == "mesh16_random":
        assert stats["components"] == 1
    # the stats are those of the two numberings
    B = H.permute_block(blocks, perm)
    for M, band, distinct in ((A, "bandwidth_given", "distinct_given"), (B, "bandwidth", "distinct")):
        row, col, _ = M.to_coo()
        assert stats[band] == (int(np.abs(row.astype(np.int64) - col.astype(np.int64)).max()) if M.nnz else 0), (name, band)
        assert stats[distinct] == int(mesh.window_stats(M)[0].max()), (name, distinct)


def test_the_order_does_not_depend_on_the_plan_threads(case):
    name, A, blocks = case
    L = H.lib()
    try:
        first, _ = H.reorder_plan(blocks)
        again, _ = H.reorder_plan(blocks)
        assert np.array_equal(first, again), name
        for threads in (1, 3, 16):
            L.bicg_set_plan_threads(threads)
            got, _ = H.reorder_plan(blocks)
            assert np.array_equal(first, got), (name, threads)
    finally:
        L.bicg_set_plan_threads(-1)


def test_permute_block_keeps_the_stored_entry_order(case):
    name, A, blocks = case
    perm, _ = H.reorder_plan(blocks)
    for p in (perm, np.random.default_rng(1).permutation(A.rows)):
        got, want = H.permute_block(blocks, p), _permuted_numpy(A, p)
        assert np.array_equal(got.ptr, want.ptr) and np.array_equal(got.col, want.col) and np.array_equal(got.val, want.val), name
    if A.rows > 1:
        bad = perm.copy()
        bad[1] = bad[0]                                         # a repeated index
        with pytest.raises(ValueError):
            H.permute_block(blocks, bad)
        bad = perm.copy()
        bad[0] = A.rows                                         # out of range
        with pytest.raises(ValueError):
            H.permute_block(blocks, bad)


def test_quality_on_the_randomly_numbered_mesh():
    """mesh m = 40 (64 000 rows) in random numbering: as given no 16-bit offsets and no window (4060 distinct columns per group);
    after the library's own order the block meets what the kernels ask for (scipy's RCM: 1501 distinct columns)"""
    A = _mesh(40, "random")
    blocks = H.single_rank_blocks(A)
    perm, stats = H.reorder_plan(blocks)
    B = H.permute_block(blocks, perm)
    assert int(mesh.window_stats(B)[0].max()) <= 2048
    assert stats["bandwidth"] < stats["bandwidth_given"] and stats["distinct"] < stats["distinct_given"], stats
    pb = H.single_rank_blocks(B)
    given, _ = H.sell_plan_digest(blocks)
    assert given["c16"] == 0 and given["window"] == 0, given
    after, _ = H.sell_plan_digest(pb)
    assert after["c16"] == 1, after
    # with the facts of a matrix 8 x as large (the list-driven window needs an average block of >= 6 M non-zeros)
    big, _ = H.sell_plan_digest(pb, rows_global=8 * A.rows, nnz_diag_global=8 * A.nnz)
    assert big["window"] == 2, big
    given_big, _ = H.sell_plan_digest(blocks, rows_global=8 * A.rows, nnz_diag_global=8 * A.nnz)
    assert given_big["c16"] == 0 and given_big["window"] == 0, given_big


def test_generator_numbering_is_not_harmed():
    A = _mesh(16, "generator")
    blocks = H.single_rank_blocks(A)
    before, _ = H.sell_plan_digest(blocks)
    assert before["window"] != 0
    perm, _ = H.reorder_plan(blocks)
    after, _ = H.sell_plan_digest(H.single_rank_blocks(H.permute_block(blocks, perm)))
    assert after["window"] != 0, after


def test_token():
    L = H.lib()
    H.switches(reorder=2)
    assert L.bicg_switch_unknown(b"BICG_PLAN", None, 0) == 0
    assert H.switch_value("BICG_PLAN", "reorder") == "2"
    H.switches(reorder=1)
    assert H.switch_value("BICG_PLAN", "reorder") == "1"
    H.switches(reorder="x")
    assert L.bicg_switch_unknown(b"BICG_PLAN", None, 0) == 1
    H.switches(reorder=None)
    assert H.switch_value("BICG_PLAN", "reorder") is None
    assert "bicg_reorder_plan" in H.EXPORTS and "bicg_permute_block" in H.EXPORTS and "bicg_reorder_info" in H.EXPORTS
    assert H.Context.FLAGS["reordered"] == 16384
