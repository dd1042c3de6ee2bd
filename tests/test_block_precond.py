"""CPU: the host side of the block-Jacobi preconditioner -- bicg_csr_block_diagonal against a numpy
restatement, the method's name, the new symbols, and the generator synth.block_coupled."""
import numpy as np
import pytest

from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import synth


def numpy_blocks(A, bs):
    """(blocks [nb, bs, bs], rows without a stored (i,i)): in-block entries at their place, duplicates added in stored order"""
    rowid = np.repeat(np.arange(A.rows, dtype=np.int64), np.diff(A.ptr.astype(np.int64)))
    col = A.col.astype(np.int64)
    on = rowid // bs == col // bs
    out = np.zeros((-(-A.rows // bs), bs, bs))
    np.add.at(out, (rowid[on] // bs, rowid[on] % bs, col[on] % bs), A.val[on])      # (unbuffered, in index order: stored order)
    have = np.zeros(A.rows, dtype=bool)
    have[rowid[rowid == col]] = True
    return out, int(A.rows - have.sum())


@pytest.fixture(scope="module")
def fem():
    return synth.fem_like(5000)


@pytest.mark.parametrize("bs", [1, 3, 4, 16])
def test_csr_block_diagonal_fem_like(fem, bs):
    got, missing = H.csr_block_diagonal(H.single_rank_blocks(fem), bs)
    want, want_missing = numpy_blocks(fem, bs)
    assert missing == want_missing == 0
    assert got.shape == want.shape == (-(-5000 // bs), bs, bs)
    assert got.tobytes() == want.tobytes()
    assert np.count_nonzero(got) > 5000 or bs == 1      # off-diagonal entries of the blocks are there


def test_partial_last_block_holds_zeros_outside_its_leading_part(fem):
    got, _ = H.csr_block_diagonal(fem, 3)               # 5000 = 1666 * 3 + 2
    assert got.shape == (1667, 3, 3)
    last = got[-1]
    assert np.all(last[2, :] == 0.0) and np.all(last[:, 2] == 0.0)
    assert np.signbit(last[2, :]).sum() == 0 and np.signbit(last[:, 2]).sum() == 0
    assert last[0, 0] >= 32.0 and last[1, 1] >= 32.0
    assert got.tobytes() == numpy_blocks(fem, 3)[0].tobytes()


def test_a_duplicated_in_block_entry_is_summed_in_stored_order():
    # row 0: (0,1) twice around the diagonal; row 1: no diagonal, an entry outside the block; row 2 (block 1): (2,3) four times, a sum
    # that depends on the order (0.5 is lost against 1e16, whose spacing is 2: left to right gives 3.0, cancelling the large pair first 3.5)
    ptr = np.array([0, 3, 5, 9, 10], dtype=np.uint32)
    col = np.array([1, 0, 1, 0, 2, 3, 3, 3, 3, 3], dtype=np.uint32)
    val = np.array([0.1, 5.0, 0.2, 7.0, 9.0, 0.5, 1.0e16, -1.0e16, 3.0, 4.0])
    got, missing = H.csr_block_diagonal(synth.CSR(4, 4, ptr, col, val), 2)
    assert missing == 2                                  # rows 1 and 2
    assert got[0, 0, 1] == 0.1 + 0.2 and got[0, 0, 0] == 5.0
    assert got[0, 1, 0] == 7.0 and got[0, 1, 1] == 0.0   # (1,2) lies outside the block
    assert got[1, 0, 1] == ((0.5 + 1.0e16) + -1.0e16) + 3.0 == 3.0
    assert got[1, 0, 0] == 0.0 and got[1, 1, 1] == 4.0 and got[1, 1, 0] == 0.0


def test_csr_block_diagonal_of_an_empty_block():
    A = synth.CSR(0, 0, np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(0))
    got, missing = H.csr_block_diagonal(A, 4)
    assert got.size == 0 and missing == 0


def test_block_size_one_is_csr_diagonal():
    for A in (synth.fem_like(5000), synth.random_rows(3000, 12)):
        d, missing = H.csr_diagonal(A)
        got, got_missing = H.csr_block_diagonal(A, 1)
        assert got_missing == missing
        assert got.reshape(-1).tobytes() == d.tobytes()


def test_block_size_outside_the_range_is_refused():
    import ctypes as C
    blk = H.single_rank_blocks(synth.fem_like(50))
    out = np.full(50 * 17, 7.0)
    for bs in (0, 17, -1):
        assert H.lib().bicg_csr_block_diagonal(C.byref(blk.diag), bs, H._d(out)) == -2
        with pytest.raises(ValueError):
            H.csr_block_diagonal(blk, bs)
    assert np.all(out == 7.0)


def test_method_name():
    assert H.METHODS["bicgstab_block"] == 5
    assert H.METHODS["bicgstab_diag"] == 4


def test_symbols_resolve():
    lib = H.lib()
    for name in ("bicg_precond_block_diagonal", "bicg_precond_block_diagonal_device", "bicg_precond_apply", "bicg_csr_block_diagonal",
                 "block_jacobi_bicgstab"):
        assert hasattr(lib, name), name
        assert name in H.EXPORTS or not name.startswith("bicg_")      # (EXPORTS: what build() checks after linking)


@pytest.mark.parametrize("gen", [synth.transport_like, synth.fem_like])
@pytest.mark.parametrize("n,bs,decades", [(2000, 4, 0.0), (2002, 4, 0.0), (1999, 3, 0.0), (2000, 16, 2.0)])
def test_block_coupled_invariants(gen, n, bs, decades):
    """the in-block part of every whole block is skew with the law's weights, every other entry is the generator's; columns ascend"""
    A, G = synth.block_coupled(n, bs, gen, scale_decades=decades), gen(n)
    nb, lim = n // bs, (n // bs) * bs
    sc = synth.row_scale(np.arange(n), decades) if decades > 0.0 else np.ones(n)

    def parts(M):
        row, col, val = M.to_coo()
        row, col = row.astype(np.int64), col.astype(np.int64)
        inb = (row != col) & (row // bs == col // bs) & (row < lim) & (col < lim)
        return row, col, val, inb
    row, col, val, inb = parts(A)
    assert np.all(np.diff(A.ptr.astype(np.int64)) > 0)
    same_row = row[1:] == row[:-1]
    assert np.all(col[1:][same_row] > col[:-1][same_row])
    # outside the blocks: the generator's entries (times the scaling, applied as the generator applies it)
    grow, gcol, gval, ginb = parts(G)
    assert np.array_equal(row[~inb], grow[~ginb]) and np.array_equal(col[~inb], gcol[~ginb])
    want = gval[~ginb] * sc[grow[~ginb]] * sc[gcol[~ginb]] if decades > 0.0 else gval[~ginb]
    assert val[~inb].tobytes() == want.tobytes()
    # inside: every pair of every whole block, +w above and -w below the diagonal
    assert int(inb.sum()) == nb * bs * (bs - 1)
    D = np.zeros((n, bs))
    D[row[inb], col[inb] % bs] = val[inb]
    B = D[:lim].reshape(nb, bs, bs)
    up = row[inb] < col[inb]
    r, c = row[inb][up], col[inb][up]
    w = 48.0 * (0.5 + 0.5 * synth._uniform(r * 64 + (c - r), 555))
    assert np.all(w >= 24.0)
    if decades > 0.0:
        w = w * sc[r] * sc[c]
        Bs = B / (sc[:lim].reshape(nb, bs, 1) * sc[:lim].reshape(nb, 1, bs))
        np.testing.assert_allclose(Bs, -np.transpose(Bs, (0, 2, 1)), rtol=1e-14, atol=0.0)
    else:
        assert np.array_equal(B, -np.transpose(B, (0, 2, 1)))
    assert val[inb][up].tobytes() == w.tobytes()
