"""No GPU: the host side of the diagonal preconditioner (include/bicgstab_hip.h section 3 "DIAGONAL PRECONDITIONER"; DESIGN.md section
4.20): bicg_csr_diagonal against numpy, the method's name in the binding, and the new symbols in the library."""
import numpy as np

from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import synth


def numpy_diagonal(A):
    """(d, missing): the (i,i) entries added in stored order (np.add.at adds in index order), 0.0 where a row has none"""
    rowid = np.repeat(np.arange(A.rows, dtype=np.int64), np.diff(A.ptr.astype(np.int64)))
    on = A.col.astype(np.int64) == rowid
    d = np.zeros(A.rows)
    np.add.at(d, rowid[on], A.val[on])
    have = np.zeros(A.rows, dtype=bool)
    have[rowid[on]] = True
    return d, int(A.rows - have.sum())


def test_csr_diagonal_fem_like():
    A = synth.fem_like(5000)
    d, missing = H.csr_diagonal(H.single_rank_blocks(A))
    want, want_missing = numpy_diagonal(A)
    assert missing == want_missing == 0
    assert d.tobytes() == want.tobytes() and np.all(d >= 32.0)


def test_csr_diagonal_counts_the_rows_without_one():
    A = synth.random_rows(3000, 12)
    d, missing = H.csr_diagonal(A)
    want, want_missing = numpy_diagonal(A)
    assert want_missing > 0, "the generator is expected to leave rows empty"
    assert missing == want_missing
    assert d.tobytes() == want.tobytes()
    assert np.count_nonzero(d == 0.0) >= missing


def test_csr_diagonal_adds_a_duplicated_entry_in_stored_order():
    # row 0: (0,0) twice around an off-diagonal entry; row 1: no diagonal; row 2: (2,2) four times, a sum that depends on the order
    # (0.5 is lost against 1e16, whose spacing is 2: left to right gives 3.0, any order that cancels the large pair first 3.5)
    ptr = np.array([0, 3, 4, 8], dtype=np.uint32)
    col = np.array([0, 1, 0, 0, 2, 2, 2, 2], dtype=np.uint32)
    val = np.array([0.1, 5.0, 0.2, 7.0, 0.5, 1.0e16, -1.0e16, 3.0])
    d, missing = H.csr_diagonal(synth.CSR(3, 3, ptr, col, val))
    assert missing == 1
    assert d[0] == 0.1 + 0.2 and d[1] == 0.0
    assert d[2] == ((0.5 + 1.0e16) + -1.0e16) + 3.0 == 3.0


def test_csr_diagonal_of_an_empty_block():
    A = synth.CSR(0, 0, np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(0))
    d, missing = H.csr_diagonal(A)
    assert d.size == 0 and missing == 0


def test_method_name():
    assert H.METHODS["bicgstab_diag"] == 4
    assert sorted(H.METHODS.values()) == [0, 1, 2, 3, 4]


def test_symbols_resolve():
    lib = H.lib()
    for name in ("bicg_precond_diagonal", "bicg_precond_diagonal_device", "bicg_precond_clear", "bicg_precond_kind", "bicg_csr_diagonal",
                 "jacobi_bicgstab"):
        assert hasattr(lib, name), name
        assert name in H.EXPORTS or not name.startswith("bicg_")      # (EXPORTS: what build() checks after linking)
