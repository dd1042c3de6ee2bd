"""`-m gpu`: the two products that read the CSR arrays as they are (csrc/bicg_spmv_csr.hip) -- k_spmv_rows, rows over lanes, and
k_spmv, the row-block stream -- on the crafted matrices of tests/csr_cases.py, each of which sits ON a limit: row blocks whose mean
row length is 79 | 80, 159 | 160, 319 | 320 (T = 8, 16, 32, 64 on both sides), rows of 8T - 1 / 8T / 8T + 1 / T - 1 / 1 / 0 entries,
row blocks of 1, 256 / T -+ 1 and 255 rows, a row of 8000 in a block of T = 8, rows of 8193 and 20011, blocks of exactly 8192
non-zeros and 256 rows, 16-bit offsets at +-32767 / 32768; blocks of exactly 2044 non-zeros, single rows of 2044 .. 2050 and 5000,
blocks at the 1024-row cap, a block of empty rows, three runs of CSR groups among sliced ones. tests/test_csr_limits.py checks on the
CPU that every matrix plans as its generator promises, and what the reference model is worth.

References, without a tolerance wherever the kernels promise an association:
  rows over lanes   csr_cases.rows_model: lane l of T adds the row's entries l, l + T, ... in stored order, then the balanced tree
  row-block stream  the CPU oracle's spmv (stored order) for every row of a block of at most 2048 non-zeros; the three single rows
                    beyond that are reduced with strided partial sums (block_sum): within 1e-13 sum |a x| of the oracle,
                    repeatable in their bytes, and the oracle's bits on integer values
  fused dots        integer systems (bitwise.IntegerSystem): dot_zero = (b, b), alpha_1 = (b, b) / (b, A b), one right answer as bytes
  shift             bicg_spmm has no SpMM kernel for these contexts: every column runs these kernels with the shift in the epilogue,
                    row j = fl(reference(x_j) + fl(sigma_j x_j))
Every context is created under switches(persist=0) and the case's own switches; the tokens are taken back at once. One context
per case and kind of values lives for the module."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import csr_cases as K
import oracle_lib as O
from bitwise import IntegerSystem, assert_same_bits, check_first_dots, oracle_spmv, same_bits
from mpi_bicgstab_amd import hipsolver as H

pytestmark = pytest.mark.gpu
METHODS = ("bicgstab", "ca_bicgstab", "pipe_bicgstab")
SIGMA3 = np.array([0.0, 0.02, 0.05])
BAR = 1e-13                                     # rows whose sum is associated by block_sum: x sum |a x|
DOT_CASES = ("t_edges", "batch_edges", "odd_rows", "full_blocks", "all_blocks", "mixed")
SHIFT_CASES = ("t_edges", "all_blocks")
SHIFT_NVEC = (1, 3, 17)
SOLVE_CASES = ("t_edges", "batch_edges", "odd_rows", "outlier_in_short_block", "full_blocks", "near16", "far32_plus", "all_blocks", "mixed")
UPDATE_CASES = ("t_edges", "near16", "all_blocks", "mixed")


@pytest.fixture(scope="module", autouse=True)
def _single_rank():
    H.lib().bicg_comm_init_single(0)      # (once: a new communicator orphans the contexts of the one before)
    yield
    for ctx in _contexts.values():
        ctx.close()
    _contexts.clear()


_contexts = {}


def new_context(A, sw):
    """a context of the one-rank block A under persist=0 and the case's switches; the tokens are taken back at once"""
    tokens = dict(sw, persist=0)
    H.switches(**tokens)
    try:
        return H.Context(H.single_rank_blocks(A))
    finally:
        H.switches(**{k: None for k in tokens})


def context(name, values="generic"):
    """the module's context of a case with these values (seed 0)"""
    if (name, values) not in _contexts:
        A, _, sw = K.build(name, values)
        _contexts[name, values] = new_context(A, sw)
    return _contexts[name, values]


def reference(A, facts, x):
    """(A x as the case's kernel promises it, the rows it promises no association for)"""
    if facts["rowsplit"]:
        return K.rows_model(A, facts["blocks"], x), np.zeros(0, dtype=np.int64)
    return oracle_spmv(A, x), K.strided_rows(facts)


@functools.lru_cache(maxsize=None)
def product_reference(name, seed=0):
    """(x, reference A x, strided rows, sum |a x| of those rows) for the generic values of a case -- computed once, never written to"""
    A, facts, _ = K.build(name, "generic", seed)
    x = np.random.default_rng(1000 + seed).standard_normal(A.rows)
    want, strided = reference(A, facts, x)
    scale = K.abs_row_sums(A, x)[strided] if len(strided) else np.zeros(0)
    for a in (x, want, strided, scale):
        a.setflags(write=False)
    return x, want, strided, scale


def check_rows(got, want, strided, scale, what):
    """got is `want` in its bytes, but in the strided rows, which are within the bar"""
    keep = np.ones(len(want), dtype=bool)
    keep[strided] = False
    assert_same_bits(got[keep], want[keep], what)
    assert np.all(np.abs(got[strided] - want[strided]) <= BAR * scale), (what, "strided rows", got[strided], want[strided])


def check_product(ctx, A, facts, ref, what):
    x, want, strided, scale = ref
    H.product_kernels()
    y1 = ctx.spmv(x)
    y2 = ctx.spmv(x)
    assert H.product_kernels() == facts["kernels"], what
    check_rows(y1, want, strided, scale, what)
    assert_same_bits(y2, y1, what + ", again")
    empty = np.diff(A.ptr.astype(np.int64)) == 0
    assert same_bits(y1[empty], np.zeros(int(empty.sum()))), (what, "rows without entries give +0.0")


def check_plan(ctx, A, facts, what):
    fl, info = ctx.flags(), ctx.plan_info()
    assert fl["rowsplit"] == bool(facts["rowsplit"]) and not fl["persist"] and not fl["spmm"], (what, fl)
    assert fl["col16"] == (facts["sell_rows"] > 0), (what, fl)      # (the flag speaks of the sliced entries: none but in `mixed`)
    assert fl["all_sell"] is False and fl["jagged"] == bool(facts["jag"] and facts["sell_rows"]), (what, fl)
    assert (info["rows"], info["nnz_diag"], info["nnz_offd"], info["halo"]) == (A.rows, A.nnz, 0, 0), (what, info)
    assert info["row_blocks"] == facts["nblk"] + -(-facts["sell_rows"] // K.GROUP) and info["boundary_blocks"] == 0, (what, info)
    assert info["sell_rows"] == facts["sell_rows"], (what, info)
    if facts["rowsplit"]:      # 10 bytes per non-zero with 16-bit offsets in CSR order, 12 without (bicg_device_matrix_bytes)
        assert (ctx.device_matrix_bytes() < 12 * A.nnz) == bool(facts["csr16"]), (what, ctx.device_matrix_bytes(), A.nnz)


# ---- product ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.CASES))
def test_product_is_the_references_bit_for_bit(name):
    A, facts, _ = K.build(name)
    ctx = context(name)
    check_plan(ctx, A, facts, name)
    check_product(ctx, A, facts, product_reference(name), name)


@pytest.mark.parametrize("name", list(K.CASES))
def test_integer_product_is_exact(name):
    """integer values: every association gives the same bits, the strided rows included"""
    S = integer_system(name)
    y = context(name, "integer").spmv(S.b.astype(np.float64))
    assert_same_bits(y, S.Ab.astype(np.float64), name)


# ---- fused dots --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def integer_system(name):
    return IntegerSystem(name, K)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", DOT_CASES)
def test_first_iterations_dots_are_exact(name, method):
    S = integer_system(name)
    ctx = context(name, "integer")
    H.product_kernels()
    check_first_dots(ctx, S, f"{name} {method}", method)
    assert H.product_kernels() == S.facts["kernels"]


# ---- shift -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shift_reference(name):
    """(X [17][n], distinct sigma [17], the reference's A x_j [17][n]) for the generic values of a case"""
    A, facts, _ = K.build(name)
    nv = max(SHIFT_NVEC)
    X = np.random.default_rng(3000).standard_normal((nv, A.rows))
    sigma = np.concatenate((SIGMA3, (np.arange(nv - 3) + 1.0) * 0.013))
    AX = np.stack([reference(A, facts, X[j])[0] for j in range(nv)])
    for a in (X, sigma, AX):
        a.setflags(write=False)
    return X, sigma, AX


@pytest.mark.parametrize("name", SHIFT_CASES)
def test_shifted_columns_run_these_kernels(name):
    A, facts, _ = K.build(name)
    ctx = context(name)
    X, sigma, AX = shift_reference(name)
    strided = K.strided_rows(facts) if not facts["rowsplit"] else np.zeros(0, dtype=np.int64)
    keep = np.ones(A.rows, dtype=bool)
    keep[strided] = False
    for nvec in SHIFT_NVEC:
        H.product_kernels()
        Y, _ = ctx.spmm(X[:nvec], sigma[:nvec])
        Y2, _ = ctx.spmm(X[:nvec], sigma[:nvec])
        assert H.product_kernels() == facts["kernels"], (name, nvec)
        want = AX[:nvec] + sigma[:nvec, None] * X[:nvec]          # one rounding for the product, one for the sum
        for j in range(nvec):
            what = f"{name}: {nvec} vectors, vector {j}, sigma {sigma[j]}"
            assert_same_bits(Y[j][keep], want[j][keep], what)
            assert_same_bits(Y2[j], Y[j], what + ", again")
            if len(strided):      # the row's own sum from a plain product, then the same two roundings
                y = ctx.spmv(X[j])
                scale = K.abs_row_sums(A, X[j])[strided]
                assert np.all(np.abs(y[strided] - AX[j][strided]) <= BAR * scale), what
                assert_same_bits(Y[j][strided], y[strided] + sigma[j] * X[j][strided], what + ", strided rows")
    Y0, _ = ctx.spmm(X[:3])                                        # no shifts: plain A X
    assert_same_bits(Y0[:, keep], AX[:3][:, keep], f"{name}: no shifts")


@pytest.mark.parametrize("name", SHIFT_CASES)
def test_three_shift_solve_seed_scalars_are_exact(name):
    """shifted_lopbicgstab on the integer system, seed shift 2 (an integer): r = r# = p = b, so dot_zero = (b, b) and
    alpha_1 = (b, b) / (b, (A + 2 I) b) = (b, b) / ((b, A b) + 2 (b, b)) in integers"""
    S = integer_system(name)
    ctx = context(name, "integer")
    sigma = np.array([2.0 - 1.0 / 64, 2.0, 2.0 + 1.0 / 64])
    H.product_kernels()
    got = ctx.solve_shifted(S.b.astype(np.float64), sigma, 1, tol=0.0, max_iter=1, check_every=1)
    assert H.product_kernels() == S.facts["kernels"] and not ctx.last_shifted_persistent()
    assert got["k"] == 1 and same_bits(got["result"].dot_zero, S.dot_zero)
    alpha = float(Fraction(S.bb, S.bAb + 2 * S.bb))
    assert same_bits(ctx.trace(1)["alpha"][0], alpha), (name, float(ctx.trace(1)["alpha"][0]), alpha)


# ---- six iterations ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dominant_system(name):
    """(A with dominant diagonals, b = A 1 by the oracle, the oracle's six iterations of the three solvers)"""
    A, facts, _ = K.build(name, "dominant")
    b = oracle_spmv(A, np.ones(A.rows))
    b.setflags(write=False)
    row, col, val = A.to_coo()
    want = {m: O.solve(m, A.rows, row, col, val, b, tol=0.0, max_iter=6) for m in METHODS}
    return A, b, want


@pytest.mark.parametrize("name", SOLVE_CASES)
def test_six_iterations_follow_the_oracle(name):
    A, b, want = dominant_system(name)
    ctx = context(name, "dominant")
    for method in METHODS:
        runs = []
        for _ in range(2):
            got = ctx.solve(method, b, tol=0.0, max_iter=6, check_every=6)
            tr = ctx.trace(6)
            assert got["k"] == 6 == want[method]["k"], (name, method, got["k"])
            runs.append(np.concatenate([tr[key] for key in ("alpha", "omega", "beta", "dotr")] + [got["x"]]))
        assert np.all(np.isfinite(runs[0])), (name, method)
        assert_same_bits(runs[1], runs[0], f"{name} {method}: the same solve twice")
        for key in ("alpha", "omega", "beta", "dotr"):
            np.testing.assert_allclose(tr[key][:6], want[method][key][:6], rtol=1e-8, atol=0.0, err_msg=f"{name} {method} {key}")


# ---- new values ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", UPDATE_CASES)
def test_new_values_at_the_same_edges(name):
    """bicg_update_values on these layouts (csrc/bicg_refresh.cpp): the next product is the reference's on the new values; the
    row-block descriptors and the 16-bit offsets in CSR order are the pattern's and survive"""
    A, facts, sw = K.build(name)
    A1, _, _ = K.build(name, "generic", 1)
    assert np.array_equal(A.col, A1.col) and not np.array_equal(A.val, A1.val)
    ctx = new_context(A, sw)
    try:
        check_product(ctx, A, facts, product_reference(name), name)
        before = (ctx.flags(), ctx.plan_info(), ctx.device_matrix_bytes())
        assert ctx.update_values(A1.val) == 0
        assert (ctx.flags(), ctx.plan_info(), ctx.device_matrix_bytes()) == before
        check_plan(ctx, A1, facts, name)
        check_product(ctx, A1, facts, product_reference(name, 1), f"{name}, new values")
    finally:
        ctx.close()
