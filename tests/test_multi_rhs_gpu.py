"""`-m gpu`: multi-RHS plain BiCGStab (bicg_solve_multi, csrc/bicg_multi.cpp / bicg_multi.hip): up to 16 independent recurrences of
reference src/solver.c:74-120 per pass over the matrix, every column with its own scalars and its own loop condition.

Right-hand sides b_j = A x*_j (the oracle's mult()): x*_0 = 1, x*_1 = 0 (b = 0: k = 0), x*_2 = e_{n//2}, x*_3 = 1 on the first
third of the rows, x*_j (j >= 4) = 0.5 + default_rng(7).random(n) drawn in order. tol = 1e-12 unless stated.

Bars. Against the oracle: |k_j - k_oracle_j| <= 2 and |x_j - x*_j|_inf <= 1e-9 (tests/test_gpu_parity.py), the first min(6, k)
trace entries at rtol 1e-8 (tests/test_shifted.py): only the association of the dot sums differs from the oracle, whose own
scalars of the first six iterations move by at most 6.2e-12 between 1 and 8 virtual ranks on these inputs. Everything else is
compared BIT FOR BIT, as bytes: the order of a column's dot sums depends on the number of rows only and every SpMM column is
bit-identical to bicg_spmv, so a column does not know how many columns run beside it, where it stands in its set, which SpMM
kernel multiplied it, or how often the host looked.

Shapes: stencil7(12), 1 728 rows -- the columns stop at three or more different iterations; 5-7 diagonals on 30 011 rows -- not a
multiple of 64, the pipelined SpMM, 21 = 16 + 5 columns; a dense band on 4 099 rows whose rows go to the rows-over-lanes kernel, where
bicg_spmm does not exist and every column takes the per-column product; n = 1 .. 257 for the odd tail and the single workgroup."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-12


def _context(A, **sw):
    """a context created under the given tokens; the tokens are cleared again whatever happens"""
    H.switches(**sw)
    try:
        return H.Context(H.single_rank_blocks(A))
    finally:
        H.switches(**{k: None for k in sw})


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def solutions(n, nrhs):
    """x*_j, j < nrhs"""
    rng = np.random.default_rng(7)
    xs = np.zeros((nrhs, n))
    for j in range(nrhs):
        if j == 0:
            xs[j] = 1.0
        elif j == 2:
            xs[j, n // 2] = 1.0
        elif j == 3:
            xs[j, :n // 3] = 1.0
        elif j >= 4:
            xs[j] = 0.5 + rng.random(n)
    return xs


def _matrix(name):
    if name == "stencil12":
        return synth.stencil7(12)
    if name == "offsets30011":
        return synth.from_offsets(30011, (0, 1, -1, 37, -37, 2999, -2999), diag_base=9.0, seed=5)
    if name == "band4099":
        return synth.banded(4099, 200)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name, nrhs, tol=TOL):
    """(A, x* [nrhs][n], B [nrhs][n], the oracle's solve of every column) -- computed once, never written to"""
    A = _matrix(name) if isinstance(name, str) else synth.from_offsets(name, (0, 1, -1, 3, -3), diag_base=5.0, seed=name)
    row, col, val = A.to_coo()
    xs = solutions(A.rows, nrhs)
    B = np.array([O.spmv(A.rows, row, col, val, x) for x in xs])
    orc = [O.solve("bicgstab", A.rows, row, col, val, b, tol=tol) for b in B]
    for a in (xs, B):
        a.setflags(write=False)
    return A, xs, B, orc


def column_state(ctx, got, j):
    """everything bicg_solve_multi reports about column j, as bytes"""
    q = got["results"][j]
    tr = ctx.multi_trace(j, int(got["k"][j]))
    return (int(got["k"][j]), q.iterations, q.breakdown_iteration, np.float64(q.dot_r).tobytes(), np.float64(q.dot_zero).tobytes(),
            got["x"][j].tobytes(), got["r"][j].tobytes(), tuple(tr[k].tobytes() for k in ("alpha", "omega", "beta", "dotr")))


def whole_state(ctx, got):
    return [column_state(ctx, got, j) for j in range(len(got["k"]))]


def assert_oracle_bars(ctx, got, xs, orc, what):
    for j, o in enumerate(orc):
        k = int(got["k"][j])
        print(what, "column", j, "k", k, "oracle", o["k"], "err", np.abs(got["x"][j] - xs[j]).max())
        assert abs(k - o["k"]) <= 2, (what, j, k, o["k"])
        assert np.abs(got["x"][j] - xs[j]).max() <= 1e-9, (what, j)
        tr = ctx.multi_trace(j, k)
        m = min(6, k, o["k"])
        for name in ("alpha", "omega", "beta", "dotr"):
            assert np.allclose(tr[name][:m], o[name][:m], rtol=1e-8, atol=0.0), (what, j, name, tr[name][:m], o[name][:m])


@pytest.fixture(scope="module", params=[("stencil12", 16), ("offsets30011", 21)], ids=lambda p: "%s-%d" % p)
def full(request):
    """(name, A, x*, B, oracle, context, the nrhs-column solve with its trace)"""
    H.lib().bicg_comm_init_single(0)
    name, nrhs = request.param
    A, xs, B, orc = case(name, nrhs)
    ctx = H.Context(H.single_rank_blocks(A))
    got = ctx.solve_multi(B, tol=TOL, record_trace=1)
    state = whole_state(ctx, got)
    yield name, A, xs, B, orc, ctx, got, state
    ctx.close()


# ---- 1. against the oracle
def test_against_the_oracle(full):
    name, A, xs, B, orc, ctx, got, state = full
    ks = [o["k"] for o in orc]
    if name == "stencil12":
        assert A.rows == 1728 and len(set(ks)) >= 3, ks         # the columns stop at different iterations
    else:
        assert A.rows == 30011 and A.rows % 64 != 0 and len(ks) == 21
        assert ctx.flags()["spmm"] and ctx.last_spmm_kind() == "pipelined"
    assert got["rc"] == max(got["k"])
    got = ctx.solve_multi(B, tol=TOL, record_trace=1)           # (multi_trace reads the LAST call's record) ...
    assert whole_state(ctx, got) == state                       # ... and a second run gives the bits of the first
    assert_oracle_bars(ctx, got, xs, orc, name)
    assert got["results"][1].iterations == 0 and got["k"][1] == 0
    assert got["x"][1].tobytes() == np.zeros(A.rows).tobytes()
    for q in got["results"]:
        assert q.breakdown_iteration == 0 and q.seconds > 0.0 and q.seconds == got["results"][0].seconds


# ---- 2. columns are independent and frozen exactly
def test_a_column_does_not_know_its_neighbours(full):
    name, A, xs, B, orc, ctx, got, state = full
    ks = got["k"]
    running = [j for j in range(len(ks)) if ks[j] > 0]
    fast, slow = min(running, key=lambda j: ks[j]), max(running, key=lambda j: ks[j])
    cols = {fast, slow, 1}
    if len(ks) > 16:
        cols.add(18)                                            # a column of the second set
    assert ks[fast] < ks[slow] or name != "stencil12"
    for j in sorted(cols):
        one = ctx.solve_multi(B[j:j + 1], tol=TOL, record_trace=1)
        assert column_state(ctx, one, 0) == state[j], (name, j)


def test_sixteen_identical_right_hand_sides(full):
    name, A, xs, B, orc, ctx, got, state = full
    same = ctx.solve_multi(np.tile(B[4], (16, 1)), tol=TOL, record_trace=1)
    cols = whole_state(ctx, same)
    assert cols[0] == state[4], name
    assert all(c == cols[0] for c in cols), name


# ---- 3. the three SpMM forms and the per-column product agree
def test_spmm_forms_and_per_column_product_agree():
    H.lib().bicg_comm_init_single(0)
    A, xs, B, orc = case("offsets30011", 21)
    ctx = H.Context(H.single_rank_blocks(A))
    try:
        state = whole_state(ctx, ctx.solve_multi(B, tol=TOL, record_trace=1))
        _spmm_forms(A, B, ctx, state)
    finally:
        ctx.close()


def _spmm_forms(A, B, ctx, state):
    for window, kind in ((0, "rowmajor"), (1, "windowed")):
        H.switches(spmm_window=window)                          # read when the context's SpMM buffers are made: its first product
        try:
            other = H.Context(H.single_rank_blocks(A))
            res = other.solve_multi(B, tol=TOL, record_trace=1)
        finally:
            H.switches(spmm_window=None)
        try:
            assert other.last_spmm_kind() == kind
            assert whole_state(other, res) == state, kind
        finally:
            other.close()
    assert ctx.last_spmm_kind() == "pipelined"
    H.switches(spmm=0)                                          # read at the call: one product per active column
    try:
        res = ctx.solve_multi(B, tol=TOL, record_trace=1)
    finally:
        H.switches(spmm=None)
    assert whole_state(ctx, res) == state, "spmm=0"


def test_rows_on_the_csr_kernels_take_the_per_column_product():
    """a dense band of 401 entries per row: the plan spreads every row over several lanes (bicg_sell_plan_digest: rowsplit, all
    rows in CSR row blocks), bicg_spmm does not exist for the context and every product is one bicg_spmv-style launch per active
    column -- with that kernel's own rounding of a row sum (1e-13 relative, BICG_FLAG_ROWSPLIT), far inside the bars"""
    H.lib().bicg_comm_init_single(0)
    A, xs, B, orc = case("band4099", 5)
    summary, _ = H.sell_plan_digest(H.single_rank_blocks(A))
    assert summary["rowsplit"] or summary["nblk"], summary
    ctx = H.Context(H.single_rank_blocks(A))
    try:
        assert not ctx.flags()["spmm"]
        got = ctx.solve_multi(B, tol=TOL, record_trace=1)
        assert_oracle_bars(ctx, got, xs, orc, "band4099")
        assert got["k"][1] == 0 and not got["x"][1].any()
    finally:
        ctx.close()


# ---- 4. edges
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_tiny_and_odd_sizes(n):
    H.lib().bicg_comm_init_single(0)
    A, xs, B, orc = case(n, 17, 1e-13)
    ctx = H.Context(H.single_rank_blocks(A))
    try:
        for nrhs in (1, 3, 16, 17):
            got = ctx.solve_multi(B[:nrhs], tol=1e-13)
            assert len(got["k"]) == nrhs
            for j in range(nrhs):
                o = orc[j]
                assert abs(got["k"][j] - o["k"]) <= 2, (n, nrhs, j, got["k"][j], o["k"])
                if np.isfinite(o["x"]).all():
                    assert np.abs(got["x"][j] - xs[j]).max() <= 1e-9, (n, nrhs, j)
                else:
                    # n = 1: q = r - alpha s is exactly 0 after one step, omega = 0/0 -- the reference returns NaN there
                    assert got["k"][j] == o["k"] and np.array_equal(np.isnan(got["x"][j]), np.isnan(o["x"])), (n, nrhs, j)
    finally:
        ctx.close()


def test_zero_iterations_initial_guess_and_check_interval():
    H.lib().bicg_comm_init_single(0)
    A, xs, B, orc = case("stencil12", 16)
    row, col, val = A.to_coo()
    ctx = H.Context(H.single_rank_blocks(A))
    try:
        nrhs = 5
        X0 = np.array([np.linspace(-1.0, 1.0 + j, A.rows) for j in range(nrhs)])
        got = ctx.solve_multi(B[:nrhs], X0=X0, max_iter=0)                   # set-up only: r = b - A x0 (src/solver.c:74-75)
        assert got["rc"] == 0 and not got["k"].any()
        assert same_bits(got["x"], X0)
        assert same_bits(got["r"], np.array([B[j] - O.spmv(A.rows, row, col, val, X0[j]) for j in range(nrhs)]))
        got = ctx.solve_multi(B[:nrhs], X0=X0, tol=TOL)                      # a non-zero guess converges to x*
        for j in range(nrhs):
            o = O.solve("bicgstab", A.rows, row, col, val, B[j], x0=X0[j], tol=TOL)
            assert abs(got["k"][j] - o["k"]) <= 2, (j, got["k"][j], o["k"])
            assert np.abs(got["x"][j] - xs[j]).max() <= 1e-9, j
        a = ctx.solve_multi(B, tol=TOL, record_trace=1, check_every=1)
        sa = whole_state(ctx, a)
        b = ctx.solve_multi(B, tol=TOL, record_trace=1, check_every=7)
        assert whole_state(ctx, b) == sa
        capped = ctx.solve_multi(B, tol=TOL, max_iter=7, check_every=16)     # every running column stops inside the interval
        assert [int(k) for k in capped["k"]] == [0 if j == 1 else 7 for j in range(16)]
        assert ctx.multi_trace(0, 7) is None                                 # nothing recorded by the last call
    finally:
        ctx.close()


# ---- 5. a reordered context
def test_reordered_context_keeps_the_callers_numbering():
    H.lib().bicg_comm_init_single(0)
    A, xs, B, orc = case("stencil12", 16)
    ctx = _context(A, reorder=1)
    try:
        assert ctx.flags()["reordered"]
        got = ctx.solve_multi(B, tol=TOL, record_trace=1)
        assert_oracle_bars(ctx, got, xs, orc, "reordered")
        state = whole_state(ctx, got)
        for j in (0, 1, 9):
            one = ctx.solve_multi(B[j:j + 1], tol=TOL, record_trace=1)
            assert column_state(ctx, one, 0) == state[j], j
    finally:
        ctx.close()


# ---- 6. refusals
def test_refusals_touch_nothing():
    H.lib().bicg_comm_init_single(0)
    A, xs, B, orc = case("stencil12", 16)
    ctx = H.Context(H.single_rank_blocks(A))
    try:
        X0 = np.full((3, A.rows), 0.25)
        for method in ("ca_bicgstab", "pipe_bicgstab", "pipe_bicgstab_rr"):
            got = ctx.solve_multi(B[:3], X0=X0, method=method, tol=TOL)
            assert got["rc"] == -2
            assert same_bits(got["x"], X0) and same_bits(got["r"], B[:3])
        assert ctx.solve_multi(np.zeros((0, A.rows)))["rc"] == -2
        assert ctx.multi_trace(0, 1) is None and H.lib().bicg_multi_trace(ctx.h, 99, None, None, None, None) != 0
    finally:
        ctx.close()


# ---- 7. no leak
def test_contexts_do_not_leak_device_memory():
    import torch
    H.lib().bicg_comm_init_single(0)
    A, xs, B, orc = case("offsets30011", 21)

    def cycle():
        ctx = H.Context(H.single_rank_blocks(A))
        ctx.solve_multi(B[:17], tol=TOL, max_iter=4, record_trace=1)
        ctx.close()
    cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(4):
        cycle()
    torch.cuda.synchronize()
    assert abs(torch.cuda.mem_get_info()[0] - free0) < 8 * 1024 * 1024
