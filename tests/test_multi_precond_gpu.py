"""`-m gpu`, one rank: bicg_solve_multi / bicg_solve_multi_device with the right-preconditioned methods 4 (BICG_BICGSTAB_DIAG) and
5 (BICG_BICGSTAB_BLOCK) -- csrc/bicg_multi.cpp, the MV_*_D / MV_XR_H phases of csrc/bicg_multi.hip, k_bjac_apply_set of
csrc/bicg_bjacobi.hip; DESIGN.md section 4.22. Contexts as in tests/test_precond_gpu.py, always under switches(persist=0).

Everything but section F is compared BIT FOR BIT, as bytes, and rests on three facts: multiplying by 1.0 or a power of two is exact;
every dot of the multi path is an element-wise pass of its own whose order of summation depends on the number of rows only; every
column of an SpMM is bit-identical to bicg_spmv of that column.
  A. d = 1, and identity blocks of bs = 1, 3, 4, 16, reproduce the plain multi call on the same context and inputs.
  B. d = powers of two: method 4 on A is the plain multi call on A D^-1 (x0 scaled), x up to the scaling.
  C. method 5 with bs = 1, and with blocks that hold d on their diagonals (bs = 3, 4, 16), is method 4 with that d.
  D. column j of a preconditioned call is the one-column call on (x0_j, b_j) whatever the number of columns, its place in the set,
     check_every, spmm=0, the SpMM kernel, host or device arrays.
  E. (across ranks: tests/test_multi_precond_ranks_gpu.py)
  F. convergence on badly scaled systems where the plain multi call does not converge, against the single-RHS solve of the same
     method: |k_j - k_single_j| <= 2 (the project's bar wherever only the association of the dot sums differs) and a true relative
     residual ||b - A x_j|| / ||b|| of at most twice the single-RHS solve's (both stop on the same test; the room of one iteration).
Shapes of A, B, D: stencil7(12) with 16 columns (the columns stop at different iterations, b = 0 has k = 0); 5-7 diagonals on 30 011
rows with 21 = 16 + 5 columns (not a multiple of 64, the pipelined SpMM, a partial second set); a dense band on 4 099 rows with 3
columns (rows on the rows-over-lanes kernel: per-column products); transport_like(n), n = 1, 2, 63, 65, 257 with 5 columns (a single
workgroup, the odd pair tail, below a wavefront; n = 1 and n = 2 are solved exactly within n iterations and break down on the next
quotient, 0 / 0, in the plain call as well: they are compared with every NaN canonical, as tests/test_precond_gpu.py does)."""
import numpy as np
import pytest
import torch

import test_precond_gpu as P
from test_block_precond_gpu import diagonal_blocks, skew_blocks
from test_multi_rhs_gpu import column_state, solutions, whole_state
from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import synth

pytestmark = pytest.mark.gpu
raw, context = P.raw, P.context

SHAPES = {"stencil12": 16, "offsets30011": 21, "band4099": 3, "transport_1": 5, "transport_2": 5, "transport_63": 5, "transport_65": 5,
          "transport_257": 5}
BREAKS_DOWN = ("transport_1", "transport_2")      # an n x n system is solved exactly by iteration n: the next quotient is 0 / 0
OPTS = dict(tol=1e-12, max_iter=40, record_trace=1)
FIXED = dict(tol=0.0, max_iter=12, record_trace=1)
REAL = dict(tol=1e-10, max_iter=1000)


@pytest.fixture(scope="module", autouse=True)
def single_rank():
    """once for the module: a second bicg_comm_init_single would orphan the contexts the fixtures below keep"""
    H.lib().bicg_comm_init_single(0)


def identity_blocks(n, bs):
    return diagonal_blocks(np.ones(n), bs)


def shape_matrix(name):
    if name == "stencil12":
        return synth.stencil7(12)
    if name == "offsets30011":
        return synth.from_offsets(30011, (0, 1, -1, 37, -37, 2999, -2999), diag_base=9.0, seed=5)
    if name == "band4099":
        return synth.banded(4099, 200)
    return synth.transport_like(int(name.split("_")[1]))


def start_vectors(n, nrhs, seed=90):
    """x0_j without a zero entry, but x0_1 = 0 (with b_1 = 0: the column that never starts)"""
    idx = np.arange(n, dtype=np.int64)
    X0 = np.array([0.25 * synth._uniform(idx, seed + j) - 0.125 for j in range(nrhs)])
    if nrhs > 1:
        X0[1] = 0.0
    return X0


class Case:
    """a shape's matrix, right-hand sides b_j = A x*_j (solutions() of tests/test_multi_rhs_gpu.py), start vectors, powers of two, its
    context and, when asked for, the context of A D^-1 -- made once, never written to"""

    def __init__(self, name):
        self.name, self.A, self.nrhs = name, shape_matrix(name), SHAPES[name]
        n = self.A.rows
        self.B = np.array([self.A.matvec(x) for x in solutions(n, self.nrhs)])
        self.X0 = start_vectors(n, self.nrhs)
        self.d = P.powers_of_two(n)
        for a in (self.B, self.X0, self.d):
            a.setflags(write=False)
        self.nan_ok = name in BREAKS_DOWN
        self.ctx = context(self.A)
        self.ctx_b = None

    def scaled_context(self):
        if self.ctx_b is None:
            self.ctx_b = context(P.scaled_columns(self.A, self.d))
        return self.ctx_b

    def close(self):
        for c in (self.ctx, self.ctx_b):
            if c is not None:
                c.close()


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name)
        return made[name]
    yield get
    for c in made.values():
        c.close()


def nan_column_state(ctx, got, j):
    """column_state with every NaN canonical (BREAKS_DOWN only: the sign and payload of an invalid operation's result are undefined)"""
    q, k = got["results"][j], int(got["k"][j])
    tr = ctx.multi_trace(j, k)
    return (k, q.iterations, q.breakdown_iteration, raw(q.dot_r, True), raw(q.dot_zero, True), raw(got["x"][j], True), raw(got["r"][j], True),
            tuple(raw(tr[key], True) for key in ("alpha", "omega", "beta", "dotr")))


def states(ctx, got, nan_ok=False, with_x=True):
    """everything a multi call reports, per column, as bytes; with_x=False: all of it but x"""
    assert got["rc"] >= 0, got["rc"]
    if nan_ok:
        out = [nan_column_state(ctx, got, j) for j in range(len(got["k"]))]
    else:
        assert not np.isnan(got["x"]).any() and not np.isnan(got["r"]).any(), "a NaN in what a solve reports"
        out = whole_state(ctx, got)
    return out if with_x else [s[:5] + s[6:] for s in out]


# ---------------------------------------------------------------- A. identity preconditioners
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_identity_preconditioners_reproduce_the_plain_call(cases, name):
    c = cases(name)
    ctx, n = c.ctx, c.A.rows
    plain = ctx.solve_multi(c.B, X0=c.X0, **OPTS)
    want = states(ctx, plain, c.nan_ok)
    ks = [int(k) for k in plain["k"]]
    print(name, "k per column", ks)
    assert ks[1] == 0 and max(ks) >= 1
    if name == "stencil12":
        assert len(set(ks)) >= 3, ks                       # the columns stop at different iterations
    if name == "offsets30011":
        assert ctx.flags()["spmm"] and ctx.last_spmm_kind() == "pipelined" and n % 64 != 0
    if name == "band4099":
        assert not ctx.flags()["spmm"]
    assert ctx.set_diagonal(np.ones(n)) == 0
    assert states(ctx, ctx.solve_multi(c.B, X0=c.X0, method="bicgstab_diag", **OPTS), c.nan_ok) == want, "d = 1"
    for bs in (1, 3, 4, 16):
        assert ctx.set_block_diagonal(identity_blocks(n, bs), bs) == 0
        assert states(ctx, ctx.solve_multi(c.B, X0=c.X0, method="bicgstab_block", **OPTS), c.nan_ok) == want, f"identity blocks, bs = {bs}"
    # ... and the plain call is what it was with the preconditioner installed and the hat sets allocated
    assert states(ctx, ctx.solve_multi(c.B, X0=c.X0, **OPTS), c.nan_ok) == want
    ctx.clear_preconditioner()


# ---------------------------------------------------------------- B. powers of two
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_power_of_two_diagonal_is_the_plain_call_on_the_scaled_columns(cases, name):
    c = cases(name)
    ca, cb = c.ctx, c.scaled_context()
    assert ca.flags() == cb.flags() and ca.plan_info() == cb.plan_info()      # void unless both matrices got the same plan and kernel
    masks = []
    for ctx in (ca, cb):
        H.product_kernels(reset=True)
        ctx.spmv(c.X0[0])
        masks.append(H.product_kernels(reset=True))
    assert masks[0] == masks[1] and masks[0]
    assert ca.set_diagonal(c.d) == 0
    got = ca.solve_multi(c.B, X0=c.X0, method="bicgstab_diag", **OPTS)
    want = cb.solve_multi(c.B, X0=c.d * c.X0, **OPTS)
    assert max(int(k) for k in got["k"]) >= 1 and int(got["k"][1]) == 0
    assert states(ca, got, c.nan_ok, with_x=False) == states(cb, want, c.nan_ok, with_x=False)
    assert raw(got["x"], c.nan_ok) == raw(want["x"] / c.d, c.nan_ok)
    ca.clear_preconditioner()


# ---------------------------------------------------------------- C. method 5 against method 4
def columns_without_zeros(A, nrhs=5):
    idx = np.arange(A.rows, dtype=np.int64)
    B = np.array([A.matvec(1.0 + 0.5 * synth._uniform(idx, 80 + j)) for j in range(nrhs)])
    X0 = np.array([0.25 * synth._uniform(idx, 90 + j) - 0.125 for j in range(nrhs)])
    assert np.all(B != 0.0) and np.all(X0 != 0.0)
    return B, X0


@pytest.fixture(scope="module")
def bundles():
    made = {}

    def get(name):
        if name not in made:
            b = P.Bundle(name)
            b.B, b.X0 = columns_without_zeros(b.A)
            assert b.ctx.set_diagonal(b.d) == 0
            b.diag_want = states(b.ctx, b.ctx.solve_multi(b.B, X0=b.X0, method="bicgstab_diag", **FIXED))
            assert all(1 <= s[0] <= 12 for s in b.diag_want)
            made[name] = b
        return made[name]
    yield get
    for b in made.values():
        b.close()


@pytest.mark.parametrize("bs", [1, 3, 4, 16])
@pytest.mark.parametrize("name", ["transport_4099", "fem_4099", "fem_4099_reordered"])
def test_diagonal_blocks_are_method_four_bit_for_bit(bundles, name, bs):
    b = bundles(name)
    assert b.ctx.flags()["reordered"] == name.endswith("_reordered")      # ... which runs the RO form of the set kernel
    blocks = b.d if bs == 1 else diagonal_blocks(b.d, bs)
    assert b.ctx.set_block_diagonal(blocks, bs) == 0 and b.ctx.preconditioner() == "block_diagonal"
    got = states(b.ctx, b.ctx.solve_multi(b.B, X0=b.X0, method="bicgstab_block", **FIXED))
    assert got == b.diag_want


# ---------------------------------------------------------------- partial last block, frozen columns, against k_bjac_apply
def one_iteration_by_hand(ctx, b, x0, alpha, omega):
    """the first iteration with the context's own product (bicg_spmv: the bytes of an SpMM column) and its SINGLE application
    (bicg_precond_apply, k_bjac_apply), the element-wise phases in numpy with csrc/bicg_multi.hip's roundings, alpha and omega as the
    call reported them: (x, r)"""
    r = b + (-1.0) * ctx.spmv(x0)
    ph = ctx.apply_preconditioner(r)                     # p = r
    q = r + (-alpha) * ctx.spmv(ph)
    qh = ctx.apply_preconditioner(q)
    y = ctx.spmv(qh)
    x = (x0 + alpha * ph) + omega * qh
    return x, q + (-omega) * y


@pytest.mark.parametrize("bs", [16, 3])
def test_partial_last_block_and_columns_frozen_from_the_start(bundles, bs):
    b = bundles("transport_4099")
    ctx, n = b.ctx, b.A.rows
    assert n == 4099 and n % bs != 0
    assert ctx.set_block_diagonal(skew_blocks(n, bs), bs) == 0
    B, X0 = np.array(b.B), np.array(b.X0)
    for j in (1, 3):                                      # b = 0 and x0 = 0: r = 0, never active
        B[j] = 0.0; X0[j] = 0.0
    once = dict(method="bicgstab_block", tol=0.0, max_iter=1, record_trace=1)
    got = ctx.solve_multi(B, X0=X0, **once)
    whole = states(ctx, got)
    scalars = {j: ctx.multi_trace(j, 1) for j in (0, 2, 4)}
    assert [int(k) for k in got["k"]] == [1, 0, 1, 0, 1]
    for j in (1, 3):
        assert got["x"][j].tobytes() == X0[j].tobytes() and got["r"][j].tobytes() == B[j].tobytes()
    for j in (0, 2, 4):
        x, r = one_iteration_by_hand(ctx, B[j], X0[j], scalars[j]["alpha"][0], scalars[j]["omega"][0])
        assert got["x"][j].tobytes() == x.tobytes(), (bs, j)
        assert got["r"][j].tobytes() == r.tobytes(), (bs, j)
        one = ctx.solve_multi(B[j:j + 1], X0=X0[j:j + 1], **once)
        assert column_state(ctx, one, 0) == whole[j], (bs, j)


# ---------------------------------------------------------------- D. column independence
def install(ctx, A, method):
    """a real preconditioner from the matrix itself: diag(A), or its 4 x 4 diagonal blocks"""
    if method == "bicgstab_diag":
        d, missing = H.csr_diagonal(A)
        assert missing == 0 and ctx.set_diagonal(d) == 0
    else:
        blocks, missing = H.csr_block_diagonal(A, 4)
        assert missing == 0 and ctx.set_block_diagonal(blocks, 4) == 0


def device_call(ctx, B, X0, method, pad, **kw):
    """the call on CUDA tensors, in place, rows pad doubles longer than n: the dict of the host call"""
    nrhs, n = B.shape
    xs = torch.full((nrhs, n + pad), float("nan"), dtype=torch.float64, device="cuda")
    rs = torch.full((nrhs, n + pad), float("nan"), dtype=torch.float64, device="cuda")
    xs[:, :n] = torch.from_numpy(np.array(X0)).cuda()
    rs[:, :n] = torch.from_numpy(np.array(B)).cuda()
    got = ctx.solve_multi(rs[:, :n], X0=xs[:, :n], method=method, inplace=True, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(xs[:, n:]).all() and torch.isnan(rs[:, n:]).all()      # nothing written behind a row
    got["x"], got["r"] = xs[:, :n].cpu().numpy().copy(), rs[:, :n].cpu().numpy().copy()
    return got


@pytest.mark.parametrize("method", ["bicgstab_diag", "bicgstab_block"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_a_column_does_not_know_its_neighbours(cases, name, method):
    c = cases(name)
    ctx, nrhs = c.ctx, c.nrhs
    install(ctx, c.A, method)
    solve = lambda B, X0, **kw: ctx.solve_multi(B, X0=X0, method=method, **dict(OPTS, **kw))
    whole = states(ctx, solve(c.B, c.X0), c.nan_ok)
    ks = [s[0] for s in whole]
    print(name, method, "k per column", ks)
    assert ks[1] == 0 and max(ks) >= 1
    alone = {0, 1, 2, nrhs - 1} | ({18} if nrhs > 16 else set())
    for j in sorted(alone):                               # the number of columns; a frozen column holds its own one-column solve
        assert states(ctx, solve(c.B[j:j + 1], c.X0[j:j + 1]), c.nan_ok)[0] == whole[j], (name, j)
    assert states(ctx, solve(c.B[2:], c.X0[2:]), c.nan_ok) == whole[2:], "place in the set"
    assert states(ctx, solve(c.B, c.X0, check_every=7), c.nan_ok) == whole, "check_every"
    H.switches(spmm=0)                                    # read at the call
    try:
        assert states(ctx, solve(c.B, c.X0), c.nan_ok) == whole, "spmm=0"
    finally:
        H.switches(spmm=None)
    assert states(ctx, device_call(ctx, c.B, c.X0, method, 5, **OPTS), c.nan_ok) == whole, "device arrays, ld = n + 5"
    if name == "offsets30011":                            # the other two SpMM kernels
        for window, kind in ((0, "rowmajor"), (1, "windowed")):
            H.switches(spmm_window=window)                # read when the context's SpMM buffers are made: its first product
            try:
                other = context(c.A)
                install(other, c.A, method)
                res = other.solve_multi(c.B, X0=c.X0, method=method, **OPTS)
            finally:
                H.switches(spmm_window=None)
            try:
                assert other.last_spmm_kind() == kind
                assert states(other, res) == whole, kind
            finally:
                other.close()
    ctx.clear_preconditioner()


# ---------------------------------------------------------------- F. where the plain multi call does not converge
def true_residuals(A, X, B):
    return np.array([P.relres(A, x, b) for x, b in zip(X, B)])


def check_convergence(A, method, installer, what):
    idx = np.arange(A.rows, dtype=np.int64)
    B = np.array([A.matvec(np.ones(A.rows) if j == 0 else 1.0 + 0.5 * synth._uniform(idx, 60 + j)) for j in range(5)])
    ctx = context(A)
    try:
        plain = ctx.solve_multi(B, **REAL)
        print(what, "plain multi k", [int(k) for k in plain["k"]])
        assert int(plain["k"][0]) == 1000                  # b = A 1: the system the README's figures are about
        installer(ctx)
        got = ctx.solve_multi(B, method=method, **REAL)
        single = [ctx.solve(method, b, **REAL) for b in B]
        res, res_1 = true_residuals(A, got["x"], B), true_residuals(A, [s["x"] for s in single], B)
        for j in range(len(B)):
            print(f"{what} column {j}: k = {int(got['k'][j])} (single-RHS {single[j]['k']}), true relative residual {res[j]:.3e} "
                  f"(single-RHS {res_1[j]:.3e}, ratio {res[j] / res_1[j]:.3f})")
        for j in range(len(B)):
            assert 1 <= single[j]["k"] <= 20 and abs(int(got["k"][j]) - single[j]["k"]) <= 2, (what, j)
            assert res[j] <= 2.0 * res_1[j], (what, j, res[j], res_1[j])
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["transport", "fem"])
def test_block_jacobi_set_converges_on_coupled_blocks(kind):
    gen = synth.transport_like if kind == "transport" else synth.fem_like
    A = synth.block_coupled(20000, 4, gen, scale_decades=4.0)
    blocks, _ = H.csr_block_diagonal(A, 4)
    check_convergence(A, "bicgstab_block", lambda ctx: ctx.set_block_diagonal(blocks, 4) == 0 or pytest.fail("install"), f"block_coupled {kind}")


@pytest.mark.parametrize("kind", ["transport", "fem"])
def test_jacobi_set_converges_on_badly_scaled_matrices(kind):
    gen = synth.transport_like if kind == "transport" else synth.fem_like
    A = gen(20000, scale_decades=4)
    d, missing = H.csr_diagonal(A)
    assert missing == 0
    check_convergence(A, "bicgstab_diag", lambda ctx: ctx.set_diagonal(d) == 0 or pytest.fail("install"), f"scaled {kind}")


# ---------------------------------------------------------------- interface
@pytest.fixture(scope="module")
def fem():
    A = synth.fem_like(4099, scale_decades=2)
    B, X0 = columns_without_zeros(A, 3)
    for a in (B, X0):
        a.setflags(write=False)
    return A, B, X0


def test_refusals_touch_nothing_and_allocate_nothing(fem):
    A, B, X0 = fem
    ctx = context(A)
    try:
        d = H.csr_diagonal(A)[0]
        before = H.device_allocations()

        def refused(method):
            got = ctx.solve_multi(B, X0=X0, method=method, record_trace=1, **REAL)
            assert got["rc"] == -2 and got["x"].tobytes() == X0.tobytes() and got["r"].tobytes() == B.tobytes(), method
            tb, tx = torch.from_numpy(np.array(B)).cuda(), torch.from_numpy(np.array(X0)).cuda()
            got = ctx.solve_multi(tb, X0=tx, method=method, inplace=True, **REAL)
            assert got["rc"] == -2 and tx.cpu().numpy().tobytes() == X0.tobytes() and tb.cpu().numpy().tobytes() == B.tobytes(), method
            assert ctx.multi_trace(0, 1) is None
        for method in ("bicgstab_diag", "bicgstab_block"):      # no preconditioner
            refused(method)
        assert H.device_allocations() == before
        assert ctx.set_diagonal(d) == 0
        held = H.device_allocations()
        refused("bicgstab_block")                               # the other kind
        assert ctx.set_block_diagonal(d, 1) == 0 and H.device_allocations() == held
        refused("bicgstab_diag")
        for method in ("ca_bicgstab", "pipe_bicgstab", "pipe_bicgstab_rr"):
            refused(method)
        assert H.device_allocations() == held
        assert ctx.solve_multi(B, X0=X0, method="bicgstab_block", **REAL)["rc"] >= 1
    finally:
        ctx.close()


def test_one_allocation_more_and_none_later(fem):
    A, B, X0 = fem
    torch.cuda.synchronize()
    before_create = H.device_allocations()
    ctx = context(A)
    try:
        opts = dict(record_trace=1, **REAL)
        assert ctx.set_diagonal(H.csr_diagonal(A)[0]) == 0
        ctx.solve_multi(B, X0=X0, **opts)
        plain = H.device_allocations()
        ctx.solve_multi(B, X0=X0, method="bicgstab_diag", **opts)
        assert H.device_allocations() == plain + 1              # the two hat sets
        ctx.solve_multi(B, X0=X0, **opts)
        ctx.solve_multi(B, X0=X0, method="bicgstab_diag", **opts)
        assert H.device_allocations() == plain + 1
        assert ctx.set_block_diagonal(H.csr_block_diagonal(A, 4)[0], 4) == 0      # (the planes replace 1 / d: one freed, one made)
        assert H.device_allocations() == plain + 1
        ctx.solve_multi(B, X0=X0, method="bicgstab_block", **opts)
        ctx.solve_multi(B, X0=X0, **opts)
        assert H.device_allocations() == plain + 1
    finally:
        ctx.close()
    assert H.device_allocations() == before_create


def test_a_replaced_diagonal_is_used_as_installed_at_the_call(fem):
    A, B, X0 = fem
    d1 = H.csr_diagonal(A)[0]
    d2 = d1 * (1.0 + synth._uniform(np.arange(A.rows, dtype=np.int64), 13))
    ctx = context(A)
    try:
        seen = {}
        for key, d in (("d1", d1), ("d2", d2), ("again", d1)):
            assert ctx.set_diagonal(d) == 0
            got = ctx.solve_multi(B, X0=X0, method="bicgstab_diag", record_trace=1, **REAL)
            seen[key] = states(ctx, got)
            alphas = [ctx.multi_trace(j, int(got["k"][j]))["alpha"] for j in range(len(B))]
            for j, (b, x0) in enumerate(zip(B, X0)):            # the single-RHS method follows the diagonal in the same way
                single = ctx.solve("bicgstab_diag", b, x0=x0, record_trace=1, **REAL)
                assert 1 <= single["k"] < 1000 and abs(int(got["k"][j]) - single["k"]) <= 2, (key, j)
                m = min(4, single["k"], int(got["k"][j]))
                np.testing.assert_allclose(alphas[j][:m], ctx.trace(single["k"])["alpha"][:m], rtol=1e-9, atol=0.0)
        assert seen["d1"] != seen["d2"] and seen["again"] == seen["d1"]
    finally:
        ctx.close()


def test_device_arrays_with_a_padded_leading_dimension_equal_the_host_call(fem):
    A, B, X0 = fem
    ctx = context(A)
    try:
        for method in ("bicgstab_diag", "bicgstab_block"):
            install(ctx, A, method)
            want = states(ctx, ctx.solve_multi(B, X0=X0, method=method, record_trace=1, **REAL))
            assert all(1 <= s[0] < 1000 for s in want)
            assert states(ctx, device_call(ctx, B, X0, method, 29, record_trace=1, **REAL)) == want
    finally:
        ctx.close()
