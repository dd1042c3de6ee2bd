"""`-m gpu`, one rank: the block-Jacobi preconditioner and BICG_BICGSTAB_BLOCK (bicg_precond_block_diagonal, bicg_precond_apply,
Driver::iter_plain, csrc/bicg_bjacobi.hip) through Context.set_block_diagonal / apply_preconditioner /
solve("bicgstab_block"). Contexts as in tests/test_precond_gpu.py, whose matrices, bundles and byte comparisons are reused: always
under switches(persist=0).

  1. the operator alone, on blocks whose inverse and product are exact (bytes) and on well-conditioned real blocks (1e-12);
  2. bs = 1 is method 4, bit for bit;  3. diagonal blocks of bs = 3, 4, 16 are method 4, bit for bit;
  4. real blocks: convergence against a numpy restatement, and against the plain and the point-Jacobi method;
  5. the interface: refusals, allocations, kinds, update_values, streams, tensors, graph replay, the drop-in symbol."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_precond_gpu as P
from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import synth

pytestmark = pytest.mark.gpu
ROOT = P.ROOT
FIXED, REAL = P.FIXED, P.REAL
state, raw, context = P.state, P.raw, P.context

LAYOUTS = ("transport_63", "transport_4099", "transport_40000", "fem_4099", "fem_40000", "grid7", P.PLANES, "fem_4099_reordered")


@pytest.fixture(scope="module", autouse=True)
def single_rank():
    """once for the module: a second bicg_comm_init_single would orphan the contexts the fixtures below keep"""
    H.lib().bicg_comm_init_single(0)


@pytest.fixture(scope="module")
def bundles():
    made = {}

    def get(name):
        if name not in made:
            made[name] = P.Bundle(name)
        return made[name]
    yield get
    for b in made.values():
        b.close()


# ---------------------------------------------------------------- block builders (caller's layout: [nb, bs, bs])
def block_rows(n, bs):
    """rows each block covers"""
    nb = -(-n // bs)
    return np.minimum(bs, n - bs * np.arange(nb))


def exact_blocks(n, bs):
    """every block a cyclic row shift times powers of two in [2^-8, 2^8]: the diagonal of every block with more than one row is zero,
    every elimination step exchanges rows, and the inverse and its product with a vector are exact. What a partial last block does
    not cover holds NaN: it is not read. Returns (blocks, src, scale): z[src] / scale is M^-1 v for v given."""
    nb, m = -(-n // bs), block_rows(n, bs)
    out = np.full((nb, bs, bs), np.nan)
    src, scale = np.zeros(n, dtype=np.int64), np.zeros(n)
    for k in range(nb):
        mk = int(m[k])
        s = 1 + k % (mk - 1) if mk > 1 else 0
        a = np.arange(mk)
        e = np.floor(17.0 * synth._uniform(k * bs + a, 41)).astype(np.int64) - 8
        blk = np.zeros((mk, mk))
        blk[a, (a + s) % mk] = np.ldexp(1.0, e)          # row a: c_a at column (a + s) % m  ->  z[(a + s) % m] = v[a] / c_a
        out[k, :mk, :mk] = blk
        src[k * bs + (a + s) % mk] = k * bs + a
        scale[k * bs + (a + s) % mk] = np.ldexp(1.0, e)
    return out, src, scale


def skew_blocks(n, bs):
    """I + S, S skew with entries from _uniform in [-3, 3] (condition <= ~10); NaN outside a partial block's leading part"""
    nb, m = -(-n // bs), block_rows(n, bs)
    a, b = np.triu_indices(bs, 1)
    idx = (np.arange(nb, dtype=np.int64) * 1024)[:, None] + (a * 32 + b)[None, :]
    S = np.zeros((nb, bs, bs))
    S[:, a, b] = 6.0 * synth._uniform(idx, 43) - 3.0
    S = S - np.transpose(S, (0, 2, 1))
    out = S + np.eye(bs)[None]
    mk = int(m[-1])
    if mk < bs:
        out[-1, mk:, :] = np.nan
        out[-1, :, mk:] = np.nan
    return out


def solve_blocks(blocks, v, bs):
    """numpy.linalg.solve per block (the leading part of a partial one), and the max norm of each row's block result"""
    n, nb = v.size, blocks.shape[0]
    whole = n // bs
    z = np.zeros(n)
    if whole:
        z[:whole * bs] = np.linalg.solve(blocks[:whole], v[:whole * bs].reshape(whole, bs, 1)).reshape(-1)
    if whole < nb:
        mk = n - whole * bs
        z[whole * bs:] = np.linalg.solve(blocks[-1, :mk, :mk], v[whole * bs:])
    pad = np.zeros(nb * bs)
    pad[:n] = np.abs(z)
    norm = np.repeat(pad.reshape(nb, bs).max(axis=1), bs)[:n]
    return z, norm


def diagonal_blocks(d, bs):
    """blocks that hold d on their diagonals and zeros elsewhere"""
    nb = -(-d.size // bs)
    dd = np.ones(nb * bs)
    dd[:d.size] = d
    out = np.zeros((nb, bs, bs))
    out[:, np.arange(bs), np.arange(bs)] = dd.reshape(nb, bs)
    return out


def vector(n, seed=47):
    return 1.0 + 0.5 * synth._uniform(np.arange(n, dtype=np.int64), seed)      # no zero, no sign change


# ---------------------------------------------------------------- 1. the operator alone
SIZES = (1, 3, 63, 64, 65, 257, 4099)
WIDTHS = (1, 2, 3, 4, 5, 8, 16)


@pytest.fixture(scope="module")
def small():
    made = {}

    def get(n):
        if n not in made:
            made[n] = context(synth.transport_like(n))
        return made[n]
    yield get
    for c in made.values():
        c.close()


def check_exact(ctx, n, bs):
    blocks, src, scale = exact_blocks(n, bs)
    v = vector(n)
    assert ctx.set_block_diagonal(blocks, bs) == 0 and ctx.preconditioner() == "block_diagonal"
    z = ctx.apply_preconditioner(v)
    assert z.tobytes() == (v[src] / scale).tobytes()


def check_real(ctx, n, bs):
    blocks = skew_blocks(n, bs)
    v = vector(n, 53) - 1.2                                                     # both signs
    assert ctx.set_block_diagonal(blocks, bs) == 0
    z = ctx.apply_preconditioner(v)
    want, norm = solve_blocks(blocks, v, bs)
    err = np.abs(z - want) / norm
    print(f"n = {n}, bs = {bs}: largest |z - z_ref| / ||z_ref||_inf of a block = {err.max():.3e}")
    assert np.all(np.abs(z - want) <= 1e-12 * norm)


@pytest.mark.parametrize("bs", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_apply_is_exact_on_scaled_permutation_blocks(small, n, bs):
    check_exact(small(n), n, bs)


@pytest.mark.parametrize("bs", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_apply_matches_lapack_on_well_conditioned_blocks(small, n, bs):
    check_real(small(n), n, bs)


@pytest.mark.parametrize("bs", [3, 4])
def test_apply_on_a_reordered_context(bundles, bs):
    B = bundles("fem_4099_reordered")
    assert B.ctx.flags()["reordered"]
    check_exact(B.ctx, B.A.rows, bs)
    check_real(B.ctx, B.A.rows, bs)
    B.ctx.clear_preconditioner()


def test_apply_with_a_diagonal_and_without_a_preconditioner(small):
    ctx, n = small(257), 257
    ctx.clear_preconditioner()
    with pytest.raises(RuntimeError):
        ctx.apply_preconditioner(vector(n))
    d, v = P.powers_of_two(n), vector(n)
    assert ctx.set_diagonal(d) == 0
    assert ctx.apply_preconditioner(v).tobytes() == (v / d).tobytes()
    ctx.clear_preconditioner()


# ---------------------------------------------------------------- 2. / 3. method 4, bit for bit
def diag_state(B):
    """method 4 with the bundle's powers of two, once per bundle"""
    if not hasattr(B, "diag_want"):
        assert B.ctx.set_diagonal(B.d) == 0
        B.diag_want = state(B.ctx, B.ctx.solve("bicgstab_diag", B.b, x0=B.x0, **FIXED))
        assert 1 <= B.diag_want[0] <= 12
    return B.diag_want


@pytest.mark.parametrize("name", LAYOUTS)
def test_block_size_one_is_the_diagonal_method_bit_for_bit(bundles, name):
    B = bundles(name)
    want = diag_state(B)
    assert B.ctx.set_block_diagonal(B.d, 1) == 0 and B.ctx.preconditioner() == "block_diagonal"
    got = state(B.ctx, B.ctx.solve("bicgstab_block", B.b, x0=B.x0, **FIXED))
    assert got[0] == want[0]
    assert got == want


@pytest.mark.parametrize("bs", [3, 4, 16])
@pytest.mark.parametrize("name", LAYOUTS)
def test_diagonal_blocks_are_the_diagonal_method_bit_for_bit(bundles, name, bs):
    B = bundles(name)
    want = diag_state(B)
    assert B.ctx.set_block_diagonal(diagonal_blocks(B.d, bs), bs) == 0
    got = state(B.ctx, B.ctx.solve("bicgstab_block", B.b, x0=B.x0, **FIXED))
    assert got == want


# ---------------------------------------------------------------- 4. real blocks
def reference_block_bicgstab(A, blocks, bs, b, x0, tol, max_iter):
    """tests/test_precond_gpu.py's numpy restatement of the right-preconditioned recurrence with `dinv *` replaced by the block solve"""
    def minv(v):
        return solve_blocks(blocks, v, bs)[0]
    x = x0.copy()
    r = b - A.matvec(x)
    rh, p = r.copy(), r.copy()
    ph = minv(p)
    rr = r0 = rtr = float(r @ r)
    k, alphas, omegas = 0, [], []
    while rr > tol * tol * r0 and k < max_iter:
        s = A.matvec(ph)
        alpha = rtr / float(rh @ s)
        q = r - alpha * s
        qh = minv(q)
        y = A.matvec(qh)
        omega = float(q @ y) / float(y @ y)
        x = x + alpha * ph
        x = x + omega * qh
        r = q - omega * y
        rr, rtr_old = float(r @ r), rtr
        rtr = float(rh @ r)
        beta = (alpha / omega) * (rtr / rtr_old)
        k += 1
        alphas.append(alpha); omegas.append(omega)
        p = beta * p
        p = p + r
        p = p + (-beta * omega) * s
        ph = minv(p)
    return k, x, np.array(alphas), np.array(omegas)


# (generator, rows, scale_decades) -> (k, true relative residual) of the float64 numpy reference
MEASURED = {("transport", 20000, 0): (5, 2.5e-11), ("fem", 20000, 0): (4, 1.8e-11),
            ("transport", 20000, 4): (5, 8.1e-12), ("fem", 20000, 4): (4, 1.4e-11),
            ("transport", 20002, 0): (5, None), ("fem", 20002, 0): (4, None)}


@pytest.mark.parametrize("kind,n,decades", sorted(MEASURED))
def test_block_jacobi_on_coupled_blocks(kind, n, decades):
    """A = block_coupled(n, 4, gen[, scale_decades=4]), b = A 1, x0 = 0, tol 1e-10, max_iter 1000. The CPU reference needs 5
    (transport_like) and 4 (fem_like) iterations, unscaled, scaled over 4 decades and with a partial last block (20002 rows), and
    reaches a true relative residual of 2.5e-11 / 1.8e-11 (unscaled) and 8.1e-12 / 1.4e-11 (scaled). Plain BiCGStab and point Jacobi
    need 491 / 486 (transport) and 112 / 114 (fem) iterations on the unscaled pair; on the scaled pair plain does not converge in
    1000 iterations and point Jacobi breaks down on the CPU (nothing is asserted about it there). The device's k may differ by the
    last iterations (summation order), its true residual by the same cause: 10 x."""
    gen = synth.transport_like if kind == "transport" else synth.fem_like
    A = synth.block_coupled(n, 4, gen, scale_decades=float(decades))
    blocks, _ = H.csr_block_diagonal(A, 4)
    b, x0 = A.matvec(np.ones(n)), np.zeros(n)
    k_ref, res_tab = MEASURED[(kind, n, decades)]
    k_cpu, x_cpu, al, om = reference_block_bicgstab(A, blocks, 4, b, x0, REAL["tol"], REAL["max_iter"])
    ref_res = P.relres(A, x_cpu, b)
    print(f"{kind} {n} decades {decades}: CPU reference k = {k_cpu}, true relative residual {ref_res:.3e}")
    assert k_cpu == k_ref
    if res_tab is not None:
        assert 0.5 * res_tab <= ref_res <= 2.0 * res_tab
    ctx = context(A)
    try:
        assert ctx.set_block_diagonal(blocks, 4) == 0
        got = ctx.solve("bicgstab_block", b, **REAL)
        tr = ctx.trace(got["k"])
        res = P.relres(A, got["x"], b)
        print(f"{kind} {n} decades {decades}: block Jacobi k = {got['k']}, true relative residual {res:.3e}")
        assert abs(got["k"] - k_cpu) <= 2
        assert res <= 10.0 * ref_res
        np.testing.assert_allclose(tr["alpha"][:4], al[:4], rtol=1e-9, atol=0.0)
        np.testing.assert_allclose(tr["omega"][:4], om[:4], rtol=1e-9, atol=0.0)
        if n == 20000:
            plain = ctx.solve("bicgstab", b, **REAL)
            print(f"{kind} {n} decades {decades}: plain k = {plain['k']}")
            if decades:
                assert plain["k"] == 1000
            else:
                d, missing = H.csr_diagonal(A)
                assert missing == 0 and ctx.set_diagonal(d) == 0
                point = ctx.solve("bicgstab_diag", b, **REAL)
                print(f"{kind} {n} decades {decades}: point Jacobi k = {point['k']}")
                assert plain["k"] >= 10 * got["k"] and point["k"] >= 10 * got["k"]
    finally:
        ctx.close()


# ---------------------------------------------------------------- 5. interface
@pytest.fixture(scope="module")
def coupled():
    """(A, blocks, x0, b) of the scaled block_coupled(20000, 4, fem_like) and a context on it; the tests leave it without a preconditioner"""
    A = synth.block_coupled(20000, 4, synth.fem_like, scale_decades=4.0)
    blocks, _ = H.csr_block_diagonal(A, 4)
    b = A.matvec(np.ones(A.rows))
    x0 = 0.01 * synth._uniform(np.arange(A.rows, dtype=np.int64), 3)
    for a in (blocks, b, x0):
        a.setflags(write=False)
    ctx = context(A)
    yield A, blocks, x0, b, ctx
    ctx.close()


def test_a_method_without_its_preconditioner_is_refused_and_touches_nothing(coupled):
    A, blocks, x0, b, ctx = coupled
    L = H.lib()
    d, _ = H.csr_diagonal(A)

    def refused(method):
        ctx.load(x0, b)
        o, res = ctx.options(quiet=1), H.Result()
        assert L.bicg_run(ctx.h, H.METHODS[method], C.byref(o), C.byref(res)) == -2
        assert L.bicg_run_begin(ctx.h, H.METHODS[method], C.byref(o)) == -2
        x, r = ctx.fetch()
        assert x.tobytes() == x0.tobytes() and r.tobytes() == b.tobytes()
        got = ctx.solve(method, b, x0=x0)
        assert got["k"] == -2 and got["x"].tobytes() == x0.tobytes() and got["r"].tobytes() == b.tobytes()
        tb, tx = torch.from_numpy(np.array(b)).cuda(), torch.from_numpy(np.array(x0)).cuda()
        got = ctx.solve(method, tb, x0=tx, inplace=True)
        assert got["k"] == -2 and tx.cpu().numpy().tobytes() == x0.tobytes() and tb.cpu().numpy().tobytes() == b.tobytes()
        with pytest.raises(RuntimeError, match="set_block_diagonal" if method == "bicgstab_block" else "set_diagonal"):
            ctx.run_begin(method)
        with pytest.raises(RuntimeError):
            ctx.run(method)
        x, r = ctx.fetch()
        assert x.tobytes() == x0.tobytes() and r.tobytes() == b.tobytes()

    ctx.clear_preconditioner()
    ctx.solve("bicgstab", b, x0=x0, tol=0.0, max_iter=6, record_trace=1)
    trace = ctx.trace(6)
    refused("bicgstab_block")                                        # kind 0
    assert ctx.set_diagonal(d) == 0
    refused("bicgstab_block")                                        # kind 1
    assert ctx.set_block_diagonal(blocks, 4) == 0
    refused("bicgstab_diag")                                         # kind 2
    after = ctx.trace(6)
    assert all(after[k].tobytes() == trace[k].tobytes() for k in trace)
    ctx.clear_preconditioner()


def test_refused_blocks_leave_what_was_installed_and_installs_allocate_once(coupled):
    A, blocks, x0, b, ctx = coupled
    n = A.rows
    ctx.clear_preconditioner()
    ctx.solve("bicgstab", b, x0=x0, **REAL)      # (the trace buffer grows with the first solve of this max_iter: not what is counted here)
    before = H.device_allocations()

    def bad_blocks():
        z = np.array(blocks); z[n // 8, 2, :] = 0.0                  # a zero row
        yield z
        z = np.array(blocks); z[17, 1, 3] = np.nan
        yield z
        z = np.array(blocks); z[-1, 0, 0] = np.inf
        yield z
    two = diagonal_blocks(np.ones(n), 2)
    two[n // 5] = [[0.5, 2.0], [0.25, 1.0]]                          # exactly singular, powers of two
    for z in bad_blocks():                                           # nothing installed yet: refused, still nothing
        assert ctx.set_block_diagonal(z, 4) == 1 and ctx.preconditioner() is None
    assert ctx.set_block_diagonal(two, 2) == 1 and ctx.preconditioner() is None
    for bs in (0, 17, -3):
        assert ctx.set_block_diagonal(blocks, bs) == -2 and ctx.preconditioner() is None
    assert H.device_allocations() == before
    assert ctx.set_block_diagonal(blocks, 4) == 0
    assert H.device_allocations() == before + 1
    want = state(ctx, ctx.solve("bicgstab_block", b, x0=x0, **REAL))
    for z in bad_blocks():
        assert ctx.set_block_diagonal(z, 4) == 1 and ctx.preconditioner() == "block_diagonal"
        assert state(ctx, ctx.solve("bicgstab_block", b, x0=x0, **REAL)) == want
    assert ctx.set_block_diagonal(two, 2) == 1                       # another bs, refused: the planes of bs = 4 stay
    assert ctx.set_block_diagonal(blocks, 0) == -2 and ctx.set_block_diagonal(blocks, 17) == -2
    assert ctx.set_block_diagonal(None, 4) == -1
    assert state(ctx, ctx.solve("bicgstab_block", b, x0=x0, **REAL)) == want
    assert ctx.set_block_diagonal(blocks, 4) == 0                    # a second install with the same bs
    assert H.device_allocations() == before + 1
    assert state(ctx, ctx.solve("bicgstab_block", b, x0=x0, **REAL)) == want
    # a refused block install leaves a DIAGONAL preconditioner too; switching kinds releases the other array
    d, _ = H.csr_diagonal(A)
    assert ctx.set_diagonal(d) == 0 and ctx.preconditioner() == "diagonal"
    assert H.device_allocations() == before + 1
    dw = state(ctx, ctx.solve("bicgstab_diag", b, x0=x0, tol=0.0, max_iter=8, record_trace=1))
    assert ctx.set_block_diagonal(next(bad_blocks()), 4) == 1 and ctx.preconditioner() == "diagonal"
    assert state(ctx, ctx.solve("bicgstab_diag", b, x0=x0, tol=0.0, max_iter=8, record_trace=1)) == dw
    assert ctx.set_block_diagonal(blocks, 4) == 0 and ctx.preconditioner() == "block_diagonal"
    assert H.device_allocations() == before + 1
    assert state(ctx, ctx.solve("bicgstab_block", b, x0=x0, **REAL)) == want
    assert ctx.clear_preconditioner() == 0 and ctx.preconditioner() is None
    assert H.device_allocations() == before
    assert ctx.set_block_diagonal(blocks, 4) == 0                    # install after a clear: one array again, the same solve
    assert H.device_allocations() == before + 1
    assert state(ctx, ctx.solve("bicgstab_block", b, x0=x0, **REAL)) == want
    assert ctx.clear_preconditioner() == 0 and H.device_allocations() == before


def test_one_context_holds_one_preconditioner_through_a_sequence_of_installs():
    """diagonal, block (bs = 4), block (bs = 2), diagonal, clear on ONE context (4099 rows: a partial last block for both widths).
    After every install the context names the kind just installed, its method solves bit for bit as on a fresh context that holds
    nothing else, and the other kind's method is refused without touching x and r. A refused install (a singular block while the
    diagonal is held) changes nothing, and the final clear gives back the one array that was ever held at a time."""
    A = synth.block_coupled(4099, 4, synth.fem_like, scale_decades=2.0)
    n = A.rows
    b, x0 = A.matvec(np.ones(n)), 0.01 * synth._uniform(np.arange(n, dtype=np.int64), 3)
    opts = dict(tol=0.0, max_iter=8, record_trace=1)
    d, missing = H.csr_diagonal(A)
    assert missing == 0
    install = {"diagonal": lambda c: c.set_diagonal(d),
               "block4": lambda c: c.set_block_diagonal(H.csr_block_diagonal(A, 4)[0], 4),
               "block2": lambda c: c.set_block_diagonal(H.csr_block_diagonal(A, 2)[0], 2)}
    method = {"diagonal": "bicgstab_diag", "block4": "bicgstab_block", "block2": "bicgstab_block"}
    want = {}
    for key in install:                                              # once each: a fresh context that holds only this one
        fresh = context(A)
        try:
            assert install[key](fresh) == 0
            want[key] = state(fresh, fresh.solve(method[key], b, x0=x0, **opts))
        finally:
            fresh.close()
    assert len(set(want.values())) == 3
    singular = np.array(H.csr_block_diagonal(A, 4)[0]); singular[n // 8, 2, :] = 0.0
    ctx = context(A)
    try:
        ctx.solve("bicgstab", b, x0=x0, **opts)                      # (the trace buffer grows with the first solve)
        before = H.device_allocations()
        for step, key in enumerate(("diagonal", "block4", "block2", "diagonal")):
            assert install[key](ctx) == 0
            assert ctx.preconditioner() == ("diagonal" if key == "diagonal" else "block_diagonal")
            assert H.device_allocations() == before + 1
            if step == 3:                                            # refused: the diagonal stays and answers as before
                assert ctx.set_block_diagonal(singular, 4) == 1 and ctx.preconditioner() == "diagonal"
                assert H.device_allocations() == before + 1
            assert state(ctx, ctx.solve(method[key], b, x0=x0, **opts)) == want[key]
            other = "bicgstab_block" if key == "diagonal" else "bicgstab_diag"
            got = ctx.solve(other, b, x0=x0, **opts)
            assert got["k"] == -2 and got["x"].tobytes() == x0.tobytes() and got["r"].tobytes() == b.tobytes()
        assert ctx.clear_preconditioner() == 0 and ctx.preconditioner() is None
        assert H.device_allocations() == before
    finally:
        ctx.close()


def test_update_values_then_install_equals_a_fresh_context():
    A1 = synth.block_coupled(4099, 4, synth.fem_like, scale_decades=2.0)
    A2 = synth.CSR(A1.rows, A1.cols, A1.ptr, A1.col, A1.val * (1.0 + 0.25 * synth._uniform(np.arange(A1.nnz, dtype=np.int64), 9)))
    b1, b2 = H.csr_block_diagonal(A1, 4)[0], H.csr_block_diagonal(A2, 4)[0]
    bb = A2.matvec(np.ones(A2.rows))
    ctx, fresh = context(A1), context(A2)
    try:
        assert ctx.set_block_diagonal(b1, 4) == 0
        stale = ctx.solve("bicgstab_block", bb, **REAL)
        assert ctx.update_values(A2) == 0
        assert ctx.preconditioner() == "block_diagonal"              # update_values never touches it
        assert ctx.set_block_diagonal(b2, 4) == 0
        assert fresh.set_block_diagonal(b2, 4) == 0
        got, want = ctx.solve("bicgstab_block", bb, **REAL), fresh.solve("bicgstab_block", bb, **REAL)
        assert state(ctx, got) == state(fresh, want)
        assert got["x"].tobytes() != stale["x"].tobytes()
    finally:
        ctx.close(); fresh.close()


def test_install_from_a_tensor_filled_on_a_side_stream(coupled):
    A, blocks, x0, b, ctx = coupled
    assert ctx.set_block_diagonal(blocks, 4) == 0
    want = state(ctx, ctx.solve("bicgstab_block", b, x0=x0, **REAL))
    assert ctx.set_block_diagonal(diagonal_blocks(np.ones(A.rows), 4), 4) == 0      # something else in between
    src = torch.from_numpy(np.array(blocks)).cuda()
    m = torch.ones((2048, 2048), dtype=torch.float64, device="cuda")
    t = torch.full(tuple(blocks.shape), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(4):
            m = (m @ m) * 1.0e-4                                     # the stream is busy when the fill is enqueued
        t.copy_(src)
    assert ctx.set_block_diagonal(t, 4, stream=side) == 0
    assert state(ctx, ctx.solve("bicgstab_block", b, x0=x0, **REAL)) == want
    torch.cuda.synchronize()
    ctx.clear_preconditioner()


def test_solve_on_tensors_is_the_host_solve(coupled):
    A, blocks, x0, b, ctx = coupled
    assert ctx.set_block_diagonal(blocks, 4) == 0
    ws = state(ctx, ctx.solve("bicgstab_block", b, x0=x0, **REAL))
    got = ctx.solve("bicgstab_block", torch.from_numpy(np.array(b)).cuda(), x0=torch.from_numpy(np.array(x0)).cuda(), **REAL)
    got["x"], got["r"] = got["x"].cpu().numpy(), got["r"].cpu().numpy()
    assert state(ctx, got) == ws
    ctx.clear_preconditioner()


GRAPH_CHILD = r"""
import os, sys
import numpy as np
import torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
from mpi_bicgstab_amd import hipsolver as H, synth
import test_precond_gpu as P
H.lib().bicg_comm_init_single(0)
A = synth.block_coupled(20000, 4, synth.fem_like, scale_decades=4.0)
b4 = H.csr_block_diagonal(A, 4)[0]
b2 = H.csr_block_diagonal(A, 2)[0]
b4x = b4 * (1.0 + synth._uniform(np.arange(b4.size, dtype=np.int64), 13)).reshape(b4.shape)
b = A.matvec(np.ones(A.rows))
x0 = 0.01 * synth._uniform(np.arange(A.rows, dtype=np.int64), 3)
opts = dict(tol=0.0, max_iter=10, record_trace=1, check_every=1)
eager = P.context(A)
os.environ["BICG_GRAPH"] = "1"
graph = P.context(A)
os.environ.pop("BICG_GRAPH")
want = {}
for key, (blk, bs) in dict(b4=(b4, 4), b2=(b2, 2), b4x=(b4x, 4)).items():
    assert eager.set_block_diagonal(blk, bs) == 0
    want[key] = P.state(eager, eager.solve("bicgstab_block", b, x0=x0, **opts))
assert len(set(want.values())) == 3
assert graph.set_block_diagonal(b4, 4) == 0
assert P.state(graph, graph.solve("bicgstab_block", b, x0=x0, **opts)) == want["b4"], "first capture"
assert graph.clear_preconditioner() == 0
squatters = [torch.full((4 * A.rows,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(4)]
torch.cuda.synchronize()
assert graph.set_block_diagonal(b2, 2) == 0                          # another bs, another array
assert P.state(graph, graph.solve("bicgstab_block", b, x0=x0, **opts)) == want["b2"], "after clear + install with bs = 2"
assert graph.set_block_diagonal(b4x, 4) == 0                         # another bs again, without a clear
assert P.state(graph, graph.solve("bicgstab_block", b, x0=x0, **opts)) == want["b4x"], "after an install with bs = 4"
assert graph.set_block_diagonal(b4, 4) == 0                          # the same array: the captured iteration stays and reads the new values
assert P.state(graph, graph.solve("bicgstab_block", b, x0=x0, **opts)) == want["b4"], "after an install into the same array"
del squatters
eager.close(); graph.close()
print("GRAPH-OK")
"""


def test_graph_replay_follows_the_planes_through_clear_and_install():
    """BICG_GRAPH=1: the captured iteration of method 5 holds the address of the planes and their bs. Solve (two eager iterations,
    then capture and replay), clear, install with ANOTHER bs -- a new array; the freed one is handed to someone else and filled with
    NaN first --, solve: the bytes of the eager context with those blocks. In a child process: the variable is read at bicg_create."""
    p = subprocess.run([sys.executable, "-c", GRAPH_CHILD % dict(root=ROOT)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and "GRAPH-OK" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])


def test_block_jacobi_bicgstab_drop_in(coupled):
    A, blocks, _, b, ctx = coupled
    assert ctx.set_block_diagonal(blocks, 4) == 0
    want = ctx.solve("bicgstab_block", b, tol=1e-10, max_iter=1000)
    ctx.clear_preconditioner()
    assert abs(want["k"] - 4) <= 2
    L = H.lib()
    blk = H.single_rank_blocks(A)
    x, r = np.zeros(A.rows), np.array(b)
    os.environ.update(BICG_TOL="1e-10", BICG_MAX_ITER="1000", BICG_QUIET="1")
    H.switches(persist=0)
    try:
        L.bicg_dropin_release()
        for _ in range(2):                                           # created, then reused with the blocks in place
            x[:] = 0.0; r[:] = b
            k = L.block_jacobi_bicgstab(C.byref(blk.diag), C.byref(blk.offd), C.byref(blk.info), H._d(x), H._d(r), 4)
            assert k == want["k"]
            assert x.tobytes() == want["x"].tobytes() and r.tobytes() == want["r"].tobytes()
        # the plain drop-in on the same resident context is unaffected by the installed blocks
        x[:] = 0.0; r[:] = b
        os.environ["BICG_MAX_ITER"] = "20"
        assert L.bicgstab(C.byref(blk.diag), C.byref(blk.offd), C.byref(blk.info), H._d(x), H._d(r)) == 20
    finally:
        for k_ in ("BICG_TOL", "BICG_MAX_ITER", "BICG_QUIET"):
            os.environ.pop(k_, None)
        H.switches(persist=None)
        L.bicg_dropin_release()


SINGULAR_CHILD = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %(root)r)
from mpi_bicgstab_amd import hipsolver as H, synth
L = H.lib()
L.bicg_comm_init_single(0)
n = 64
ptr = np.concatenate([[0, 2, 4], 4 + np.arange(1, n - 1)]).astype(np.uint32)
col = np.concatenate([[0, 1, 0, 1], np.arange(2, n)]).astype(np.uint32)
val = np.concatenate([[0.5, 2.0, 0.25, 1.0], np.full(n - 2, 4.0)])      # the first 2 x 2 block is exactly singular
A = synth.CSR(n, n, ptr, col, val)
blk = H.single_rank_blocks(A)
x, r = np.zeros(n), np.ones(n)
bs = int(sys.argv[1])
L.block_jacobi_bicgstab(C.byref(blk.diag), C.byref(blk.offd), C.byref(blk.info), H._d(x), H._d(r), bs)
print("RETURNED")
"""


@pytest.mark.parametrize("bs,line", [(2, "Error: matrix has a singular diagonal block."), (17, "Error: block size 17 is outside 1..16.")])
def test_block_jacobi_bicgstab_exits_on_what_it_cannot_install(bs, line):
    env = dict(os.environ, BICG_QUIET="1", BICG_MAX_ITER="5")
    p = subprocess.run([sys.executable, "-c", SINGULAR_CHILD % dict(root=ROOT), str(bs)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 1, (p.returncode, p.stderr[-2000:])
    assert line in p.stderr.splitlines() and "RETURNED" not in p.stdout
