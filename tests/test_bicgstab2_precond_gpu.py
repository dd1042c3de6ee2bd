"""`-m gpu`, one rank: the right-preconditioned BiCGStab(2), methods BICG_BICGSTAB2_DIAG = 7 and BICG_BICGSTAB2_BLOCK = 8
(Driver::iter_stab2 with a hat in csrc/bicg_solver.cpp, the DIAGONAL / BLOCK forms of the FS2* functors of csrc/bicg_stab2.hip, which
method 6 shares with them as their NONE form) through
Context.solve("bicgstab2_diag" / "bicgstab2_block") and the run_* calls.

Contexts are created under switches(persist=0); matrices, x0, b and the powers of two d are those of tests/test_precond_gpu.py (its
Bundle), the block builders those of tests/test_block_precond_gpu.py, the reference is tests/bicgstab2_precond_ref.py.
  1. bit for bit        three sweeps (tol 0, max_iter 6, trace on), everything a solve reports as bytes: method 7 with d = 1 and
                        method 8 with identity blocks (bs 1, 4, and 5: a partial last block) are method 6; method 8 with bs = 1 or with
                        diagonal blocks (bs 3, 4, 16) is method 7 with that d; method 7 with powers of two d on A is method 6 on A D^-1
                        (x = y / d, x0 scaled by d). The last one needs the scaled matrix to get the same plan, which rules out the
                        plane-marching layout (scaled columns are no constant stencil), as in tests/test_precond_gpu.py.
  2. three sweeps       against hat_sweeps with a real preconditioner: diag(A) for method 7 on every layout, the 4 x 4 blocks for method
                        8 on three. Tolerance per matrix as in tests/test_bicgstab2_gpu.py: 16 x the largest gap between hat_sweeps
                        with numpy's dots and with every dot accumulated in np.longdouble, floor 1e-12. Printed; profiles/NOTES.md.
  3. invariances        as bytes: check_every, bicg_run against stepped run_iterate(2) / (3), host arrays against CUDA tensors, a solve
                        repeated, methods 0, 4 / 5 and 6 around it, no allocation by any solve
  4. convergence        seed 78 on the issue's S1 / Jacobi, S2 / Jacobi, S3 / blocks, S3 / Jacobi, S4 / blocks: no breakdown, true
                        relative residual <= 1e-9 from the fetched x, k <= 1.25 x hat_sweeps' k. The device's methods 0, 4 / 5 and 6 on
                        the same systems are printed, not asserted.
  5. edges              1 x 1 system, max_iter 0 / 1 / 7, b = 0, refusals (no preconditioner, the other kind, multi-RHS), a reinstall
                        between two solves, BICG_GRAPH=1
  6. tiled form         transport_like(2^24 + 3): method 7 with d = 1, one sweep, is method 6; b - A x = r to 1e-12 ||b||"""
import ctypes as C
import functools
import subprocess
import sys

import numpy as np
import pytest
import torch

import bicgstab2_precond_ref as Q
import bicgstab2_ref as R
import test_block_precond_gpu as BP
import test_precond_gpu as P
from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import synth

pytestmark = pytest.mark.gpu
ROOT = P.ROOT
MATRICES = ("transport_63", "transport_257", "transport_4099", "transport_40000", "fem_4099", "fem_40000", "grid7", P.PLANES,
            "fem_4099_reordered")
INVARIANT_ON = ("transport_4099", "fem_4099", "grid7")
THREE = dict(tol=0.0, max_iter=6, record_trace=1)
REAL = dict(tol=1e-10, max_iter=40, record_trace=1)
KEYS = ("alpha", "beta", "omega", "dotr")
DIAG, BLOCK = "bicgstab2_diag", "bicgstab2_block"


@pytest.fixture(scope="module", autouse=True)
def _single_rank():
    H.lib().bicg_comm_init_single(0)      # (once: a new communicator orphans the contexts of the one before)
    yield


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


def state(ctx, got, with_x=True, nan_ok=False):
    return P.state(ctx, got, with_x=with_x, nan_ok=nan_ok) + (got["result"].breakdown_iteration,)


def install(ctx, kind, A):
    """the real preconditioner of a kind: diag(A), or its 4 x 4 blocks"""
    if kind == DIAG:
        assert ctx.set_diagonal(Q.diagonal(A)) == 0 and ctx.preconditioner() == "diagonal"
    else:
        assert ctx.set_block_diagonal(Q.blocks_of(A, 4), 4) == 0 and ctx.preconditioner() == "block_diagonal"


# ---- 1. bit for bit
@pytest.mark.parametrize("name", MATRICES)
def test_identity_and_diagonal_blocks_bit_for_bit(bundles, name):
    B = bundles(name)
    ctx, n = B.ctx, B.A.rows
    want6 = state(ctx, ctx.solve("bicgstab2", B.b, x0=B.x0, **THREE))
    assert want6[0] == 6 and want6[-1] == 0
    assert ctx.set_diagonal(np.ones(n)) == 0
    assert state(ctx, ctx.solve(DIAG, B.b, x0=B.x0, **THREE)) == want6, "method 7, d = 1"
    for bs in (1, 4, 5):
        assert ctx.set_block_diagonal(BP.diagonal_blocks(np.ones(n), bs), bs) == 0
        assert state(ctx, ctx.solve(BLOCK, B.b, x0=B.x0, **THREE)) == want6, ("method 8, identity blocks", bs)
    assert ctx.set_diagonal(B.d) == 0
    want7 = state(ctx, ctx.solve(DIAG, B.b, x0=B.x0, **THREE))
    assert want7[0] == 6 and want7[-1] == 0 and want7 != want6
    assert ctx.set_block_diagonal(B.d, 1) == 0
    assert state(ctx, ctx.solve(BLOCK, B.b, x0=B.x0, **THREE)) == want7, "method 8, bs = 1"
    for bs in (3, 4, 16):
        assert ctx.set_block_diagonal(BP.diagonal_blocks(B.d, bs), bs) == 0
        assert state(ctx, ctx.solve(BLOCK, B.b, x0=B.x0, **THREE)) == want7, ("method 8, diagonal blocks", bs)
    ctx.clear_preconditioner()


@pytest.mark.parametrize("name", [m for m in MATRICES if m != P.PLANES])
def test_power_of_two_diagonal_is_method_6_on_the_scaled_columns(bundles, name):
    B = bundles(name)
    ca, cb = B.ctx, B.scaled_context()
    assert ca.flags() == cb.flags() and ca.plan_info() == cb.plan_info()      # the comparison is void unless both got the same plan
    assert ca.set_diagonal(B.d) == 0
    got = ca.solve(DIAG, B.b, x0=B.x0, **THREE)
    want = cb.solve("bicgstab2", B.b, x0=B.d * B.x0, **THREE)
    assert got["k"] == 6 and np.any(B.x0 != 0.0)
    assert state(ca, got, with_x=False) == state(cb, want, with_x=False)
    assert P.raw(got["x"]) == P.raw(want["x"] / B.d)
    ca.clear_preconditioner()


# ---- 2. three sweeps against the restatement
@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """(hat_sweeps' three sweeps, the matrix's tolerance, the gaps it was computed from)"""
    A, _ = P.matrix(name)
    idx = np.arange(A.rows, dtype=np.int64)
    x0, b = 0.25 * synth._uniform(idx, 77) - 0.125, A.matvec(1.0 + 0.5 * synth._uniform(idx, 78))      # (Bundle's x0 and b)
    mul = R.Product(A)
    minv = Q.jacobi(A, reciprocal=True) if kind == DIAG else Q.block_inverse(A, 4)
    plain, ext = Q.hat_sweeps(mul, minv, b, x0, 6, 0.0), Q.hat_sweeps(mul, minv, b, x0, 6, 0.0, extended=True)
    gaps = {q: R.gap(ext["trace"][q], plain["trace"][q]) for q in KEYS}
    gaps.update(x=R.gap(ext["x"], plain["x"]), r=R.gap(ext["r"], plain["r"]))
    return plain, max(16.0 * max(gaps.values()), 1e-12), gaps


@pytest.mark.parametrize("name,kind", [(m, DIAG) for m in MATRICES] + [(m, BLOCK) for m in INVARIANT_ON])
def test_three_sweeps_against_the_restatement(bundles, name, kind):
    B = bundles(name)
    want, tol, gaps = reference(name, kind)
    install(B.ctx, kind, B.A)
    got = B.ctx.solve(kind, B.b, x0=B.x0, **THREE)
    tr = B.ctx.trace(got["k"])
    B.ctx.clear_preconditioner()
    print(name, kind, "tolerance %.3e" % tol, "from the restatement's gaps", {q: "%.2e" % v for q, v in gaps.items()})
    assert got["k"] == 6 == want["k"] and got["result"].breakdown_iteration == 0 and want["breakdown"] == 0
    for q in KEYS:
        g = R.gap(want["trace"][q], tr[q])
        print("  ", q, "gap %.3e" % g)
        assert g <= tol, (name, q, g, tol)
    for q in ("x", "r"):
        g = R.gap(want[q], got[q])
        print("  ", q, "gap %.3e" % g)
        assert g <= tol, (name, q, g, tol)
    assert R.gap([want["dot_r"]], [got["result"].dot_r]) <= tol and R.gap([want["dot_zero"]], [got["result"].dot_zero]) <= tol
    assert tr["dotr"][4] == tr["dotr"][5] == got["result"].dot_r and tr["dotr"][0] == tr["dotr"][1]


# ---- 3. invariances, as bytes
def stepped(B, method, step, **opts):
    ctx = B.ctx
    ctx.load(B.x0, B.b)
    ctx.run_begin(method, **opts)
    k, calls = 0, 0
    while calls < 64:
        k_new = ctx.run_iterate(step)
        calls += 1
        if k_new == k:
            break
        k = k_new
    res = ctx.run_end()
    x, r = ctx.fetch()
    return dict(k=res.iterations, x=x, r=r, result=res), calls


@pytest.mark.parametrize("kind", [DIAG, BLOCK])
@pytest.mark.parametrize("name", INVARIANT_ON)
def test_invariances(bundles, name, kind):
    B = bundles(name)
    ctx = B.ctx
    older = "bicgstab_diag" if kind == DIAG else "bicgstab_block"
    install(ctx, kind, B.A)
    before = [state(ctx, ctx.solve(m, B.b, x0=B.x0, **REAL)) for m in ("bicgstab", older, "bicgstab2")]
    want = state(ctx, ctx.solve(kind, B.b, x0=B.x0, check_every=1, **REAL))
    live = H.device_allocations()
    assert 2 <= want[0] <= 40 and want[0] % 2 == 0 and want[-1] == 0
    for every in (5, 40):
        assert state(ctx, ctx.solve(kind, B.b, x0=B.x0, check_every=every, **REAL)) == want, every
    assert state(ctx, ctx.solve(kind, B.b, x0=B.x0, check_every=1, **REAL)) == want, "the same solve twice"
    ctx.load(B.x0, B.b)
    res = ctx.run(kind, **REAL)
    x, r = ctx.fetch()
    assert state(ctx, dict(k=res.iterations, x=x, r=r, result=res)) == want, "bicg_run"
    got, calls = stepped(B, kind, 2, **REAL)
    assert state(ctx, got) == want and calls >= want[0] // 2, "run_iterate(2)"
    got, _ = stepped(B, kind, 3, **REAL)      # three steps round up to two sweeps
    assert state(ctx, got) == want, "run_iterate(3)"
    ctx.load(B.x0, B.b)
    ctx.run_begin(kind, **dict(REAL, tol=0.0))
    assert ctx.run_iterate(3) == 4 and ctx.run_iterate(1) == 6 and ctx.run_iterate(2) == 8
    ctx.run_end()
    dev = ctx.solve(kind, torch.from_numpy(np.array(B.b)).cuda(), x0=torch.from_numpy(np.array(B.x0)).cuda(), check_every=1, **REAL)
    dev["x"], dev["r"] = dev["x"].cpu().numpy(), dev["r"].cpu().numpy()
    assert state(ctx, dev) == want, "bicg_solve_device"
    assert H.device_allocations() == live
    after = [state(ctx, ctx.solve(m, B.b, x0=B.x0, **REAL)) for m in ("bicgstab", older, "bicgstab2")]
    assert after == before, "methods 0, 4 / 5 and 6 around it"
    assert H.device_allocations() == live
    ctx.clear_preconditioner()


# ---- 4. convergence where it matters
@pytest.mark.parametrize("name,kind", [("S1", DIAG), ("S2", DIAG), ("S3", BLOCK), ("S3", DIAG), ("S4", BLOCK)])
def test_convergence_on_the_systems_every_other_method_fails_on(name, kind):
    A = Q.systems()[name]()
    b, x0 = R.rhs(A, 78), np.zeros(A.rows)
    mul = R.Product(A)
    want = Q.hat_sweeps(mul, Q.jacobi(A, reciprocal=True) if kind == DIAG else Q.block_inverse(A, 4), b, x0, 1000, 1e-10)
    ctx = P.context(A)
    try:
        install(ctx, kind, A)
        got = ctx.solve(kind, b, x0=x0, tol=1e-10, max_iter=1000)
        rel = R.true_relres(mul, b, got["x"])
        print(name, kind, "k", got["k"], "restatement k", want["k"], "true relres %.3e" % rel)
        for m in ("bicgstab", "bicgstab_diag" if kind == DIAG else "bicgstab_block", "bicgstab2"):
            o = ctx.solve(m, b, x0=x0, tol=1e-10, max_iter=1000)
            print("   device", m, "k", o["k"], "breakdown", o["result"].breakdown_iteration, "relres %.3e" % np.sqrt(o["result"].dot_r / o["result"].dot_zero))
        assert want["breakdown"] == 0 and got["result"].breakdown_iteration == 0
        assert rel <= 1e-9, rel
        assert got["k"] <= 1.25 * want["k"], (got["k"], want["k"])
    finally:
        ctx.close()


# ---- 5. edges
@pytest.mark.parametrize("kind", [DIAG, BLOCK])
def test_one_row_breaks_down_in_its_first_sweep(bundles, kind):
    B = bundles("transport_1")
    d = Q.diagonal(B.A)
    assert (B.ctx.set_diagonal(d) if kind == DIAG else B.ctx.set_block_diagonal(d, 1)) == 0
    got = B.ctx.solve(kind, B.b, x0=B.x0, tol=0.0, max_iter=12)
    B.ctx.clear_preconditioner()
    assert got["k"] == 2 and got["result"].breakdown_iteration == 2, (got["k"], got["result"].breakdown_iteration)
    want = Q.hat_sweeps(B.A, Q.jacobi(B.A, reciprocal=True), B.b, B.x0, 12, 0.0)
    assert want["k"] == 2 and want["breakdown"] == 2


@pytest.mark.parametrize("kind", [DIAG, BLOCK])
def test_iteration_limits(bundles, kind):
    B = bundles("transport_4099")
    ctx = B.ctx
    install(ctx, kind, B.A)
    for cap in (0, 1):
        got = ctx.solve(kind, B.b, x0=B.x0, tol=0.0, max_iter=cap)
        assert got["k"] == 0 and got["result"].iterations == 0 and got["x"].tobytes() == B.x0.tobytes(), cap
    got = ctx.solve(kind, B.b, x0=B.x0, tol=0.0, max_iter=7, record_trace=1)
    assert got["k"] == 6
    six = ctx.solve(kind, B.b, x0=B.x0, **THREE)
    assert state(ctx, got) == state(ctx, six)
    zero = ctx.solve(kind, np.zeros(B.A.rows), x0=np.zeros(B.A.rows), tol=1e-10, max_iter=10)
    assert zero["k"] == 0 and not zero["x"].any()
    ctx.clear_preconditioner()


@pytest.mark.parametrize("kind", [DIAG, BLOCK])
@pytest.mark.parametrize("held", [None, "other"])
def test_without_its_preconditioner_a_method_is_refused_and_touches_nothing(bundles, kind, held):
    B = bundles("transport_4099")
    ctx, L = B.ctx, H.lib()
    ctx.clear_preconditioner()
    if held:
        install(ctx, BLOCK if kind == DIAG else DIAG, B.A)      # the OTHER kind
    ctx.solve("bicgstab2", B.b, x0=B.x0, **THREE)                # (the trace buffer grows with the first solve of this max_iter)
    live = H.device_allocations()
    ctx.load(B.x0, B.b)
    o, res = ctx.options(quiet=1, **THREE), H.Result()
    assert L.bicg_run(ctx.h, H.METHODS[kind], C.byref(o), C.byref(res)) == -2
    assert L.bicg_run_begin(ctx.h, H.METHODS[kind], C.byref(o)) == -2
    x, r = ctx.fetch()
    assert x.tobytes() == B.x0.tobytes() and r.tobytes() == B.b.tobytes()
    got = ctx.solve(kind, B.b, x0=B.x0, **THREE)
    assert got["k"] == -2 and got["x"].tobytes() == B.x0.tobytes() and got["r"].tobytes() == B.b.tobytes()
    tb, tx = torch.from_numpy(np.array(B.b)).cuda(), torch.from_numpy(np.array(B.x0)).cuda()
    got = ctx.solve(kind, tb, x0=tx, inplace=True, **THREE)
    assert got["k"] == -2 and tx.cpu().numpy().tobytes() == B.x0.tobytes() and tb.cpu().numpy().tobytes() == B.b.tobytes()
    with pytest.raises(RuntimeError):
        ctx.run_begin(kind)
    with pytest.raises(RuntimeError):
        ctx.run(kind)
    x, r = ctx.fetch()
    assert x.tobytes() == B.x0.tobytes() and r.tobytes() == B.b.tobytes()
    assert H.device_allocations() == live
    ctx.clear_preconditioner()


@pytest.mark.parametrize("kind", [DIAG, BLOCK])
def test_multi_rhs_refuses_the_methods(bundles, kind):
    B = bundles("transport_4099")
    install(B.ctx, kind, B.A)
    live = H.device_allocations()
    Bs, X0 = np.stack([B.b, 2.0 * B.b]), np.stack([B.x0, B.x0])
    got = B.ctx.solve_multi(Bs, X0=X0, method=kind, tol=0.0, max_iter=4)
    assert got["rc"] == -2 and got["x"].tobytes() == X0.tobytes() and got["r"].tobytes() == Bs.tobytes()
    assert H.device_allocations() == live
    B.ctx.clear_preconditioner()


def test_a_reinstall_between_two_solves_takes_effect(bundles):
    B = bundles("fem_4099")
    ctx, n = B.ctx, B.A.rows
    d = Q.diagonal(B.A)
    d2 = d * (1.0 + synth._uniform(np.arange(n, dtype=np.int64), 13))
    fresh = P.context(B.A)
    try:
        assert fresh.set_diagonal(d2) == 0
        want2 = state(fresh, fresh.solve(DIAG, B.b, x0=B.x0, **THREE))
        assert fresh.set_block_diagonal(Q.blocks_of(B.A, 4), 4) == 0
        want_b = state(fresh, fresh.solve(BLOCK, B.b, x0=B.x0, **THREE))
    finally:
        fresh.close()
    assert ctx.set_diagonal(d) == 0
    first = state(ctx, ctx.solve(DIAG, B.b, x0=B.x0, **THREE))
    assert ctx.set_diagonal(d2) == 0                                   # the same array, other values
    assert state(ctx, ctx.solve(DIAG, B.b, x0=B.x0, **THREE)) == want2 != first
    assert ctx.set_block_diagonal(Q.blocks_of(B.A, 4), 4) == 0         # the other kind
    assert state(ctx, ctx.solve(BLOCK, B.b, x0=B.x0, **THREE)) == want_b
    ctx.clear_preconditioner()


GRAPH_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
from mpi_bicgstab_amd import hipsolver as H, synth
import test_precond_gpu as P
import bicgstab2_precond_ref as Q
H.lib().bicg_comm_init_single(0)
A = synth.transport_like(4099)
idx = np.arange(A.rows, dtype=np.int64)
x0, b = 0.25 * synth._uniform(idx, 77) - 0.125, A.matvec(1.0 + 0.5 * synth._uniform(idx, 78))
opts = dict(tol=0.0, max_iter=12, record_trace=1, check_every=1)
eager = P.context(A)
os.environ["BICG_GRAPH"] = "1"
graph = P.context(A)
os.environ.pop("BICG_GRAPH")
assert eager.flags()["tail_finish"] and not graph.flags()["tail_finish"], (eager.flags(), graph.flags())
for method in ("bicgstab2_diag", "bicgstab_diag", "bicgstab2_diag", "bicgstab2_block", "bicgstab_block", "bicgstab2_block"):
    for c in (eager, graph):
        if method.endswith("diag"):
            assert c.set_diagonal(Q.diagonal(A)) == 0
        else:
            assert c.set_block_diagonal(Q.blocks_of(A, 4), 4) == 0
    want = P.state(eager, eager.solve(method, b, x0=x0, **opts))
    assert want[0] == 12
    assert P.state(graph, graph.solve(method, b, x0=x0, **opts)) == want, method
    assert eager.flags()["tail_finish"] and not graph.flags()["tail_finish"], (method, graph.flags())
eager.close(); graph.close()
print("GRAPH-OK")
"""


def test_under_graph_replay_the_methods_run_eagerly():
    """BICG_GRAPH=1 (read at bicg_create, hence a child process): methods 7 and 8 have no captured iteration; their bytes are the
    eager context's, also after methods 4 and 5 have captured and replayed their own on the same context"""
    p = subprocess.run([sys.executable, "-c", GRAPH_CHILD % dict(root=ROOT)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and "GRAPH-OK" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])


# ---- 6. the tiled form
def test_tiled_form_with_a_unit_diagonal_is_method_6(bundles):
    """transport_like(2^24 + 3), the smallest shape that reaches kVecTile; one context, nearly all of the time is building the
    matrix on the host"""
    B = bundles(f"transport_{P.TILED_FROM + 3}")
    ctx, n = B.ctx, B.A.rows
    one = dict(tol=0.0, max_iter=2, record_trace=1)
    want = state(ctx, ctx.solve("bicgstab2", B.b, x0=B.x0, **one))
    assert ctx.set_diagonal(np.ones(n)) == 0
    got = ctx.solve(DIAG, B.b, x0=B.x0, **one)
    assert got["k"] == 2 and state(ctx, got) == want
    gap = np.linalg.norm(B.b - ctx.spmv(got["x"]) - got["r"]) / np.linalg.norm(B.b)
    print("tiled: || b - A x - r || / || b || = %.3e" % gap)
    assert gap <= 1e-12
    ctx.clear_preconditioner()
