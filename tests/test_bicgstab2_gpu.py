"""`-m gpu`, one rank: BiCGStab(2), method BICG_BICGSTAB2 = 6 (Driver::iter_stab2 without a hat in csrc/bicg_solver.cpp, the PH_S2_* phases of
csrc/bicg_devfn.h, the functors of csrc/bicg_stab2.hip in their form for Precond::NONE) through Context.solve("bicgstab2") and the run_* calls.

Contexts are created under switches(persist=0), matrices, x0 and b are those of tests/test_precond_gpu.py (its Bundle), the
reference is the numpy restatement tests/bicgstab2_ref.py.
  1. exact first step   the integer systems of tests/exact_dots.py: dot_zero = (b,b), alpha[0] = (b,b)/(b,Ab) = 1/4 and beta[0] = 0 as
                        bytes -- u0 = r0 = b because alpha starts at 0, so the set-up group and the first product group are exact
  2. three sweeps       trace, x and r against the restatement. The tolerance is computed per matrix, on the restatement alone:
                        16 x the largest relative gap between its run with numpy's dots and its run with every dot accumulated in
                        np.longdouble (what another association of the dot sums does to the recurrence; the factor covers the
                        device's grouping, 256-row partials against numpy's pairwise blocks), floor 1e-12, relative to the largest
                        magnitude of the compared array. The computed values are printed (profiles/NOTES.md keeps them).
  3. invariances        as bytes: check_every, bicg_run against run_begin / run_iterate / run_end, host arrays against CUDA tensors,
                        a solve repeated, method 0 around a method 6 solve, no allocation after the first solve
  4. convergence        the convection stencils of the issue's table at (m, c) = (16, 5), (12, 20), (16, 20): no breakdown, true
                        relative residual <= 1e-9 from the fetched x, k <= 1.25 x the restatement's. The device's method 0 on the
                        same systems is printed, not asserted.
  5. edges              1 x 1 system, max_iter 0 / 1 / 7, b = 0, bicg_solve_multi refuses the method, BICG_GRAPH=1 runs it eagerly"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bicgstab2_ref as R
import exact_dots as E
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


def state(ctx, got, nan_ok=False):
    return P.state(ctx, got, nan_ok=nan_ok) + (got["result"].breakdown_iteration,)


# ---- 1. exact first step
@pytest.mark.parametrize("shape", list(E.SHAPES))
def test_first_step_is_exact(shape):
    n, groups, L, (want_groups, want_blocks) = E.SHAPES[shape]
    A, b = E.system(n, groups, L)
    F = E.first(n, groups, L)
    sliced, blocks = E.producer_units(A.ptr, n, groups)
    assert E.preconditions(F, sliced + blocks) >= 1
    ctx = P.context(synth.CSR(n, n, A.ptr, A.col, A.val))
    try:
        plan = ctx.plan_info()
        assert plan["rows"] == n and plan["row_blocks"] == want_groups + want_blocks and len(sliced) == want_groups, plan
        assert ctx.flags()["all_sell"] == (want_blocks == 0) and not ctx.flags()["persist"]
        got = ctx.solve("bicgstab2", b.astype(np.float64), tol=0.0, max_iter=2, record_trace=1)
        tr = ctx.trace(got["k"])
        print(shape, "dot_zero", got["result"].dot_zero, F.dot_zero, "alpha", tr["alpha"], "beta", tr["beta"])
        assert got["k"] == 2 and got["result"].breakdown_iteration == 0
        assert E.same_bytes(got["result"].dot_zero, F.dot_zero)
        assert E.same_bytes(tr["alpha"][0], 0.25)
        assert tr["beta"][0] == 0.0
    finally:
        ctx.close()


# ---- 2. three sweeps against the restatement
@functools.lru_cache(maxsize=None)
def reference(name):
    """(restatement's three sweeps, the matrix's tolerance, the gaps it was computed from)"""
    A, _ = P.matrix(name)
    idx = np.arange(A.rows, dtype=np.int64)
    x0, b = 0.25 * synth._uniform(idx, 77) - 0.125, A.matvec(1.0 + 0.5 * synth._uniform(idx, 78))      # (Bundle's x0 and b)
    mul = R.Product(A)
    plain, ext = R.sweeps(mul, b, x0, 6, 0.0), R.sweeps(mul, b, x0, 6, 0.0, extended=True)
    gaps = {q: R.gap(ext["trace"][q], plain["trace"][q]) for q in KEYS}
    gaps.update(x=R.gap(ext["x"], plain["x"]), r=R.gap(ext["r"], plain["r"]))
    return plain, max(16.0 * max(gaps.values()), 1e-12), gaps


@pytest.mark.parametrize("name", MATRICES)
def test_three_sweeps_against_the_restatement(bundles, name):
    B = bundles(name)
    want, tol, gaps = reference(name)
    assert B.b.tobytes() == B.A.matvec(1.0 + 0.5 * synth._uniform(np.arange(B.A.rows, dtype=np.int64), 78)).tobytes()
    got = B.ctx.solve("bicgstab2", B.b, x0=B.x0, **THREE)
    tr = B.ctx.trace(got["k"])
    print(name, "tolerance %.3e" % tol, "from the restatement's gaps", {q: "%.2e" % v for q, v in gaps.items()})
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
def stepped(B, step, **opts):
    ctx = B.ctx
    ctx.load(B.x0, B.b)
    ctx.run_begin("bicgstab2", **opts)
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


@pytest.mark.parametrize("name", INVARIANT_ON)
def test_invariances(bundles, name):
    B = bundles(name)
    ctx = B.ctx
    plain_before = state(ctx, ctx.solve("bicgstab", B.b, x0=B.x0, **REAL))
    want = state(ctx, ctx.solve("bicgstab2", B.b, x0=B.x0, check_every=1, **REAL))
    live = H.device_allocations()
    assert 2 <= want[0] <= 40 and want[0] % 2 == 0 and want[-1] == 0
    for every in (5, 40):
        assert state(ctx, ctx.solve("bicgstab2", B.b, x0=B.x0, check_every=every, **REAL)) == want, every
    assert state(ctx, ctx.solve("bicgstab2", B.b, x0=B.x0, check_every=1, **REAL)) == want, "the same solve twice"
    # one bicg_run against the stepped solve
    ctx.load(B.x0, B.b)
    res = ctx.run("bicgstab2", **REAL)
    x, r = ctx.fetch()
    assert state(ctx, dict(k=res.iterations, x=x, r=r, result=res)) == want, "bicg_run"
    got, calls = stepped(B, 2, **REAL)
    assert state(ctx, got) == want and calls >= want[0] // 2, "run_iterate(2)"
    got, calls3 = stepped(B, 3, **REAL)      # three steps round up to two sweeps
    assert state(ctx, got) == want, "run_iterate(3)"
    ctx.load(B.x0, B.b)
    ctx.run_begin("bicgstab2", **dict(REAL, tol=0.0))
    assert ctx.run_iterate(3) == 4 and ctx.run_iterate(1) == 6 and ctx.run_iterate(2) == 8
    ctx.run_end()
    # CUDA tensors
    dev = ctx.solve("bicgstab2", torch.from_numpy(np.array(B.b)).cuda(), x0=torch.from_numpy(np.array(B.x0)).cuda(), check_every=1, **REAL)
    dev["x"], dev["r"] = dev["x"].cpu().numpy(), dev["r"].cpu().numpy()
    assert state(ctx, dev) == want, "bicg_solve_device"
    assert H.device_allocations() == live
    assert state(ctx, ctx.solve("bicgstab", B.b, x0=B.x0, **REAL)) == plain_before, "method 0 after method 6"


# ---- 4. convergence where it matters
@pytest.mark.parametrize("m,c", [(16, 5), (12, 20), (16, 20)])
def test_convergence_on_convection_stencils(m, c):
    A = R.convection(m, c)
    b, x0 = R.rhs(A, 78), np.zeros(A.rows)
    mul = R.Product(A)
    want = R.sweeps(mul, b, x0, 1000, 1e-10)
    ctx = P.context(A)
    try:
        got = ctx.solve("bicgstab2", b, x0=x0, tol=1e-10, max_iter=1000)
        rel = R.true_relres(mul, b, got["x"])
        plain = ctx.solve("bicgstab", b, x0=x0, tol=1e-10, max_iter=1000)
        print("m", m, "c", c, "BiCGStab(2) k", got["k"], "restatement k", want["k"], "true relres %.3e" % rel, "| method 0: k", plain["k"],
              "breakdown", plain["result"].breakdown_iteration, "relres %.3e" % np.sqrt(plain["result"].dot_r / plain["result"].dot_zero))
        assert got["result"].breakdown_iteration == 0
        assert rel <= 1e-9, rel
        assert got["k"] <= 1.25 * want["k"], (got["k"], want["k"])
    finally:
        ctx.close()


# ---- 5. edges
def test_one_row_breaks_down_in_its_first_sweep(bundles):
    B = bundles("transport_1")
    got = B.ctx.solve("bicgstab2", B.b, x0=B.x0, tol=0.0, max_iter=12)
    assert got["k"] == 2 and got["result"].breakdown_iteration == 2, (got["k"], got["result"].breakdown_iteration)
    want = R.sweeps(B.A, B.b, B.x0, 12, 0.0)
    assert want["k"] == 2 and want["breakdown"] == 2


def test_iteration_limits(bundles):
    B = bundles("transport_4099")
    ctx = B.ctx
    for cap in (0, 1):
        got = ctx.solve("bicgstab2", B.b, x0=B.x0, tol=0.0, max_iter=cap)
        assert got["k"] == 0 and got["result"].iterations == 0 and got["x"].tobytes() == B.x0.tobytes(), cap
    got = ctx.solve("bicgstab2", B.b, x0=B.x0, tol=0.0, max_iter=7, record_trace=1)
    assert got["k"] == 6
    six = ctx.solve("bicgstab2", B.b, x0=B.x0, **THREE)
    assert state(ctx, got) == state(ctx, six)
    zero = ctx.solve("bicgstab2", np.zeros(B.A.rows), x0=np.zeros(B.A.rows), tol=1e-10, max_iter=10)
    assert zero["k"] == 0 and not zero["x"].any()


def test_multi_rhs_refuses_the_method(bundles):
    B = bundles("transport_4099")
    live = H.device_allocations()
    Bs, X0 = np.stack([B.b, 2.0 * B.b]), np.stack([B.x0, B.x0])
    got = B.ctx.solve_multi(Bs, X0=X0, method="bicgstab2", tol=0.0, max_iter=4)
    assert got["rc"] == -2 and got["x"].tobytes() == X0.tobytes() and got["r"].tobytes() == Bs.tobytes()
    assert H.device_allocations() == live


GRAPH_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
from mpi_bicgstab_amd import hipsolver as H, synth
import test_precond_gpu as P
H.lib().bicg_comm_init_single(0)
A = synth.transport_like(4099)
idx = np.arange(A.rows, dtype=np.int64)
x0, b = 0.25 * synth._uniform(idx, 77) - 0.125, A.matvec(1.0 + 0.5 * synth._uniform(idx, 78))
opts = dict(tol=0.0, max_iter=12, record_trace=1, check_every=1)
eager = P.context(A)
os.environ["BICG_GRAPH"] = "1"
graph = P.context(A)
os.environ.pop("BICG_GRAPH")
# BICG_FLAG_TAIL_FINISH is clear while a context replays captured iterations (include/bicgstab_hip.h) and comes back when a
# capture fails and the context falls back to eager launches: the one context is in graph mode, and still is after method 0
# has captured and replayed its iteration
assert eager.flags()["tail_finish"] and not graph.flags()["tail_finish"], (eager.flags(), graph.flags())
for method in ("bicgstab2", "bicgstab", "bicgstab2"):
    want = P.state(eager, eager.solve(method, b, x0=x0, **opts))
    assert want[0] == 12
    assert P.state(graph, graph.solve(method, b, x0=x0, **opts)) == want, method
    assert eager.flags()["tail_finish"] and not graph.flags()["tail_finish"], (method, graph.flags())
eager.close(); graph.close()
print("GRAPH-OK")
"""


def test_under_graph_replay_the_method_runs_eagerly():
    """BICG_GRAPH=1 (read at bicg_create, hence a child process): method 6 has no captured iteration; its bytes are the eager
    context's, also after method 0 has captured and replayed its own on the same context"""
    p = subprocess.run([sys.executable, "-c", GRAPH_CHILD % dict(root=ROOT)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and "GRAPH-OK" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])
