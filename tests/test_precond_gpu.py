"""`-m gpu`, one rank: the diagonal preconditioner and BICG_BICGSTAB_DIAG (bicg_precond_diagonal, Driver::iter_plain, the FDiag*
functors of csrc/bicg_vec.hip, csrc/bicg_precond.hip) through Context.set_diagonal / solve("bicgstab_diag").

The exact comparisons rest on two facts: multiplying by 1.0 or by a power of two is exact, and the element-wise dots depend on n
only while the product dots depend on the plan only. So
  1. with d = 1 the method must reproduce method 0 on the same context byte for byte, and
  2. with d = powers of two, method 4 on A must reproduce method 0 on A D^-1 (columns scaled, exactly), x up to the scaling.
Every context is created under switches(persist=0): the persistent kernels associate their sums in their own way, and method 4
always takes the multi-launch form.

Matrices: synth.transport_like(n) (padded 16-bit layout), synth.fem_like(n) (jagged), synth.grid7(16, 16, 16) under
BICG_PLAN=constant=0 (a stencil whose 16-row lines give it jagged slices with x windows; its columns can be scaled without changing
the plan). The plane-marching product needs constant slices, so case 1 alone also runs synth.grid7(64, 8, 8) under the default
plan, where it is in use. List-driven slices: the interior of transport_like from 4099 rows on. Sizes of transport_like: 1, 63,
257, 4099 (below a wavefront, below a workgroup, odd: the 16-byte pair tail), 40000 (many workgroups) and TILED_FROM + 3, just past
the row count from which run_vec takes its tiled form (vec_ppt() in csrc/bicg_vec.hip: n >= 1 << 24) -- that matrix has 251 M
non-zeros and is generated slab by slab, once for cases 1 and 2 (9 s and 5 s on an MI355X host, nearly all of it generating and
planning on the host)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TILED_FROM = 1 << 24      # csrc/bicg_vec.hip, vec_ppt(): rows from which vec_tiled(n) holds and run_vec launches k_vec<.., kVecTile>
NAMES = ("transport_1", "transport_63", "transport_257", "transport_4099", "transport_40000", f"transport_{TILED_FROM + 3}",
         "fem_4099", "fem_40000", "grid7", "fem_4099_reordered")
PLANES = "grid7_planes"      # case 1 only
FIXED = dict(tol=0.0, max_iter=12, record_trace=1)
REAL = dict(tol=1e-10, max_iter=1000, record_trace=1)


def transport_in_slabs(n, step=1 << 21):
    """synth.transport_like(n) built from row slabs (the generator's temporaries are 15 x 8 bytes per row, several times over)"""
    ptr, col, val, base = [np.zeros(1, dtype=np.int64)], [], [], 0
    for lo in range(0, n, step):
        S = synth.transport_like(n, rows=(lo, min(lo + step, n)))
        ptr.append(S.ptr[1:].astype(np.int64) + base)
        col.append(S.col); val.append(S.val)
        base += S.nnz
    return synth.CSR(n, n, np.concatenate(ptr).astype(np.uint32), np.concatenate(col), np.concatenate(val))


def matrix(name):
    """(A, BICG_PLAN tokens the contexts are created under)"""
    if name.startswith("transport_"):
        n = int(name.split("_")[1])
        return (transport_in_slabs(n) if n > (1 << 22) else synth.transport_like(n)), {}
    if name == PLANES:
        return synth.grid7(64, 8, 8), {}
    if name == "grid7":
        return synth.grid7(16, 16, 16), dict(constant=0)
    A = synth.fem_like(int(name.split("_")[1]))
    if name.endswith("_reordered"):
        perm = np.random.default_rng(5).permutation(A.rows).astype(np.uint32)      # a numbering without locality: reorder=1 has work to do
        return H.permute_block(H.single_rank_blocks(A), perm), dict(reorder=1)
    return A, {}


def context(A, **sw):
    H.switches(persist=0, **sw)
    try:
        return H.Context(H.single_rank_blocks(A))
    finally:
        H.switches(persist=None, **{k: None for k in sw})


def scaled_columns(A, d):
    """A D^-1: column j times 1 / d_j (exact for powers of two)"""
    return synth.CSR(A.rows, A.cols, A.ptr, A.col, A.val * (1.0 / d)[A.col])


def powers_of_two(n, seed=31):
    e = np.floor(17.0 * synth._uniform(np.arange(n, dtype=np.int64), seed)).astype(np.int64) - 8      # e_i in [-8, 8]
    return np.ldexp(1.0, e)


class Bundle:
    def __init__(self, name):
        self.A, self.sw = matrix(name)
        n = self.A.rows
        self.ctx = context(self.A, **self.sw)
        idx = np.arange(n, dtype=np.int64)
        self.x0 = 0.25 * synth._uniform(idx, 77) - 0.125
        self.b = self.A.matvec(1.0 + 0.5 * synth._uniform(idx, 78))
        self.d = powers_of_two(n)
        for a in (self.x0, self.b, self.d):
            a.setflags(write=False)
        self.ctx_b = None

    def scaled_context(self):
        if self.ctx_b is None:
            self.ctx_b = context(scaled_columns(self.A, self.d), **self.sw)
        return self.ctx_b

    def close(self):
        for c in (self.ctx, self.ctx_b):
            if c is not None:
                c.close()


@pytest.fixture(scope="module")
def bundles():
    H.lib().bicg_comm_init_single(0)
    made = {}

    def get(name):
        if name not in made:
            made[name] = Bundle(name)
        return made[name]
    yield get
    for b in made.values():
        b.close()


BREAKS_DOWN = "transport_1"      # a 1 x 1 system is solved exactly half way through its first iteration: omega = 0 / 0


def raw(a, nan_ok=False):
    """the bytes of an array. nan_ok (BREAKS_DOWN only): every NaN as the one canonical quiet NaN -- the sign and payload of an invalid
    operation's result are not defined by IEEE 754 and differ between two kernels that evaluate the same expression. Everywhere
    else a NaN is a failure of its own: no other system of this file breaks down, and a NaN must not pass for a value."""
    a = np.array(a, dtype=np.float64)
    if nan_ok:
        a[np.isnan(a)] = np.nan
    else:
        assert not np.isnan(a).any(), "a NaN in what a solve reports"
    return a.tobytes()


def state(ctx, got, with_x=True, nan_ok=False):
    """everything a solve reports, as bytes"""
    k, q = got["k"], got["result"]
    tr = ctx.trace(k)
    return (k, q.iterations, raw(q.dot_r, nan_ok), raw(q.dot_zero, nan_ok), raw(got["x"], nan_ok) if with_x else b"",
            raw(got["r"], nan_ok), tuple(raw(tr[key], nan_ok) for key in ("alpha", "omega", "beta", "dotr")))


def test_layouts_are_the_ones_the_cases_are_about(bundles):
    t = bundles("transport_40000").ctx
    f = t.flags()
    assert f["col16"] and not f["jagged"] and f["all_sell"] and t.uniform_entries() > 0      # padded, 16-bit, list-driven slices
    f = bundles("fem_40000").ctx.flags()
    assert f["jagged"] and f["window"]
    g = bundles("grid7").ctx
    assert g.constant_entries() == 0 and not g.stencil_info()["on"]
    assert bundles(PLANES).ctx.stencil_info()["on"]
    assert bundles("fem_4099_reordered").ctx.flags()["reordered"]


# ---- 1. d = 1
@pytest.mark.parametrize("name", NAMES + (PLANES,))
def test_unit_diagonal_is_the_plain_method_bit_for_bit(bundles, name):
    B = bundles(name)
    ctx = B.ctx
    assert ctx.set_diagonal(np.ones(B.A.rows)) == 0 and ctx.preconditioner() == "diagonal"
    plain = ctx.solve("bicgstab", B.b, x0=B.x0, **FIXED)
    want = state(ctx, plain, nan_ok=name == BREAKS_DOWN)
    diag = ctx.solve("bicgstab_diag", B.b, x0=B.x0, **FIXED)
    got = state(ctx, diag, nan_ok=name == BREAKS_DOWN)
    assert 1 <= plain["k"] <= 12 and got[0] == want[0]
    assert got == want


# ---- 2. d = powers of two
@pytest.mark.parametrize("name", NAMES)
def test_power_of_two_diagonal_is_the_plain_method_on_the_scaled_columns(bundles, name):
    B = bundles(name)
    ca, cb = B.ctx, B.scaled_context()
    # the comparison is void unless both matrices got the same plan and the same product kernel
    assert ca.flags() == cb.flags()
    assert ca.plan_info() == cb.plan_info()
    masks = []
    for c in (ca, cb):
        H.product_kernels(reset=True)
        c.spmv(B.x0)
        masks.append(H.product_kernels(reset=True))
    assert masks[0] == masks[1] and masks[0]
    assert ca.set_diagonal(B.d) == 0
    got = ca.solve("bicgstab_diag", B.b, x0=B.x0, **FIXED)
    want = cb.solve("bicgstab", B.b, x0=B.d * B.x0, **FIXED)
    assert np.any(B.x0 != 0.0)
    nan_ok = name == BREAKS_DOWN
    assert state(ca, got, with_x=False, nan_ok=nan_ok) == state(cb, want, with_x=False, nan_ok=nan_ok)
    assert raw(got["x"], nan_ok) == raw(want["x"] / B.d, nan_ok)


# ---- 3. a real diagonal
def reference_diag_bicgstab(A, d, b, x0, tol, max_iter):
    """float64 numpy restatement of the right-preconditioned recurrence (the loop of reference
    src/solver.c:74-120 with p^ = p / d and q^ = q / d): (k, x, alphas, omegas)"""
    dinv = 1.0 / d
    x = x0.copy()
    r = b - A.matvec(x)
    rh, p = r.copy(), r.copy()
    ph = dinv * p
    rr = r0 = rtr = float(r @ r)
    k, alphas, omegas = 0, [], []
    while rr > tol * tol * r0 and k < max_iter:
        s = A.matvec(ph)
        alpha = rtr / float(rh @ s)
        q = r - alpha * s
        qh = dinv * q
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
        ph = dinv * p
    return k, x, np.array(alphas), np.array(omegas)


def relres(A, x, b):
    return float(np.linalg.norm(b - A.matvec(x)) / np.linalg.norm(b))


@pytest.mark.parametrize("kind,k_ref", [("transport", 8), ("fem", 5)])
def test_jacobi_on_a_badly_scaled_matrix(kind, k_ref):
    """A <- D A D with scale_decades=4, 20000 rows, d = diag(A), b = A 1, x0 = 0, tol 1e-10, max_iter 1000. The CPU reference
    converges in 8 (transport_like) and 5 (fem_like) iterations and reaches a true relative residual ||b - A x|| / ||b|| of
    9.03e-11 (transport_like) and 4.33e-11 (fem_like); plain BiCGStab does not converge in 1000 iterations (1.0e-6 to 1.5e-6).
    The device's k may differ by the last iteration (summation order), its true residual by the same cause: 10 x."""
    H.lib().bicg_comm_init_single(0)
    gen = synth.transport_like if kind == "transport" else synth.fem_like
    A = gen(20000, scale_decades=4)
    d, missing = H.csr_diagonal(A)
    assert missing == 0
    b, x0 = A.matvec(np.ones(A.rows)), np.zeros(A.rows)
    k_cpu, x_cpu, al, om = reference_diag_bicgstab(A, d, b, x0, REAL["tol"], REAL["max_iter"])
    ref_res = relres(A, x_cpu, b)
    print(f"{kind}: CPU reference k = {k_cpu}, true relative residual {ref_res:.3e}")
    assert k_cpu == k_ref
    ctx = context(A)
    try:
        plain = ctx.solve("bicgstab", b, **REAL)
        print(f"{kind}: plain k = {plain['k']}, recursive residual {np.sqrt(plain['dot_r'] / plain['dot_zero']):.3e}")
        assert ctx.set_diagonal(d) == 0
        got = ctx.solve("bicgstab_diag", b, **REAL)
        tr = ctx.trace(got["k"])
        res = relres(A, got["x"], b)
        print(f"{kind}: preconditioned k = {got['k']}, true relative residual {res:.3e}")
        assert plain["k"] == 1000
        assert abs(got["k"] - k_cpu) <= 2
        assert res <= 10.0 * ref_res
        np.testing.assert_allclose(tr["alpha"][:4], al[:4], rtol=1e-9, atol=0.0)
        np.testing.assert_allclose(tr["omega"][:4], om[:4], rtol=1e-9, atol=0.0)
    finally:
        ctx.close()


# ---- 4. interface
@pytest.fixture(scope="module")
def fem():
    """(A, d, x0, b) of the badly scaled fem_like(20000) and a context on it; the tests leave the context without a preconditioner"""
    H.lib().bicg_comm_init_single(0)
    A = synth.fem_like(20000, scale_decades=4)
    d, _ = H.csr_diagonal(A)
    b = A.matvec(np.ones(A.rows))
    x0 = 0.01 * synth._uniform(np.arange(A.rows, dtype=np.int64), 3)
    for a in (d, b, x0):
        a.setflags(write=False)
    ctx = context(A)
    yield A, d, x0, b, ctx
    ctx.close()


def test_method_without_a_preconditioner_is_refused_and_touches_nothing(fem):
    A, d, x0, b, ctx = fem
    ctx.clear_preconditioner()
    assert ctx.preconditioner() is None
    ctx.load(x0, b)
    o, res = ctx.options(quiet=1), H.Result()
    L = H.lib()
    assert L.bicg_run(ctx.h, H.METHODS["bicgstab_diag"], C.byref(o), C.byref(res)) == -2
    assert L.bicg_run_begin(ctx.h, H.METHODS["bicgstab_diag"], C.byref(o)) == -2
    x, r = ctx.fetch()
    assert x.tobytes() == x0.tobytes() and r.tobytes() == b.tobytes()
    got = ctx.solve("bicgstab_diag", b, x0=x0)
    assert got["k"] == -2 and got["x"].tobytes() == x0.tobytes() and got["r"].tobytes() == b.tobytes()
    tb, tx = torch.from_numpy(np.array(b)).cuda(), torch.from_numpy(np.array(x0)).cuda()
    got = ctx.solve("bicgstab_diag", tb, x0=tx, inplace=True)
    assert got["k"] == -2 and tx.cpu().numpy().tobytes() == x0.tobytes() and tb.cpu().numpy().tobytes() == b.tobytes()
    x, r = ctx.fetch()
    assert x.tobytes() == x0.tobytes() and r.tobytes() == b.tobytes()
    # the binding does not drop the refusal: after a run_begin that began nothing, run_iterate would go on with the solve before
    with pytest.raises(RuntimeError):
        ctx.run_begin("bicgstab_diag")
    with pytest.raises(RuntimeError):
        ctx.run("bicgstab_diag")
    x, r = ctx.fetch()
    assert x.tobytes() == x0.tobytes() and r.tobytes() == b.tobytes()


def test_graph_replay_follows_the_preconditioner_through_clear_and_install(fem):
    """BICG_GRAPH=1: the captured iteration of method 4 holds the address of 1/d. Solve (two eager iterations, then capture and
    replay), clear, install ANOTHER d -- into a new array; the freed one is handed to someone else and filled with NaN first --,
    solve: the bytes of the eager context with that d. Then an install into the existing array, which keeps the graph."""
    A, d, x0, b, _ = fem
    d2 = d * (1.0 + synth._uniform(np.arange(A.rows, dtype=np.int64), 13))
    opts = dict(tol=0.0, max_iter=10, record_trace=1, check_every=1)
    eager = context(A)
    os.environ["BICG_GRAPH"] = "1"
    try:
        graph = context(A)
    finally:
        os.environ.pop("BICG_GRAPH", None)
    try:
        want = {}
        for key, dd in (("d", d), ("d2", d2)):
            assert eager.set_diagonal(dd) == 0
            want[key] = state(eager, eager.solve("bicgstab_diag", b, x0=x0, **opts))
        assert want["d"] != want["d2"]
        assert graph.set_diagonal(d) == 0
        assert state(graph, graph.solve("bicgstab_diag", b, x0=x0, **opts)) == want["d"]
        assert graph.clear_preconditioner() == 0
        squatters = [torch.full((A.rows,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        assert graph.set_diagonal(d2) == 0
        assert state(graph, graph.solve("bicgstab_diag", b, x0=x0, **opts)) == want["d2"]
        assert graph.set_diagonal(d) == 0                            # the same array: the captured iteration stays and reads the new values
        assert state(graph, graph.solve("bicgstab_diag", b, x0=x0, **opts)) == want["d"]
        del squatters
    finally:
        eager.close(); graph.close()


JACOBI_DROPIN = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %(root)r)
from mpi_bicgstab_amd import hipsolver as H, synth
L = H.lib()
L.bicg_comm_init_single(0)
A = synth.from_offsets(30011, (0, 1, -1, 37, -37, 2999, -2999), 9.0, seed=5, scale_decades=2.0)
blk = H.single_rank_blocks(A)
b = A.matvec(np.ones(A.rows))
dp = C.POINTER(C.c_double)
def call(fn):
    x, r = np.zeros(A.rows), b.copy()
    k = fn(C.byref(blk.diag), C.byref(blk.offd), C.byref(blk.info), x.ctypes.data_as(dp), r.ctypes.data_as(dp))
    return k, x, r
call(L.jacobi_bicgstab)                                   # diag(A1) installed on the resident context
rowid = np.repeat(np.arange(A.rows), np.diff(A.ptr.astype(np.int64)))
on = A.col.astype(np.int64) == rowid
blk._keep[0][on] *= 1.0 + 2.0 * synth._uniform(np.arange(A.rows, dtype=np.int64), 3)      # in place: same arrays, same pattern, another diagonal
call(L.bicgstab)                                          # cache mode 2: refreshes the resident context, leaves the preconditioner alone
k, x, r = call(L.jacobi_bicgstab)                         # ... a full hit: must run with diag(A2)
ctx = L.bicg_dropin_context(C.byref(blk.diag), C.byref(blk.offd), C.byref(blk.info))
ones = np.ones(A.rows)
assert L.bicg_precond_diagonal(C.c_void_p(ctx), ones.ctypes.data_as(dp)) == 0       # the caller's own diagonal on the resident context
k2, x2, r2 = call(L.jacobi_bicgstab)
h, m = C.c_uint(0), C.c_uint(0)
L.bicg_dropin_stats(C.byref(h), C.byref(m))
L.bicg_dropin_release()
np.savez(sys.argv[1], k=k, x=x, r=r, k2=k2, x2=x2, r2=r2, refreshes=H.dropin_refreshes(), hits=h.value, misses=m.value)
"""


def _jacobi_child(tmp_path, tag, cache):
    env = {k: v for k, v in os.environ.items() if k != "BICG_DROPIN_CACHE"}
    env.update(BICG_QUIET="1", BICG_MAX_ITER="40", BICG_TOL="1e-10", BICG_DROPIN_CACHE=cache)
    out = str(tmp_path / (tag + ".npz"))
    p = subprocess.run([sys.executable, "-c", JACOBI_DROPIN % dict(root=ROOT), out], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return np.load(out)


def test_jacobi_bicgstab_after_a_refresh_and_after_a_diagonal_of_the_callers(tmp_path):
    """the drop-in cache is read once per process: children. jacobi(A1); the diagonal edited in place; bicgstab(A2), which under
    BICG_DROPIN_CACHE=2 refreshes the resident context's values; jacobi(A2), a full hit -- it must solve with diag(A2), as the
    child that creates a context per call does; and again after the caller put a diagonal of its own on the resident context."""
    off, refresh = _jacobi_child(tmp_path, "off", "0"), _jacobi_child(tmp_path, "refresh", "2")
    assert int(refresh["refreshes"]) == 1 and int(refresh["hits"]) >= 2 and int(off["refreshes"]) == 0
    for tag in ("", "2"):
        assert int(refresh["k" + tag]) == int(off["k" + tag]) == int(off["k"])
        assert refresh["x" + tag].tobytes() == off["x" + tag].tobytes() == off["x"].tobytes()
        assert refresh["r" + tag].tobytes() == off["r" + tag].tobytes()
    assert not np.isnan(off["x"]).any()


def test_refused_diagonals_leave_the_previous_one_and_installs_allocate_once(fem):
    A, d, x0, b, ctx = fem
    ctx.clear_preconditioner()
    ctx.solve("bicgstab", b, x0=x0, **REAL)      # (the trace buffer grows with the first solve of this max_iter: not what is counted here)
    before = H.device_allocations()
    for bad in (0.0, np.inf, np.nan):       # nothing installed yet: refused, still nothing
        dd = np.array(d); dd[A.rows // 3] = bad
        assert ctx.set_diagonal(dd) == 1 and ctx.preconditioner() is None
    assert H.device_allocations() == before
    assert ctx.set_diagonal(d) == 0
    assert H.device_allocations() == before + 1
    want = state(ctx, ctx.solve("bicgstab_diag", b, x0=x0, **REAL))
    for bad, at in ((0.0, 0), (-0.0, 1), (np.inf, A.rows - 1), (-np.inf, 64), (np.nan, A.rows // 2)):
        dd = np.array(d); dd[at] = bad
        assert ctx.set_diagonal(dd) == 1 and ctx.preconditioner() == "diagonal"
        assert state(ctx, ctx.solve("bicgstab_diag", b, x0=x0, **REAL)) == want
    assert ctx.set_diagonal(d) == 0                                  # a second install of the same d
    assert H.device_allocations() == before + 1
    assert state(ctx, ctx.solve("bicgstab_diag", b, x0=x0, **REAL)) == want
    assert ctx.set_diagonal(None) == -1 and ctx.preconditioner() == "diagonal"
    assert ctx.clear_preconditioner() == 0 and ctx.preconditioner() is None
    assert H.device_allocations() == before


def test_update_values_then_install_equals_a_fresh_context(fem):
    A, d, x0, b, _ = fem
    A1 = synth.fem_like(4099, scale_decades=2)
    A2 = synth.CSR(A1.rows, A1.cols, A1.ptr, A1.col, A1.val * (1.0 + 0.25 * synth._uniform(np.arange(A1.nnz, dtype=np.int64), 9)))
    d1, d2 = H.csr_diagonal(A1)[0], H.csr_diagonal(A2)[0]
    bb = A2.matvec(np.ones(A2.rows))
    ctx, fresh = context(A1), context(A2)
    try:
        assert ctx.set_diagonal(d1) == 0
        stale = ctx.solve("bicgstab_diag", bb, **REAL)
        assert ctx.update_values(A2) == 0
        assert ctx.preconditioner() == "diagonal"                    # update_values never touches it
        assert ctx.set_diagonal(d2) == 0
        assert fresh.set_diagonal(d2) == 0
        got, want = ctx.solve("bicgstab_diag", bb, **REAL), fresh.solve("bicgstab_diag", bb, **REAL)
        assert state(ctx, got) == state(fresh, want)
        assert got["x"].tobytes() != stale["x"].tobytes()
    finally:
        ctx.close(); fresh.close()


def test_install_from_a_tensor_filled_on_a_side_stream(fem):
    A, d, x0, b, ctx = fem
    assert ctx.set_diagonal(d) == 0
    want = state(ctx, ctx.solve("bicgstab_diag", b, x0=x0, **REAL))
    assert ctx.set_diagonal(np.ones(A.rows)) == 0                    # something else in between
    src = torch.from_numpy(np.array(d)).cuda()
    m = torch.ones((2048, 2048), dtype=torch.float64, device="cuda")
    t = torch.full((A.rows,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(4):
            m = (m @ m) * 1.0e-4                                     # the stream is busy when the fill is enqueued
        t.copy_(src)
    assert ctx.set_diagonal(t, stream=side) == 0
    assert state(ctx, ctx.solve("bicgstab_diag", b, x0=x0, **REAL)) == want
    torch.cuda.synchronize()
    ctx.clear_preconditioner()


def test_solve_on_tensors_is_the_host_solve(fem):
    A, d, x0, b, ctx = fem
    assert ctx.set_diagonal(d) == 0
    want = ctx.solve("bicgstab_diag", b, x0=x0, **REAL)
    ws = state(ctx, want)
    got = ctx.solve("bicgstab_diag", torch.from_numpy(np.array(b)).cuda(), x0=torch.from_numpy(np.array(x0)).cuda(), **REAL)
    got["x"], got["r"] = got["x"].cpu().numpy(), got["r"].cpu().numpy()
    assert state(ctx, got) == ws
    ctx.clear_preconditioner()


def test_jacobi_bicgstab_drop_in(fem):
    A, d, _, b, ctx = fem
    assert ctx.set_diagonal(d) == 0
    want = ctx.solve("bicgstab_diag", b, tol=1e-10, max_iter=1000)
    ctx.clear_preconditioner()
    assert abs(want["k"] - 5) <= 2
    L = H.lib()
    blk = H.single_rank_blocks(A)
    x, r = np.zeros(A.rows), np.array(b)
    os.environ.update(BICG_TOL="1e-10", BICG_MAX_ITER="1000", BICG_QUIET="1")
    H.switches(persist=0)
    try:
        L.bicg_dropin_release()
        for _ in range(2):                                           # created, then reused with the diagonal in place
            x[:] = 0.0; r[:] = b
            k = L.jacobi_bicgstab(C.byref(blk.diag), C.byref(blk.offd), C.byref(blk.info), H._d(x), H._d(r))
            assert k == want["k"]
            assert x.tobytes() == want["x"].tobytes() and r.tobytes() == want["r"].tobytes()
        # the plain drop-in on the same resident context is unaffected by the installed diagonal
        x[:] = 0.0; r[:] = b
        os.environ["BICG_MAX_ITER"] = "20"
        assert L.bicgstab(C.byref(blk.diag), C.byref(blk.offd), C.byref(blk.info), H._d(x), H._d(r)) == 20
    finally:
        for k_ in ("BICG_TOL", "BICG_MAX_ITER", "BICG_QUIET"):
            os.environ.pop(k_, None)
        L.bicg_dropin_release()
