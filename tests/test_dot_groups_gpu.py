"""`-m gpu`: every finish of a dot group (csrc/bicg_reduce.h: arrival tickets, tail finish, hand-over, consumer-side finish, and
the persistent launches' tables) against an EXACT answer, at the workgroup counts where the finishes change shape: fewer than,
exactly and more than the 32 shards, a shard of one member or two, 4 x workgroups partials per wavefront crossing 32, and groups
whose partial slots are filled by two launches (sliced-ELL groups, then CSR row blocks).

The systems are those of tests/exact_dots.py: integer data for which dot_zero, alpha[0] = 1/4 and omega[0] of the first iteration
have one right answer as bytes whatever the association of the sums, so a missing, doubled or misplaced partial cannot pass;
tests/test_exact_dots.py checks without a GPU that no producer's partial is zero and pins the plans. (r, r) and beta of the first
iteration are compared with a rational replay within derived bounds (exact_dots.residual_dots). Every context also takes
ctx.dot(u, v) of two integer vectors -- the element-wise kernel's own finish -- against the integer sum.

One context per (shape, setting); a setting's run of a shape is made once and shared by the tests (`run`). Settings:
  default      persist=0 (a matrix this small would otherwise run plain BiCGStab as one persistent launch). One launch per product:
               hand-over on the shapes without long rows. Two launches: tail finish where the second launch has min(all, 32)
               workgroups or more, else arrival tickets (spmv(), csrc/bicg_solver.cpp)
  tickets      BICG_TAIL_FINISH=0: arrival tickets everywhere
  handover0    BICG_PLAN="handover=0": the producer finishes the group itself (tail finish / tickets as above)
  comm0/comm1  BICG_TEST="force-comm" on the trivial transport with BICG_OVERLAP=0 / 1 (tests/test_comm_path_one_gpu.py): the sums
               are left in Scal::red for the all-reduce and the apply kernel
  persistent   no persist=0, wherever the context then reports `persist`: the persistent launch's tables
  pipe0/pipe1  pipe_bicgstab with BICG_PLAN="fuse-pipe=0" / "fuse-pipe=1": consumer-side finish (wave_publish, finish_sum_shard,
               finish_group), the consuming kernel an element-wise one / the product with the phase in its epilogue

What the pipelined solver's first scalars are (PH_INIT_ALPHA, PH_OMEGA in csrc/bicg_devfn.h, Driver::init and iter_pipe in
csrc/bicg_solver.cpp, FPipe1 in csrc/bicg_vec.hip): init leaves r = b, w = A b and (r, w) -> alpha = (b, b)/(b, Ab) = 1/4, which is
the alpha the first iteration uses and the trace records; t = A w. Phase 1 starts from p = s = z = 0 and beta = omega = 0, so
p = b, s = w = Ab, z = t = A(Ab), q = b - Ab/4 and y = w - z/4 = Ab - A(Ab)/4, all exact; that y is A q entry for entry, so (q, y)
and (y, y) are the plain solver's exact (y, s) and (y, y) and omega[0] = (q, y)/(y, y) is the same correctly rounded quotient. The
(r, w) group has one partial per wavefront of the product -- nparts = 4 x row groups, 28 / 32 / 36 at n = 1792 / 2048 / 2049 --
and is the only check of wave_publish / finish_sum_shard at those counts.

Default, tickets and handover0 must agree in k, x, r and the whole three-iteration trace as bytes: the same slots, shard
membership and order under every finish -- the claim that lets spmv() pick the finish by the launch geometry."""
import functools
import os

import numpy as np
import pytest

import exact_dots as E
import mp_workers
from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import synth

pytestmark = pytest.mark.gpu
SOLVE = dict(tol=0.0, max_iter=3, check_every=3, record_trace=1)
WALL_LIMIT = 240.0      # seconds for a two-rank case (tests/test_update_values_ranks_gpu.py)

# setting -> (tokens, variables, solver)
SETTINGS = {
    "default": (dict(persist=0), {}, "bicgstab"),
    "tickets": (dict(persist=0), dict(BICG_TAIL_FINISH="0"), "bicgstab"),
    "handover0": (dict(persist=0, handover=0), {}, "bicgstab"),
    "comm0": (dict(persist=0, force_comm=1), dict(BICG_GRAPH="0", BICG_OVERLAP="0"), "bicgstab"),
    "comm1": (dict(persist=0, force_comm=1), dict(BICG_GRAPH="0", BICG_OVERLAP="1"), "bicgstab"),
    "persistent": (dict(), {}, "bicgstab"),
    "pipe0": (dict(persist=0, fuse_pipe=0), {}, "pipe_bicgstab"),
    "pipe1": (dict(persist=0, fuse_pipe=1), {}, "pipe_bicgstab"),
}
PLAIN = ("default", "tickets", "handover0", "comm0", "comm1")


@pytest.fixture(scope="module", autouse=True)
def _single_rank():
    H.lib().bicg_comm_init_single(0)      # (once: a new communicator orphans the contexts of the one before)
    yield


def integer_vectors(n):
    i = np.arange(n)
    return 1 + i % 7, 1 + i % 5


@functools.lru_cache(maxsize=None)
def run(shape, setting):
    """everything one context of `shape` created under `setting` reports; tokens and variables are put back whatever happens"""
    n, groups, L, _ = E.SHAPES[shape]
    A, b = E.system(n, groups, L)
    tokens, variables, method = SETTINGS[setting]
    saved = {k: os.environ.get(k) for k in variables}
    H.switches(**tokens)
    os.environ.update(variables)
    try:
        ctx = H.Context(H.single_rank_blocks(synth.CSR(n, n, A.ptr, A.col, A.val)))
    finally:
        H.switches(**{k: None for k in tokens})
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        out = dict(flags=ctx.flags(), plan=ctx.plan_info())
        if setting == "persistent" and not out["flags"]["persist"]:
            return out
        H.product_kernels()
        got = ctx.solve(method, b.astype(np.float64), **SOLVE)
        out["kernels"] = H.product_kernels()
        tr = ctx.trace(got["k"])
        out.update(k=got["k"], x=got["x"].tobytes(), r=got["r"].tobytes(), trace=tuple(tr[key].tobytes() for key in ("alpha", "omega", "beta", "dotr")),
                   dot_zero=got["result"].dot_zero, alpha=tr["alpha"][0], omega=tr["omega"][0], beta=tr["beta"][0], dotr=tr["dotr"][0],
                   allreduces=ctx.comm_counts()["allreduces"])
        u, v = integer_vectors(n)
        out["dot"] = ctx.dot(u.astype(np.float64), v.astype(np.float64))
        return out
    finally:
        ctx.close()


def check_geometry(shape, got):
    """the workgroup counts the case is there for, from the context itself"""
    n, groups, L, (want_groups, want_blocks) = E.SHAPES[shape]
    A, _ = E.system(n, groups, L)
    sliced, _ = E.producer_units(A.ptr, n, groups)
    assert got["plan"]["rows"] == n and got["plan"]["row_blocks"] == want_groups + want_blocks, got["plan"]
    assert got["plan"]["sell_rows"] == sum(hi - lo for lo, hi in sliced) and len(sliced) == want_groups, got["plan"]
    assert got["flags"]["all_sell"] == (want_blocks == 0) and not got["flags"]["p2p"], got["flags"]


def check_exact(shape, got):
    F = E.first(*E.SHAPES[shape][:3])
    print(shape, "dot_zero", got["dot_zero"], F.dot_zero, "alpha", got["alpha"], "omega", got["omega"].hex(), F.omega.hex())
    assert got["k"] == 3
    assert E.same_bytes(got["dot_zero"], F.dot_zero), (got["dot_zero"], F.dot_zero)
    assert E.same_bytes(got["alpha"], F.alpha), (got["alpha"], F.alpha)
    assert E.same_bytes(got["omega"], F.omega), (got["omega"], F.omega)
    u, v = integer_vectors(len(F.b))
    assert E.same_bytes(got["dot"], float(E.isum(u * v))), (got["dot"], E.isum(u * v))
    return F


@functools.lru_cache(maxsize=None)
def residual_reference(shape):
    return E.residual_dots(E.first(*E.SHAPES[shape][:3]))


@pytest.mark.parametrize("setting", PLAIN)
@pytest.mark.parametrize("shape", list(E.SHAPES))
def test_plain_first_iteration(shape, setting):
    got = run(shape, setting)
    check_geometry(shape, got)
    fl, one_launch = got["flags"], E.SHAPES[shape][3][1] == 0
    assert not fl["persist"], fl
    assert fl["tail_finish"] == (setting != "tickets"), fl
    assert fl["handover"] == (one_launch and setting == "default"), fl
    if setting.startswith("comm"):
        assert fl["overlap"] == (setting == "comm1") and got["allreduces"] > 0, (fl, got["allreduces"])
    else:
        assert got["allreduces"] == 0
    assert ("csr" in got["kernels"]) == (not one_launch), got["kernels"]
    check_exact(shape, got)
    R = residual_reference(shape)
    print("dotr", got["dotr"], float(R["dotr"]), "bound", float(R["dotr_bound"]), "beta", got["beta"], float(R["beta"]), "bound", float(R["beta_bound"]))
    assert E.within(got["dotr"], R["dotr"], R["dotr_bound"]), (got["dotr"], float(R["dotr"]), float(R["dotr_bound"]))
    assert E.within(got["beta"], R["beta"], R["beta_bound"]), (got["beta"], float(R["beta"]), float(R["beta_bound"]))


@pytest.mark.parametrize("shape", list(E.SHAPES))
def test_every_finish_gives_the_same_bytes(shape):
    want = run(shape, "default")
    for setting in ("tickets", "handover0"):
        got = run(shape, setting)
        for key in ("k", "x", "r", "trace"):
            assert got[key] == want[key], (shape, setting, key)


@pytest.mark.parametrize("setting", ["pipe0", "pipe1"])
@pytest.mark.parametrize("shape", list(E.SHAPES))
def test_pipelined_first_scalars(shape, setting):
    got = run(shape, setting)
    check_geometry(shape, got)
    one_launch = E.SHAPES[shape][3][1] == 0
    assert not got["flags"]["persist"]
    fused = one_launch and setting == "pipe1"      # (a product of two launches keeps the phases as separate kernels whatever the token says)
    assert got["flags"]["fuse_pipe"] == fused, got["flags"]
    assert ("sell_epilogue" in got["kernels"]) == fused, got["kernels"]
    check_exact(shape, got)


def test_persistent_launches():
    """the default context of every shape that is planned as persistent launches: the same exact answers from its own tables"""
    ran = []
    for shape in E.SHAPES:
        got = run(shape, "persistent")
        if not got["flags"]["persist"]:
            continue
        check_geometry(shape, got)
        check_exact(shape, got)
        R = residual_reference(shape)
        assert E.within(got["dotr"], R["dotr"], R["dotr_bound"]) and E.within(got["beta"], R["beta"], R["beta_bound"]), shape
        ran.append(shape)
    print("persistent:", ran)
    assert len([s for s in ran if not E.SHAPES[s][1]]) >= 8, ran      # the shapes without long rows are what the persistent plan is for


@pytest.mark.parametrize("shape", list(E.RANK_SHAPES))
def test_two_ranks(shape):
    """two ranks on the host-staged transport (tests/mp_dot_workers.py): interior launches, then halo-touching ones of one or two
    workgroups in the same dot group; every rank reports the whole matrix's exact scalars"""
    import mp_dot_workers as W
    skips = mp_workers.run_ranks(W.dot_worker, 2, shape, WALL_LIMIT)
    assert not skips, skips
