"""`-m gpu`: plain BiCGStab with its dot groups closed by hand-over against the same library
with BICG_PLAN="handover=0", where the producing kernel's last workgroup finishes the group and applies the recurrence itself.
Both paths add the same partial sums in the same order and run the same recurrence code, so everything is compared BIT FOR BIT
(as bytes: a NaN equals itself) -- x, r, the result's scalars and the per-iteration trace of alpha, omega, beta, (r,r).

Two contexts per matrix in one process, created under the two settings; BICG_PERSIST="0" for both, because a matrix this small
would otherwise run plain BiCGStab as one persistent launch, which has no dot groups to hand over. The shapes:
  7-point stencil, m = 12     1 728 rows: 7 row groups and 4 element-wise workgroups -- fewer producers than the 32 shards.
                              Created with layout=pad, constant=0, masked=0 (left alone the plan gives a block this small
                              jagged slices with an x window): padded slices with 16-bit offsets and streamed values are the
                              layout whose product has the hand-over epilogue (the flag `handover` is asserted).
  5 diagonals, n = 70 001     odd n: the element-wise kernels' single trailing element; 274 row groups = 8-9 members per shard,
                              the last group partly filled.
  3 diagonals, n = 1 100 003  more than 2 048 x 256 element pairs: the element-wise grid is capped and strides; x/r has 2 048
                              partials, the product 4 297.
"""
import numpy as np
import pytest

from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import synth

pytestmark = pytest.mark.gpu
K = 12


def _context(A, **sw):
    """a context created under the given tokens; the tokens are cleared again whatever happens"""
    H.switches(**sw)
    try:
        return H.Context(H.single_rank_blocks(A))
    finally:
        H.switches(**{k: None for k in sw})


def _matrix(name):
    if name == "stencil12":
        return synth.stencil7(12), dict(layout="pad", constant=0, masked=0)
    if name == "diag70001":
        return synth.from_offsets(70001, (-300, -1, 0, 1, 257), diag_base=3.0, seed=11), {}
    return synth.from_offsets(1100003, (-1, 0, 1), diag_base=1.5, seed=12), {}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def scalars(ctx, got):
    r = got["result"]
    tr = ctx.trace(got["k"])
    return (got["k"], r.iterations, r.breakdown_iteration, np.float64(r.dot_r).tobytes(), np.float64(r.dot_zero).tobytes(),
            tuple(tr[k].tobytes() for k in ("alpha", "omega", "beta", "dotr")))


def assert_same_solve(ca, a, cb, b, what):
    assert scalars(ca, a) == scalars(cb, b), what
    assert same_bits(a["x"], b["x"]), what
    assert same_bits(a["r"], b["r"]), what


@pytest.fixture(scope="module", params=["stencil12", "diag70001", "diag1100003"])
def pair(request):
    """(A, b, hand-over context, handover=0 context, the tokens both were created under)"""
    H.lib().bicg_comm_init_single(0)
    A, sw = _matrix(request.param)
    hand, ref = _context(A, persist=0, **sw), _context(A, persist=0, handover=0, **sw)
    b = ref.spmv(np.ones(A.rows))
    yield A, b, hand, ref, sw
    hand.close()
    ref.close()


def test_paths_and_shapes(pair):
    A, _, hand, ref, _ = pair
    assert A.rows in (1728, 70001, 1100003)
    assert hand.flags()["handover"] and not ref.flags()["handover"]
    assert not hand.flags()["persist"] and not ref.flags()["persist"]


def test_twelve_iterations_bit_for_bit(pair):
    A, b, hand, ref, _ = pair
    want = ref.solve("bicgstab", b, tol=0.0, max_iter=K)
    got = hand.solve("bicgstab", b, tol=0.0, max_iter=K)
    assert got["k"] == K and want["k"] == K
    assert_same_solve(hand, got, ref, want, "hand-over against handover=0")
    again = hand.solve("bicgstab", b, tol=0.0, max_iter=K)
    assert_same_solve(hand, again, hand, got, "run to run")


def test_stops_inside_a_check_interval(pair):
    """max_iter = 7 with the host looking every 16 iterations: the device raises `done` itself and the launches that follow store
    nothing, on either path"""
    A, b, hand, ref, _ = pair
    want = ref.solve("bicgstab", b, tol=0.0, max_iter=7, check_every=16)
    got = hand.solve("bicgstab", b, tol=0.0, max_iter=7, check_every=16)
    assert got["k"] == 7
    assert_same_solve(hand, got, ref, want, "max_iter = 7")


def test_time_kernels_same_bits(pair):
    A, b, hand, _, _ = pair
    plain = hand.solve("bicgstab", b, tol=0.0, max_iter=K)
    timed = hand.solve("bicgstab", b, tol=0.0, max_iter=K, time_kernels=1)
    assert timed["result"].spmv_launches > 0
    assert_same_solve(hand, timed, hand, plain, "time_kernels = 1")


@pytest.fixture(scope="module")
def small():
    H.lib().bicg_comm_init_single(0)
    A, sw = _matrix("stencil12")
    hand, ref = _context(A, persist=0, **sw), _context(A, persist=0, handover=0, **sw)
    b = ref.spmv(np.ones(A.rows))
    yield A, b, hand, ref, sw
    hand.close()
    ref.close()


def test_converging_solve_stops_where_the_reference_stops(small):
    A, b, hand, ref, _ = small
    want = ref.solve("bicgstab", b, tol=1e-10, check_every=16)
    got = hand.solve("bicgstab", b, tol=1e-10, check_every=16)
    assert 0 < want["k"] < 1000, want["k"]
    assert got["dot_r"] <= 1e-20 * got["dot_zero"]          # the loop condition of reference src/solver.c:86 with tol = 1e-10
    assert_same_solve(hand, got, ref, want, "converging solve")


def test_nothing_left_behind_on_the_context(small):
    """after a hand-over solve (the scalar blocks and shard tables have alternated an odd number of times: 3 per iteration, 7
    iterations) every other entry point gives the bits of a context that has never run one"""
    A, b, hand, _, sw = small
    fresh = _context(A, persist=0, **sw)
    try:
        hand.solve("bicgstab", b, tol=0.0, max_iter=7)
        x = np.random.default_rng(3).standard_normal(A.rows)
        y = x + 0.25
        assert same_bits(hand.spmv(x), fresh.spmv(x))
        assert np.float64(hand.dot(x, y)).tobytes() == np.float64(fresh.dot(x, y)).tobytes()
        for method in ("ca_bicgstab", "pipe_bicgstab", "bicgstab"):
            got = hand.solve(method, b, tol=0.0, max_iter=K)
            want = fresh.solve(method, b, tol=0.0, max_iter=K)
            assert_same_solve(hand, got, fresh, want, method)
    finally:
        fresh.close()
