"""`-m gpu`: the ragged-row products (k_spmv_jagw, k_spmv_jagl, k_spmv_jagd in csrc/bicg_jagw.hip; k_spmm_jpipe in
csrc/bicg_spmm_jag.hip) on the crafted matrices of tests/ragged_cases.py, each of which sits ON a plan limit -- 64 / 65 runs per group,
2048 / 2049 window slots, rows of 255 / 256 entries, the batch edges of both kernels, empty groups and slices, every shape of the
partly filled last group, 16-bit offsets at +-32767 / 32768, the list-driven window at 2048 distinct columns from -32768 to +32767,
the SpMM's window and LDS budget. tests/test_ragged_limits.py checks on the CPU that every matrix plans as its generator promises.

No tolerance anywhere. References:
  products    the CPU oracle's spmv (tests/oracle_lib.py): a row's products added in stored order, one rounding per product and per
              sum, no FMA -- what these kernels promise bit for bit; a row without entries is exactly +0.0
  fused dots  integer matrices and vectors (entries from {1, 2, 3}): dot_zero = (b, b) and alpha_1 = (b, b) / (b, A b) are Python
              integers / one correctly rounded Fraction, whichever way the partial sums are added (`IntegerSystem` asserts what
              that rests on: every sum below 2^53, no 256-row group that holds an entry with a zero partial)
  SpMM        row j = oracle spmv(x_j) + sigma_j x_j in float64 numpy: two more roundings
  jagw=0      k_spmv_sell's loop over the same slices: product, the first 6 iterations of three solvers and a 3-shift solve are
              identical in every bit (the claim tests/test_full_size.py makes for natural shapes)
Every context is created under switches(persist=0): a matrix this small would otherwise iterate in one persistent launch.
A stand-alone product always walks the groups in the same (reversed) direction -- bicg_spmv resets bicg_ctx::spmv_dir --, so the
product is taken twice for its repeatability; both directions alternate inside the solves, whose scalars and x are compared.
A group whose rows are all empty has a zero partial by construction: `IntegerSystem` allows exactly the crafted one.

The small cases build their contexts per test; the large one (`list_limits`, 6.9 M non-zeros) has one context per value of jagw
for the whole module, and its values are replaced in place (update_values, itself checked) where a test needs other values."""
import functools

import numpy as np
import pytest

import ragged_cases as R
from bitwise import IntegerSystem, assert_same_bits, check_first_dots, oracle_spmv, same_bits
from mpi_bicgstab_amd import hipsolver as H

pytestmark = pytest.mark.gpu
SIGMA3 = np.array([0.0, 0.02, 0.05])
METHODS = ("bicgstab", "ca_bicgstab", "pipe_bicgstab")
SPMM_CASES = ("runs64", "slots2048", "tail1", "tail193", "jpipe960", "jpipe961", "jpipe960_slots2048")
SPMM_NVEC = (1, 3, 16, 17)
UPDATE_CASES = ("lengths_jagw", "lengths_jagd", "runs64", "tail65")


@pytest.fixture(scope="module", autouse=True)
def _single_rank():
    H.lib().bicg_comm_init_single(0)      # (once: a new communicator orphans the contexts of the one before)
    yield


def context(A, sw, jagw):
    """a context of the one-rank block A under persist=0, the case's switches and jagw=; the tokens are taken back at once"""
    tokens = dict(sw, persist=0, jagw=jagw)
    H.switches(**tokens)
    try:
        return H.Context(H.single_rank_blocks(A))
    finally:
        H.switches(**{k: None for k in tokens})


def kernel_at(facts, jagw):
    """the product kernel a case runs: the three-trip one its facts name, or -- jagw=0 hands no lane words to the launch --
    k_spmv_sell's loop over the window / over the gathered slices"""
    return facts["kernel"] if jagw else ("sell_window_loop" if facts["window"] else "sell_jagged")


@functools.lru_cache(maxsize=None)
def product_reference(name, seed=0):
    """(x, the oracle's A x) for the generic values of a case -- computed once, shared, never written to"""
    A, _, _ = R.build(name, "generic", seed)
    x = np.random.default_rng(1000 + seed).standard_normal(A.rows)
    want = oracle_spmv(A, x)
    x.setflags(write=False); want.setflags(write=False)
    return x, want


def check_product(ctx, A, facts, jagw, x, want, what):
    H.product_kernels()
    y1 = ctx.spmv(x)
    y2 = ctx.spmv(x)
    assert H.product_kernels() == [kernel_at(facts, jagw)], what
    assert_same_bits(y1, want, what)
    assert_same_bits(y2, want, what + ", again")
    empty = np.diff(A.ptr.astype(np.int64)) == 0
    assert same_bits(y1[empty], np.zeros(int(empty.sum()))), (what, "rows without entries give +0.0")


@functools.lru_cache(maxsize=None)
def integer_system(name):
    return IntegerSystem(name, R)


@functools.lru_cache(maxsize=None)
def dominant_system(name):
    """(A with dominant diagonals, b = A 1 by the oracle): six iterations stay finite"""
    A, facts, sw = R.build(name, "dominant")
    b = oracle_spmv(A, np.ones(A.rows))
    b.setflags(write=False)
    return A, facts, sw, b


def six_iterations(ctx, b):
    """the traces of 6 iterations of the three solvers with their x, and the x set of a 3-shift solve (has_shift in the products)"""
    out = []
    for method in METHODS:
        got = ctx.solve(method, b, tol=0.0, max_iter=6, check_every=6)
        tr = ctx.trace(6)
        out.append(np.concatenate([tr[key] for key in ("alpha", "omega", "beta", "dotr")] + [got["x"]]))
    sh = ctx.solve_shifted(b, SIGMA3, 1, tol=0.0, max_iter=6, check_every=6)
    out.append(sh["x"].ravel().copy())
    return out


def check_six_iterations(fast, slow, what):
    for name, a, b in zip(METHODS + ("solve_shifted",), fast, slow):
        assert np.all(np.isfinite(a)), (what, name)
        assert len(a) == len(b)
        assert_same_bits(a, b, f"{what} {name}: jagw=1 against jagw=0")


def spmm_kind(facts):
    """which SpMM kernel takes a block with x windows. Read in launch_spmm_jpipe (csrc/bicg_spmm_jag.hip) and spmm_pass
    (csrc/bicg_solver.cpp): k_spmm_jpipe ("pipelined") needs windows within 16 bits of their groups (win_near16), at most 8 staged
    slots per thread beside the zero slot -- W = (win_slots + 2) & ~1 with W - 1 <= 2048, i.e. win_slots <= 2047 --, and
    2 W 8 + 8192 bytes of window and results + 640 static + 40 bytes per entry of roundup64(jag_tail16_max) within 80 KB;
    k_spmm_win ("windowed") takes every other block. (2048 slots, the product's own limit, is one more than k_spmm_jpipe takes:
    the case jpipe960_slots2048.)"""
    W = (facts["win_slots"] + 2) & ~1
    lds = 16 * W + 8192 + 640 + 40 * (-(-facts["jag_tail16_max"] // 64) * 64)
    return "pipelined" if facts["win_near16"] and W - 1 <= 2048 and lds <= 80 * 1024 else "windowed"


@functools.lru_cache(maxsize=None)
def spmm_reference(name):
    """(X [17][n], distinct sigma [17], the oracle's A x_j [17][n]) for the generic values of a case"""
    A, _, _ = R.build(name)
    X = np.random.default_rng(3000).standard_normal((max(SPMM_NVEC), A.rows))
    sigma = (np.arange(max(SPMM_NVEC)) + 1.0) * 0.013
    AX = np.stack([oracle_spmv(A, X[j]) for j in range(len(X))])
    for a in (X, sigma, AX):
        a.setflags(write=False)
    return X, sigma, AX


def check_spmm(ctx, name, facts):
    X, sigma, AX = spmm_reference(name)
    for nvec in SPMM_NVEC:
        for sg in (np.zeros(nvec), sigma[:nvec]):
            Y, _ = ctx.spmm(X[:nvec], sg)
            assert ctx.last_spmm_kind() == spmm_kind(facts), (name, nvec, facts)
            want = AX[:nvec] + sg[:, None] * X[:nvec]          # one rounding for the product, one for the sum
            for j in range(nvec):
                assert_same_bits(Y[j], want[j], f"{name}: SpMM of {nvec} vectors, vector {j}, sigma {sg[j]}")


# ---- the small cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.SMALL))
def test_product_is_the_oracles_bit_for_bit(name):
    A, facts, sw = R.build(name)
    x, want = product_reference(name)
    for jagw in (1, 0):
        ctx = context(A, sw, jagw)
        try:
            check_product(ctx, A, facts, jagw, x, want, f"{name} jagw={jagw}")
        finally:
            ctx.close()


@pytest.mark.parametrize("name", list(R.SMALL))
def test_first_iterations_dots_are_exact(name):
    S = integer_system(name)
    for jagw in (1, 0):
        ctx = context(S.A, S.sw, jagw)
        try:
            H.product_kernels()
            check_first_dots(ctx, S, f"{name} jagw={jagw}")
            assert kernel_at(S.facts, jagw) in H.product_kernels()
        finally:
            ctx.close()


@pytest.mark.parametrize("name", list(R.SMALL))
def test_six_iterations_same_bits_with_the_short_chain(name):
    A, facts, sw, b = dominant_system(name)
    runs = []
    for jagw in (1, 0):
        ctx = context(A, sw, jagw)
        try:
            runs.append(six_iterations(ctx, b))
        finally:
            ctx.close()
    check_six_iterations(runs[0], runs[1], name)


@pytest.mark.parametrize("name", SPMM_CASES)
def test_spmm_at_the_window_and_lds_limits(name):
    """jpipe960 is the pipelined kernel's last fit, jpipe961 (one more entry behind the heads: 64 more LDS entries per wavefront)
    and jpipe960_slots2048 (one more window slot) go to the windowed kernel: `spmm_kind` says where the limits were read"""
    A, facts, sw = R.build(name)
    edge = {"jpipe960": "pipelined", "jpipe961": "windowed", "jpipe960_slots2048": "windowed"}
    assert name not in edge or spmm_kind(facts) == edge[name]
    ctx = context(A, sw, 1)
    try:
        check_spmm(ctx, name, facts)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", UPDATE_CASES)
def test_new_values_at_the_same_edges(name):
    """bicg_update_values replays the jagged packing (csrc/bicg_refresh.hip): the next product is the oracle's on the new values"""
    A, facts, sw = R.build(name)
    A1, _, _ = R.build(name, "generic", 1)
    assert np.array_equal(A.col, A1.col) and not np.array_equal(A.val, A1.val)
    x, want = product_reference(name)
    x1, want1 = product_reference(name, 1)
    for jagw in (1, 0):
        ctx = context(A, sw, jagw)
        try:
            check_product(ctx, A, facts, jagw, x, want, f"{name} jagw={jagw}")
            assert ctx.update_values(A1.val) == 0
            check_product(ctx, A1, facts, jagw, x1, want1, f"{name} jagw={jagw}, new values")
        finally:
            ctx.close()


# ---- the large case: one context per jagw for the module -----------------------------------------------------------------------------
class Large:
    name = "list_limits"

    def __init__(self):
        self.A, self.facts, self.sw = R.build(self.name)
        self.ctx = {jagw: context(self.A, self.sw, jagw) for jagw in (1, 0)}
        self.holds = {1: ("generic", 0), 0: ("generic", 0)}

    def use(self, jagw, values, seed=0):
        """the context of `jagw` holding these values of the pattern (replaced in place where it holds others)"""
        A, _, _ = R.build(self.name, values, seed)
        if self.holds[jagw] != (values, seed):
            assert self.ctx[jagw].update_values(A.val) == 0
            self.holds[jagw] = (values, seed)
        return self.ctx[jagw], A

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def large():
    L = Large()
    yield L
    L.close()


def test_large_product_is_the_oracles_bit_for_bit(large):
    x, want = product_reference(large.name)
    for jagw in (1, 0):
        ctx, A = large.use(jagw, "generic")
        fl = ctx.flags()
        assert fl["jagged"] and fl["window"] and fl["all_sell"], fl
        check_product(ctx, A, large.facts, jagw, x, want, f"{large.name} jagw={jagw}")


def test_large_first_iterations_dots_are_exact(large):
    S = integer_system(large.name)
    for jagw in (1, 0):
        ctx, _ = large.use(jagw, "integer")
        H.product_kernels()
        check_first_dots(ctx, S, f"{large.name} jagw={jagw}")
        assert kernel_at(S.facts, jagw) in H.product_kernels()


def test_large_six_iterations_same_bits_with_the_short_chain(large):
    _, _, _, b = dominant_system(large.name)
    runs = [six_iterations(large.use(jagw, "dominant")[0], b) for jagw in (1, 0)]
    check_six_iterations(runs[0], runs[1], large.name)


def test_large_spmm(large):
    ctx, _ = large.use(1, "generic")
    assert spmm_kind(large.facts) == "windowed"          # (a column 32768 to the left of its group: the windows are not within 16 bits)
    check_spmm(ctx, large.name, large.facts)


def test_large_new_values(large):
    x1, want1 = product_reference(large.name, 1)
    for jagw in (1, 0):
        ctx, A1 = large.use(jagw, "generic", 1)
        check_product(ctx, A1, large.facts, jagw, x1, want1, f"{large.name} jagw={jagw}, new values")
