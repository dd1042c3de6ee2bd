"""`-m gpu`: the shifted family -- shifted_lopbicgstab, shifted_pipe_lopbicgstab, shifted_bicgstab, shifted_lopbicg and
shifted_lopbicg_switching -- against answers that have ONE right value, at the shift counts where its per-shift machinery changes
shape: the batches of 8 of shift_pass (csrc/bicg_persist.hip: 8 / 9 shifts, a seed that is the last of a batch, the first of the
next, the last shift), the 64 lanes of comm_coefs fetching 6 nsig coefficients (10 / 11, 21 / 22), kPersistMaxShifts (32 / 33: the
33rd shift silently takes the multi-launch form, run_shifted in csrc/bicg_shifted.cpp) and the per-shift buffers of shifted_setup
growing, shrinking and growing on one context (exact_dots.SHIFT_LISTS, in that order).

The systems are the integer ones of tests/exact_dots.py with sigma_j = sigma_seed + (j - seed) / 64 and 4 + sigma_seed a power of
two: dot_zero, alpha[0], omega[0] -- and for the lop-type recurrences beta[0] and dotr[0] -- of the first iteration are exact
(exact_dots.ShiftedFirst), and the per-shift coefficients are scalar IEEE operations on them in the reference's order
(shift_beta_cp, shift_eta_alpha, shift_omega_coeffs, apply_phase_shifted in csrc/bicg_devfn.h; the build keeps fp-contract off).
So after ONE iteration every x_j and r must be the CPU oracle's bit for bit, in both forms; tests/test_exact_dots.py checks
without a GPU that the oracle's scalars are the integer replay's, that no producer's or element-wise workgroup's partial is
zero, and that a swapped, dropped or seed-shifted update is rejected. Where omega is not dyadic (pipe, shifted_bicgstab) dotr[0]
and beta[0] are compared with a rational replay within derived bounds (ShiftedFirst.residual_dots).

Forms, one context per (shape, form), every list and variant on it in turn:
  persistent   the default: k_shlop_persist / k_shpipe_persist for up to 32 shifts on the shapes without CSR row blocks
  launches     the context is created and the solves run under BICG_PERSIST="shifted=0": one launch per phase. The span_* shapes
               have CSR row blocks -- a dot group's slots are filled by two launches -- and exist in this form only.
Which form ran is asserted through ctx.last_shifted_persistent(), never assumed.

Four iterations (every x_j within 1e-8 max|x_j| of the oracle's, the traces within rtol 1e-8: the bars of tests/test_shifted.py
and tests/test_bench_workloads.py; tests/test_exact_dots.py shows that every iteration moves every shift by 1000 bars and more)
and a run to tol = 1e-10 (|k - k_oracle| <= 2, every shift's true residual from the integer matrix within max(10 x the oracle's
own, 1e-11)) follow on n2049 and span_3_1, on the cases exact_dots.ITER_CASES -- the same four lists with d = 16 and 8, where the
lop recurrence converges at all (see there) --; two ranks sharing the device run the persistent kernels across the peer-to-peer
path (tests/mp_shifted_workers.py)."""
import functools
import hashlib

import numpy as np
import pytest

import exact_dots as E
import mp_workers
from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import synth

pytestmark = pytest.mark.gpu
WALL_LIMIT = 240.0      # seconds for the two-rank case (tests/test_dot_groups_gpu.py)
FIRST = dict(tol=0.0, max_iter=1, check_every=1, record_trace=1)
FOUR = dict(tol=0.0, max_iter=4, check_every=4, record_trace=1)
KEYS = ("alpha", "omega", "beta", "dotr")
LOP, PIPE, XI = "shifted_lopbicgstab", "shifted_pipe_lopbicgstab", "shifted_bicgstab"
PERSISTENT_KERNELS = (LOP, PIPE)                       # the variants that have a persistent kernel
VARIANTS = {"persistent": PERSISTENT_KERNELS, "launches": E.SHIFTED_VARIANTS}
PLAIN_SHAPES = [s for s in E.SHIFTED_SHAPES if not E.SHIFTED_SHAPES[s][1]]
CASES = [(s, f, w) for s in E.SHIFTED_SHAPES for f in VARIANTS for w in VARIANTS[f] if f == "launches" or s in PLAIN_SHAPES]
ITER_SHAPES = ("n2049", "span_3_1")
ITER_CASES = [(s, f, w) for s in ITER_SHAPES for f in VARIANTS for w in (LOP, PIPE, XI)
              if (f == "launches" or (s in PLAIN_SHAPES and w != XI))]


@pytest.fixture(scope="module", autouse=True)
def _single_rank():
    H.lib().bicg_comm_init_single(0)      # (once: a new communicator orphans the contexts of the one before)
    yield


class Session:
    """one context of `shape` in `form`; the switch is held while the context lives (run_shifted reads it at every solve)"""

    def __init__(self, shape, form):
        self.shape, self.form = shape, form
        self.A, self.b = E.shifted_system(shape)
        self.plain = shape in PLAIN_SHAPES
        assert form == "launches" or self.plain

    def __enter__(self):
        if self.form == "launches":
            H.switches(persist_shifted=0)
        try:
            A = self.A
            self.ctx = H.Context(H.single_rank_blocks(synth.CSR(A.n, A.n, A.ptr, A.col, A.val)))
        except BaseException:
            H.switches(persist_shifted=None)
            raise
        return self

    def __exit__(self, *exc):
        try:
            self.ctx.close()
        finally:
            H.switches(persist_shifted=None)

    def expect_persistent(self, which, nsig):
        return self.form == "persistent" and self.plain and which in PERSISTENT_KERNELS and nsig <= 32

    def solve(self, which, case, **kw):
        """(got, trace, sigma, seed, ran persistent) of variant `which` on the case (nsig, seed, sigma_seed)"""
        nsig, seed, sg = case
        sigma, seed, sg = E.shifted_case(which, nsig, seed, sg)
        got = self.ctx.solve_shifted(self.b.astype(np.float64), sigma, seed, which=which, **kw)
        return got, self.ctx.trace(max(got["k"], 1)), sigma, seed, self.ctx.last_shifted_persistent()

    def oracle(self, which, sigma, seed, **kw):
        return E.oracle_shifted(self.A, self.b, which, sigma, seed, **kw)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def differing(got, want):
    """where two [nsig][n] sets differ as bytes: [(shift, rows that differ, first such row)], for the failure message"""
    out = []
    for j, (g, w) in enumerate(zip(np.atleast_2d(got), np.atleast_2d(want))):
        bad = np.flatnonzero(g.view(np.uint64) != w.view(np.uint64))
        if len(bad):
            out.append((j, len(bad), int(bad[0])))
    return out


@functools.lru_cache(maxsize=None)
def first_iterations(shape, form):
    """every variant of the form on every list of SHIFT_LISTS, in the lists' order on ONE context: {(which, i): record}. A record
    holds what the tests compare; the x sets themselves are compared with the oracle's here and only the verdict is kept."""
    out = {}
    with Session(shape, form) as s:
        out["flags"] = s.ctx.flags()
        H.product_kernels()
        for i in range(len(E.SHIFT_LISTS)):
            for which in VARIANTS[form]:
                got, tr, sigma, seed, persistent = s.solve(which, E.list_case(i), **FIRST)
                o = s.oracle(which, sigma, seed, tol=0.0, max_iter=1)
                out[which, i] = dict(
                    k=got["k"], k_oracle=o["k"], dot_zero=got["result"].dot_zero, persistent=persistent,
                    expect_persistent=s.expect_persistent(which, len(sigma)),
                    x_diff=differing(got["x"], o["x"]), r_diff=differing(got["r"], o["r"]),
                    digest=digest(got["x"], got["r"], tr["alpha"], tr["omega"]), digest_end=digest(tr["beta"], tr["dotr"]),
                    **{key: float(tr[key][0]) for key in KEYS})
        out["kernels"] = H.product_kernels()
    return out


@functools.lru_cache(maxsize=None)
def residual_reference(shape, sigma_seed, kind):
    return E.shifted_first_of(shape, sigma_seed).residual_dots(kind)


@pytest.mark.parametrize("shape,form,which", CASES)
def test_first_iteration_is_the_oracles_bytes(shape, form, which):
    run = first_iterations(shape, form)
    plain = shape in PLAIN_SHAPES
    assert run["flags"]["persist"] == plain, run["flags"]          # (the plain solver's persistent plan: what run_shifted asks for)
    assert ("csr" in run["kernels"]) == (not plain), run["kernels"]
    kind = E.recurrence(which)
    for i in range(len(E.SHIFT_LISTS)):
        nsig, seed, sg = E.list_case(i)
        _, seed, sg = E.shifted_case(which, nsig, seed, sg)
        got, where = run[which, i], (shape, form, which, (nsig, seed, sg))
        want = E.shifted_first_of(shape, sg).scalars(which)
        assert got["persistent"] == got["expect_persistent"], where
        assert got["k"] == got["k_oracle"], where + (got["k"], got["k_oracle"])
        assert E.same_bytes(got["dot_zero"], want["dot_zero"]), where + (got["dot_zero"], want["dot_zero"])
        for key in KEYS:
            if key in want:
                assert E.same_bytes(got[key], want[key]), where + (key, got[key].hex(), want[key].hex())
        if kind != "lop":
            R = residual_reference(shape, sg, kind)
            assert E.within(got["dotr"], R["dotr"], R["dotr_bound"]), where + (got["dotr"], float(R["dotr"]), float(R["dotr_bound"]))
            assert E.within(got["beta"], R["beta"], R["beta_bound"]), where + (got["beta"], float(R["beta"]), float(R["beta_bound"]))
        assert not got["x_diff"], where + ("x: (shift, rows, first row)", got["x_diff"][:8])
        assert not got["r_diff"], where + ("r: (0, rows, first row)", got["r_diff"])


@pytest.mark.parametrize("shape", PLAIN_SHAPES)
def test_the_form_follows_the_shift_count(shape):
    """32 shifts run persistent, 33 take the launches, and the solve after a 33-shift one is persistent again"""
    run = first_iterations(shape, "persistent")
    sizes = [nsig for nsig, _ in E.SHIFT_LISTS]
    for which in PERSISTENT_KERNELS:
        ran = [run[which, i]["persistent"] for i in range(len(sizes))]
        assert ran == [nsig <= 32 for nsig in sizes], (shape, which, ran)
        assert sizes[2] == 33 and not ran[2] and ran[3] and sizes[10] == 33 and not ran[10] and ran[11]
    launches = first_iterations(shape, "launches")
    assert not any(launches[which, i]["persistent"] for which in E.SHIFTED_VARIANTS for i in range(len(sizes)))


@pytest.mark.parametrize("which", PERSISTENT_KERNELS)
@pytest.mark.parametrize("shape", PLAIN_SHAPES)
def test_both_forms_give_the_same_bytes(shape, which):
    """k, every x_j, r, alpha[0] and omega[0] in both forms, and for lop the end group's beta[0] and dotr[0] too. pipe's r is rounded
    (omega is not dyadic), so its (r, r) and (r#, r) depend on the association of the sums, and the forms add them differently:
    helper_group (csrc/bicg_persist.hip) adds the workgroups' table in workgroup order with a fixed tree, the launches add by
    shards and arrival tickets (csrc/bicg_reduce.h). Both forms' values are held to the rational replay's derived bounds in
    test_first_iteration_is_the_oracles_bytes instead."""
    a, b = first_iterations(shape, "persistent"), first_iterations(shape, "launches")
    for i in range(len(E.SHIFT_LISTS)):
        assert a[which, i]["k"] == b[which, i]["k"] and a[which, i]["digest"] == b[which, i]["digest"], (shape, which, E.list_case(i))
        if E.recurrence(which) == "lop":
            assert a[which, i]["digest_end"] == b[which, i]["digest_end"], (shape, which, E.list_case(i))


@functools.lru_cache(maxsize=None)
def later_iterations(shape, form):
    """four iterations, and (n2049) the run to tol = 1e-10, of lop / pipe / shifted_bicgstab on the cases of ITER_CASES, on one
    context: {(which, i): dict(four=..., stop=...)} with the differences from the oracle measured here"""
    out = {}
    with Session(shape, form) as s:
        for i in E.ITER_CASES:
            for which in (LOP, PIPE, XI):
                if form == "persistent" and which == XI:
                    continue
                rec = {}
                got, tr, sigma, seed, persistent = s.solve(which, i, **FOUR)
                o = s.oracle(which, sigma, seed, tol=0.0, max_iter=4)
                scale = np.abs(o["x"]).max(axis=1)
                rec["four"] = dict(k=got["k"], k_oracle=o["k"], persistent=persistent, expect=s.expect_persistent(which, len(sigma)),
                                   x=float((np.abs(got["x"] - o["x"]).max(axis=1) / scale).max()), finite=bool(np.isfinite(got["x"]).all()),
                                   trace={key: (tr[key][:4].copy(), o[key][:4].copy()) for key in KEYS})
                if shape == "n2049":
                    got, tr, sigma, seed, persistent = s.solve(which, i, tol=1e-10)
                    o = s.oracle(which, sigma, seed, tol=1e-10)
                    sg_true = sigma.copy()
                    if which == XI:
                        sg_true[0] = 0.0                  # the seed system of shifted_bicgstab is A
                    rec["stop"] = dict(k=got["k"], k_oracle=o["k"], persistent=persistent, expect=s.expect_persistent(which, len(sigma)),
                                       res=E.true_residuals(s.A, s.b, got["x"], sg_true), res_oracle=E.true_residuals(s.A, s.b, o["x"], sg_true))
                out[which, i] = rec
    return out


@pytest.mark.parametrize("shape,form,which", ITER_CASES)
def test_four_iterations_every_shift(shape, form, which):
    run = later_iterations(shape, form)
    worst_x, worst_tr = 0.0, 0.0
    for i in E.ITER_CASES:
        got, where = run[which, i]["four"], (shape, form, which, i)
        assert got["k"] == got["k_oracle"] == 4 and got["persistent"] == got["expect"] and got["finite"], where
        worst_x = max(worst_x, got["x"])
        for key in KEYS:
            mine, ref = got["trace"][key]
            worst_tr = max(worst_tr, float(np.abs(mine / ref - 1.0).max()))
    print(shape, form, which, "largest |x_j - oracle| / max|x_j|: %.3e" % worst_x, "largest relative trace difference: %.3e" % worst_tr)
    for i in E.ITER_CASES:
        got, where = run[which, i]["four"], (shape, form, which, i)
        assert got["x"] <= 1e-8, where + (got["x"],)
        for key in KEYS:
            mine, ref = got["trace"][key]
            np.testing.assert_allclose(mine, ref, rtol=1e-8, err_msg=str(where + (key,)))


@pytest.mark.parametrize("form,which", [(f, w) for s, f, w in ITER_CASES if s == "n2049"])
def test_stops_where_the_oracle_stops(form, which):
    run = later_iterations("n2049", form)
    for i in E.ITER_CASES:
        got, where = run[which, i]["stop"], (form, which, i)
        print(where, "k", got["k"], "oracle", got["k_oracle"], "largest true residual %.3e" % got["res"].max(), "oracle's %.3e" % got["res_oracle"].max())
        assert got["persistent"] == got["expect"], where
        assert abs(got["k"] - got["k_oracle"]) <= 2, where + (got["k"], got["k_oracle"])
        assert got["k_oracle"] < 128                          # the persistent form stops inside its first chunk
        assert (got["res"] <= np.maximum(10 * got["res_oracle"], 1e-11)).all(), where + (got["res"].tolist(), got["res_oracle"].tolist())


def test_two_ranks_persistent():
    """two ranks sharing the device over the peer-to-peer path (tests/mp_shifted_workers.py): the persistent kernels' helper sums
    across ranks, every rank reports the whole system's exact scalars and its rows of every x_j as the oracle's bytes"""
    import mp_shifted_workers as W
    skips = mp_workers.run_ranks(W.shifted_worker, 2, "ranks", WALL_LIMIT)
    assert not skips, skips
