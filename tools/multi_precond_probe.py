#!/usr/bin/env python3
"""What the right-preconditioned methods cost in bicg_solve_multi (methods 4 and 5) on one MI355X, measured on
one context per matrix in one process, for the Transport-shaped matrix (synth.transport_like) and the unstructured FEM matrix in "rcm"
numbering (mpi_bicgstab_amd.mesh, m = 117), both at 1.6 M rows:

  (a) the set application k_bjac_apply_set on 16 columns, ONE launch (bicg_precond_apply_set_bench, device events around --apply-reps
      launches back to back), at bs = 1, 4, 8, 16 and column chunks of 4, 8 and 16, against 16 x k_bjac_apply on one vector
      (bicg_precond_apply_bench) measured in the same run on the same planes; the best of --reps regions each. Byte model per row:
      set (16 / chunk) * 8 bs + 16 * 16, sixteen single applications 16 * (8 bs + 16).
  (b) ms per iteration of a 16-column set for methods 0, 4 (d = 1) and 5 (identity blocks, bs = 4) -- all three then do the same
      arithmetic on the same iterates (tests/test_multi_precond_gpu.py), tol = 0 so that no column freezes -- as
      tools/multi_rhs_probe.py measures it: the iteration loop of a solve with max_iter = warmup + steps minus that of one with
      max_iter = warmup (bicg_result.iter_seconds; both loops are enqueued without a host check in between and end in one
      synchronisation), the least of three pairs; against 16 x the single-RHS iteration of the same method on the device clock
      (bicg_run_iterate_timed).
A measuring tool, not a test: no threshold; it asserts only that every timed region ran its iterations and that the three methods end
on the same bytes.
    python tools/multi_precond_probe.py [--matrix transport|mesh|both] [--n ROWS] [--m 117] [--steps 20] [--warmup 5] [--reps 5]
                                        [--apply-reps 100] [--out FILE.json]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--matrix", default="both", choices=("transport", "mesh", "both"))
ap.add_argument("--n", type=int, default=None, help="rows of the Transport-shaped matrix (default: Transport's)")
ap.add_argument("--m", type=int, default=117)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--apply-reps", type=int, default=100)
ap.add_argument("--out", default=None)
a = ap.parse_args()
NRHS = 16

from mpi_bicgstab_amd import hipsolver as H, mesh, synth  # noqa: E402

H.lib().bicg_comm_init_single(0)


def identity_blocks(n, bs):
    out = np.zeros((-(-n // bs), bs, bs))
    out[:, np.arange(bs), np.arange(bs)] = 1.0
    return out


results = []
for name in (("transport", "mesh") if a.matrix == "both" else (a.matrix,)):
    if name == "transport":
        A = synth.transport_like(a.n, scale_decades=4.0) if a.n else synth.transport_like(scale_decades=4.0)
    else:
        cache = os.path.join(tempfile.gettempdir(), "bicg_mesh_cache")
        os.makedirs(cache, exist_ok=True)
        A = mesh.fem_unstructured(a.m, "rcm", scale_decades=2.0, cache_dir=cache)
    ctx = H.Context(H.single_rank_blocks(A))
    n = A.rows
    out = dict(matrix=name, rows=n, nnz=A.nnz, nrhs=NRHS, steps=a.steps, reps=a.reps, spmm=bool(ctx.flags()["spmm"]))
    # ---- (a) the set application against sixteen single ones
    for bs in (1, 4, 8, 16):
        assert ctx.set_block_diagonal(identity_blocks(n, bs), bs) == 0
        single = min(ctx.apply_preconditioner_bench(a.apply_reps) for _ in range(a.reps))
        row = dict(single_ms=round(single, 5), sixteen_single_ms=round(NRHS * single, 5), single_model_bytes=NRHS * (8 * bs + 16) * n)
        for chunk in (4, 8, 16):
            ms = min(ctx.apply_preconditioner_set_bench(NRHS, a.apply_reps, chunk) for _ in range(a.reps))
            model = ((NRHS // chunk) * 8 * bs + 16 * NRHS) * n
            row[f"chunk{chunk}"] = dict(ms=round(ms, 5), set_over_sixteen=round(ms / (NRHS * single), 4), model_bytes=model,
                                        gbps=round(model / ms / 1e6, 1))
        row["default_chunk_ms"] = round(min(ctx.apply_preconditioner_set_bench(NRHS, a.apply_reps, 0) for _ in range(a.reps)), 5)
        out[f"apply_bs{bs}"] = row
    # ---- (b) the iteration of a set against sixteen single-RHS iterations
    X = 0.5 + np.random.default_rng(7).random((NRHS, n))
    B = ctx.spmm(X)[0] if ctx.flags()["spmm"] else np.array([ctx.spmv(x) for x in X])
    w, total = max(a.warmup, 1), max(a.warmup, 1) + a.steps
    final = {}
    for method in ("bicgstab", "bicgstab_diag", "bicgstab_block"):
        if method == "bicgstab_diag":
            assert ctx.set_diagonal(np.ones(n)) == 0
        if method == "bicgstab_block":
            assert ctx.set_block_diagonal(identity_blocks(n, 4), 4) == 0
        pairs = []
        for _ in range(3):
            t = {}
            for iters in (w, total):
                got = ctx.solve_multi(B, method=method, tol=0.0, max_iter=iters, check_every=total)
                assert all(int(k) == iters for k in got["k"]), f"{name} {method}: a column froze (converged or broke down)"
                t[iters] = got["results"][0].iter_seconds
            pairs.append(t[total] - t[w])
        final[method] = got["x"].tobytes()
        multi = 1e3 * min(pairs) / a.steps
        runs = []
        for _ in range(3):
            ctx.load(np.zeros(n), B[0])
            ctx.run_begin(method, tol=0.0, max_iter=total, check_every=max(a.warmup, a.steps, 1))
            ctx.run_iterate(w)
            ctx.sync()
            _, clocks = ctx.run_iterate_timed(a.steps)
            ctx.run_end()
            runs.append(clocks["device_ms"])
        single = min(runs) / a.steps
        out[method] = dict(multi_ms_per_iteration=round(multi, 4), single_ms_per_iteration=round(single, 4),
                           ratio_16_single_over_multi=round(NRHS * single / multi, 3))
    assert final["bicgstab"] == final["bicgstab_diag"] == final["bicgstab_block"], "identity preconditioners did not reproduce the plain set"
    out["diag_over_plain"] = round(out["bicgstab_diag"]["multi_ms_per_iteration"] / out["bicgstab"]["multi_ms_per_iteration"], 4)
    out["block_over_plain"] = round(out["bicgstab_block"]["multi_ms_per_iteration"] / out["bicgstab"]["multi_ms_per_iteration"], 4)
    ctx.close()
    results.append(out)
    print(json.dumps(out), flush=True)

if a.out:
    with open(a.out, "w") as f:
        json.dump(dict(cases=results), f, indent=1)
