#!/usr/bin/env python3
"""What BICG_PLAN="reorder" buys on a badly numbered matrix, measured in one process on one build: the unstructured FEM matrix
(mpi_bicgstab_amd.mesh) in RANDOM numbering with reorder = 0 / 1 / 2, and in the "rcm" numbering (scipy's reverse Cuthill-McKee)
without the switch. Per case: the product back to back (bicg_spmv_bench), the plain iteration (20 timed after 5 warm-up, the
benchmark's way: wall clock around bicg_run_iterate_timed), the seconds bicg_create took, bicg_reorder_info, flags and the product
kernel. A measuring tool, not a test: nothing is asserted but the bit-exactness of y = A x between the cases on the same numbering.
    python tools/reorder_probe.py [--m 117] [--steps 20] [--warmup 5] [--out FILE.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=117)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()

from mpi_bicgstab_amd import hipsolver as H, mesh  # noqa: E402

H.lib().bicg_comm_init_single(0)
cache = os.path.join(tempfile.gettempdir(), "bicg_mesh_cache")
os.makedirs(cache, exist_ok=True)
results, y_random = [], None
for numbering, reorder in (("random", 0), ("random", 1), ("random", 2), ("rcm", 0)):
    A = mesh.fem_unstructured(a.m, numbering, scale_decades=2.0, cache_dir=cache)
    blocks = H.single_rank_blocks(A)
    H.switches(reorder=reorder if reorder else None)
    try:
        t0 = time.perf_counter()
        ctx = H.Context(blocks)
        create_s = time.perf_counter() - t0
    finally:
        H.switches(reorder=None)
    out = dict(numbering=numbering, reorder=reorder, rows=A.rows, nnz=A.nnz, create_s=round(create_s, 3),
               flags=[k for k, v in ctx.flags().items() if v], reorder_info=ctx.reorder_info())
    H.product_kernels()
    ctx.spmv_bench(200)                                      # clocks and caches in steady state
    out["spmv_us"] = round(1e3 * min(ctx.spmv_bench(200) for _ in range(3)), 2)
    out["kernels"] = H.product_kernels()
    ones = np.ones(A.rows)
    b = ctx.spmv(ones)
    runs = []
    for _ in range(3):
        ctx.load(np.zeros(A.rows), b)
        ctx.run_begin("bicgstab", tol=0.0, max_iter=a.warmup + a.steps, check_every=max(a.warmup, a.steps, 1), krr=50, nrr=2)
        if a.warmup:
            ctx.run_iterate(a.warmup)
        ctx.sync()
        t0 = time.perf_counter()
        _, clocks = ctx.run_iterate_timed(a.steps)
        ctx.sync()
        runs.append((time.perf_counter() - t0, clocks["device_ms"]))
        ctx.run_end()
    out["bicgstab_us_per_iteration"] = round(1e6 * min(r[0] for r in runs) / a.steps, 2)
    out["bicgstab_device_us_per_iteration"] = round(1e3 * min(r[1] for r in runs) / a.steps, 2)
    if numbering == "random":                                # the caller's numbering is the same: so are the bits
        x = 1.0 + 1e-3 * np.cos(np.arange(A.rows))
        y = ctx.spmv(x)
        if y_random is None:
            y_random = y
        assert np.array_equal(y, y_random), "reordered product differs from the product as given"
        out["spmv_bits_equal_as_given"] = True
    ctx.close()
    results.append(out)
    print(json.dumps(out), flush=True)

by = {(r["numbering"], r["reorder"]): r for r in results}
summary = dict(reordered_over_rcm_spmv=round(by[("random", 1)]["spmv_us"] / by[("rcm", 0)]["spmv_us"], 3),
               as_given_over_reordered_spmv=round(by[("random", 0)]["spmv_us"] / by[("random", 1)]["spmv_us"], 3),
               reorder_cost_s=round(by[("random", 1)]["create_s"] - by[("random", 0)]["create_s"], 3))
print(json.dumps(summary), flush=True)
if a.out:
    with open(a.out, "w") as f:
        json.dump(dict(cases=results, summary=summary), f, indent=1)
