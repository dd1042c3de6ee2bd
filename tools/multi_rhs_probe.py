#!/usr/bin/env python3
"""What 16 right-hand sides per pass over the matrix buy (bicg_solve_multi), measured in one process on one build and one context
per matrix: the Transport-shaped synthetic (synth.transport_like()) and the unstructured FEM matrix in the "rcm" numbering
(mpi_bicgstab_amd.mesh). Per matrix:
  multi_ms_per_iteration   one 16-column set, tol = 0 so that no column freezes: the iteration loop of a solve with max_iter =
                           warmup + steps minus that of a solve with max_iter = warmup (bicg_result.iter_seconds; both loops are
                           enqueued without a host check in between and end in one synchronisation, so the difference is `steps`
                           iterations of device work), the least of three pairs
  single_ms_per_iteration  bicg_run_iterate_timed for ONE right-hand side, device events around `steps` iterations after `warmup`
  spmm_ms                  bicg_spmm's device time for 16 vectors; two of them per iteration are the SpMM's share
  ratio                    16 x single / multi: above 1, sixteen systems cost less as a set than one after the other
A measuring tool, not a test: nothing is asserted.
    python tools/multi_rhs_probe.py [--n 1602111] [--m 117] [--steps 20] [--warmup 5] [--only transport|mesh] [--out FILE.json]

--world P: the collective call instead. P fresh child processes (this script with --rank) share GPU 0 through the host-staged
transport (gloo on 127.0.0.1) and solve one 16-column set on the tests' "offsets" matrix (4 001 rows; --n N: the Transport-shaped
synthetic with N rows), tol = 0. Printed by rank 0: ms per iteration (same two-solve difference as above, the slowest rank) and the
bicg_comm_counts deltas of the `steps`-iteration difference, with the set exchange (halo-set on) and with one exchange per column
(BICG_PLAN=halo-set=0). Ranks sharing one device through a host transport say nothing about a real link.
    python tools/multi_rhs_probe.py --world 2 [--n N] [--steps 20] [--warmup 5] [--out FILE.json]"""
import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=None, help="rows of the Transport-shaped synthetic (default: Transport's)")
ap.add_argument("--m", type=int, default=117, help="the mesh has m^3 rows")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--only", choices=("transport", "mesh"), default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--world", type=int, default=0, help="ranks sharing the GPU through the host-staged transport")
ap.add_argument("--rank", type=int, default=-1, help=argparse.SUPPRESS)
ap.add_argument("--port", type=int, default=0, help=argparse.SUPPRESS)
a = ap.parse_args()
NRHS = 16


def world_parent():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    args = [sys.executable, os.path.abspath(__file__), "--world", str(a.world), "--port", str(port), "--steps", str(a.steps),
            "--warmup", str(a.warmup)] + (["--n", str(a.n)] if a.n else []) + (["--out", a.out] if a.out else [])
    kids = [subprocess.Popen(args + ["--rank", str(r)]) for r in range(a.world)]
    try:
        codes = [k.wait(timeout=600) for k in kids]
    finally:
        for k in kids:
            if k.poll() is None:
                k.kill()
    sys.exit(max(abs(c) for c in codes))


def world_child():
    from datetime import timedelta
    import torch
    torch.set_num_threads(1)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(a.port)
    dist.init_process_group("gloo", rank=a.rank, world_size=a.world, timeout=timedelta(seconds=120))
    from mpi_bicgstab_amd import dist_transport as T, hipsolver as H, synth
    T.init_host_transport(0)
    if a.n:
        name, A = "transport_like", synth.transport_like(n=a.n)
    else:
        name, A = "offsets", synth.from_offsets(4001, (0, 1, -1, 7, -7, 300, -300, 1999, -1999), diag_base=12.0, seed=3)
    diag, offd, counts, displs = synth.split_blocks(A, a.world, a.rank)
    lo, nl = int(displs[a.rank]), int(counts[a.rank])
    ctx = H.Context(H.HostBlocks(diag, offd, A.rows, counts, displs))
    X = (0.5 + np.random.default_rng(7).random((NRHS, A.rows)))[:, lo:lo + nl]
    B = ctx.spmm(X)[0] if ctx.flags()["spmm"] else np.array([ctx.spmv(x) for x in X])
    w, total = max(a.warmup, 1), max(a.warmup, 1) + a.steps
    out = dict(matrix=name, rows=A.rows, nnz=A.nnz, nrhs=NRHS, world=a.world, transport="host", spmm=bool(ctx.flags()["spmm"]),
               label="ranks sharing one device, host transport")
    for key, tok in (("halo_set", None), ("per_column", 0)):
        H.switches(halo_set=tok)
        pairs, delta = [], None
        for _ in range(3):
            t, c = {}, {}
            for iters in (w, total):
                c0 = ctx.comm_counts()
                got = ctx.solve_multi(B, nrhs=NRHS, tol=0.0, max_iter=iters, check_every=total)
                c1 = ctx.comm_counts()
                t[iters], c[iters] = got["results"][0].iter_seconds, {k: c1[k] - c0[k] for k in c1}
            pairs.append(t[total] - t[w])
            delta = {k: c[total][k] - c[w][k] for k in c[total]}
        mine = 1e3 * min(pairs) / a.steps
        every = [None] * a.world
        dist.all_gather_object(every, mine)
        out[key] = dict(ms_per_iteration=round(max(every), 4), exchanges_per_iteration=delta["exchanges"] / a.steps,
                        allreduces_per_iteration=delta["allreduces"] / a.steps)
    H.switches(halo_set=None)
    ctx.close()
    dist.barrier()
    H.lib().bicg_comm_finalize()
    dist.destroy_process_group()
    if a.rank == 0:
        print(json.dumps(out), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(dict(cases=[out]), f, indent=1)


if a.world > 1:
    world_parent() if a.rank < 0 else world_child()
    sys.exit(0)

from mpi_bicgstab_amd import hipsolver as H, mesh, synth  # noqa: E402

H.lib().bicg_comm_init_single(0)


def matrices():
    if a.only != "mesh":
        yield "transport_like", synth.transport_like() if a.n is None else synth.transport_like(n=a.n)
    if a.only != "transport":
        cache = os.path.join(tempfile.gettempdir(), "bicg_mesh_cache")
        os.makedirs(cache, exist_ok=True)
        yield "fem_rcm", mesh.fem_unstructured(a.m, "rcm", scale_decades=2.0, cache_dir=cache)


results = []
for name, A in matrices():
    ctx = H.Context(H.single_rank_blocks(A))
    out = dict(matrix=name, rows=A.rows, nnz=A.nnz, nrhs=NRHS, flags=[k for k, v in ctx.flags().items() if v])
    X = 0.5 + np.random.default_rng(7).random((NRHS, A.rows))
    if ctx.flags()["spmm"]:
        B, _ = ctx.spmm(X)
        out["spmm_ms"] = round(min(ctx.spmm(X)[1] for _ in range(3)), 4)
        out["spmm_kind"] = ctx.last_spmm_kind()
    else:
        B = np.array([ctx.spmv(x) for x in X])
    total = a.warmup + a.steps
    pairs = []
    for _ in range(3):
        t = {}
        for iters in (max(a.warmup, 1), total):
            got = ctx.solve_multi(B, tol=0.0, max_iter=iters, check_every=total)
            out["every_column_ran_all_iterations"] = out.get("every_column_ran_all_iterations", True) and all(int(k) == iters for k in got["k"])
            t[iters] = got["results"][0].iter_seconds
        pairs.append(t[total] - t[max(a.warmup, 1)])
    timed = total - max(a.warmup, 1)
    out["multi_ms_per_iteration"] = round(1e3 * min(pairs) / timed, 4)
    runs = []
    for _ in range(3):
        ctx.load(np.zeros(A.rows), B[0])
        ctx.run_begin("bicgstab", tol=0.0, max_iter=total, check_every=max(a.warmup, a.steps, 1))
        if a.warmup:
            ctx.run_iterate(a.warmup)
        ctx.sync()
        _, clocks = ctx.run_iterate_timed(a.steps)
        ctx.run_end()
        runs.append(clocks["device_ms"])
    out["single_ms_per_iteration"] = round(min(runs) / a.steps, 4)
    out["ratio_16_single_over_multi"] = round(NRHS * out["single_ms_per_iteration"] / out["multi_ms_per_iteration"], 3)
    if "spmm_ms" in out:
        out["spmm_share"] = round(2.0 * out["spmm_ms"] / out["multi_ms_per_iteration"], 3)
    out["us_per_system_iteration"] = round(1e3 * out["multi_ms_per_iteration"] / NRHS, 2)
    ctx.close()
    results.append(out)
    print(json.dumps(out), flush=True)

if a.out:
    with open(a.out, "w") as f:
        json.dump(dict(cases=results), f, indent=1)
