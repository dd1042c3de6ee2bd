"""Worker of tests/test_bicgstab2_ranks_gpu.py: `world` spawned processes share cuda:0 through the host-staged transport (gloo
rendezvous on 127.0.0.1, as tests/mp_multi_workers.py) and run BiCGStab(2), method 6, collectively.

kinds "transport" (synth.transport_like(40000)) and "six" (mp_multi_workers.matrix("six"), the last rank without rows): three sweeps at
tol = 0. k, dot_r, dot_zero, the breakdown field and the whole trace are the same bytes on every rank; this rank's rows of x and r and
the trace stay within the tolerance of tests/test_bicgstab2_gpu.py's case 2 of the numpy restatement on the WHOLE system (computed on
the restatement alone: 16 x the gap between its numpy-dot and its longdouble-dot runs, floor 1e-12, relative to the largest magnitude
of the whole array); a sweep moves bicg_comm_counts by 4 halo exchanges (ranks with a halo) and GROUPS_PER_SWEEP all-reduces.
On "six" the Krylov space is exhausted after six steps and that tolerance comes out of order 10 (the third sweep works on a residual
of 1e-22), so there the values are compared after TWO sweeps as well, where the same formula gives about 3e-11.
kind "convection": one solve at tol 1e-10 on the (m, c) = (16, 20) stencil, converging as on one rank.
A rank reports through the ok<rank> / fail<rank> files of mp_workers.py."""
from __future__ import annotations

import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GROUPS_PER_SWEEP = 5      # the dot groups a sweep opens = its all-reduces (at least 5, at most 6)
HALOS_PER_SWEEP = 4       # one per product
KEYS = ("alpha", "beta", "omega", "dotr")


def stab2_worker(rank, world, port, kind, outdir):
    try:
        import numpy as np
        import bicgstab2_ref as R
        import mp_multi_workers as M
        import mp_precond_workers as W
        dist = M._init(rank, world, port)
        from mpi_bicgstab_amd import hipsolver as H, synth
        from mpi_bicgstab_amd import dist_transport as T

        T.init_host_transport(0)
        convection = kind == "convection"
        A = R.convection(16, 20) if convection else W.matrix(kind)
        n = A.rows
        idx = np.arange(n, dtype=np.int64)
        H.switches(persist=0)
        diag, offd, counts, displs = synth.split_blocks(A, world, rank)
        ctx = H.Context(H.HostBlocks(diag, offd, n, counts, displs))
        lo, nl = int(displs[rank]), int(counts[rank])
        halo = ctx.plan_info()["halo"]
        if kind == "six":
            assert (nl == 0) == (rank >= 6)
        else:
            assert halo > 0
        mul = R.Product(A)

        def scalars(got):
            tr = ctx.trace(got["k"])
            q = got["result"]
            return (got["k"], q.iterations, q.breakdown_iteration, np.float64(q.dot_r).tobytes(), np.float64(q.dot_zero).tobytes(),
                    tuple(tr[k].tobytes() for k in KEYS)), tr

        if convection:
            x0g, bg = np.zeros(n), R.rhs(A, 78)
            want = R.sweeps(mul, bg, x0g, 1000, 1e-10)
            got = ctx.solve("bicgstab2", bg[lo:lo + nl], x0=x0g[lo:lo + nl], tol=1e-10, max_iter=1000, record_trace=1)
            sc, _ = scalars(got)
            M.same_on_every_rank(dist, world, sc, "convection")
            parts = [None] * world
            dist.all_gather_object(parts, got["x"])
            rel = R.true_relres(mul, bg, np.concatenate(parts))
            print("rank", rank, "k", got["k"], "restatement k", want["k"], "true relres %.3e" % rel, flush=True)
            assert got["result"].breakdown_iteration == 0 and rel <= 1e-9 and got["k"] <= 1.25 * want["k"], (got["k"], want["k"], rel)
        else:
            x0g = 0.25 * synth._uniform(idx, 77) - 0.125
            bg = A.matvec(1.0 + 0.5 * synth._uniform(idx, 78))
            x0, b = x0g[lo:lo + nl], bg[lo:lo + nl]

            def reference(steps):
                """(the restatement's `steps` steps, the tolerance computed from its own two runs)"""
                want, ext = R.sweeps(mul, bg, x0g, steps, 0.0), R.sweeps(mul, bg, x0g, steps, 0.0, extended=True)
                gaps = [R.gap(ext["trace"][q], want["trace"][q]) for q in KEYS] + [R.gap(ext["x"], want["x"]), R.gap(ext["r"], want["r"])]
                return want, max(16.0 * max(gaps), 1e-12)

            def compare(want, tol, got, tr, what):
                print("rank", rank, kind, what, "tolerance %.3e" % tol, flush=True)
                for q in KEYS:
                    assert R.gap(want["trace"][q], tr[q]) <= tol, (what, q, R.gap(want["trace"][q], tr[q]), tol)
                for q in ("x", "r"):
                    scale = float(np.max(np.abs(want[q])))
                    if nl:
                        g = float(np.max(np.abs(want[q][lo:lo + nl] - got[q]))) / scale
                        assert g <= tol, (what, q, g, tol)

            def counted(**opts):
                c0 = ctx.comm_counts()
                out = ctx.solve("bicgstab2", b, x0=x0, tol=0.0, record_trace=1, **opts)
                c1 = ctx.comm_counts()
                return out, {k: c1[k] - c0[k] for k in c1}
            one, moved1 = counted(max_iter=2)
            got, moved3 = counted(max_iter=6)
            want, tol = reference(6)
            assert one["k"] == 2 and got["k"] == 6 == want["k"], (one["k"], got["k"])
            sc, tr = scalars(got)
            M.same_on_every_rank(dist, world, sc, kind)
            compare(want, tol, got, tr, "three sweeps")
            if kind == "six":
                # six rows: the Krylov space is exhausted after six steps, the third sweep works on a residual of 1e-22 and the
                # tolerance computed above is of order 10 -- no check of the values. After TWO sweeps it is one.
                want2, tol2 = reference(4)
                assert tol2 <= 1e-8, tol2
                two = ctx.solve("bicgstab2", b, x0=x0, tol=0.0, record_trace=1, max_iter=4)
                sc2, tr2 = scalars(two)
                assert two["k"] == 4 == want2["k"]
                M.same_on_every_rank(dist, world, sc2, "six, two sweeps")
                compare(want2, tol2, two, tr2, "two sweeps")
            per_sweep = {k: (moved3[k] - moved1[k]) / 2 for k in moved3}
            assert per_sweep["allreduces"] == GROUPS_PER_SWEEP, (moved1, moved3)
            if halo > 0:
                assert per_sweep["exchanges"] == HALOS_PER_SWEEP, (moved1, moved3)
        assert not ctx.comm_failed()
        ctx.close()
        dist.barrier()
        H.lib().bicg_comm_finalize()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise
