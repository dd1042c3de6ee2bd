"""Worker of tests/test_bicgstab2_precond_ranks_gpu.py: `world` <= 3 spawned processes share cuda:0 through the host-staged
transport (gloo rendezvous on 127.0.0.1, as tests/mp_bicgstab2_workers.py) and run the right-preconditioned BiCGStab(2), methods 7
(diag(A)) and 8 (4 x 4 blocks, local to a rank: block k covers the rank's rows [4 k, 4 k + 4)), collectively.

kinds "transport" (synth.transport_like(40000), equal rows: partial last blocks on every rank) and "empty" (transport_like(4099), the
third rank without rows): three sweeps at tol = 0. k, dot_r, dot_zero, the breakdown field and the whole trace are the same bytes on
every rank; this rank's rows of x and r and the trace stay within the tolerance of tests/test_bicgstab2_precond_gpu.py's case 2 of
hat_sweeps on the WHOLE system with the ranks' preconditioners side by side (16 x the gap between its numpy-dot and its longdouble-dot
runs, floor 1e-12); a sweep moves bicg_comm_counts by 4 halo exchanges (ranks with a halo) and 5 all-reduces, installs and
applications by nothing.
kind "cleared": the refusal is a rank's own (include/bicgstab_hip.h, "across ranks"), as for methods 4 and 5 -- bicg_solve asks no
other rank. Rank 1 clears its preconditioner and calls the solve ALONE: -2, x and r untouched, no counter moved, while the others,
which would enter the solve and wait for it, do not call. After rank 1 has installed again the collective solve gives the bytes it
gave before.
kind "convection": one solve at tol 1e-10 on the issue's S3 with its 4 x 4 blocks, the rows split 1368 / 1364 / 1364 so that no block
crosses a rank's boundary, converging within 1.25 x the one-rank restatement's steps.
A rank reports through the ok<rank> / fail<rank> files of mp_workers.py."""
from __future__ import annotations

import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GROUPS_PER_SWEEP = 5      # DESIGN.md sections 4.23, 4.24: the dot groups a sweep opens = its all-reduces
HALOS_PER_SWEEP = 4       # one per product
KEYS = ("alpha", "beta", "omega", "dotr")
DIAG, BLOCK = "bicgstab2_diag", "bicgstab2_block"
BS = 4


def stab2_precond_worker(rank, world, port, kind, outdir):
    try:
        import numpy as np
        import bicgstab2_precond_ref as Q
        import bicgstab2_ref as R
        import mp_multi_workers as M
        dist = M._init(rank, world, port)
        from mpi_bicgstab_amd import hipsolver as H, synth
        from mpi_bicgstab_amd import dist_transport as T

        T.init_host_transport(0)
        assert world == 3
        part = None
        if kind == "convection":
            A = Q.systems()["S3"]()
            part = (np.array([1368, 1364, 1364], dtype=np.int32), np.array([0, 1368, 2732], dtype=np.int32))
        elif kind == "transport":
            A = synth.transport_like(40000)
        else:
            A = synth.transport_like(4099)
            if kind == "empty":
                part = (np.array([2050, 2049, 0], dtype=np.int32), np.array([0, 2050, 4099], dtype=np.int32))
        n = A.rows
        idx = np.arange(n, dtype=np.int64)
        H.switches(persist=0)
        pieces = [synth.split_blocks(A, world, p, part) for p in range(world)]      # (every rank's diag block: the whole M^-1 below)
        diag, offd, counts, displs = pieces[rank]
        ctx = H.Context(H.HostBlocks(diag, offd, n, counts, displs))
        lo, nl = int(displs[rank]), int(counts[rank])
        halo = ctx.plan_info()["halo"]
        if kind == "empty":
            assert (nl == 0) == (rank == 2)
        else:
            assert halo > 0
        mul = R.Product(A)
        d_loc = Q.diagonal(diag) if nl else None
        b_loc = Q.blocks_of(diag, BS) if nl else None

        def whole_minv(method):
            """M^-1 on the whole system: the ranks' preconditioners side by side"""
            if method == DIAG:
                return Q.jacobi(A, reciprocal=True)
            parts = [(int(pc[3][p]), int(pc[2][p]), Q.block_inverse(pc[0], BS)) for p, pc in enumerate(pieces) if int(pc[2][p])]

            def apply(v):
                return np.concatenate([f(v[at:at + m]) for at, m, f in parts])
            return apply

        def counted(call):
            c0 = ctx.comm_counts()
            out = call()
            c1 = ctx.comm_counts()
            return out, {k: c1[k] - c0[k] for k in c1}

        def install(method):
            rc, moved = counted(lambda: ctx.set_diagonal(d_loc) if method == DIAG else ctx.set_block_diagonal(b_loc, BS))
            assert rc == 0 and moved == dict(exchanges=0, allreduces=0), (method, rc, moved)
            if nl:
                _, moved = counted(lambda: ctx.apply_preconditioner(np.ones(nl)))
                assert moved == dict(exchanges=0, allreduces=0), (method, moved)

        def scalars(got):
            tr = ctx.trace(got["k"])
            q = got["result"]
            return (got["k"], q.iterations, q.breakdown_iteration, np.float64(q.dot_r).tobytes(), np.float64(q.dot_zero).tobytes(),
                    tuple(tr[k].tobytes() for k in KEYS)), tr

        if kind == "convection":
            x0g, bg = np.zeros(n), R.rhs(A, 78)
            want = Q.hat_sweeps(mul, Q.block_inverse(A, BS), bg, x0g, 1000, 1e-10)      # the one-rank restatement
            install(BLOCK)
            got = ctx.solve(BLOCK, bg[lo:lo + nl], x0=x0g[lo:lo + nl], tol=1e-10, max_iter=1000, record_trace=1)
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
            three = dict(tol=0.0, record_trace=1, max_iter=6)
            for method in (DIAG, BLOCK):
                refused = ctx.solve(method, b, x0=x0, **three)      # not installed yet (or the other kind): every rank is refused
                assert refused["k"] == -2 and refused["x"].tobytes() == x0.tobytes() and refused["r"].tobytes() == b.tobytes()
                install(method)
                one, moved1 = counted(lambda: ctx.solve(method, b, x0=x0, tol=0.0, record_trace=1, max_iter=2))
                got, moved3 = counted(lambda: ctx.solve(method, b, x0=x0, **three))
                assert one["k"] == 2 and got["k"] == 6, (one["k"], got["k"])
                sc, tr = scalars(got)
                M.same_on_every_rank(dist, world, sc, (kind, method))
                per_sweep = {k: (moved3[k] - moved1[k]) / 2 for k in moved3}
                assert per_sweep["allreduces"] == GROUPS_PER_SWEEP, (moved1, moved3)
                if halo > 0:
                    assert per_sweep["exchanges"] == HALOS_PER_SWEEP, (moved1, moved3)
                if kind == "cleared":
                    before = (sc, got["x"].tobytes(), got["r"].tobytes())
                    dist.barrier()
                    if rank == 1:
                        assert ctx.clear_preconditioner() == 0 and ctx.preconditioner() is None
                        alone, moved = counted(lambda: ctx.solve(method, b, x0=x0, **three))
                        assert alone["k"] == -2 and alone["x"].tobytes() == x0.tobytes() and alone["r"].tobytes() == b.tobytes()
                        assert moved == dict(exchanges=0, allreduces=0), moved
                        install(method)
                    dist.barrier()
                    again = ctx.solve(method, b, x0=x0, **three)
                    assert (scalars(again)[0], again["x"].tobytes(), again["r"].tobytes()) == before, "after the reinstall"
                    continue
                minv = whole_minv(method)
                want, ext = Q.hat_sweeps(mul, minv, bg, x0g, 6, 0.0), Q.hat_sweeps(mul, minv, bg, x0g, 6, 0.0, extended=True)
                gaps = [R.gap(ext["trace"][q], want["trace"][q]) for q in KEYS] + [R.gap(ext["x"], want["x"]), R.gap(ext["r"], want["r"])]
                tol = max(16.0 * max(gaps), 1e-12)
                print("rank", rank, kind, method, "tolerance %.3e" % tol, flush=True)
                assert want["k"] == 6 and want["breakdown"] == 0 and got["result"].breakdown_iteration == 0
                for q in KEYS:
                    assert R.gap(want["trace"][q], tr[q]) <= tol, (method, q, R.gap(want["trace"][q], tr[q]), tol)
                for q in ("x", "r"):
                    if nl:
                        g = float(np.max(np.abs(want[q][lo:lo + nl] - got[q]))) / float(np.max(np.abs(want[q])))
                        assert g <= tol, (method, q, g, tol)
        assert not ctx.comm_failed()
        ctx.close()
        dist.barrier()
        H.lib().bicg_comm_finalize()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise
