"""Worker of tests/test_precond_ranks_gpu.py: `world` spawned processes share cuda:0 through the host-staged transport (gloo
rendezvous on 127.0.0.1, as tests/mp_multi_workers.py). Every rank holds two contexts at the same partition -- A, and A D^-1 with
d = powers of two (diag AND offd columns scaled by their owner's 1 / d_j, which is exact) -- and compares as bytes:
  d = 1          method 4 against method 0 on A;
  d = 2^e        method 4 on A with (x0, b) against method 0 on A D^-1 with (d o x0, b): k, r, the result fields, the traces, and
                 x_A == x_B / d -- the products of method 4 read the hat vectors' halo tails, so this covers their exchange;
  counts         method 4 moves bicg_comm_counts by what method 0 moves it, the install by nothing.
A rank reports through the ok<rank> / fail<rank> files of mp_workers.py."""
from __future__ import annotations

import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXED = dict(tol=0.0, max_iter=12, record_trace=1, check_every=4)


def matrix(name):
    import mp_multi_workers as M
    from mpi_bicgstab_amd import synth
    return synth.transport_like(40000) if name == "transport" else M.matrix(name)


def precond_worker(rank, world, port, kind, outdir):
    try:
        import numpy as np
        import mp_multi_workers as M
        dist = M._init(rank, world, port)
        from mpi_bicgstab_amd import hipsolver as H, synth
        from mpi_bicgstab_amd import dist_transport as T

        T.init_host_transport(0)
        A = matrix(kind)
        n = A.rows
        idx = np.arange(n, dtype=np.int64)
        d_glob = np.ldexp(1.0, np.floor(17.0 * synth._uniform(idx, 31)).astype(np.int64) - 8)      # 2^e, e in [-8, 8]
        Bm = synth.CSR(n, n, A.ptr, A.col, A.val * (1.0 / d_glob)[A.col])                          # A D^-1, exactly
        H.switches(persist=0)
        ctxs = []
        for mat in (A, Bm):
            diag, offd, counts, displs = synth.split_blocks(mat, world, rank)
            ctxs.append(H.Context(H.HostBlocks(diag, offd, n, counts, displs)))
        ca, cb = ctxs
        lo, nl = int(displs[rank]), int(counts[rank])
        if kind == "six":
            assert (nl == 0) == (rank >= 6)                 # the seventh rank has no rows: it passes NULL
        else:
            assert ca.plan_info()["halo"] > 0
        assert ca.flags() == cb.flags() and ca.plan_info() == cb.plan_info(), "the comparison is void: the two matrices got different plans"
        x0 = (0.25 * synth._uniform(idx, 77) - 0.125)[lo:lo + nl]
        b = A.matvec(1.0 + 0.5 * synth._uniform(idx, 78))[lo:lo + nl]
        d = d_glob[lo:lo + nl]

        def counted(call):
            c0 = ca.comm_counts()
            out = call()
            c1 = ca.comm_counts()
            return out, {k: c1[k] - c0[k] for k in c1}

        def raw(a):      # bytes; neither system breaks down within twelve iterations, so a NaN anywhere is a failure of its own
            a = np.array(a, dtype=np.float64)
            assert not np.isnan(a).any(), "a NaN in what a solve reports"
            return a.tobytes()

        def state(ctx, got, with_x=True):
            tr = ctx.trace(got["k"])
            q = got["result"]
            return (got["k"], q.iterations, q.breakdown_iteration, raw(q.dot_r), raw(q.dot_zero),
                    raw(got["x"]) if with_x else b"", raw(got["r"]), tuple(raw(tr[k]) for k in ("alpha", "omega", "beta", "dotr")))

        # ---- without a preconditioner: refused on every rank, nothing moves
        got, moved = counted(lambda: ca.solve("bicgstab_diag", b, x0=x0, **FIXED))
        assert got["k"] == -2 and got["x"].tobytes() == x0.tobytes() and got["r"].tobytes() == b.tobytes()
        assert moved == dict(exchanges=0, allreduces=0), moved
        # ---- d = 1
        rc, moved = counted(lambda: ca.set_diagonal(np.ones(nl) if nl else None))
        assert rc == 0 and moved == dict(exchanges=0, allreduces=0), (rc, moved)
        assert ca.preconditioner() == "diagonal"
        want, d_plain = counted(lambda: state(ca, ca.solve("bicgstab", b, x0=x0, **FIXED)))
        got, d_diag = counted(lambda: state(ca, ca.solve("bicgstab_diag", b, x0=x0, **FIXED)))
        assert want[0] == 12 or kind == "six", want[0]
        assert got == want, "d = 1"
        assert d_diag == d_plain and d_plain["allreduces"] > 0, (d_plain, d_diag)
        M.same_on_every_rank(dist, world, (got[0], got[3], got[4], got[7]), "d = 1")
        # ---- d = powers of two
        rc, moved = counted(lambda: ca.set_diagonal(d if nl else None))
        assert rc == 0 and moved == dict(exchanges=0, allreduces=0), (rc, moved)
        ga, d_diag = counted(lambda: ca.solve("bicgstab_diag", b, x0=x0, **FIXED))
        gb = cb.solve("bicgstab", b, x0=d * x0, **FIXED)
        assert state(ca, ga, with_x=False) == state(cb, gb, with_x=False), "d = 2^e"
        assert raw(ga["x"]) == raw(gb["x"] / d), "d = 2^e: x"
        assert d_diag == d_plain, (d_plain, d_diag)
        assert not ca.comm_failed() and not cb.comm_failed()
        ca.close(); cb.close()
        dist.barrier()
        H.lib().bicg_comm_finalize()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise
