"""Worker functions for the world_size-2 tests (spawned processes, gloo rendezvous on 127.0.0.1)."""
from __future__ import annotations

import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _init(rank, world, port):
    import torch
    torch.set_num_threads(1)      # 8 ranks x (cores) OpenMP threads spinning would starve the gloo exchanges
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def run_ranks(fn, world, kind, wall_limit, prepare=None):
    """Spawn `world` ranks of worker fn(rank, world, port, kind, outdir) and wait for them, wall_limit seconds at the most; ranks
    still alive then, or after one of them raised, are ended. prepare(outdir) runs before the ranks start. Asserts that no rank
    left a fail* file and that every rank left ok* -- unless some left skip*: their texts are returned for the caller to skip on."""
    import glob
    import socket
    import tempfile
    import time
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    with tempfile.TemporaryDirectory() as td:
        if prepare:
            prepare(td)
        procs = mp.start_processes(fn, args=(world, port, kind, td), nprocs=world, join=False, start_method="spawn")
        t0, error = time.monotonic(), None
        try:
            while not procs.join(timeout=2.0):
                if time.monotonic() - t0 > wall_limit:
                    error = f"the ranks were still running after {wall_limit:.0f} s"
                    break
        except Exception as e:      # a rank raised: join() has ended the others
            error = str(e)
        for p in procs.processes:
            if p.is_alive():
                p.terminate()
        for p in procs.processes:
            p.join(10)
            if p.is_alive():
                p.kill()
        fails = sorted(glob.glob(os.path.join(td, "fail*")))
        assert not fails, open(fails[0]).read()
        assert error is None, error
        skips = [open(f).read() for f in sorted(glob.glob(os.path.join(td, "skip*")))]
        assert skips or len(glob.glob(os.path.join(td, "ok*"))) == world
        return skips


def test_matrix(kind):
    from mpi_bicgstab_amd import synth
    if kind == "offsets":
        return synth.from_offsets(4001, (0, 1, -1, 7, -7, 300, -300, 1999, -1999), diag_base=12.0, seed=3)
    if kind == "stencil":
        return synth.stencil7(14)
    if kind == "laplace":      # BASELINE.json configs[3] family, z-slabs over the ranks
        return synth.stencil7(40, synth.LAPLACE_WEIGHTS)
    if kind == "ragged":
        return synth.random_rows(900, 9, seed=21, empty_frac=0.05, long_rows={40: 700})
    raise ValueError(kind)


def plan_worker(rank, world, port, kind, outdir):
    """CPU only: halo plan + send lists through the library's host code and gloo callbacks, then a
    numpy emulation of the halo SpMV compared with the oracle's distributed SpMV."""
    try:
        import ctypes as C
        import numpy as np
        dist = _init(rank, world, port)
        import oracle_lib as O
        from mpi_bicgstab_amd import hipsolver as H, synth
        from mpi_bicgstab_amd import dist_transport as T

        A = test_matrix(kind)
        diag, offd, counts, displs = synth.split_blocks(A, world, rank)
        blk = H.HostBlocks(diag, offd, A.rows, counts, displs)
        h, halo_cols, rc, ren = H.halo_plan(blk, world)
        ar, a2a = T.callbacks()
        L = H.lib()
        sc = np.zeros(world, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        up = C.POINTER(C.c_uint)
        hc = np.ascontiguousarray(halo_cols if h else np.zeros(1, dtype=np.uint32))
        total = L.bicg_halo_send_counts(world, rc.ctypes.data_as(ip), a2a, None, sc.ctypes.data_as(ip))
        send_idx = np.zeros(max(total, 1), dtype=np.uint32)
        got = L.bicg_halo_send_lists(rank, world, C.byref(blk.info), blk.n_loc, hc.ctypes.data_as(up),
                                     rc.ctypes.data_as(ip), sc.ctypes.data_as(ip), a2a, None, send_idx.ctypes.data_as(up))
        assert got == total >= 0
        assert rc[rank] == 0 and sc[rank] == 0            # own columns never travel
        # value exchange with the same callback the library would use (counts in bytes)
        x = np.random.default_rng(1234).standard_normal(A.rows)
        lo = int(displs[rank])
        x_loc = x[lo:lo + blk.n_loc]
        sendbuf = np.ascontiguousarray(x_loc[send_idx[:total]])
        recvbuf = np.zeros(max(h, 1))
        sdsp = np.concatenate(([0], np.cumsum(sc)[:-1])).astype(np.int32)
        rdsp = np.concatenate(([0], np.cumsum(rc)[:-1])).astype(np.int32)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        a2a(sendbuf.ctypes.data, i32(sc * 8).ctypes.data_as(ip), i32(sdsp * 8).ctypes.data_as(ip),
            recvbuf.ctypes.data, i32(rc * 8).ctypes.data_as(ip), i32(rdsp * 8).ctypes.data_as(ip), None)
        assert np.array_equal(recvbuf[:h], x[halo_cols])   # the halo holds exactly the requested entries
        x_ext = np.concatenate((x_loc, recvbuf[:h]))
        off_r = synth.CSR(offd.rows, blk.n_loc + h, offd.ptr, ren.astype(np.uint32) if offd.nnz else offd.col, offd.val)
        y = diag.matvec(x_loc) + (off_r.matvec(x_ext) if offd.nnz else 0.0)
        row, col, val = A.to_coo()
        y_orc = O.spmv(A.rows, row, col, val, x, nranks=world)[lo:lo + blk.n_loc]
        scale = np.abs(A.val).max() * np.abs(x).max() * 64
        assert np.abs(y - y_orc).max() <= 1e-13 * scale
        # packed all-reduce callback
        v = np.arange(5, dtype=np.float64) + rank
        ar(v.ctypes.data_as(C.POINTER(C.c_double)), 5, None)
        assert np.array_equal(v, world * np.arange(5) + sum(range(world)))
        dist.barrier()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise


def gpu_worker(rank, world, port, kind, outdir):
    """GPU box: `world` ranks share cuda:0 through the host-staged transport; the full multi-rank
    path (halo plan, interior/boundary SpMV, packed dot groups, all four solvers) vs the oracle."""
    try:
        import numpy as np
        dist = _init(rank, world, port)
        import oracle_lib as O
        from mpi_bicgstab_amd import hipsolver as H, synth
        from mpi_bicgstab_amd import dist_transport as T

        T.init_host_transport(0)
        p2p = kind.endswith("+p2p")
        kind = kind.replace("+p2p", "")
        if p2p:
            # data path through IPC-mapped mailboxes (bicg_p2p.cpp); gloo only bootstraps
            assert H.lib().bicg_comm_enable_p2p() == 0, "peer-to-peer transport did not come up"
            assert H.lib().bicg_comm_p2p_active() > 0
        balanced = kind.endswith("+nnz")
        kind = kind.replace("+nnz", "")
        A = test_matrix(kind)
        part = synth.partition_nnz(A, world) if balanced else None     # non-zero balanced cuts
        diag, offd, counts, displs = synth.split_blocks(A, world, rank, part=part)
        lo, nl = int(displs[rank]), int(counts[rank])
        if balanced:
            assert not np.array_equal(counts, synth.partition(A.rows, world)[0]), "test matrix does not move the cuts"
            O_spmv, O_solve = O.spmv, O.solve
            O.spmv = lambda *a, **k: O_spmv(*a, counts=counts, **k)
            O.solve = lambda *a, **k: O_solve(*a, counts=counts, **k)
        ctx = H.Context(H.HostBlocks(diag, offd, A.rows, counts, displs))
        info = ctx.plan_info()
        assert info["halo"] > 0 and info["boundary_blocks"] > 0
        row, col, val = A.to_coo()
        if p2p:
            # more back-to-back exchanges than the landing ring has slots: wrap-around + flow control
            rng = np.random.default_rng(5)
            lens = np.diff(A.ptr.astype(np.int64))[lo:lo + nl]
            for rep in range(2 * 8 + 3):
                xs = rng.standard_normal(A.rows)
                ys = ctx.spmv(xs[lo:lo + nl])
                ys_orc = O.spmv(A.rows, row, col, val, xs, nranks=world)[lo:lo + nl]
                assert np.array_equal(ys[lens <= 2048], ys_orc[lens <= 2048]), f"exchange {rep} delivered stale or wrong halo values"
            ctx.spmv_bench(40)
        x = np.random.default_rng(99).standard_normal(A.rows)
        y = ctx.spmv(x[lo:lo + nl])
        y_orc = O.spmv(A.rows, row, col, val, x, nranks=world)[lo:lo + nl]
        lens = np.diff(A.ptr.astype(np.int64))[lo:lo + nl]
        assert np.array_equal(y[lens <= 2048], y_orc[lens <= 2048]), "distributed SpMV is not bit-exact"
        if ctx.flags()["spmm"]:      # the same on every rank: the SpMM exchanges halos
            # distributed SpMM (halo of every vector, offd part per column): columns = the distributed SpMV of each vector
            X = np.random.default_rng(17).standard_normal((5, A.rows))
            Y, _ = ctx.spmm(X[:, lo:lo + nl], 0.25 * np.arange(5))
            for j in range(5):
                yj = O.spmv(A.rows, row, col, val, X[j], nranks=world)[lo:lo + nl] + 0.25 * j * X[j, lo:lo + nl]
                assert np.array_equal(Y[j], yj), f"SpMM column {j}"
        d = ctx.dot(x[lo:lo + nl], y_orc)
        d_ref = float(np.dot(x, O.spmv(A.rows, row, col, val, x, nranks=world)))
        assert abs(d - d_ref) <= 1e-11 * abs(d_ref) + 1e-9
        b_full = O.spmv(A.rows, row, col, val, np.ones(A.rows), nranks=world)
        b = ctx.spmv(np.ones(nl))
        assert np.array_equal(b, b_full[lo:lo + nl])
        for method, tol in (("bicgstab", 1e-15), ("ca_bicgstab", 1e-15), ("pipe_bicgstab", 1e-9), ("pipe_bicgstab_rr", 1e-15)):
            orc = O.solve(method, A.rows, row, col, val, b_full, nranks=world, tol=tol, krr=10, nrr=3)
            got = ctx.solve(method, b, tol=tol, krr=10, nrr=3, check_every=4)
            # the Laplacian's trajectories, and the replacement variant's at tol 1e-15 on any matrix, are sensitive to
            # the association of the dot sums (the reference's own count moves by a few iterations with the rank
            # count): rows, hence wavefront partial sums, are grouped differently by every storage layout
            slack = max(2, orc["k"] // 15) if kind == "laplace" else max(2, orc["k"] // 12) if method == "pipe_bicgstab_rr" else 2
            assert abs(got["k"] - orc["k"]) <= slack, (method, got["k"], orc["k"])
            lo_err = np.abs(orc["x"] - 1.0).max()             # what the reference itself achieves
            assert np.abs(got["x"] - 1.0).max() <= max(100 * lo_err, 1e-6 if tol > 1e-12 else 1e-9), method
            tr = ctx.trace(got["k"])
            h = min(5, got["k"], orc["k"])
            np.testing.assert_allclose(tr["dotr"][:h], orc["dotr"][:h], rtol=1e-7)
        if p2p:
            # the pipelined solver's three forms across ranks: persistent one-launch chunks (the default when the plan fits on
            # every rank), two launches per iteration, separate kernels -- same answer up to the association of the dot sums
            fl = ctx.flags()
            orcs = {m: O.solve(m, A.rows, row, col, val, b_full, nranks=world, tol=1e-9) for m in ("pipe_bicgstab", "bicgstab", "ca_bicgstab")}
            for name, env in (("persistent", dict(persist=1, fuse_pipe=None)), ("two-launch", dict(persist=0, fuse_pipe=1)),
                              ("separate", dict(persist=0, fuse_pipe=0))):
                H.switches(**env)
                c2 = H.Context(H.HostBlocks(diag, offd, A.rows, counts, displs))
                if name == "persistent" and kind in ("offsets", "stencil", "laplace"):      # (a block with a 700-entry row does not qualify)
                    assert c2.flags()["persist"], c2.flags()
                for m in (("pipe_bicgstab", "bicgstab", "ca_bicgstab") if name == "persistent" else ("pipe_bicgstab",)):
                    orc = orcs[m]
                    g2 = c2.solve(m, b, tol=1e-9, check_every=4)
                    slack = max(2, orc["k"] // 15) if kind == "laplace" else 2
                    assert abs(g2["k"] - orc["k"]) <= slack, (name, m, g2["k"], orc["k"])
                    assert np.abs(g2["x"] - 1.0).max() <= max(100 * np.abs(orc["x"] - 1.0).max(), 1e-6), (name, m)
                    g3 = c2.solve(m, b, tol=1e-9, check_every=4)          # run to run: same bits
                    assert g3["k"] == g2["k"] and np.array_equal(g3["x"], g2["x"]), (name, m)
                c2.close()
            H.switches(persist=None, fuse_pipe=None)
        # shifted systems, 5 shifts, seed 2 (reference src/test_shifted.c:95-111 set-up)
        sigma, seed = 0.01 * (np.arange(5) + 1.0), 2
        bs_full = b_full + sigma[seed] * np.ones(A.rows)
        # (the pipelined shifted recurrence on the Laplacian is too sensitive to the association of the dot sums for an
        # iteration-count comparison: 81 / 96 iterations for two summation orders)
        for which in (() if balanced else ("shifted_lopbicgstab",) if kind == "laplace" else ("shifted_lopbicgstab", "shifted_pipe_lopbicgstab")):
            orc = O.solve_shifted(A.rows, row, col, val, bs_full, sigma, seed, nranks=world, which=which)
            got = ctx.solve_shifted(bs_full[lo:lo + nl], sigma, seed, check_every=4, which=which)
            assert abs(got["k"] - orc["k"]) <= (max(2, orc["k"] // 15) if kind == "laplace" else 2), (which, got["k"], orc["k"])
            assert np.abs(got["x"] - orc["x"][:, lo:lo + nl]).max() <= 1e-8 * max(1.0, np.abs(orc["x"]).max()), which
        # seed-switching variants (reference src/shifted_switching_solver.c): the seed (largest shift)
        # converges first, the device pauses, every rank re-points to the same new seed
        if not balanced and kind not in ("ragged", "laplace"):
            sg8, sd8 = 0.02 * 2.0 ** np.arange(8), 7
            b8 = b_full + sg8[sd8] * np.ones(A.rows)
            for which in ("shifted_lopbicg", "shifted_lopbicg_switching"):
                orc = O.solve_switching(A.rows, row, col, val, b8, sg8, sd8, nranks=world, which=which)
                got = ctx.solve_shifted(b8[lo:lo + nl], sg8, sd8, check_every=5, which=which)
                assert abs(got["k"] - orc["k"]) <= 3, (which, got["k"], orc["k"])
                assert got["switches"] == orc["switches"], (which, got["switches"], orc["switches"])
                assert np.abs(got["x"] - orc["x"][:, lo:lo + nl]).max() <= 1e-8 * max(1.0, np.abs(orc["x"]).max()), which
            assert orc["switches"] >= 1, "test set-up: no seed switch happened"
        ctx.close()
        dist.barrier()
        H.lib().bicg_comm_finalize()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise


def memory_worker(rank, world, port, kind, outdir):
    """GPU box: tests/test_device_memory_gpu.py across ranks. Every call that allocates lazily runs on a context of the host
    transport with the peer-to-peer data path; after close() the rank's count of live device allocations is what it was before
    the context was built (the transport's own memory is not counted)."""
    try:
        import numpy as np
        dist = _init(rank, world, port)
        from mpi_bicgstab_amd import hipsolver as H, synth
        from mpi_bicgstab_amd import dist_transport as T
        from test_device_memory_gpu import check_product, exercise

        T.init_host_transport(0)
        assert kind.endswith("+p2p")
        assert H.lib().bicg_comm_enable_p2p() == 0, "peer-to-peer transport did not come up"
        A = test_matrix(kind.replace("+p2p", ""))
        diag, offd, counts, displs = synth.split_blocks(A, world, rank)
        lo, nl = int(displs[rank]), int(counts[rank])
        before = H.device_allocations()
        ctx = H.Context(H.HostBlocks(diag, offd, A.rows, counts, displs))
        fl = ctx.flags()
        assert fl["p2p"] and fl["ll_fused"] and fl["spmm"] and fl["persist"], fl
        assert H.device_allocations() > before
        b = exercise(ctx, A.matvec(np.ones(A.rows))[lo:lo + nl])
        check_product(b, A, np.ones(A.rows), lo, world)
        x = np.random.default_rng(3).standard_normal(A.rows)
        check_product(ctx.spmv(x[lo:lo + nl]), A, x, lo, world)
        assert not ctx.comm_failed()
        ctx.close()
        assert H.device_allocations() == before
        dist.barrier()
        H.lib().bicg_comm_finalize()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise


def empty_rank_worker(rank, world, port, kind, outdir):
    """More ranks than rows (reference src/matrix.c:295-298: the trailing ranks get ZERO rows and its loops run empty): a
    6-row matrix over 8 ranks, ranks 6 and 7 own nothing. Every rank creates its context (the empty ones hold a phantom row,
    bicg_ctx::phantom), takes part in every exchange, and the four solvers + a shifted solve give the oracle's iterates at
    P = 8; the empty ranks pass and get back empty vectors."""
    try:
        import numpy as np
        dist = _init(rank, world, port)
        import oracle_lib as O
        from mpi_bicgstab_amd import hipsolver as H, synth
        from mpi_bicgstab_amd import dist_transport as T

        T.init_host_transport(0)
        if kind == "p2p":
            assert H.lib().bicg_comm_enable_p2p() == 0, "peer-to-peer transport did not come up"
        A = synth.from_offsets(6, (0, 1, -1, 2), diag_base=5.0, seed=1)
        diag, offd, counts, displs = synth.split_blocks(A, world, rank)
        lo, nl = int(displs[rank]), int(counts[rank])
        assert counts[-1] == 0 and counts[-2] == 0 and (nl == 0) == (rank >= 6)
        ctx = H.Context(H.HostBlocks(diag, offd, A.rows, counts, displs))
        row, col, val = A.to_coo()
        x = np.random.default_rng(3).standard_normal(A.rows)
        y = ctx.spmv(x[lo:lo + nl])
        assert y.shape == (nl,) and np.array_equal(y, O.spmv(A.rows, row, col, val, x, nranks=world)[lo:lo + nl])
        d = ctx.dot(x[lo:lo + nl], x[lo:lo + nl])
        assert abs(d - float(np.dot(x, x))) <= 1e-13 * float(np.dot(x, x))
        b_full = O.spmv(A.rows, row, col, val, np.ones(A.rows), nranks=world)
        b = ctx.spmv(np.ones(nl))
        for method in ("bicgstab", "ca_bicgstab", "pipe_bicgstab", "pipe_bicgstab_rr"):
            orc = O.solve(method, A.rows, row, col, val, b_full, nranks=world, tol=1e-12, krr=10, nrr=3)
            got = ctx.solve(method, b, tol=1e-12, krr=10, nrr=3, check_every=2)
            assert abs(got["k"] - orc["k"]) <= 1, (method, got["k"], orc["k"])
            assert got["x"].shape == (nl,) and (nl == 0 or np.abs(got["x"] - 1.0).max() <= 1e-9), method
        sigma, seed = 0.01 * (np.arange(3) + 1.0), 1
        bs_full = b_full + sigma[seed] * np.ones(A.rows)
        for which in ("shifted_lopbicgstab", "shifted_pipe_lopbicgstab"):
            orc = O.solve_shifted(A.rows, row, col, val, bs_full, sigma, seed, nranks=world, which=which)
            got = ctx.solve_shifted(bs_full[lo:lo + nl], sigma, seed, check_every=2, which=which)
            assert abs(got["k"] - orc["k"]) <= 1, (which, got["k"], orc["k"])
            assert got["x"].shape == (3, nl) and (nl == 0 or np.abs(got["x"] - orc["x"][:, lo:lo + nl]).max() <= 1e-9), which
        ctx.close()
        dist.barrier()
        H.lib().bicg_comm_finalize()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise


def fullsize_worker(rank, world, port, kind, outdir):
    """GPU box: `world` ranks (4 or 8) share cuda:0 and hold the reference's row partition
    (src/matrix.c:295-308) of the FULL-SIZE Transport-shaped matrix -- 200 k-row slabs with their
    +-13 807-column halos at world = 8 (BASELINE.json configs[2]). `kind` = "host" (gloo-staged
    exchanges) or "host-p2p" (kernels store into IPC-mapped mailboxes / halo rings). Distributed SpMV
    bit-exact against the oracle at the same P; the first iterations of all four solvers against
    the oracle's trajectory. The oracle's outputs come from the parent (one CPU run per P)."""
    try:
        import numpy as np
        dist = _init(rank, world, port)
        from mpi_bicgstab_amd import hipsolver as H, synth
        from mpi_bicgstab_amd import dist_transport as T

        os.environ.setdefault("BICG_P2P_TIMEOUT_MS", "20000")
        T.init_host_transport(0)
        p2p = kind == "host-p2p"
        if p2p:
            assert H.lib().bicg_comm_enable_p2p() == 0, "peer-to-peer transport did not come up"
            assert H.lib().bicg_comm_p2p_active() > 0
        ref = np.load(os.path.join(outdir, "oracle.npz"))
        n = int(ref["n"]); k_fix = int(ref["k_fix"])
        counts, displs = synth.partition(n, world)
        lo, nl = int(displs[rank]), int(counts[rank])
        grid = int(ref["grid"]) if "grid" in ref else 0
        mesh_kind = str(ref["mesh_numbering"]) if "mesh_numbering" in ref else ""
        if grid:      # BASELINE.json configs[3] family: z-slabs of the 7-point Laplacian (64 planes per GPU at 512^3 / 8 GPUs)
            slab = synth.stencil7(grid, synth.LAPLACE_WEIGHTS, rows=(lo, lo + nl))
        elif mesh_kind:   # the unstructured FEM matrix (the parent left the assembled matrix in str(ref["mesh_cache"]))
            from mpi_bicgstab_amd import mesh
            slab = mesh.fem_unstructured(int(ref["mesh_m"]), mesh_kind, float(ref["scale_decades"]), rows=(lo, lo + nl), cache_dir=str(ref["mesh_cache"]))
        else:
            slab = synth.transport_like(n=n, rows=(lo, lo + nl), scale_decades=float(ref["scale_decades"]))
        diag, offd = synth.split_row_slab(slab, lo)
        wide = int(ref["stencil_wide"]) if "stencil_wide" in ref else 0
        if wide:
            H.switches(wide=wide)
        ctx = H.Context(H.HostBlocks(diag, offd, n, counts, displs))
        info, flags = ctx.plan_info(), ctx.flags()
        assert info["halo"] > 0 and info["boundary_blocks"] > 0
        assert info["sell_rows"] == nl and flags["all_sell"] and (flags["col16"] or grid or mesh_kind == "random")
        assert flags["p2p"] == p2p
        if mesh_kind:
            assert flags["jagged"] and info["sell_padding"] == 0, (flags, info)       # ragged rows across ranks: jagged slices, no padding
            if p2p:
                # ranks of 4 M non-zeros and more take the exchange as separate launches: their halo-free rows go through the
                # three-trip products (csrc/bicg_jagw.hip); smaller ranks keep the launch with the exchange inside
                big = info["nnz_diag"] >= 4_000_000
                assert flags["ll_fused"] == (not big), (flags, info["nnz_diag"])
                H.product_kernels()
                ctx.spmv(np.ones(nl))
                ran = H.product_kernels()
                assert (("jagd" in ran or "jagw" in ran) == big), (ran, info["nnz_diag"])
        if p2p and not mesh_kind:
            assert flags["ll_fused"], "banded slab: the halo exchange must be folded into the SpMV launch"
        if grid:
            # a z-slab of the grid: the planes without halo entries go to the plane-marching product (csrc/bicg_stencil.hip), the two
            # (one, at either end of the grid) halo-touching planes to the slice-by-slice kernel behind the exchange
            assert ctx.stencil_info()["on"] == 1, ctx.stencil_info()
            assert ctx.stencil_info()["rows_per_lane"] == (wide or 1), ctx.stencil_info()      # (slabs of < 4 M rows keep one row per lane unless asked)
        if "expect_persist" in ref and int(ref["expect_persist"]):
            # ranks small enough for one persistent launch per chunk of iterations (bicg_persist.hip) AND with neighbours:
            # halo pushes by the communication wavefronts, window loads from the landing ring, sums through the mailboxes
            assert flags["persist"] and info["halo"] > 0 and p2p, (flags, info)
        # distributed SpMV: every row bit for bit; enough back-to-back exchanges to wrap the landing ring
        for rep in range(11 if p2p else 2):
            x = ref["x_in"] * (1.0 + 0.125 * rep)
            y = ctx.spmv(x[lo:lo + nl])
            if rep == 0:
                assert np.array_equal(y, ref["y"][lo:lo + nl]), "distributed SpMV is not bit-exact"
            else:
                # scaling x by 1 + rep/8 scales products and sums: not bit-comparable with the stored y, but
                # a stale halo value (ring slot of an earlier exchange) would show up at the 1e-1 level
                np.testing.assert_allclose(y, ref["y"][lo:lo + nl] * (1.0 + 0.125 * rep), rtol=1e-12, atol=1e-9)
        b = ctx.spmv(np.ones(nl))
        assert np.array_equal(b, ref["b"][lo:lo + nl])
        if mesh_kind and flags["spmm"]:      # (the same on every rank: the SpMM exchanges halos)
            # BASELINE.json configs[4] "batched SpMV" across ranks on ragged rows (reference src/test_shifted.c:129-154, one product per
            # shift): 5 vectors, every column bit for bit the distributed product (checked against the oracle above) + shift. A block
            # that kept its x windows (generator order) goes through k_spmm_jpipe with the offd part per column (csrc/bicg_spmm_jag.hip)
            X = np.stack([ref["x_in"][lo:lo + nl] * (1.0 + 0.25 * j) for j in range(5)])
            sg = 0.01 * (np.arange(5) + 1.0)
            Y, _ = ctx.spmm(X, sg)
            if flags["window"] and flags["jagged"]:
                assert ctx.last_spmm_kind() == "pipelined", ctx.last_spmm_kind()
            for j in range(5):
                assert np.array_equal(Y[j], ctx.spmv(X[j]) + sg[j] * X[j]), f"SpMM column {j} ({ctx.last_spmm_kind()})"
        methods = [str(m) for m in ref["methods"]] if "methods" in ref else ["bicgstab", "ca_bicgstab", "pipe_bicgstab", "pipe_bicgstab_rr"]
        rtol = float(ref["rtol"]) if "rtol" in ref else 1e-7          # (the mesh matrix: see tests/test_mesh_gpu.py)
        for method in ([str(m) for m in ref["expect_no_product_kernels"]] if "expect_no_product_kernels" in ref else []):
            # the iterations of these methods run inside persistent launches: no product kernel between run_begin and run_end
            ctx.load(np.zeros(nl), b)
            ctx.run_begin(method, tol=0.0, max_iter=k_fix, check_every=k_fix)
            ctx.sync()
            H.product_kernels()
            ctx.run_iterate(k_fix)
            ctx.sync()
            ran = H.product_kernels()
            assert ctx.run_end().iterations == k_fix and not ran, (method, ran)
        for method in methods:
            got = ctx.solve(method, b, tol=0.0, max_iter=k_fix, krr=5, nrr=1, check_every=k_fix)
            assert got["k"] == k_fix, (method, got["k"])
            tr = ctx.trace(k_fix)
            for key in ("alpha", "omega", "beta", "dotr"):
                np.testing.assert_allclose(tr[key], ref[f"{method}_{key}"], rtol=rtol, err_msg=f"{method} {key}")
            xo = ref[f"{method}_x"]
            assert np.abs(got["x"] - xo[lo:lo + nl]).max() <= 0.1 * rtol * np.abs(xo).max(), method
        # ... and all the way to convergence (oracle run at the same rank count, tolerance in ref): the iteration count
        # within the spread the dot-sum association causes, the manufactured solution x = 1 reached
        for method in ([str(m) for m in ref["converge_methods"]] if "converge_methods" in ref else []):
            tol = float(ref["converge_tol"])
            got = ctx.solve(method, b, tol=tol, max_iter=4000, check_every=16)
            kmin, kmax = int(ref[f"{method}_conv_kmin"]), int(ref[f"{method}_conv_kmax"])
            assert 0.95 * kmin <= got["k"] <= 1.05 * kmax, (method, got["k"], kmin, kmax)      # inside the reference's own spread over P
            relres = np.sqrt(got["result"].dot_r / got["result"].dot_zero)
            assert relres <= tol, (method, relres)
            assert np.abs(got["x"] - 1.0).max() <= 3.0 * float(ref[f"{method}_conv_err"]), (method, np.abs(got["x"] - 1.0).max())
        # BASELINE.json configs[4] across ranks: 16 shifts, seed 7 (reference src/shifted_solver.c:257-319, 794-848); the oracle's
        # seed scalars and a few of its x_j come from the parent
        for which in ([str(m) for m in ref["shifted_methods"]] if "shifted_methods" in ref else []):
            sigma, seed = ref["shifted_sigma"], int(ref["shifted_seed"])
            bs = b + sigma[seed] * np.ones(nl)
            got = ctx.solve_shifted(bs, sigma, seed, tol=0.0, max_iter=k_fix, check_every=k_fix, which=which)
            assert got["k"] == k_fix, (which, got["k"])
            tr = ctx.trace(k_fix)
            for key in ("alpha", "omega", "beta", "dotr"):
                np.testing.assert_allclose(tr[key], ref[f"{which}_{key}"], rtol=1e-7, err_msg=f"{which} {key}")
            for j in ref["shifted_sel"]:
                xo = ref[f"{which}_x{int(j)}"]
                assert np.abs(got["x"][int(j)] - xo[lo:lo + nl]).max() <= 1e-8 * np.abs(xo).max(), (which, int(j))
        assert not ctx.comm_failed()
        ctx.close()
        dist.barrier()
        H.lib().bicg_comm_finalize()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise
