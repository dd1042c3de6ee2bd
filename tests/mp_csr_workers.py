"""Worker of tests/test_csr_limits_ranks_gpu.py: `world` spawned processes share cuda:0 through the host-staged transport (gloo
rendezvous on 127.0.0.1, as tests/mp_multi_workers.py) and run the products of csrc/bicg_spmv_csr.hip on a case of tests/csr_cases.py
cut into equal row ranges: the row blocks next to a cut touch the halo and run with the offd part in their epilogue.

Per rank the product is, in its bytes, the reference on the rank's diag block followed by + (the offd products added in stored
order) -- y = 0.0 + diag sum; y += offd sum (reference src/matrix.c:434-440). For a stream case that is the oracle's spmv over
`world` virtual ranks (rows of more than 2048 diag entries, reduced with strided partial sums, within 1e-13 sum |a x|); for a
rows-over-lanes case csr_cases.rows_model on the diag block with the blocks cut from the diag block's own row pointers. Then six
iterations of bicgstab on the dominant values against the oracle over `world` virtual ranks, traces at rtol 1e-8.
A rank reports through the ok<rank> / fail<rank> files of mp_workers.py."""
from __future__ import annotations

import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

KEYS = ("alpha", "omega", "beta", "dotr")
BAR = 1e-13


def csr_worker(rank, world, port, kind, outdir):
    try:
        import numpy as np
        import csr_cases as K
        import mp_multi_workers as M
        import oracle_lib as O
        from bitwise import assert_same_bits
        dist = M._init(rank, world, port)
        from mpi_bicgstab_amd import hipsolver as H, synth
        from mpi_bicgstab_amd import dist_transport as T

        T.init_host_transport(0)
        A, facts, sw = K.build(kind)
        n = A.rows
        H.switches(persist=0, **sw)
        diag, offd, counts, displs = synth.split_blocks(A, world, rank)
        lo, nl = int(displs[rank]), int(counts[rank])
        middle = rank == world // 2
        ctx = H.Context(H.HostBlocks(diag, offd, n, counts, displs))
        info, fl = ctx.plan_info(), ctx.flags()
        assert fl["rowsplit"] == bool(facts["rowsplit"]) and not fl["persist"], fl
        if middle:
            assert info["halo"] > 0 and info["boundary_blocks"] > 0 and info["sell_rows"] == 0, info
            assert info["boundary_blocks"] < info["row_blocks"], info

        # the product
        x = np.random.default_rng(1000).standard_normal(n)
        xl = x[lo:lo + nl]
        H.product_kernels()
        y1 = ctx.spmv(xl)
        y2 = ctx.spmv(xl)
        ran = H.product_kernels()
        if middle:
            assert ran == facts["kernels"], ran
        dlen = np.diff(diag.ptr.astype(np.int64))
        row, col, val = A.to_coo()
        if facts["rowsplit"]:
            assert ran == ["rows"], ran
            desc = K.descriptors(diag.ptr, K.row_blocks(diag.ptr, 0, nl, K.ROWS_CHUNK, K.ROWS_MAX_ROWS))
            if middle:
                assert len(set(K.lanes_of(desc).tolist())) >= 3, "several lane counts on the middle rank"
            orow = np.repeat(np.arange(nl, dtype=np.uint32), np.diff(offd.ptr.astype(np.int64))) + np.uint32(lo)
            so = O.spmv(n, orow, offd.col, offd.val, x)[lo:lo + nl]          # the offd products added in stored order
            want = K.rows_model(diag, desc, xl) + so
            strided = np.zeros(0, dtype=np.int64)
        else:
            want = O.spmv(n, row, col, val, x, nranks=world)[lo:lo + nl]
            strided = np.flatnonzero(dlen > K.STAGED)
            if middle:
                assert len(strided) == 1, "the row of 5000: more than 2048 of its entries are this rank's"
        keep = np.ones(nl, dtype=bool)
        keep[strided] = False
        assert_same_bits(y1[keep], want[keep], f"{kind} rank {rank}")
        assert_same_bits(y2, y1, f"{kind} rank {rank}, again")
        if len(strided):
            rows = lo + strided
            scale = np.array([np.abs(val[row == r] * x[col[row == r]]).sum() for r in rows])
            assert np.all(np.abs(y1[strided] - want[strided]) <= BAR * scale), (y1[strided], want[strided])
        ctx.close()

        # six iterations on the dominant values
        D, _, _ = K.build(kind, "dominant")
        drow, dcol, dval = D.to_coo()
        b = O.spmv(n, drow, dcol, dval, np.ones(n), nranks=world)
        want = O.solve("bicgstab", n, drow, dcol, dval, b, nranks=world, tol=0.0, max_iter=6)
        diag, offd, counts, displs = synth.split_blocks(D, world, rank)
        ctx = H.Context(H.HostBlocks(diag, offd, n, counts, displs))
        got = ctx.solve("bicgstab", b[lo:lo + nl], tol=0.0, max_iter=6, check_every=6)
        tr = ctx.trace(6)
        assert got["k"] == 6 == want["k"], (got["k"], want["k"])
        M.same_on_every_rank(dist, world, tuple(tr[k].tobytes() for k in KEYS), kind)
        for k in KEYS:
            assert np.allclose(tr[k][:6], want[k][:6], rtol=1e-8, atol=0.0), (kind, k, tr[k][:6], want[k][:6])
        scale = float(np.abs(want["x"]).max())
        assert np.abs(got["x"] - want["x"][lo:lo + nl]).max() <= 1e-8 * scale
        assert not ctx.comm_failed()
        ctx.close()
        dist.barrier()
        H.lib().bicg_comm_finalize()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise
