"""Worker of tests/test_padded_limits_ranks_gpu.py: `world` spawned processes share cuda:0 through the host-staged transport (gloo
rendezvous on 127.0.0.1, as tests/mp_multi_workers.py) and run the SpMM kernels over padded slices on a case of
tests/padded_cases.py cut into equal row ranges -- the OFFD instantiations: k_spmm_pipe<true, 512 | 256>, k_spmm_win<0, true, NV>,
k_spmm_sell<LAY_PAD16, true>, every row adding its offd part in the kernel's epilogue.

Per rank and form (as planned, spmm-window=1, spmm-window=0): the SpMM of 17 vectors with 17 distinct shifts is, in its bytes, the
oracle's spmv over `world` virtual ranks (y = 0.0 + diag sum; y += offd sum in stored order, reference src/matrix.c:434-440) for the
rank's rows + sigma_j x_j in float64 numpy; the kernel and tile are what padded_cases.spmm_kind derives from the rank's own diag
block. Then the integer system of the case: bicg_shifted_residuals, summed over the ranks, is the exact value's bytes.
A rank reports through the ok<rank> / fail<rank> files of mp_workers.py."""
from __future__ import annotations

import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FORMS = ({}, {"spmm_window": 1}, {"spmm_window": 0})
NVEC = (1, 3, 16, 17)


def padded_worker(rank, world, port, kind, outdir):
    try:
        import numpy as np
        import padded_cases as K
        import mp_multi_workers as M
        import oracle_lib as O
        from bitwise import assert_same_bits
        from ragged_cases import Pattern
        dist = M._init(rank, world, port)
        from mpi_bicgstab_amd import hipsolver as H, synth
        from mpi_bicgstab_amd import dist_transport as T

        T.init_host_transport(0)
        A, _, sw = K.build(kind)
        n = A.rows
        diag, offd, counts, displs = synth.split_blocks(A, world, rank)
        lo, nl = int(displs[rank]), int(counts[rank])
        middle = rank == world // 2
        assert all(int(c) % 64 for c in counts), counts
        # the facts of this rank's own diag block: the plan sees nothing else
        drow = np.repeat(np.arange(nl, dtype=np.int64), np.diff(diag.ptr.astype(np.int64)))
        facts = K.plan_facts(Pattern(nl, drow, diag.col.astype(np.int64), presorted=True))
        if middle:
            assert offd.nnz > 0
            if kind == "clusters4_odd":          # halo on both sides
                assert int(offd.col.min()) < lo and int(offd.col.max()) >= lo + nl

        row, col, val = A.to_coo()
        X = np.random.default_rng(3000).standard_normal((K.MAX_VECTORS, n))
        sigma = (np.arange(K.MAX_VECTORS) + 1.0) * 0.013
        want = np.stack([O.spmv(n, row, col, val, X[j], nranks=world)[lo:lo + nl] + sigma[j] * X[j, lo:lo + nl] for j in range(len(X))])
        S = K.integer_system(kind)
        Ai, Xi, si, bi, norms = S[0], S[3], S[4], S[5], S[6]
        idiag, ioffd, _, _ = synth.split_blocks(Ai, world, rank)

        for tokens in FORMS:
            expect = K.spmm_kind(facts, spmm_window=tokens.get("spmm_window"))
            tok = dict(sw, persist=0, **tokens)
            H.switches(**tok)
            ctx = H.Context(H.HostBlocks(diag, offd, n, counts, displs))
            info, fl = ctx.plan_info(), ctx.flags()
            assert fl["spmm"] and not fl["jagged"] and info["sell_rows"] == nl, (fl, info)
            if middle:
                assert info["halo"] > 0, info
            for turn in ("", ", again"):
                Y, _ = ctx.spmm(X[:, lo:lo + nl], sigma)
                got = (ctx.last_spmm_kind(), ctx.last_spmm_tile())
                assert got == expect[:2], (kind, rank, tokens, got, expect)
                for j in range(len(X)):
                    assert_same_bits(Y[j], want[j], f"{kind} rank {rank} {tokens}: vector {j}{turn}")
            print(f"{kind} rank {rank} {tokens}: {expect[0]}, tile {expect[1]}, {expect[2]} vectors per window, rows {nl}", flush=True)
            ctx.close()

            ctx = H.Context(H.HostBlocks(idiag, ioffd, n, counts, displs))
            for nvec in NVEC:
                res = ctx.shifted_residuals(Xi[:nvec, lo:lo + nl], bi[lo:lo + nl], si[:nvec])
                assert (ctx.last_spmm_kind(), ctx.last_spmm_tile()) == expect[:2], (kind, rank, tokens)
                assert_same_bits(res, norms[:nvec], f"{kind} rank {rank} {tokens}: residual norms of {nvec} shifts")
            assert not ctx.comm_failed()
            ctx.close()
            H.switches(**{k: None for k in tok})
        dist.barrier()
        H.lib().bicg_comm_finalize()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise
