"""The crafted matrices of tests/padded_cases.py sit where they say: for every case the host-only sliced-ELL plan
(hipsolver.sell_plan_digest, csrc/bicg_sell_plan.cpp) of the REAL matrix, under the case's switches, keeps every row in padded
slices -- no jagged slices, no x window, no rows over lanes, no CSR row blocks -- and reports 16-bit offsets and the number of
fused-window clusters the facts promise; and the limits the cases were built for are spelled out once, both sides of each, with
the kernel and the tile the mirror `padded_cases.spmm_kind` derives for them. A generator that drifted off its limit fails here,
on the CPU, instead of passing quietly on the GPU (tests/test_padded_limits_gpu.py runs exactly these matrices)."""
import os

import pytest

import padded_cases as K
from mpi_bicgstab_amd import hipsolver as H


def plan(A, sw):
    """the summary of the plan of the one-rank block A under the BICG_PLAN switches sw alone"""
    os.environ.pop("BICG_PLAN", None)          # (tests/conftest.py puts the variable back after the test)
    H.switches(**sw)
    summary, _ = H.sell_plan_digest(H.single_rank_blocks(A), 1)
    return summary


@pytest.mark.parametrize("values", ["generic", "integer"])
@pytest.mark.parametrize("name", K.CASES)
def test_case_plans_as_promised(name, values):
    if name == "walk" and values == "integer":
        values = "generic"          # (the large case once: its plan does not look at the values)
    A, facts, sw = K.build(name, values)
    s = plan(A, sw)
    print(name, {k: s[k] for k in ("jag", "window", "rowsplit", "nblk", "sell_rows", "sell_nnz", "c16", "clusters")}, K.spmm_kind(facts))
    assert (s["jag"], s["window"], s["rowsplit"], s["nblk"]) == (0, 0, 0, 0)
    assert s["sell_rows"] == A.rows == facts["rows"] and s["sell_nnz"] == A.nnz
    assert {k: s[k] for k in K.FACT_KEYS} == {k: facts[k] for k in K.FACT_KEYS}


def test_lengths_needs_its_switch():
    """without layout=pad the hand-built rows are ragged enough for jagged slices: the case would not reach the padded kernels"""
    A, _, sw = K.build("lengths")
    assert sw == {"layout": "pad"} and plan(A, {})["jag"] == 1


@pytest.mark.parametrize("name,kinds", [("clusters4_odd", ("pipelined", 256, 0)), ("lengths_x3", ("pipelined", 512, 0))])
def test_rank_blocks_of_the_three_rank_cases_plan_padded(name, kinds):
    """tests/test_padded_limits_ranks_gpu.py cuts these two into three equal row ranges: every rank's diag block keeps all its rows in
    padded slices, the ranges are no multiples of 64, and the mirror names the same kernel for every rank"""
    from mpi_bicgstab_amd import synth
    from ragged_cases import Pattern
    import numpy as np
    A, _, sw = K.build(name)
    os.environ.pop("BICG_PLAN", None)
    H.switches(**sw)
    parts = [synth.split_blocks(A, 3, rank) for rank in range(3)]
    for rank, (diag, offd, counts, displs) in enumerate(parts):
        assert all(int(c) % 64 for c in counts)
        s, _ = H.sell_plan_digest(H.HostBlocks(diag, offd, A.rows, counts, displs), 3, A.rows, sum(p[0].nnz for p in parts))
        drow = np.repeat(np.arange(diag.rows, dtype=np.int64), np.diff(diag.ptr.astype(np.int64)))
        f = K.plan_facts(Pattern(diag.rows, drow, diag.col.astype(np.int64), presorted=True))
        assert (s["jag"], s["window"], s["rowsplit"], s["nblk"], s["sell_rows"]) == (0, 0, 0, 0, diag.rows), (rank, s)
        assert (s["c16"], s["clusters"]) == (f["c16"], f["clusters"]) and K.spmm_kind(f) == kinds, (rank, s, f["cluster_list"])
        assert (offd.nnz > 0) == (rank < 2 or name == "clusters4_odd")


def test_limits_as_the_generators_state_them():
    """what the cases promise, spelled out once: both sides of every limit are among them"""
    f = {name: K.build(name)[1] for name in K.SMALL}
    kind = {name: K.spmm_kind(f[name]) for name in f}
    # a gap of 512 columns joins two offsets into one cluster, 513 separates them -- and the separated pair, rounded to even
    # distances (0 .. 514), is exactly one 512-row tile apart: 514 <= 0 + 2 + 512 refuses that tile
    assert f["gap512"]["offsets"] == [-1, 0, 512] and f["gap512"]["cluster_list"] == [(-1, 512)] and kind["gap512"] == ("pipelined", 512, 0)
    assert f["gap513"]["offsets"] == [0, 513]
    assert f["gap513"]["cluster_list"] == [(0, 0), (513, 513)] and K.rounded(f["gap513"]["cluster_list"]) == [(0, 0), (512, 514)]
    assert not K.pipe_fits(f["gap513"]["cluster_list"], 512) and kind["gap513"] == ("pipelined", 256, 0)
    # 514 apart: lo' = 514 > 0 + 512 fits the 512-row tile; with an odd end in front of it (hi = 1 -> hi' = 2) it does not
    assert f["gap514_even"]["cluster_list"] == [(0, 0), (514, 514)] and kind["gap514_even"] == ("pipelined", 512, 0)
    assert f["gap514_odd"]["cluster_list"] == [(0, 1), (515, 515)] and K.rounded(f["gap514_odd"]["cluster_list"]) == [(0, 2), (514, 516)]
    assert kind["gap514_odd"] == ("pipelined", 256, 0)
    # 4 clusters are the most; 5 leave no cluster plan: the row-major kernel with 16-bit offsets
    assert f["clusters4"]["clusters"] == 4 and f["clusters5"]["clusters"] == 0 and f["clusters5"]["c16"] == 1
    assert kind["clusters5"] == ("rowmajor", 0, 0) and K.row_layout(f["clusters5"]) == "LAY_PAD16"
    # the pipeline's window of 512-row tiles: exactly 2048 slots fit, 2050 (one odd offset, rounded) do not
    assert K.pipe_slots(f["clusters4"]["cluster_list"], 512) == 2048 and kind["clusters4"] == ("pipelined", 512, 0)
    assert K.pipe_slots(f["clusters4_odd"]["cluster_list"], 512) == 2050 and kind["clusters4_odd"] == ("pipelined", 256, 0)
    # ... of 256-row tiles: exactly 1536 fit, 1538 go to the windowed kernel (neither fits 512-row tiles: 2304 and 2306 slots)
    assert [K.pipe_slots(f[c]["cluster_list"], 256) for c in ("pipe1536", "pipe1538")] == [1536, 1538]
    assert [K.pipe_slots(f[c]["cluster_list"], 512) for c in ("pipe1536", "pipe1538")] == [2304, 2306]
    assert kind["pipe1536"] == ("pipelined", 256, 0) and kind["pipe1538"] == ("windowed", 0, 4) and f["pipe1538"]["W256"] == 1537
    # the window of a 256-row group: 2048 slots are a cluster plan (no pipeline tile fits: 2048 > 1536), 2049 are none
    assert (f["slots2048"]["W256"], f["slots2048"]["clusters"]) == (2048, 4) and kind["slots2048"] == ("windowed", 0, 4)
    assert f["slots2049"]["clusters"] == 0 and kind["slots2049"] == ("rowmajor", 0, 0) and K.row_layout(f["slots2049"]) == "LAY_PAD16"
    # the windowed kernel's vectors per window: 8 at 1280 slots, 4 at 1281 -- single clusters the pipeline takes by default
    assert [(f[c]["clusters"], f[c]["W256"]) for c in ("win1280", "win1281")] == [(1, 1280), (1, 1281)]
    assert kind["win1280"] == ("pipelined", 512, 0) and kind["win1281"] == ("pipelined", 512, 0)
    assert K.spmm_kind(f["win1280"], spmm_window=1) == ("windowed", 0, 8) and K.spmm_kind(f["win1281"], spmm_window=1) == ("windowed", 0, 4)
    # 16-bit offsets reach +-32767; one column further: 32-bit columns, no clusters
    assert (f["far32767"]["c16"], f["far32767"]["clusters"]) == (1, 3) and kind["far32767"] == ("pipelined", 512, 0)
    assert (f["far32768"]["c16"], f["far32768"]["clusters"]) == (0, 0) and f["far32768"]["offsets"][-1] == 32768
    assert kind["far32768"] == ("rowmajor", 0, 0) and K.row_layout(f["far32768"]) == "LAY_PAD32"
    # the switches: spmm-window=0 / 1 select the other two forms wherever there are clusters; a forced 256-row tile is never retried at 512
    for name in f:
        if f[name]["clusters"]:
            assert K.spmm_kind(f[name], spmm_window=0)[0] == "rowmajor" and K.spmm_kind(f[name], spmm_window=1)[0] == "windowed"
    assert K.spmm_kind(f["clusters4"], spmm_tile=256) == ("pipelined", 256, 0) and K.spmm_kind(f["slots2048"], spmm_tile=256)[0] == "windowed"
    # the hand-built rows: every length of LENGTHS is the longest row of its slice, one cluster 0 .. 64
    assert f["lengths"]["slices"] == list(K.LENGTHS) + [K.LENGTHS_TAIL[1]] and kind["lengths"] == ("pipelined", 512, 0)
    assert len(f["lengths"]["empty_rows"]) >= 64 + 10
    # the tridiagonal cases: 1 .. 9 tiles of 512 rows, the last one from one row to full
    assert [-(-n // 512) for n in K.TRI_ROWS] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 8, 9]
    assert all(kind[f"tri{n}"] == ("pipelined", 512, 0) for n in K.TRI_ROWS)


def test_some_workgroup_owns_two_tiles():
    """the arithmetic of spmm_pipe_shape for the cases of tests/test_padded_limits_gpu.py that cross a tile change: every tile has
    exactly one owner, and some workgroup owns at least two"""
    f = K.pattern("walk")[1]
    assert K.spmm_kind(f) == ("pipelined", 512, 0) and K.spmm_kind(f, spmm_tile=256) == ("pipelined", 256, 0)
    for rows, T, gstep, tiles, grid, most in ((K.WALK_ROWS, 512, None, 516, 512, 2), (K.WALK_ROWS, 256, None, 1031, 768, 2),
                                              (9000, 512, 2500, 18, 8, 3), (9000, 512, 1000, 18, 24, 1)):
        g, own = K.pipe_ownership(rows, T, gstep)
        assert g == grid and sorted(t for o in own for t in o) == list(range(tiles)), (rows, T, gstep)
        assert max(len(o) for o in own) == most, (rows, T, gstep)
