"""The sliced-ELL plan of a diag block, made on the host (sell_plan_host, csrc/bicg_sell_plan.cpp), pinned array by array.

bicg_sell_plan_digest returns a summary of the plan's decisions and one FNV-1a digest per array of the plan. The expected values
in tests/golden/sell_plan_digests.json were NOT produced by the code under test: they come from the commit named in the file's
"parent" entry, where the plan was still a section of bicg_create() -- that section, verbatim, with the device uploads stubbed
out, hashed the same arrays with the same hash for the case list below (`python tests/test_sell_plan.py --write FILE` against
such a library, BICG_HIP_LIB). So a passing test says: splitting the plan from the upload changed no decision and no byte.

The case list is only good if it reaches every branch of the plan; test_the_cases_reach_every_branch_of_the_plan checks that on
the recorded summaries."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sell_plan_digests.json")


def _fixture(name):
    g = np.load(os.path.join(HERE, "golden", name + ".npz"))
    return synth.CSR(int(g["n"]), int(g["n"]), g["ptr"], g["col"], g["val"])


# name -> matrix (built once per process). Small enough for the CPU suite; every one is cut into rank 1 of 2 and of 4 as well.
MATRICES = {
    "transport_like": lambda: synth.transport_like(40000),
    "fem_like": lambda: synth.fem_like(n=117 * 117 * 3),
    "banded_b8": lambda: synth.banded(30000, 8),
    "banded_b512": lambda: synth.banded(6000, 512),
    "stencil7_m24": lambda: synth.stencil7(24),
    "grid7_wrap_y": lambda: synth.grid7(64, 12, 16, wrap_y=True),
    # ragged rows, empty rows, rows far longer than the rest (in every rank's share: their groups go to the CSR row blocks)
    "random_rows": lambda: synth.random_rows(8000, 12, seed=3, empty_frac=0.1, long_rows={100: 3000, 2500: 2000, 4100: 5000, 6000: 900}),
    # ragged rows whose columns span < 4096: the run window fits its 4096 slots but not the three-trip product's 2048, the
    # distinct columns do -- the list-driven window (with the shared facts of a large matrix)
    "random_rows_n3000": lambda: synth.random_rows(3000, 12, seed=11, empty_frac=0.05),
    "rows_300": lambda: synth.banded(300, 3),          # last group partly filled
    # equal rows, 19 offsets 400 columns apart: 19 x 256 columns per group exceed the 4096-slot window -- window=1 takes the
    # jagged layout for the window's sake, finds that it does not fit, and selects the groups again for padded slices
    "offsets19_x400": lambda: synth.from_offsets(30000, [400 * k for k in range(-9, 10)], diag_base=20.0),
    "ragged_n400": lambda: _fixture("ragged_n400"),
    "band_n700_b5": lambda: _fixture("band_n700_b5"),
}
SWITCHES = [{}, {"layout": "pad"}, {"layout": "jag"}, {"window": 0}, {"window": 1}, {"window_list": 0}, {"col16": 0}, {"uniform": 0},
            {"constant": 0}, {"masked": 0}]
RANKS = [(1, 0), (2, 1), (4, 1)]            # (ranks, this rank)
_built = {}


def _blocks(name, nranks, rank):
    """-> (HostBlocks of the rank, rows of the matrix, diag non-zeros of ALL ranks: what bicg_create's first collective gives)"""
    key = (name, nranks, rank)
    if key not in _built:
        if name not in _built:
            _built[name] = MATRICES[name]()
        A = _built[name]
        if nranks == 1:
            _built[key] = (H.single_rank_blocks(A), A.rows, A.nnz)
        else:
            parts = [synth.split_blocks(A, nranks, r) for r in range(nranks)]
            diag, offd, counts, displs = parts[rank]
            _built[key] = (H.HostBlocks(diag, offd, A.rows, counts, displs), A.rows, sum(int(p[0].nnz) for p in parts))
    return _built[key]


def _switch_id(sw):
    return ",".join(f"{k}={v}" for k, v in sw.items()) or "default"


def case_ids():
    for name in MATRICES:
        for nranks, rank in RANKS:
            for sw in SWITCHES:
                for big in (False, True):
                    yield f"{name}/P{nranks}r{rank}/{_switch_id(sw)}/{'inflated' if big else 'true'}"


def plan_of(case):
    """run bicg_sell_plan_digest for one case id -> {"summary": [...], "digest": [hex, ...]}"""
    name, pr, swid, facts = case.split("/")
    nranks, rank = (int(v) for v in pr[1:].split("r"))
    sw = next(s for s in SWITCHES if _switch_id(s) == swid)
    blk, rows, nnz = _blocks(name, nranks, rank)
    if facts == "inflated":
        # the same block as a share of a larger matrix of the same shape: more than 6 M diag non-zeros per rank (the plan's
        # "large ranks" branches), the same mean row length (rows and non-zeros grow by the same factor)
        f = -(-6500000 * nranks // max(nnz, 1))
        rows, nnz = rows * f, nnz * f
    saved = os.environ.get("BICG_PLAN")
    try:
        os.environ.pop("BICG_PLAN", None)
        H.switches(**sw)
        summary, digest = H.sell_plan_digest(blk, nranks, rows, nnz)
    finally:
        os.environ.pop("BICG_PLAN", None)
        if saved is not None:
            os.environ["BICG_PLAN"] = saved
    return {"summary": [summary[k] for k in H.SELL_SUMMARY], "digest": ["%016x" % digest[k] for k in H.SELL_ARRAYS]}


def _golden():
    g = json.load(open(GOLDEN))
    assert g["summary_fields"] == list(H.SELL_SUMMARY) and g["digest_arrays"] == list(H.SELL_ARRAYS)
    return g


@pytest.mark.parametrize("name", list(MATRICES))
def test_the_plan_is_the_parents_byte_for_byte(name):
    g = _golden()
    mine = [c for c in case_ids() if c.startswith(name + "/")]
    assert len(mine) == len(RANKS) * len(SWITCHES) * 2
    for case in mine:
        want = g["plans"][g["cases"][case]]
        got = plan_of(case)
        assert got["summary"] == want["summary"], (case, dict(zip(H.SELL_SUMMARY, zip(got["summary"], want["summary"]))))
        differ = [a for a, x, y in zip(H.SELL_ARRAYS, got["digest"], want["digest"]) if x != y]
        assert not differ, (case, differ)


def test_the_cases_reach_every_branch_of_the_plan():
    """on the recorded (parent's) summaries: every layout, window form and slice kind occurs, a group selection was retried,
    row blocks stand beside sliced-ELL groups, and halo-touching groups and row blocks exist"""
    g = _golden()
    assert set(g["cases"]) == set(case_ids())
    S = [dict(zip(H.SELL_SUMMARY, g["plans"][i]["summary"])) for i in g["cases"].values()]
    E = "%016x" % 0xcbf29ce484222325          # digest of no bytes
    D = [dict(zip(H.SELL_ARRAYS, g["plans"][i]["digest"])) for i in g["cases"].values()]
    some = lambda f: any(f(s) for s in S)
    assert some(lambda s: not s["jag"] and s["c16"] and s["clusters"] > 0), "padded, 16-bit offsets, clusters"
    assert some(lambda s: not s["jag"] and not s["c16"] and s["sell_entries"] > 0), "padded, 32-bit columns"
    assert some(lambda s: s["jag"] and s["window"] == 1), "jagged with run windows"
    assert some(lambda s: s["jag"] and s["window"] == 2), "jagged with the list-driven window"
    assert some(lambda s: s["jag"] and s["window"] == 0 and s["sell_entries"] > 0 and s["lane_info"]), "jagged without window"
    assert some(lambda s: s["retried"] and not s["jag"] and s["sell_entries"] > 0), "a retried group selection"
    assert some(lambda s: s["rowsplit"] and s["csr16"] and s["nblk"] > 0), "rows over lanes with 16-bit offsets"
    assert some(lambda s: s["nblk"] > 0 and s["sell_entries"] > 0), "row blocks beside sliced-ELL groups"
    assert some(lambda s: s["uniform_entries"] > 0 and s["constant_entries"] == 0), "uniform slices that are not constant"
    assert some(lambda s: s["constant_entries"] > 0 and s["masked_rows"] > 0), "constant and masked slices"
    assert some(lambda s: s["ng_bnd"] > 0) and some(lambda s: s["n_bnd"] > 0), "halo-touching groups / row blocks"
    assert any(d["perm"] != E for d in D) and any(d["list"] != E for d in D) and any(d["dcol16"] != E for d in D)


def test_the_plan_does_not_depend_on_the_number_of_threads():
    """digests equal for 1, 3 and 16 plan threads (csrc/bicg_parallel.h), on a padded, a windowed, a list-driven and a mixed block"""
    L = H.lib()
    L.bicg_set_plan_threads.argtypes = [C.c_int]; L.bicg_set_plan_threads.restype = C.c_int
    g = _golden()
    cases = ["transport_like/P1r0/default/true", "fem_like/P2r1/default/true", "random_rows_n3000/P1r0/default/inflated",
             "random_rows/P4r1/default/true", "stencil7_m24/P1r0/default/true", "banded_b512/P1r0/default/true"]
    try:
        for nt in (1, 3, 16):
            assert L.bicg_set_plan_threads(nt) == nt
            for case in cases:
                assert plan_of(case) == g["plans"][g["cases"][case]], (nt, case)
    finally:
        L.bicg_set_plan_threads(-1)


if __name__ == "__main__":
    # python tests/test_sell_plan.py --write FILE PARENT_HASH   (with BICG_HIP_LIB = a library of the parent commit whose
    # bicg_sell_plan_digest hashes bicg_create's locals: see this file's head)
    assert sys.argv[1] == "--write"
    plans, index, cases = [], {}, {}
    for case in case_ids():
        p = plan_of(case)
        key = json.dumps(p)
        if key not in index:
            index[key] = len(plans)
            plans.append(p)
        cases[case] = index[key]
    with open(sys.argv[2], "w") as f:
        json.dump({"parent": sys.argv[3], "hash": "64-bit FNV-1a over the array's bytes", "summary_fields": list(H.SELL_SUMMARY),
                   "digest_arrays": list(H.SELL_ARRAYS), "plans": plans, "cases": cases}, f, separators=(",", ":"))
    print(len(cases), "cases,", len(plans), "distinct plans")
