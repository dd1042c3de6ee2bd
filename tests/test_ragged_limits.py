"""The crafted matrices of tests/ragged_cases.py sit where they say: for every case the host-only sliced-ELL plan
(hipsolver.sell_plan_digest, csrc/bicg_sell_plan.cpp) of the REAL matrix reports the facts its generator promises -- window kind,
win_slots, win_max_runs, lane_info, c16, win_near16, jag_tail16_max, no CSR row blocks -- and the one-past-the-limit neighbours take
the documented fallback. A generator that drifted off its limit fails here, on the CPU, instead of passing quietly on the GPU
(tests/test_ragged_limits_gpu.py runs exactly these matrices)."""
import os

import pytest

import ragged_cases as R
from mpi_bicgstab_amd import hipsolver as H


def plan(A, sw, rows_global=None, nnz_global=None):
    """the summary of the plan of the one-rank block A under the BICG_PLAN switches sw alone"""
    os.environ.pop("BICG_PLAN", None)          # (tests/conftest.py puts the variable back after the test)
    H.switches(**sw)
    summary, _ = H.sell_plan_digest(H.single_rank_blocks(A), 1, rows_global, nnz_global)
    return summary


def check(A, facts, summary):
    assert {k: summary[k] for k in R.FACT_KEYS} == {k: facts[k] for k in R.FACT_KEYS}
    # jagged slices hold every row and nothing else
    assert summary["jag"] == 1 and summary["rowsplit"] == 0 and summary["retried"] == 0
    assert summary["sell_rows"] == A.rows and summary["sell_nnz"] == summary["sell_entries"] == A.nnz


@pytest.mark.parametrize("name", list(R.SMALL))
def test_small_case_plans_as_promised(name):
    A, facts, sw = R.build(name)
    assert A.nnz < R.LIST_MIN_NNZ
    check(A, facts, plan(A, sw))


@pytest.fixture(scope="module")
def large():
    A, facts, sw = R.build("list_limits")
    return A, facts, plan(A, sw)


def test_large_case_takes_the_list_driven_window_with_real_facts(large):
    A, facts, summary = large
    assert A.nnz >= R.LIST_MIN_NNZ and A.rows % R.GROUP
    assert (facts["window"], facts["win_slots"]) == (2, R.MAX_SLOTS)
    check(A, facts, summary)


def test_limits_as_the_generators_state_them():
    """what the cases promise, spelled out once: both sides of every limit are among them"""
    f = {name: R.build(name)[1] for name in R.SMALL}
    assert [f[f"runs{k}"]["win_max_runs"] for k in (63, 64)] == [63, 64] and f["runs65"]["window"] == 0 and f["runs65"]["kernel"] == "jagd"
    assert [f[f"slots{w}"]["win_slots"] for w in (2040, 2048)] == [2040, 2048] and f["slots2049"]["window"] == 0
    assert (f["longrow255"]["lane_info"], f["longrow256"]["lane_info"]) == (1, 0) and f["longrow256"]["kernel"] == "sell_window_loop"
    assert (f["far32_near"]["c16"], f["far32"]["c16"]) == (1, 0) and f["far32"]["kernel"] == f["far32_near"]["kernel"] == "jagd"
    assert (f["jpipe960"]["jag_tail16_max"], f["jpipe961"]["jag_tail16_max"]) == (960, 961)
    assert f["jpipe960"]["win_slots"] == f["jpipe961"]["win_slots"] == 2047 and f["jpipe960_slots2048"]["win_slots"] == 2048
    assert f["lengths_jagw"]["kernel"] == "jagw" and f["lengths_jagd"]["kernel"] == "jagd"
    assert sorted(f[f"tail{t}"]["slices_of_last_group"] for t in (1, 64, 65, 128, 129, 192, 193, 255)) == [1, 1, 2, 2, 3, 3, 4, 4]


@pytest.mark.parametrize("neighbour", [None] + list(R.LIST_NEIGHBOURS))
def test_one_past_a_list_limit_falls_to_gathers_with_32_bit_columns(neighbour):
    """90 000-row versions of the large case, planned as a share of a matrix of more than 6 M non-zeros (inflated facts, as in
    tests/test_sell_plan.py): as crafted the list-driven window; with 2049 distinct columns in one group, or a distance of -32769
    or +32768, no window and 32-bit columns"""
    A, facts = R.list_limits(90000, neighbour)
    f = -(-6500000 // A.nnz)
    summary = plan(A, {}, A.rows * f, A.nnz * f)
    check(A, facts, summary)
    assert (summary["window"], summary["c16"]) == ((2, 1) if neighbour is None else (0, 0))
    if neighbour is None:      # ... and with its real facts such a small block has no list: the far groups cost it the window
        small = plan(A, {})
        assert (small["window"], small["c16"], small["lane_info"]) == (0, 0, 1)
