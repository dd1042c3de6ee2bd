"""The launch plan of the distributed product (spmv_plan, csrc/bicg_spmv_plan.cpp), pinned launch by launch on the CPU.

bicg_spmv_launch_plan turns a context's shape and one call's facts -- a handful of integers -- into the launches the product
consists of: kernel family, list, entries, offd / fused flags, first partial slot, before or after the halo has landed; and into
what they share: groups per workgroup, the partial slots the dot group expects, whether its tail finish stays.

The expected values in tests/golden/spmv_launch_plans.json were NOT produced by the code under test. They come from the commit
named in the file's "parent" entry, where all of this was interleaved with the enqueueing in spmv() (csrc/bicg_solver.cpp). That
function's text, unedited (with stencil_product and the three grid functions sell_grid / spmv_grid / stencil_grid it calls), was
compiled in a scratch harness outside the repository against the parent's headers and against stubs of everything it enqueues:
every launch_* stub declines as the real wrapper does (nlist == 0, except a launch with the exchange inside that has values to
push; the plane-marching launch with an epilogue and a per-wavefront group) and otherwise RECORDS family, list (by the pointer it
was handed), nlist, with_offd, fused_halo, red.slot_base, red.expected, whether red.tail_seq survived, groups_per_wg, and
whether the halo had landed by then (launch_halo_unpack was enqueued, or the "halo-touching rows" section mark was set; a hosted
product without that mark runs every launch behind one in-order exchange). die() recorded its message. It was fed a
default-constructed bicg_ctx with the case's integers filled in -- two ranks and a P2p / a stream-ordered stub transport for the
peer-to-peer / two-stream cases, a StencilDev whose own grid is the case's `stencil_wgs` -- and a Reduce with a tail tag, the
per-wavefront flag, or (every group that is not per-wavefront) the hand-over flag, so that bicg_ctx::Hand::nsh and Group::nparts
could be read back afterwards (-1: left untouched). `python tests/test_spmv_plan.py --cases` prints the lines that harness reads,
`--write FILE PARENT_HASH < its output` makes the golden file. So a passing test says: moving the decisions into spmv_plan changed
no launch, no slot and no count.

What the comparison cannot reach, because the parent kept these values in the arguments of its launches only: a case without a
launch compares its steps (none), hand_nsh and nparts, but the plan's `expected`, `tail` and `groups_per_wg` with nothing (there
`expected` is seen only through nparts, when the group is per-wavefront); a case that ends in an error compares the message alone.

The case list is only good if it reaches every branch; test_the_cases_reach_every_branch_of_the_plan checks that on the
recorded launches. Where the parent's result looks odd (DESIGN.md section 5.1 lists what was found), the golden decides."""
import json
import os
import sys

import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mpi_bicgstab_amd import hipsolver as H

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "spmv_launch_plans.json")
LAUNCH_FIELDS = ["family", "list", "nlist", "with_offd", "fused_halo", "slot_base", "expected", "tail", "groups_per_wg", "after_halo"]
# the three messages the parent's spmv() ended the program with, by the plan's error code
ERRORS = {1: "CA-BiCGStab's fused q / y epilogue without the plane-marching product",
          2: "SpMV epilogue on a multi-launch SpMV",
          3: "the plane-marching product declined a launch its plan had selected (lines per wavefront / reduction mode)"}
SINGLE, P2P, HOSTED = 0, 1, 2
K_SHARDS, WAVES_PER_WG = 32, 4


def S(**kw):
    """a shape: 2 groups per workgroup without dots, 4 with"""
    return dict({"sell_gpw": 2, "sell_gpw_dots": 4}, **kw)


ALL_SELL = dict(glist_all=1, nblk=0)
MIXED = dict(ng_int=6, ng_bnd=4, n_int=3, n_bnd=2, nblk=5)
# id -> (shape, call). sell_grid(n, per) for the sizes used: (10, 2) = 5, (10, 4) = 3, (6, 2) = 3, (4, 2) = 2, (6, 4) = 2, (4, 4) = 1,
# (40, 4) = 10, (128, 4) = 32.
CASES = {
    # ---- one rank
    "single/sell": (S(ng_int=10, **ALL_SELL), {}),
    "single/sell/dot1/tail-one-launch": (S(ng_int=10, **ALL_SELL), dict(ndot=1, tail=1)),
    "single/sell/dot2/wave": (S(ng_int=10, **ALL_SELL), dict(ndot=2, wave=1)),
    "single/sell/shift": (S(ng_int=10, **ALL_SELL), dict(has_shift=1)),
    "single/sell+csr": (S(ng_int=10, n_int=7, nblk=7), {}),
    "single/csr-only": (S(n_int=7, nblk=7), dict(ndot=1, tail=1)),
    # the tail finish: expected below / at / above kShards = 32, one launch and several
    "single/tail/below/two-launches": (S(ng_int=10, n_int=7, nblk=7), dict(ndot=1, tail=1)),            # 3 + 7: last 7 < 10
    "single/tail/at/one-launch": (S(ng_int=128, **ALL_SELL), dict(ndot=1, tail=1)),                     # 32
    "single/tail/at/two-launches": (S(ng_int=40, n_int=22, nblk=22), dict(ndot=1, tail=1)),             # 10 + 22: last 22 < 32
    "single/tail/above/last-has-32": (S(ng_int=40, n_int=32, nblk=32), dict(ndot=1, tail=1)),           # 10 + 32: kept
    "single/tail/above/last-has-31": (S(ng_int=40, n_int=31, nblk=31), dict(ndot=1, tail=1)),           # 10 + 31: dropped
    "single/tail/above/one-launch": (S(ng_int=200, **ALL_SELL), dict(ndot=2, tail=1)),                  # 50
    "single/stencil": (S(ng_int=12, stencil_ok=1, stencil_wgs=24, **ALL_SELL), {}),
    "single/stencil/dot1/tail": (S(ng_int=12, stencil_ok=1, stencil_wgs=24, **ALL_SELL), dict(ndot=1, tail=1)),
    "single/stencil/dot2/wave": (S(ng_int=12, stencil_ok=1, stencil_wgs=24, **ALL_SELL), dict(ndot=2, wave=1)),
    "single/stencil/shift": (S(ng_int=12, stencil_ok=1, stencil_wgs=24, **ALL_SELL), dict(has_shift=1)),
    "single/epi1": (S(ng_int=10, **ALL_SELL), dict(epi=1, wave=1)),
    "single/epi2": (S(ng_int=10, **ALL_SELL), dict(epi=2, wave=1)),
    "single/epi1/stencil-available": (S(ng_int=12, stencil_ok=1, stencil_wgs=24, **ALL_SELL), dict(epi=1, wave=1)),
    "single/epi3/stencil": (S(ng_int=12, stencil_ok=1, stencil_wgs=24, **ALL_SELL), dict(epi=3, tail=1)),
    "single/epi3/stencil/tickets": (S(ng_int=12, stencil_ok=1, stencil_wgs=24, **ALL_SELL), dict(epi=3)),
    # the epilogue cap: more than 8192 groups, or more than a small wg_cap
    "single/epi1/8192-groups": (S(ng_int=8192, sell_gpw=1, **ALL_SELL), dict(epi=1, wave=1)),
    "single/epi1/8193-groups": (S(ng_int=8193, sell_gpw=1, **ALL_SELL), dict(epi=1, wave=1)),
    "single/epi2/8193-groups/not-wave": (S(ng_int=8193, sell_gpw=1, **ALL_SELL), dict(epi=2)),
    "single/epi2/wg-cap-20/20-groups": (S(ng_int=20, wg_cap=20, **ALL_SELL), dict(epi=2, wave=1)),
    "single/epi2/wg-cap-20/50-groups": (S(ng_int=50, wg_cap=20, **ALL_SELL), dict(epi=2, wave=1)),
    "single/epi1/halo-touching-groups": (S(ng_int=6, ng_bnd=4, **ALL_SELL), dict(epi=1, wave=1)),
    "single/halo-touching-counts": (S(glist_all=1, **MIXED), dict(ndot=1, tail=1)),
    "single/nothing": (S(**ALL_SELL), dict(ndot=1, wave=1)),
    # ---- hosted transports
    "hosted/merged": (S(transport=HOSTED, ng_int=6, ng_bnd=4, **ALL_SELL), {}),
    "hosted/merged/three-launches": (S(transport=HOSTED, glist_all=1, **MIXED), dict(ndot=1, tail=1)),
    "hosted/merged/three-launches/last-has-32": (S(transport=HOSTED, glist_all=1, ng_int=6, ng_bnd=4, n_int=3, n_bnd=32, nblk=35), dict(ndot=2, tail=1)),
    "hosted/merged/dot2/wave": (S(transport=HOSTED, ng_int=6, ng_bnd=4, **ALL_SELL), dict(ndot=2, wave=1)),
    "hosted/in-order/row-blocks": (S(transport=HOSTED, **MIXED), dict(ndot=1)),
    "hosted/two-streams": (S(transport=HOSTED, own_stream=1, glist_all=1, **MIXED), dict(ndot=1, tail=1)),
    "hosted/two-streams/all-sell": (S(transport=HOSTED, own_stream=1, ng_int=6, ng_bnd=4, **ALL_SELL), {}),
    "hosted/two-streams/all-sell/last-has-32": (S(transport=HOSTED, own_stream=1, ng_int=6, ng_bnd=128, **ALL_SELL), dict(ndot=1, tail=1)),
    "hosted/two-streams/stencil": (S(transport=HOSTED, own_stream=1, ng_int=6, ng_bnd=4, stencil_ok=1, stencil_wgs=9, **ALL_SELL), dict(ndot=1, wave=1)),
    "hosted/in-order/stencil": (S(transport=HOSTED, ng_int=6, ng_bnd=4, stencil_ok=1, stencil_wgs=9, **ALL_SELL), {}),
    "hosted/two-streams/stencil/shift": (S(transport=HOSTED, own_stream=1, ng_int=6, ng_bnd=4, stencil_ok=1, stencil_wgs=9, **ALL_SELL), dict(has_shift=1)),
    "hosted/two-streams/no-halo-rows": (S(transport=HOSTED, own_stream=1, ng_int=6, **ALL_SELL), dict(ndot=1, tail=1)),
    "hosted/nothing": (S(transport=HOSTED, **ALL_SELL), dict(ndot=2, wave=1)),
    "hosted/two-streams/nothing": (S(transport=HOSTED, own_stream=1, **ALL_SELL), {}),
    # ---- peer-to-peer
    "p2p/fused": (S(transport=P2P, ll_fused=1, has_send=1, ng_int=6, ng_bnd=4, **ALL_SELL), {}),
    "p2p/fused/dot1/wave": (S(transport=P2P, ll_fused=1, has_send=1, ng_int=6, ng_bnd=4, **ALL_SELL), dict(ndot=1, wave=1)),
    "p2p/fused/dot2": (S(transport=P2P, ll_fused=1, has_send=1, ng_int=6, ng_bnd=4, **ALL_SELL), dict(ndot=2)),
    "p2p/fused/row-blocks": (S(transport=P2P, ll_fused=1, has_send=1, ng_int=6, ng_bnd=4, n_int=3, nblk=3), dict(ndot=1)),
    "p2p/fused/epi1": (S(transport=P2P, ll_fused=1, has_send=1, ng_int=6, ng_bnd=4, **ALL_SELL), dict(epi=1, wave=1)),
    "p2p/fused/epi2": (S(transport=P2P, ll_fused=1, has_send=1, ng_int=6, ng_bnd=4, **ALL_SELL), dict(epi=2, wave=1)),
    "p2p/fused/only-pushes": (S(transport=P2P, ll_fused=1, has_send=1, **ALL_SELL), {}),
    "p2p/fused/nothing": (S(transport=P2P, ll_fused=1, **ALL_SELL), dict(ndot=1, wave=1)),
    "p2p/fused/stencil-available": (S(transport=P2P, ll_fused=1, has_send=1, ng_int=6, ng_bnd=4, stencil_ok=1, stencil_wgs=9, **ALL_SELL), dict(ndot=1, wave=1)),
    "p2p/separate": (S(transport=P2P, has_send=1, **MIXED), dict(ndot=1, wave=1)),
    "p2p/separate/all-sell": (S(transport=P2P, has_send=1, ng_int=6, ng_bnd=4, **ALL_SELL), {}),
    "p2p/separate/nothing": (S(transport=P2P, **ALL_SELL), {}),
    # ranks sharing a GPU: room beside the other ranks' launches (wg_cap - 64, at least 16), and the epilogue cap at wg_cap
    "p2p/fused/wg-cap-100": (S(transport=P2P, ll_fused=1, has_send=1, ng_int=150, ng_bnd=50, wg_cap=100, **ALL_SELL), dict(ndot=1, wave=1)),
    "p2p/fused/wg-cap-50": (S(transport=P2P, ll_fused=1, has_send=1, ng_int=150, ng_bnd=50, wg_cap=50, **ALL_SELL), {}),
    "p2p/fused/wg-cap-100/few-groups": (S(transport=P2P, ll_fused=1, has_send=1, ng_int=6, ng_bnd=4, wg_cap=100, **ALL_SELL), {}),
    "p2p/fused/epi1/wg-cap-100": (S(transport=P2P, ll_fused=1, has_send=1, ng_int=100, ng_bnd=50, wg_cap=100, **ALL_SELL), dict(epi=1, wave=1)),
    "p2p/separate/wg-cap-100": (S(transport=P2P, has_send=1, ng_int=150, ng_bnd=50, wg_cap=100, **ALL_SELL), {}),
    # ---- the three errors
    "error/epi3/no-stencil": (S(ng_int=10, **ALL_SELL), dict(epi=3)),
    "error/epi3/hosted": (S(transport=HOSTED, own_stream=1, ng_int=6, ng_bnd=4, stencil_ok=1, stencil_wgs=9, **ALL_SELL), dict(epi=3)),
    "error/epi3/shift": (S(ng_int=12, stencil_ok=1, stencil_wgs=24, **ALL_SELL), dict(epi=3, has_shift=1)),
    "error/epi1/row-blocks": (S(ng_int=10, n_int=7, nblk=7), dict(epi=1, wave=1)),
    "error/epi1/hosted": (S(transport=HOSTED, ng_int=6, ng_bnd=4, **ALL_SELL), dict(epi=1, wave=1)),
    "error/epi2/p2p-separate": (S(transport=P2P, has_send=1, ng_int=6, ng_bnd=4, **ALL_SELL), dict(epi=2, wave=1)),
    "error/epi3/stencil/wave": (S(ng_int=12, stencil_ok=1, stencil_wgs=24, **ALL_SELL), dict(epi=3, wave=1)),
}


def _golden():
    g = json.load(open(GOLDEN))
    assert g["launch_fields"] == LAUNCH_FIELDS and g["shape_fields"] == list(H.SPMV_SHAPE) and g["call_fields"] == list(H.SPMV_CALL)
    return g


def _line(case):
    shape, call = CASES[case]
    return [int(shape.get(k, 0)) for k in H.SPMV_SHAPE] + [int(call.get(k, 0)) for k in H.SPMV_CALL]


@pytest.mark.parametrize("case", list(CASES))
def test_the_plan_is_the_parents_launch_for_launch(case):
    g = _golden()
    want = g["cases"][case]
    assert want["input"] == _line(case), "the golden was recorded for another table"
    shape, call = CASES[case]
    plan, steps = H.spmv_launch_plan(shape, call)
    if want["error"] is not None:
        assert ERRORS.get(plan["error"]) == want["error"]
        return
    assert plan["error"] == 0
    launches = [dict(zip(LAUNCH_FIELDS, l)) for l in want["launches"]]
    step_fields = [f for f in LAUNCH_FIELDS if f in H.SPMV_STEP]
    assert [[s[f] for f in step_fields] for s in steps] == [[l[f] for f in step_fields] for l in launches]
    for l in launches:      # what every launch of the product was handed
        assert (l["expected"], l["tail"], l["groups_per_wg"]) == (plan["expected"], plan["tail"], plan["groups_per_wg"]), l
    if want["hand_nsh"] >= 0:
        assert plan["hand_nsh"] == want["hand_nsh"]
    assert plan["sets_nparts"] == (want["nparts"] >= 0)
    if plan["sets_nparts"]:
        assert plan["expected"] * WAVES_PER_WG == want["nparts"]
    if launches:
        assert plan["stencil"] == any(l["family"] == H.SPMV_FAMILIES.index("stencil") for l in launches)
        assert plan["fused"] == any(l["fused_halo"] for l in launches)
        if shape.get("transport", 0) == HOSTED:
            assert plan["merged"] == any(l["list"] == H.SPMV_LISTS.index("all") and l["with_offd"] for l in launches)


def test_the_cases_reach_every_branch_of_the_plan():
    """on the recorded (parent's) launches: every family on every transport it can run on, every list, one to four launches and
    none, both group counts per workgroup and both raised ones, the tail finish kept and dropped on either side of kShards, the
    three errors"""
    g = _golden()
    assert set(g["cases"]) == set(CASES)
    fam, lst = H.SPMV_FAMILIES.index, H.SPMV_LISTS.index
    R = {}
    for case, want in g["cases"].items():
        shape, call = CASES[case]
        full = dict({k: 0 for k in H.SPMV_SHAPE + H.SPMV_CALL}, **shape, **call)
        R[case] = (full, [dict(zip(LAUNCH_FIELDS, l)) for l in want["launches"]], want)
    ok = {c: r for c, r in R.items() if r[2]["error"] is None}

    def some(f):
        return any(f(s, L, w) for s, L, w in ok.values())

    fams = lambda L: [l["family"] for l in L]
    assert some(lambda s, L, w: s["transport"] == SINGLE and fams(L) == [fam("sell")]), "one sliced-ELL launch"
    assert some(lambda s, L, w: s["transport"] == SINGLE and fams(L) == [fam("sell"), fam("csr")]), "sliced-ELL + row blocks"
    assert some(lambda s, L, w: s["transport"] == SINGLE and fams(L) == [fam("stencil")] and s["epi"] == 0), "stencil"
    for epi in (1, 2):
        assert some(lambda s, L, w: s["transport"] == SINGLE and s["epi"] == epi and fams(L) == [fam("sell_epi")]), f"epi {epi}"
    assert some(lambda s, L, w: s["epi"] == 3 and fams(L) == [fam("stencil")]), "epi 3"
    assert some(lambda s, L, w: s["stencil_ok"] and s["has_shift"] and fam("stencil") not in fams(L) and L), "a shifted product leaves the stencil"
    assert some(lambda s, L, w: s["transport"] == HOSTED and [l["list"] for l in L] == [lst("all"), lst("blk_int"), lst("blk_bnd")]
                and all(l["after_halo"] for l in L)), "hosted, merged: three launches"
    assert some(lambda s, L, w: s["transport"] == HOSTED and s["own_stream"] and [l["list"] for l in L] == [lst("int"), lst("blk_int"), lst("bnd"), lst("blk_bnd")]
                and [l["after_halo"] for l in L] == [0, 0, 1, 1]), "hosted, two streams: four launches"
    assert some(lambda s, L, w: s["transport"] == HOSTED and s["own_stream"] and fams(L) == [fam("stencil"), fam("sell")]), "hosted, two streams, stencil"
    assert some(lambda s, L, w: s["transport"] == HOSTED and not s["own_stream"] and len(L) == 4), "hosted, in order, not merged"
    assert some(lambda s, L, w: s["transport"] == P2P and L and L[0]["fused_halo"] and L[0]["list"] == lst("fused") and L[0]["family"] == fam("sell")), "p2p fused"
    assert some(lambda s, L, w: s["transport"] == P2P and L and L[0]["fused_halo"] and L[0]["family"] == fam("sell_epi")), "p2p fused with epilogue"
    assert some(lambda s, L, w: s["transport"] == P2P and L and L[0]["fused_halo"] and L[0]["nlist"] == 0), "p2p fused: pushes only"
    assert some(lambda s, L, w: s["transport"] == P2P and len(L) == 2 and L[0]["fused_halo"] and L[1]["family"] == fam("csr")), "p2p fused + row blocks"
    assert some(lambda s, L, w: s["transport"] == P2P and not s["ll_fused"] and [l["after_halo"] for l in L] == [0, 0, 1, 1]), "p2p separate"
    assert some(lambda s, L, w: s["transport"] == P2P and s["ll_fused"] and fams(L) == [fam("stencil"), fam("sell")]), "p2p: the stencil is never fused"
    for t in (SINGLE, P2P, HOSTED):
        assert some(lambda s, L, w: s["transport"] == t and not L), "a rank without work"
    for ndot in (0, 1, 2):
        assert some(lambda s, L, w: s["ndot"] == ndot and L and L[0]["groups_per_wg"] == (s["sell_gpw_dots"] if ndot else s["sell_gpw"])), f"ndot {ndot}"
    gpw0 = lambda s: s["sell_gpw_dots"] if s["ndot"] else s["sell_gpw"]
    assert some(lambda s, L, w: s["wg_cap"] > 80 and s["ll_fused"] and not s["epi"] and L and L[0]["groups_per_wg"] > gpw0(s)), "room bump, wg_cap - 64"
    assert some(lambda s, L, w: 0 < s["wg_cap"] <= 80 and s["ll_fused"] and L and L[0]["groups_per_wg"] > gpw0(s)), "room bump, 16"
    assert some(lambda s, L, w: s["wg_cap"] and s["ll_fused"] and L and L[0]["groups_per_wg"] == gpw0(s)), "room enough"
    assert some(lambda s, L, w: s["wg_cap"] and s["transport"] == P2P and not s["ll_fused"] and L and L[0]["groups_per_wg"] == gpw0(s)), "no bump unless fused"
    ng = lambda s: s["ng_int"] + s["ng_bnd"]
    assert some(lambda s, L, w: s["epi"] and not s["wg_cap"] and ng(s) == 8193 and L[0]["groups_per_wg"] > gpw0(s)), "epilogue cap at 8192"
    assert some(lambda s, L, w: s["epi"] and not s["wg_cap"] and ng(s) == 8192 and L[0]["groups_per_wg"] == gpw0(s)), "... not reached"
    assert some(lambda s, L, w: s["epi"] and s["wg_cap"] and s["transport"] == SINGLE and ng(s) > s["wg_cap"] and L[0]["groups_per_wg"] > gpw0(s)), "epilogue cap at wg_cap"
    assert some(lambda s, L, w: s["epi"] and s["wg_cap"] and ng(s) == s["wg_cap"] and L[0]["groups_per_wg"] == gpw0(s)), "... not reached"
    assert some(lambda s, L, w: s["epi"] and not s["wave"] and ng(s) > 8192 and w["nparts"] >= 0), "the cap sets the partial count of any group"
    # the tail finish
    tails = [(s, L) for s, L, w in ok.values() if s["tail"] and L]
    assert tails and all(len({l["tail"] for l in L}) == 1 for s, L in tails)
    kept = lambda L: L[0]["tail"] == 1
    need = lambda L: min(L[0]["expected"], K_SHARDS)
    assert any(len(L) == 1 and kept(L) and L[0]["expected"] < K_SHARDS for s, L in tails)
    assert any(len(L) == 1 and kept(L) and L[0]["expected"] == K_SHARDS for s, L in tails)
    assert any(len(L) == 1 and kept(L) and L[0]["expected"] > K_SHARDS for s, L in tails)
    assert any(len(L) > 1 and not kept(L) and L[0]["expected"] < K_SHARDS for s, L in tails)
    assert any(len(L) > 1 and not kept(L) and L[0]["expected"] == K_SHARDS for s, L in tails)
    assert any(len(L) > 1 and kept(L) and L[0]["expected"] > K_SHARDS and L[0]["expected"] - L[-1]["slot_base"] == need(L) for s, L in tails), "kept at exactly 32"
    assert any(len(L) > 1 and not kept(L) and L[0]["expected"] > K_SHARDS and L[0]["expected"] - L[-1]["slot_base"] == need(L) - 1 for s, L in tails), "dropped at 31"
    for t in (SINGLE, HOSTED):
        assert any(s["transport"] == t and len(L) > 1 and kept(L) for s, L in tails) and any(s["transport"] == t and len(L) > 1 and not kept(L) for s, L in tails)
    assert not any(s["tail"] and not s["wave"] and w["hand_nsh"] != min(L[0]["expected"], K_SHARDS) for s, L, w in ok.values() if L and not s["epi"])
    assert {w["error"] for s, L, w in R.values() if w["error"] is not None} == set(ERRORS.values())
    for msg in ERRORS.values():
        assert sum(w["error"] == msg for s, L, w in R.values()) >= 1


def test_the_binding_refuses_what_is_not_a_shape():
    with pytest.raises(KeyError):
        H.spmv_launch_plan({"ng": 3}, {})
    with pytest.raises(RuntimeError):
        H.spmv_launch_plan({"transport": 3}, {})
    assert "bicg_spmv_launch_plan" in H.EXPORTS


if __name__ == "__main__":
    # python tests/test_spmv_plan.py --cases                          the harness's input, one line per case of the table
    # python tests/test_spmv_plan.py --write FILE PARENT_HASH < OUT   OUT: the harness's output, one JSON object per line
    # (the harness: this file's head)
    if sys.argv[1] == "--cases":
        for case in CASES:
            print(*_line(case))
    else:
        assert sys.argv[1] == "--write"
        cases = {}
        for case, rec in zip(CASES, sys.stdin):
            rec = json.loads(rec)
            assert rec.pop("stencil_product") == CASES[case][0].get("stencil_ok", 0), (case, "stencil_ok is not what stencil_product() says of this shape")
            cases[case] = dict(input=_line(case), **rec)
        assert len(cases) == len(CASES)
        head = {"parent": sys.argv[3], "shape_fields": list(H.SPMV_SHAPE), "call_fields": list(H.SPMV_CALL), "launch_fields": LAUNCH_FIELDS}
        dumps = lambda v: json.dumps(v, separators=(",", ":"))
        with open(sys.argv[2], "w") as f:      # one case per line
            f.write("{" + ",\n".join(f"{dumps(k)}:{dumps(v)}" for k, v in head.items()) + ",\n\"cases\":{\n")
            f.write(",\n".join(f"{dumps(k)}:{dumps(v)}" for k, v in cases.items()) + "\n}}\n")
        print(len(cases), "cases")
