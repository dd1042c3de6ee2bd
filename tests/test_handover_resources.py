"""The compiler's resource report of the last build (mpi-bicgstab_amd/build/kernel_resources.txt) for the hand-over kernels
(DESIGN.md section 4.3 (c)). The hand-over exists because the producer-side finish -- ticket chain, tail finish, two workgroup
sums and the phases of every solver inlined behind the product -- left the dot-carrying sliced-ELL products of plain BiCGStab
with scratch; a product whose epilogue ends at the shard totals must be free of it, or the change has lost its reason.
Register counts of this build are on record in profiles/NOTES.md; they are not pinned here."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "mpi-bicgstab_amd", "build", "kernel_resources.txt")
RED_HAND = 3      # enum RedMode, csrc/bicg_device.h


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(REPORT):
        pytest.skip("no resource report (library not built here)")
    out, cur = {}, None
    for line in open(REPORT):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+):\s*(\d+)", line)
        if m and cur:
            out[cur][m.group(1).strip()] = int(m.group(2))
    return out


def test_hand_over_products_are_lean(kernels):
    """k_spmv_sell<NDOT, OFFD = false, NT, LAY, LL = false, RED_HAND>: no scratch, no spilled register of either kind, eight
    wavefronts per SIMD -- every such instantiation the build has, and both streaming policies of the three dot counts"""
    ks = [k for k in kernels if re.search(r"k_spmv_sellILi[0-3]ELb0ELb[01]ELi[0-7]ELb0ELi%dEEEv" % RED_HAND, k)]
    assert len(ks) >= 6, sorted(kernels)[:5]
    for k in ks:
        r = kernels[k]
        assert r["ScratchSize [bytes/lane]"] == 0 and r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, (k, r)
        assert r["Occupancy [waves/SIMD]"] == 8, (k, r)


def test_hand_over_consumers_keep_their_occupancy(kernels):
    """FPlainXR / FPlainQ / FPlainP with the consumer prologue (private scalar block, shard totals, recurrence): no scratch, and
    at least the wavefronts per SIMD of the ticket-mode instantiations they replace -- 7 / 8 / 8"""
    want = {r"8FPlainXRILb[01]EE": 7, "7FPlainQ": 8, "7FPlainP": 8}
    for name, occ in want.items():
        hand = [k for k in kernels if re.search(r"k_vecINS_%sELi%dELi0EEEv" % (name, RED_HAND), k)]
        ticket = [k for k in kernels if re.search(r"k_vecINS_%sELi0ELi0EEEv" % name, k)]
        assert hand and len(hand) == len(ticket), (name, hand, ticket)
        for k in hand:
            r = kernels[k]
            assert r["ScratchSize [bytes/lane]"] == 0, (k, r)
            assert r["Occupancy [waves/SIMD]"] >= max(occ, max(kernels[t]["Occupancy [waves/SIMD]"] for t in ticket)), (k, r)
