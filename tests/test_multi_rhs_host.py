"""Multi-RHS BiCGStab without a GPU: the two entry points are exported with the documented signatures, and the compiler's resource
report of the last build (mpi-bicgstab_amd/build/kernel_resources.txt) shows the unit's kernels (csrc/bicg_multi.hip, prefix
k_multi_) free of scratch and of spilled registers -- they are streaming kernels with at most five input streams per tile; scratch
in one of them would be traffic of its own. Register counts and occupancy of this build are on record in profiles/NOTES.md; they are
not pinned here."""
import ctypes as C
import os
import re

import pytest

from mpi_bicgstab_amd import hipsolver as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "mpi-bicgstab_amd", "build", "kernel_resources.txt")
_dp = C.POINTER(C.c_double)


def test_entry_points_are_exported_and_declared():
    L = H.lib()
    assert hasattr(L, "bicg_solve_multi") and hasattr(L, "bicg_multi_trace")
    assert {"bicg_solve_multi", "bicg_multi_trace"} <= set(H.EXPORTS)
    assert L.bicg_solve_multi.argtypes == [C.c_void_p, C.c_int, _dp, _dp, C.c_int, C.POINTER(H.Options), C.POINTER(H.Result)]
    assert L.bicg_solve_multi.restype is C.c_int
    assert L.bicg_multi_trace.argtypes == [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]
    assert callable(H.Context.solve_multi) and callable(H.Context.multi_trace)
    hdr = open(os.path.join(ROOT, "include", "bicgstab_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int bicg_solve_multi(bicg_ctx *ctx, int method, double *x_loc_set, double *r_loc_set, int nrhs, "
            "const bicg_options *opt, bicg_result *res );") in flat
    assert "int bicg_multi_trace(bicg_ctx *ctx, int column, double *alpha, double *omega, double *beta, double *dot_r);" in flat
    assert "-1" in hdr and "-2" in hdr          # both refusal codes are documented


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


def test_multi_kernels_have_no_scratch_and_no_spills(kernels):
    ks = [k for k in kernels if "k_multi_" in k]
    assert len(ks) >= 3, sorted(kernels)[:5]
    for k in ks:
        r = kernels[k]
        assert r["ScratchSize [bytes/lane]"] == 0 and r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, (k, r)
