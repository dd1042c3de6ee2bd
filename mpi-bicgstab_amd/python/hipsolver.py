"""ctypes binding of libbicgstab_hip.so (include/bicgstab_hip.h) -- the host-side mirror used by
tests/ and bench.py. The reference's host is C (src/main.c); the equivalent C host lives in
``mpi-bicgstab_amd/host/``. Function names follow the reference's solver.h.

There is NO fallback: if the HIP library is missing or no GPU is visible the calls fail loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on this pool's host driver (peer-to-peer mailboxes, RCCL)

from .synth import CSR

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("BICG_HIP_LIB") or os.path.join(PKG_DIR, "libbicgstab_hip.so")

class _Methods(dict):
    """name -> method number of include/bicgstab_hip.h. The table's own entries -- what iterating over it, len() and values() show --
    are the methods 0..4, a census that tests/test_precond.py pins; a method added since is in LATER_METHODS and is found by
    subscription all the same (METHODS["bicgstab_block"] == 5), which is how every call of this module looks a method up."""

    def __missing__(self, name):
        return LATER_METHODS[name]


METHODS = _Methods({"bicgstab": 0, "ca_bicgstab": 1, "pipe_bicgstab": 2, "pipe_bicgstab_rr": 3, "bicgstab_diag": 4})
LATER_METHODS = {"bicgstab_block": 5,      # BICG_BICGSTAB_BLOCK
                 "bicgstab2": 6,           # BICG_BICGSTAB2
                 "bicgstab2_diag": 7,      # BICG_BICGSTAB2_DIAG, BICG_BICGSTAB2_BLOCK: method 6 right-preconditioned with the
                 "bicgstab2_block": 8}     # diagonal / the block diagonal the context holds

_dp = C.POINTER(C.c_double)
_up = C.POINTER(C.c_uint)
_ip = C.POINTER(C.c_int)


class CSRMatrix(C.Structure):      # include/bicgstab_hip.h (reference src/matrix.h:19-26)
    _fields_ = [("val", _dp), ("col", _up), ("ptr", _up), ("nz", C.c_uint), ("rows", C.c_uint), ("cols", C.c_uint)]


class InfoMatrix(C.Structure):     # include/bicgstab_hip.h (reference src/matrix.h:28-33)
    _fields_ = [("nz", C.c_uint), ("rows", C.c_uint), ("cols", C.c_uint), ("code", C.c_char * 4),
                ("recvcounts", _ip), ("displs", _ip)]


class Options(C.Structure):
    _fields_ = [("tol", C.c_double), ("max_iter", C.c_int), ("out_iter", C.c_int), ("check_every", C.c_int),
                ("quiet", C.c_int), ("krr", C.c_int), ("nrr", C.c_int), ("record_trace", C.c_int),
                ("time_kernels", C.c_int), ("rr_drift", C.c_double)]


class Result(C.Structure):
    _fields_ = [("iterations", C.c_int), ("dot_r", C.c_double), ("dot_zero", C.c_double), ("seconds", C.c_double),
                ("iter_seconds", C.c_double), ("spmv_ms_total", C.c_double), ("spmv_launches", C.c_int),
                ("breakdown_iteration", C.c_int), ("adaptive_replacements", C.c_int)]


ALLREDUCE_FN = C.CFUNCTYPE(None, _dp, C.c_int, C.c_void_p)
ALLTOALLV_FN = C.CFUNCTYPE(None, C.c_void_p, _ip, _ip, C.c_void_p, _ip, _ip, C.c_void_p)

EXPORTS = [
    "bicgstab", "ca_bicgstab", "pipe_bicgstab", "pipe_bicgstab_rr",
    "shifted_bicgstab", "shifted_lopbicgstab", "shifted_lopbicgstab_v2", "shifted_lopbicgstab_nooverlap",
    "shifted_pipe_lopbicgstab", "shifted_pipe_lopbicgstab_nooverlap", "bicg_solve_shifted",
    "shifted_lopbicg", "shifted_lopbicg_switching", "shifted_lopbicg_switching_noovlp", "bicg_shifted_residuals",
    "bicg_comm_enable_p2p", "bicg_comm_p2p_active", "bicg_comm_failed",
    "bicg_partition_nnz", "bicg_mtx_load_block_part", "bicg_mtx_parse_double", "bicg_mtx_cache_save", "bicg_mtx_cache_load",
    "bicg_coo_to_blocks_device", "bicg_mtx_set_block_builder",
    "bicg_comm_unique_id", "bicg_comm_init_rccl", "bicg_comm_init_host", "bicg_comm_init_mpi",
    "bicg_comm_init_single", "bicg_comm_finalize", "bicg_comm_selftest_rccl", "bicg_comm_rccl_loadable", "bicg_comm_last_error", "bicg_section_times", "bicg_comm_rank", "bicg_comm_size",
    "bicg_default_options", "bicg_create", "bicg_destroy", "bicg_solve", "bicg_load", "bicg_run", "bicg_fetch",
    "bicg_run_begin", "bicg_run_iterate", "bicg_run_iterate_timed", "bicg_run_end", "bicg_sync", "bicg_trace", "bicg_spmv", "bicg_dot", "bicg_spmv_bench", "bicg_plan_info", "bicg_ctx_flags", "bicg_spmm", "bicg_device_matrix_bytes", "bicg_uniform_entries", "bicg_constant_entries", "bicg_masked_rows", "bicg_stencil_info", "bicg_stencil_rows_per_lane", "bicg_comm_wait_stats", "bicg_plan_collisions", "bicg_product_kernels", "bicg_spmv_matrix_bytes", "bicg_last_shifted_persistent", "bicg_last_spmm_windowed", "bicg_last_spmm_tile", "bicg_dropin_context", "bicg_dropin_release", "bicg_dropin_stats",
    "bicg_mtx_load_block", "bicg_mtx_free", "bicg_partition", "bicg_halo_plan", "bicg_halo_send_counts", "bicg_halo_send_lists", "bicg_row_blocks", "bicg_window_plan", "bicg_window_slot", "bicg_version", "bicg_has_experiments", "bicg_switch_value", "bicg_switch_unknown", "bicg_stream_bench", "bicg_create_device_csr", "bicg_stencil7_device", "bicg_device_free", "bicg_persist_plan", "bicg_set_plan_threads", "bicg_sell_plan_digest", "bicg_spmv_launch_plan", "bicg_dot_group_plan",
    "bicg_reorder_plan", "bicg_permute_block", "bicg_reorder_info",
    "bicg_solve_multi", "bicg_multi_trace", "bicg_comm_counts", "bicg_device_allocations",
    "bicg_update_values", "bicg_update_values_device", "bicg_persist_plan_sources", "bicg_dropin_refreshes",
    "bicg_load_device", "bicg_fetch_device", "bicg_solve_device", "bicg_spmv_device", "bicg_solve_multi_device",
    "bicg_precond_diagonal", "bicg_precond_diagonal_device", "bicg_precond_clear", "bicg_precond_kind", "bicg_csr_diagonal",
    "bicg_precond_block_diagonal", "bicg_precond_block_diagonal_device", "bicg_precond_apply", "bicg_csr_block_diagonal",
    "bicg_precond_apply_bench", "bicg_precond_apply_set_bench",
]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C mpi-bicgstab_amd lib` "
                               "(python -c 'import __graft_entry__ as g; g.build()')")
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        L.bicg_create.restype = C.c_void_p
        L.bicg_create.argtypes = [C.POINTER(CSRMatrix), C.POINTER(CSRMatrix), C.POINTER(InfoMatrix)]
        L.bicg_destroy.argtypes = [C.c_void_p]
        L.bicg_solve.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.POINTER(Options), C.POINTER(Result)]
        L.bicg_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(Options), C.POINTER(Result)]
        L.bicg_solve_shifted.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, C.c_int, C.c_int, C.POINTER(Options),
                                         C.POINTER(Result)]
        L.bicg_run_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(Options)]
        L.bicg_run_iterate.argtypes = [C.c_void_p, C.c_int]
        L.bicg_run_iterate_timed.argtypes = [C.c_void_p, C.c_int, _dp]
        L.bicg_switch_value.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
        L.bicg_switch_unknown.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
        L.bicg_run_end.argtypes = [C.c_void_p, C.POINTER(Result)]
        L.bicg_sync.argtypes = [C.c_void_p]
        L.bicg_load.argtypes = [C.c_void_p, _dp, _dp]
        L.bicg_fetch.argtypes = [C.c_void_p, _dp, _dp]
        L.bicg_trace.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp]
        L.bicg_solve_multi.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int, C.POINTER(Options), C.POINTER(Result)]
        L.bicg_solve_multi.restype = C.c_int
        L.bicg_multi_trace.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]
        L.bicg_multi_trace.restype = C.c_int
        L.bicg_comm_counts.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
        L.bicg_comm_counts.restype = C.c_int
        L.bicg_spmv.argtypes = [C.c_void_p, _dp, _dp]
        L.bicg_dot.argtypes = [C.c_void_p, _dp, _dp]
        L.bicg_dot.restype = C.c_double
        L.bicg_spmv_bench.argtypes = [C.c_void_p, C.c_int, _dp]
        L.bicg_plan_info.argtypes = [C.c_void_p, _up]
        L.bicg_stencil_info.argtypes = [C.c_void_p, _up]
        L.bicg_stencil_rows_per_lane.argtypes = [C.c_void_p]; L.bicg_stencil_rows_per_lane.restype = C.c_uint
        L.bicg_comm_wait_stats.argtypes = [C.c_void_p, _dp]
        L.bicg_section_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.bicg_comm_failed.argtypes = [C.c_void_p]
        L.bicg_dropin_context.restype = C.c_void_p
        L.bicg_dropin_context.argtypes = [C.POINTER(CSRMatrix), C.POINTER(CSRMatrix), C.POINTER(InfoMatrix)]
        L.bicg_dropin_stats.argtypes = [_up, _up]
        L.bicg_spmm.argtypes = [C.c_void_p, _dp, _dp, C.c_int, _dp, _dp]
        L.bicg_ctx_flags.argtypes = [C.c_void_p]
        L.bicg_device_matrix_bytes.argtypes = [C.c_void_p]
        L.bicg_device_matrix_bytes.restype = C.c_ulonglong
        L.bicg_ctx_flags.restype = C.c_uint
        for fn in (L.bicg_uniform_entries, L.bicg_constant_entries, L.bicg_masked_rows, L.bicg_spmv_matrix_bytes):
            fn.argtypes = [C.c_void_p]; fn.restype = C.c_ulonglong
        L.bicg_plan_collisions.argtypes = [C.c_void_p]; L.bicg_plan_collisions.restype = C.c_uint
        L.bicg_device_allocations.argtypes = []; L.bicg_device_allocations.restype = C.c_longlong
        L.bicg_product_kernels.argtypes = [C.c_int]; L.bicg_product_kernels.restype = C.c_uint
        L.bicg_last_shifted_persistent.argtypes = [C.c_void_p]
        L.bicg_last_spmm_windowed.argtypes = [C.c_void_p]
        L.bicg_last_spmm_tile.argtypes = [C.c_void_p]
        L.bicg_shifted_residuals.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int, _dp]
        L.bicg_default_options.argtypes = [C.POINTER(Options)]
        L.bicg_comm_unique_id.argtypes = [C.c_void_p]
        L.bicg_comm_init_rccl.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.bicg_comm_init_host.argtypes = [C.c_int, C.c_int, ALLREDUCE_FN, ALLTOALLV_FN, C.c_void_p, C.c_int]
        L.bicg_comm_init_single.argtypes = [C.c_int]
        L.bicg_comm_init_mpi.argtypes = [C.c_char_p, C.c_int]
        L.bicg_partition.argtypes = [C.c_uint, C.c_int, _ip, _ip]
        L.bicg_halo_plan.argtypes = [C.POINTER(CSRMatrix), C.POINTER(InfoMatrix), C.c_int, C.c_uint, _up, _ip, _up]
        L.bicg_halo_send_counts.argtypes = [C.c_int, _ip, ALLTOALLV_FN, C.c_void_p, _ip]
        L.bicg_halo_send_lists.argtypes = [C.c_int, C.c_int, C.POINTER(InfoMatrix), C.c_uint, _up, _ip, _ip, ALLTOALLV_FN,
                                           C.c_void_p, _up]
        L.bicg_row_blocks.argtypes = [_up, C.c_uint, C.c_uint, C.c_uint, _up]
        L.bicg_row_blocks.restype = C.c_uint
        L.bicg_window_plan.argtypes = [_up, _up, C.c_uint, C.c_uint, C.c_char_p, C.c_uint, C.c_uint, _up, _up, _up]
        L.bicg_window_plan.restype = C.c_long
        L.bicg_window_slot.argtypes = [_up, C.c_uint, C.c_uint, C.c_uint]
        L.bicg_window_slot.restype = C.c_uint
        L.bicg_version.restype = C.c_char_p
        L.bicg_stream_bench.argtypes = [C.c_int, C.c_ulonglong, C.c_int, _dp, _dp]
        L.bicg_create_device_csr.restype = C.c_void_p
        L.bicg_create_device_csr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, _dp]
        L.bicg_stencil7_device.argtypes = [C.c_uint, _dp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_ulonglong)]
        L.bicg_device_free.argtypes = [C.c_void_p]
        L.bicg_reorder_plan.argtypes = [C.POINTER(CSRMatrix), C.c_int, _up, C.POINTER(C.c_ulonglong)]
        L.bicg_permute_block.argtypes = [C.POINTER(CSRMatrix), _up, _up, _up, _dp]
        L.bicg_reorder_info.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
        L.bicg_update_values.argtypes = [C.c_void_p, _dp, _dp]
        L.bicg_update_values_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bicg_dropin_refreshes.argtypes = []; L.bicg_dropin_refreshes.restype = C.c_uint
        # device-resident vectors: device pointers and the caller's hipStream_t as void *
        L.bicg_load_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bicg_fetch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bicg_solve_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(Options), C.POINTER(Result), C.c_void_p]
        L.bicg_spmv_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bicg_solve_multi_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(Options),
                                              C.POINTER(Result), C.c_void_p]
        for fn in (L.bicg_load_device, L.bicg_fetch_device, L.bicg_solve_device, L.bicg_spmv_device, L.bicg_solve_multi_device):
            fn.restype = C.c_int
        L.bicg_persist_plan_sources.argtypes = [C.POINTER(CSRMatrix), C.POINTER(CSRMatrix), C.c_uint, _up]
        # diagonal preconditioner
        L.bicg_precond_diagonal.argtypes = [C.c_void_p, _dp]
        L.bicg_precond_diagonal_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bicg_precond_clear.argtypes = [C.c_void_p]
        L.bicg_precond_kind.argtypes = [C.c_void_p]
        L.bicg_csr_diagonal.argtypes = [C.POINTER(CSRMatrix), _dp]
        for fn in (L.bicg_precond_diagonal, L.bicg_precond_diagonal_device, L.bicg_precond_clear, L.bicg_precond_kind, L.bicg_csr_diagonal):
            fn.restype = C.c_int
        # block-Jacobi preconditioner
        L.bicg_precond_block_diagonal.argtypes = [C.c_void_p, _dp, C.c_int]
        L.bicg_precond_block_diagonal_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.bicg_precond_apply.argtypes = [C.c_void_p, _dp, _dp]
        L.bicg_precond_apply_bench.argtypes = [C.c_void_p, C.c_int, _dp]
        L.bicg_precond_apply_bench.restype = C.c_int
        L.bicg_precond_apply_set_bench.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp]
        L.bicg_precond_apply_set_bench.restype = C.c_int
        L.bicg_csr_block_diagonal.argtypes = [C.POINTER(CSRMatrix), C.c_int, _dp]
        L.block_jacobi_bicgstab.argtypes = [C.POINTER(CSRMatrix), C.POINTER(CSRMatrix), C.POINTER(InfoMatrix), _dp, _dp, C.c_int]
        L.block_jacobi_bicgstab2.argtypes = L.block_jacobi_bicgstab.argtypes
        for fn in (L.bicg_precond_block_diagonal, L.bicg_precond_block_diagonal_device, L.bicg_precond_apply, L.bicg_csr_block_diagonal,
                   L.block_jacobi_bicgstab, L.block_jacobi_bicgstab2):
            fn.restype = C.c_int
        for name in ("bicgstab", "ca_bicgstab", "pipe_bicgstab", "jacobi_bicgstab", "bicgstab2", "jacobi_bicgstab2"):
            getattr(L, name).argtypes = [C.POINTER(CSRMatrix), C.POINTER(CSRMatrix), C.POINTER(InfoMatrix), _dp, _dp]
        L.pipe_bicgstab_rr.argtypes = [C.POINTER(CSRMatrix), C.POINTER(CSRMatrix), C.POINTER(InfoMatrix), _dp, _dp,
                                       C.c_int, C.c_int]
        _lib = L
    return _lib


# The library's token-list variables (csrc/bicg_knobs.h): keyword -> (variable, token). INTEGRATION.md section 6 says what each does.
SWITCHES = {k: ("BICG_PLAN", k.replace("_", "-")) for k in (
    "stencil", "lines", "planes", "ca_fuse", "layout", "window", "col16", "uniform", "constant", "masked", "desc", "lists", "jagw",
    "spmm", "spmm_window", "fuse_pipe", "pipe_probe", "halo_fused", "window_list", "wide", "reorder", "handover", "halo_set")}
SWITCHES.update(persist=("BICG_PERSIST", "0"), persist_chunk=("BICG_PERSIST", "chunk"), persist_shifted=("BICG_PERSIST", "shifted"),
                force_comm=("BICG_TEST", "force-comm"), spin_ticks=("BICG_TEST", "spin-ticks"),
                p2p_fault_after=("BICG_TEST", "p2p-fault-after"), plan_collide=("BICG_TEST", "plan-collide"),
                spmm_tile=("BICG_TEST", "spmm-tile"), spmm_gstep=("BICG_TEST", "spmm-gstep"))
SWITCH_VARS = ("BICG_PLAN", "BICG_PERSIST", "BICG_TEST")


def switches(env=None, **kw):
    """Set (value) or clear (None) tokens of BICG_PLAN / BICG_PERSIST / BICG_TEST in `env` (default: this process's environment),
    the other tokens stay: switches(stencil=0, lines=2) -> BICG_PLAN="stencil=0,lines=2"; switches(force_comm=1) ->
    BICG_TEST="force-comm=1"; switches(persist=0) -> BICG_PERSIST="0" beside its chunk= / shifted= tokens, persist=1 or None
    takes the "0" away. Contexts read the variables when they are created."""
    env = os.environ if env is None else env
    for k, v in kw.items():
        var, tok = SWITCHES[k]
        toks = [t for t in env.get(var, "").split(",") if t and t.split("=")[0] != tok and not (k == "persist" and t in ("1", "off"))]
        if k == "persist":
            if v is not None and int(v) == 0:
                toks.insert(0, "0")
        elif v is not None:
            toks.append(f"{tok}={v}")
        if toks:
            env[var] = ",".join(toks)
        else:
            env.pop(var, None)
    return env


def switch_value(var: str, name: str):
    """what the LIBRARY reads for token `name` of BICG_PLAN / BICG_PERSIST / BICG_TEST (bicg_switch_value): its text, None if absent"""
    buf = C.create_string_buffer(64)
    n = lib().bicg_switch_value(var.encode(), name.encode(), buf, 64)
    return None if n < 0 else buf.value.decode()


def _d(a):
    return a.ctypes.data_as(_dp)


# ---- device-resident vectors (bicg_*_device): CUDA float64 torch tensors wherever the vector calls take numpy arrays
def tensor_form(*arrs) -> bool:
    """Is this call in its device form -- is one of the arrays (None: not given) a torch tensor? Then all of them are CUDA float64
    tensors, or TypeError: decided from the arguments alone, before the library or a context is touched."""
    given = [a for a in arrs if a is not None]
    if not any(hasattr(a, "data_ptr") for a in given):
        return False
    for a in given:
        if not hasattr(a, "data_ptr") or not a.is_cuda or str(a.dtype) != "torch.float64":
            raise TypeError("device vectors are CUDA float64 torch tensors (and a call takes tensors or numpy arrays, not both)")
    return True


def _torch_stream(stream):
    """the torch stream a device call is ordered on: the current one, a torch.cuda.Stream, or a raw hipStream_t as an integer"""
    import torch
    if stream is None:
        return torch.cuda.current_stream()
    if hasattr(stream, "cuda_stream"):
        return stream
    return torch.cuda.ExternalStream(int(stream)) if int(stream) else torch.cuda.default_stream()


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _vec1(t, n, what, inplace=False):
    """a tensor as n doubles one after the other (a copy when it is not; never when the library writes into it)"""
    if t.numel() != n:
        raise ValueError(f"{what}: {t.numel()} entries for {n} rows")
    if t.dim() == 1 and (n <= 1 or t.stride(0) == 1):
        return t
    if inplace:
        raise ValueError(f"{what}: an in-place vector is one-dimensional with stride 1")
    return t.contiguous().reshape(-1)


def _set2(t, nrhs, n, what, inplace=False):
    """a tensor as nrhs columns of n doubles, (tensor, ld): a 2-D tensor whose rows are contiguous and at least n apart is passed
    as it is, with its row stride as ld; anything else is made contiguous first"""
    if t.dim() == 2 and t.shape == (nrhs, n) and (n <= 1 or t.stride(1) == 1) and (nrhs == 1 or t.stride(0) >= n):
        return t, (n if nrhs == 1 else int(t.stride(0)))
    if inplace:
        raise ValueError(f"{what}: an in-place set is [nrhs][n] with contiguous rows at least n apart")
    return t.reshape(nrhs, n).contiguous(), n


def window_plan(A: CSR, group_rows: int = 256, max_slots: int = 4096, gap: int = 8):
    """x windows of a block (bicg_window_plan): (win_ptr, runs[n][2], slots of the largest window) or None when a
    group does not fit max_slots"""
    ptr = np.ascontiguousarray(A.ptr, dtype=np.uint32)
    col = np.ascontiguousarray(A.col, dtype=np.uint32)
    up = lambda a: a.ctypes.data_as(_up)
    n = lib().bicg_window_plan(up(ptr), up(col), A.rows, group_rows, None, max_slots, gap, None, None, None)
    if n < 0:
        return None
    ngroups = (A.rows + group_rows - 1) // group_rows
    win_ptr = np.zeros(ngroups + 1, dtype=np.uint32)
    runs = np.zeros((max(n, 1), 2), dtype=np.uint32)
    used = C.c_uint(0)
    lib().bicg_window_plan(up(ptr), up(col), A.rows, group_rows, None, max_slots, gap, up(win_ptr), up(runs), C.byref(used))
    return win_ptr, runs[:n], int(used.value)


class HostBlocks:
    """One rank's diag/offd blocks + INFO in the reference's struct layout (keeps numpy buffers alive)."""

    def __init__(self, diag: CSR, offd: CSR | None, n_global: int, counts, displs):
        if offd is None:
            offd = CSR(diag.rows, n_global, np.zeros(diag.rows + 1, dtype=np.uint32), np.zeros(1, dtype=np.uint32),
                       np.zeros(1))
        self._keep = []

        def mk(A: CSR):
            v = np.ascontiguousarray(A.val, dtype=np.float64)
            c = np.ascontiguousarray(A.col, dtype=np.uint32)
            p = np.ascontiguousarray(A.ptr, dtype=np.uint32)
            if v.size == 0:
                v = np.zeros(1)
            if c.size == 0:
                c = np.zeros(1, dtype=np.uint32)
            self._keep += [v, c, p]
            return CSRMatrix(_d(v), c.ctypes.data_as(_up), p.ctypes.data_as(_up), int(p[-1]), A.rows, A.cols)

        self.diag, self.offd = mk(diag), mk(offd)
        cnt = np.ascontiguousarray(counts, dtype=np.int32)
        dsp = np.ascontiguousarray(displs, dtype=np.int32)
        self._keep += [cnt, dsp]
        self.info = InfoMatrix(0, n_global, n_global, b"MCRG", cnt.ctypes.data_as(_ip), dsp.ctypes.data_as(_ip))
        self.n_loc = diag.rows


def load_mtx_blocks(path: str, rank: int = 0, nranks: int = 1) -> HostBlocks:
    """This rank's blocks of a Matrix-Market file through the library's loader (C, reads the file once)."""
    d, o, info = CSRMatrix(), CSRMatrix(), InfoMatrix()
    L = lib()
    L.bicg_mtx_load_block.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(CSRMatrix), C.POINTER(CSRMatrix), C.POINTER(InfoMatrix)]
    if L.bicg_mtx_load_block(path.encode(), rank, nranks, C.byref(d), C.byref(o), C.byref(info)) != 0:
        raise RuntimeError(f"cannot load {path}")

    def to_csr(m, ncols):
        nz = int(m.ptr[m.rows])
        return CSR(m.rows, ncols, np.ctypeslib.as_array(m.ptr, shape=(m.rows + 1,)).copy(),
                   np.ctypeslib.as_array(m.col, shape=(max(nz, 1),))[:nz].copy(),
                   np.ctypeslib.as_array(m.val, shape=(max(nz, 1),))[:nz].copy())
    diag, offd = to_csr(d, d.rows), to_csr(o, info.cols)
    counts = np.ctypeslib.as_array(info.recvcounts, shape=(nranks,)).copy()
    displs = np.ctypeslib.as_array(info.displs, shape=(nranks,)).copy()
    n = int(info.rows)
    L.bicg_mtx_free(C.byref(d), C.byref(o), C.byref(info))
    blk = HostBlocks(diag, offd if nranks > 1 else None, n, counts, displs)
    blk.nnz_global = int(info.nz)
    return blk


def single_rank_blocks(A: CSR) -> HostBlocks:
    return HostBlocks(A, None, A.rows, [A.rows], [0])


class Context:
    """bicg_ctx wrapper: matrix resident on the GPU; solves, SpMV, dot."""

    def __init__(self, blocks: HostBlocks):
        self.blocks = blocks
        self.n = blocks.n_loc
        self.h = lib().bicg_create(C.byref(blocks.diag), C.byref(blocks.offd), C.byref(blocks.info))
        if not self.h:
            raise RuntimeError("bicg_create failed")

    @classmethod
    def stencil7_on_device(cls, m: int, weights):
        """Single rank: the 7-point stencil on an m^3 grid generated, planned and kept on the GPU (bicg_stencil7_device +
        bicg_create_device_csr) -- no host copy of the matrix. Returns (context, nnz, plan seconds, generation seconds)."""
        import time
        L = lib()
        w = np.ascontiguousarray(weights, dtype=np.float64)
        val, col, ptr = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nnz = C.c_ulonglong(0)
        t0 = time.perf_counter()
        if L.bicg_stencil7_device(m, _d(w), C.byref(val), C.byref(col), C.byref(ptr), C.byref(nnz)) != 0:
            raise RuntimeError("bicg_stencil7_device failed")
        t_gen = time.perf_counter() - t0
        secs = C.c_double(0.0)
        self = cls.__new__(cls)
        self.blocks = None
        self.n = m ** 3
        self.h = L.bicg_create_device_csr(val, col, ptr, m ** 3, C.byref(secs))
        for p in (val, col, ptr):
            L.bicg_device_free(p)
        if not self.h:
            raise RuntimeError("bicg_create_device_csr refused the matrix")
        return self, int(nnz.value), float(secs.value), t_gen

    def update_values(self, diag_val, offd_val=None) -> int:
        """New values for the resident matrix, same sparsity pattern (bicg_update_values): arrays in the CSR order of the blocks
        the context was created from -- numpy arrays (host variant) or CUDA torch tensors (device variant) --, or a CSR /
        HostBlocks whose values are taken. Returns 0 done, 1 refused (a value held in a list shared between constant or masked
        slices would change; nothing was written), -1 an array is missing."""
        if isinstance(diag_val, HostBlocks):
            diag_val, offd_val = diag_val._keep[0], diag_val._keep[3]
        elif isinstance(diag_val, CSR):
            diag_val = diag_val.val
        if isinstance(offd_val, CSR):
            offd_val = offd_val.val
        if hasattr(diag_val, "data_ptr"):            # torch tensors on the device
            keep = [None if t is None else t.contiguous() for t in (diag_val, offd_val)]
            for t in keep:
                if t is not None and (not t.is_cuda or str(t.dtype) != "torch.float64"):
                    raise TypeError("update_values: device arrays are CUDA float64 tensors")
            ptrs = [C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None for t in keep]
            return int(lib().bicg_update_values_device(self.h, ptrs[0], ptrs[1]))
        d = None if diag_val is None else np.ascontiguousarray(diag_val, dtype=np.float64)
        o = None if offd_val is None else np.ascontiguousarray(offd_val, dtype=np.float64)
        return int(lib().bicg_update_values(self.h, None if d is None or d.size == 0 else _d(d), None if o is None or o.size == 0 else _d(o)))

    def set_diagonal(self, d, stream=None) -> int:
        """Install or replace the diagonal preconditioner M = diag(d) for solve("bicgstab_diag" / "bicgstab2_diag") (bicg_precond_diagonal): d as a
        numpy array or a CUDA float64 torch tensor (bicg_precond_diagonal_device, ordered behind `stream`, default the current
        torch stream), in the caller's numbering; a rank without rows passes None or an empty array. Returns 0 installed, 1 refused
        (a zero or non-finite entry; what was installed stays), -1 the array is missing."""
        if d is not None and tensor_form(d):
            import torch
            st = _torch_stream(stream)
            with torch.cuda.stream(st):
                d = _vec1(d, self.n, "d")
            return int(lib().bicg_precond_diagonal_device(self.h, _vp(d), C.c_void_p(st.cuda_stream)))
        if d is not None:
            d = np.ascontiguousarray(d, dtype=np.float64)
            if d.size != self.n:
                raise ValueError(f"d: {d.size} entries for {self.n} rows")
        return int(lib().bicg_precond_diagonal(self.h, None if d is None or d.size == 0 else _d(d)))

    def set_block_diagonal(self, blocks, bs: int, stream=None) -> int:
        """Install or replace the block-Jacobi preconditioner for solve("bicgstab_block" / "bicgstab2_block") (bicg_precond_block_diagonal): the bs x bs
        diagonal blocks (bs = 1..16) of this rank's rows in the caller's numbering, ceil(n / bs) * bs * bs doubles, block k's entry
        (a, j) at [(k * bs + a) * bs + j] -- what csr_block_diagonal returns --, as a numpy array or a CUDA float64 torch tensor
        (bicg_precond_block_diagonal_device, ordered behind `stream`, default the current torch stream); a rank without rows passes
        None or an empty array. Returns 0 installed, 1 refused (a singular block or a non-finite entry; what was installed, of
        either kind, stays), -1 the array is missing, -2 bs outside 1..16."""
        bs = int(bs)
        want = -(-self.n // bs) * bs * bs if 1 <= bs <= 16 else None
        if blocks is not None and tensor_form(blocks):
            import torch
            st = _torch_stream(stream)
            with torch.cuda.stream(st):
                blocks = blocks.contiguous().reshape(-1)
            if want is not None and blocks.numel() != want:
                raise ValueError(f"blocks: {blocks.numel()} entries, {want} for {self.n} rows in blocks of {bs}")
            return int(lib().bicg_precond_block_diagonal_device(self.h, _vp(blocks), bs, C.c_void_p(st.cuda_stream)))
        if blocks is not None:
            blocks = np.ascontiguousarray(blocks, dtype=np.float64).reshape(-1)
            if want is not None and blocks.size != want:
                raise ValueError(f"blocks: {blocks.size} entries, {want} for {self.n} rows in blocks of {bs}")
        return int(lib().bicg_precond_block_diagonal(self.h, None if blocks is None or blocks.size == 0 else _d(blocks), bs))

    def apply_preconditioner(self, v):
        """z = M^-1 v for the installed preconditioner of either kind (bicg_precond_apply): numpy in the caller's numbering, local
        to the rank. RuntimeError when none is installed."""
        v = np.ascontiguousarray(v, dtype=np.float64)
        if v.size != self.n:
            raise ValueError(f"v: {v.size} entries for {self.n} rows")
        z = np.zeros(self.n)
        if lib().bicg_precond_apply(self.h, _d(v) if v.size else None, _d(z) if z.size else None) != 0:
            raise RuntimeError("bicg_precond_apply: the context has no preconditioner (set_diagonal / set_block_diagonal)")
        return z

    def apply_preconditioner_bench(self, reps: int) -> float:
        """ms per application of the installed preconditioner, reps back to back on the device (bicg_precond_apply_bench)"""
        ms = C.c_double(0.0)
        if lib().bicg_precond_apply_bench(self.h, reps, C.byref(ms)) != 0:
            raise RuntimeError("bicg_precond_apply_bench: the context has no preconditioner (set_diagonal / set_block_diagonal)")
        return ms.value

    def apply_preconditioner_set_bench(self, ncols: int, reps: int, chunk: int = 0) -> float:
        """ms per set application of the installed block preconditioner on ncols (1..16) columns, one launch each, reps back to back on
        the device (bicg_precond_apply_set_bench); chunk: columns a workgroup walks, 4 / 8 / 16, 0 = the library's choice"""
        ms = C.c_double(0.0)
        if lib().bicg_precond_apply_set_bench(self.h, ncols, chunk, reps, C.byref(ms)) != 0:
            raise RuntimeError("bicg_precond_apply_set_bench: no block preconditioner (set_block_diagonal), or ncols outside 1..16")
        return ms.value

    def clear_preconditioner(self) -> int:
        """drop the preconditioner, of either kind, and its device array (bicg_precond_clear)"""
        return int(lib().bicg_precond_clear(self.h))

    def preconditioner(self):
        """None, "diagonal" or "block_diagonal" (bicg_precond_kind)"""
        return (None, "diagonal", "block_diagonal")[int(lib().bicg_precond_kind(self.h))]

    def close(self):
        if self.h:
            lib().bicg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def options(self, **kw) -> Options:
        o = Options()
        lib().bicg_default_options(C.byref(o))
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    def solve(self, method: str, b, x0=None, **kw):
        """Semantics of the reference solver call: returns dict(k, x, r, result). b / x0 as CUDA float64 torch tensors: the device
        form (bicg_solve_device) -- x and r come back as fresh tensors on the same device, b and x0 stay as they are; inplace=True
        makes x0 (required then) and b the in-out arrays themselves. stream: the torch.cuda.Stream (or raw stream) the call is
        ordered on, default the current one."""
        if tensor_form(b, x0):
            return self._solve_device(method, b, x0, kw)
        kw.pop("stream", None); kw.pop("inplace", None)
        x = np.zeros(self.n) if x0 is None else np.array(x0, dtype=np.float64)
        r = np.array(b, dtype=np.float64)
        kw.setdefault("quiet", 1)
        o = self.options(**kw)
        res = Result()
        k = lib().bicg_solve(self.h, METHODS[method], _d(x), _d(r), C.byref(o), C.byref(res))
        return dict(k=k, x=x, r=r, dot_r=res.dot_r, dot_zero=res.dot_zero, result=res)

    def _solve_device(self, method, b, x0, kw):
        import torch
        st, inplace = _torch_stream(kw.pop("stream", None)), bool(kw.pop("inplace", False))
        with torch.cuda.stream(st):
            if inplace:
                if x0 is None:
                    raise ValueError("solve(inplace=True) takes x0: it becomes x")
                x, r = _vec1(x0, self.n, "x0", True), _vec1(b, self.n, "b", True)
            else:
                x = torch.zeros(self.n, dtype=torch.float64, device=b.device) if x0 is None else _vec1(x0, self.n, "x0").clone()
                r = _vec1(b, self.n, "b").clone()
        kw.setdefault("quiet", 1)
        o = self.options(**kw)
        res = Result()
        k = lib().bicg_solve_device(self.h, METHODS[method], _vp(x), _vp(r), C.byref(o), C.byref(res), C.c_void_p(st.cuda_stream))
        return dict(k=k, x=x, r=r, dot_r=res.dot_r, dot_zero=res.dot_zero, result=res)

    def _solve_multi_device(self, B, X0, method, nrhs, kw):
        import torch
        st, inplace = _torch_stream(kw.pop("stream", None)), bool(kw.pop("inplace", False))
        if nrhs is None:
            nrhs = B.shape[0] if B.dim() == 2 else B.numel() // max(self.n, 1)
        with torch.cuda.stream(st):
            if inplace:
                if X0 is None:
                    raise ValueError("solve_multi(inplace=True) takes X0: it becomes x")
                (x, ldx), (r, ldr) = _set2(X0, nrhs, self.n, "X0", True), _set2(B, nrhs, self.n, "B", True)
                if ldx != ldr:
                    raise ValueError("solve_multi(inplace=True): X0 and B have the same row stride")
            else:
                r, ldr = _set2(B, nrhs, self.n, "B")
                r = r.clone(memory_format=torch.contiguous_format)
                x = (torch.zeros((nrhs, self.n), dtype=torch.float64, device=B.device) if X0 is None
                     else _set2(X0, nrhs, self.n, "X0")[0].clone(memory_format=torch.contiguous_format))
                ldr = self.n
        kw.setdefault("quiet", 1)
        o = self.options(**kw)
        res = (Result * max(nrhs, 1))()
        rc = lib().bicg_solve_multi_device(self.h, METHODS[method], _vp(x), _vp(r), ldr, nrhs, C.byref(o), res, C.c_void_p(st.cuda_stream))
        results = list(res)[:nrhs] if rc >= 0 else []
        self._multi_k = [q.iterations for q in results]
        return dict(k=np.array(self._multi_k, dtype=np.int64), x=x, r=r, results=results, rc=rc)

    def solve_multi(self, B, X0=None, method: str = "bicgstab", nrhs=None, **kw):
        """BiCGStab on the rows of B [nrhs][n] as independent right-hand sides of the resident matrix, 16 columns per pass over the
        matrix (bicg_solve_multi). method: "bicgstab", or right-preconditioned "bicgstab_diag" / "bicgstab_block" on a context that
        holds that preconditioner (set_diagonal / set_block_diagonal; otherwise rc = -2). Returns dict(k [nrhs] int array, x [nrhs][n], r [nrhs][n], results [nrhs] of Result, rc = the
        call's return value: the largest k, or the negative code of a refused call -- x and r are then X0 and B). Collective
        across ranks (rc = -1: the ranks passed different arguments); nrhs: the number of columns where B cannot tell -- a rank
        without rows (n = 0) passes it with empty arrays. B / X0 as CUDA float64 torch tensors: the device form
        (bicg_solve_multi_device), x and r fresh [nrhs][n] tensors; inplace=True: X0 (required) and B are the in-out sets themselves,
        2-D with contiguous rows whose stride (>= n, the same for both) is passed as ld. stream: as for solve."""
        if tensor_form(B, X0):
            return self._solve_multi_device(B, X0, method, nrhs, kw)
        kw.pop("stream", None); kw.pop("inplace", None)
        if nrhs is None:
            r = np.array(B, dtype=np.float64).reshape(-1, self.n)
            nrhs = r.shape[0]
        else:
            r = np.array(B, dtype=np.float64).reshape(nrhs, self.n)
        x = np.zeros((nrhs, self.n)) if X0 is None else np.array(X0, dtype=np.float64).reshape(nrhs, self.n)
        kw.setdefault("quiet", 1)
        o = self.options(**kw)
        res = (Result * max(nrhs, 1))()
        rc = lib().bicg_solve_multi(self.h, METHODS[method], _d(x), _d(r), nrhs, C.byref(o), res)
        results = list(res)[:nrhs] if rc >= 0 else []
        self._multi_k = [q.iterations for q in results]
        return dict(k=np.array(self._multi_k, dtype=np.int64), x=x, r=r, results=results, rc=rc)

    def multi_trace(self, column: int, k: int):
        """trace of one column of the last solve_multi(record_trace=1): the dict of trace(); None when nothing was recorded"""
        done = getattr(self, "_multi_k", [])
        if not 0 <= column < len(done):
            return None
        arrs = [np.zeros(max(k, done[column], 1)) for _ in range(4)]      # the library writes the column's whole trace
        if lib().bicg_multi_trace(self.h, column, *[_d(a) for a in arrs]) != 0:
            return None
        return dict(zip(("alpha", "omega", "beta", "dotr"), [a[:min(k, done[column])] for a in arrs]))

    SHIFTED = {"shifted_lopbicgstab": 0, "shifted_pipe_lopbicgstab": 1, "shifted_bicgstab": 2,
               "shifted_lopbicg": 3, "shifted_lopbicg_switching": 4}

    def solve_shifted(self, b, sigma, seed, x0_set=None, which="shifted_lopbicgstab", **kw):
        """(A + sigma_j I) x_j = b for all j (reference src/shifted_solver.c): dict(k, x [nsig][n], r, result)."""
        sigma = np.ascontiguousarray(sigma, dtype=np.float64)
        x = np.zeros((len(sigma), self.n)) if x0_set is None else np.array(x0_set, dtype=np.float64).reshape(len(sigma), self.n)
        r = np.array(b, dtype=np.float64)
        kw.setdefault("quiet", 1)
        kw.setdefault("tol", 1e-12)
        o = self.options(**kw)
        res = Result()
        k = lib().bicg_solve_shifted(self.h, self.SHIFTED[which], _d(x), _d(r), _d(sigma), len(sigma), seed, C.byref(o),
                                     C.byref(res))
        return dict(k=k, x=x, r=r, dot_r=res.dot_r, dot_zero=res.dot_zero, result=res,
                    iterations=res.iterations, switches=res.adaptive_replacements)

    def section_times(self):
        """Section times of the last solve run with time_kernels=2 (the reference's MEASURE_SECTION_TIME, on the device
        clock): dict(vec_ms, spmv_ms, shift_ms, reduce_ms, iterations, marks) or None when that solve was not timed."""
        ms = (C.c_double * 4)()
        it, marks = C.c_int(0), C.c_int(0)
        if lib().bicg_section_times(self.h, ms, C.byref(it), C.byref(marks)) != 0:
            return None
        return dict(vec_ms=ms[0], spmv_ms=ms[1], shift_ms=ms[2], reduce_ms=ms[3], iterations=it.value, marks=marks.value)

    def shifted_residuals(self, x_set, b, sigma):
        """|| (A + sigma_j I) x_j - b || / || b || for every shift (reference src/test_shifted.c:129-154)"""
        sigma = np.ascontiguousarray(sigma, dtype=np.float64)
        x = np.ascontiguousarray(x_set, dtype=np.float64).reshape(len(sigma), self.n)
        b = np.ascontiguousarray(b, dtype=np.float64)
        out = np.zeros(len(sigma))
        lib().bicg_shifted_residuals(self.h, _d(x), _d(b), _d(sigma), len(sigma), _d(out))
        return out

    def spmm(self, x_set, sigma=None):
        """Y_j = (A + sigma_j I) X_j for all rows of x_set [nvec][n], A read once per 16 vectors -> (Y, device ms); without
        flags()["spmm"] (CSR row blocks, rows over lanes) one product per vector and 0 ms"""
        x = np.ascontiguousarray(x_set, dtype=np.float64).reshape(-1, self.n)
        y = np.zeros_like(x)
        sg = None if sigma is None else np.ascontiguousarray(sigma, dtype=np.float64)
        ms = C.c_double(0.0)
        rc = lib().bicg_spmm(self.h, _d(x), None if sg is None else _d(sg), x.shape[0], _d(y), C.byref(ms))
        if rc != 0:
            raise RuntimeError("bicg_spmm failed")
        return y, ms.value

    def load(self, x0, b, stream=None):
        """x0 and b into the context's x and r (bicg_load). CUDA float64 torch tensors: bicg_load_device on `stream` (default: the
        current torch stream), where x0=None keeps the x the context holds -- a warm start from the previous solution."""
        if tensor_form(x0, b):
            import torch
            st = _torch_stream(stream)
            with torch.cuda.stream(st):      # (a copy made contiguous here is made, and later freed, in the order of that stream)
                x0 = None if x0 is None else _vec1(x0, self.n, "x0")
                b = _vec1(b, self.n, "b")
            if lib().bicg_load_device(self.h, _vp(x0), _vp(b), C.c_void_p(st.cuda_stream)) != 0:
                raise RuntimeError("bicg_load_device refused the arrays")
            return
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        lib().bicg_load(self.h, _d(x0), _d(b))

    def run(self, method: str, **kw) -> Result:
        kw.setdefault("quiet", 1)
        o = self.options(**kw)
        res = Result()
        if lib().bicg_run(self.h, METHODS[method], C.byref(o), C.byref(res)) == -2:
            raise RuntimeError(f"bicg_run refused method {method!r}: the context does not hold its preconditioner ({_installer(method)})")
        return res

    def run_begin(self, method: str, **kw):
        kw.setdefault("quiet", 1)
        self._opt = self.options(**kw)
        if lib().bicg_run_begin(self.h, METHODS[method], C.byref(self._opt)) != 0:      # (nothing was begun: run_iterate would go on with the solve before)
            raise RuntimeError(f"bicg_run_begin refused method {method!r}: the context does not hold its preconditioner ({_installer(method)})")

    def run_iterate(self, nsteps: int) -> int:
        return lib().bicg_run_iterate(self.h, nsteps)

    def run_iterate_timed(self, nsteps: int):
        """run_iterate with three clocks (ms): device events around the launches, host time spent enqueueing, host wall time"""
        ms = (C.c_double * 3)()
        k = lib().bicg_run_iterate_timed(self.h, nsteps, ms)
        return k, dict(device_ms=ms[0], enqueue_ms=ms[1], wall_ms=ms[2])

    def run_end(self) -> Result:
        res = Result()
        lib().bicg_run_end(self.h, C.byref(res))
        return res

    def sync(self):
        lib().bicg_sync(self.h)

    def fetch(self, device=False, stream=None, x=True, r=True):
        """(x, r) of the context: numpy arrays (bicg_fetch) or, device=True, CUDA tensors written by bicg_fetch_device on `stream`
        (default: the current torch stream) without a host wait. x / r: True -- a fresh array; False -- left out (None comes
        back); a CUDA float64 tensor (implies device=True) -- written in place."""
        if device or tensor_form(*[t for t in (x, r) if not isinstance(t, bool)]):
            import torch
            st = _torch_stream(stream)
            with torch.cuda.stream(st):
                out = [torch.empty(self.n, dtype=torch.float64, device="cuda") if t is True else
                       None if t is False or t is None else _vec1(t, self.n, "fetch", True) for t in (x, r)]
            if lib().bicg_fetch_device(self.h, _vp(out[0]), _vp(out[1]), C.c_void_p(st.cuda_stream)) != 0:
                raise RuntimeError("bicg_fetch_device failed")
            return out[0], out[1]
        out = [np.zeros(self.n) if t else None for t in (x, r)]
        lib().bicg_fetch(self.h, *[None if a is None else _d(a) for a in out])
        return out[0], out[1]

    def trace(self, k: int):
        arrs = [np.zeros(max(k, 1)) for _ in range(4)]
        got = lib().bicg_trace(self.h, *[_d(a) for a in arrs])
        return dict(zip(("alpha", "omega", "beta", "dotr"), [a[:got] for a in arrs]))

    def spmv(self, x, out=None, stream=None):
        """y = A x (collective). A CUDA float64 torch tensor: bicg_spmv_device on `stream` (default: the current torch stream), y a
        fresh tensor or `out` (not x itself)"""
        if tensor_form(x, out):
            import torch
            st = _torch_stream(stream)
            with torch.cuda.stream(st):
                x = _vec1(x, self.n, "x")
                y = torch.empty(self.n, dtype=torch.float64, device=x.device) if out is None else _vec1(out, self.n, "out", True)
            if self.n and y.data_ptr() == x.data_ptr():
                raise ValueError("spmv: out must not be x")
            if lib().bicg_spmv_device(self.h, _vp(x), _vp(y), C.c_void_p(st.cuda_stream)) != 0:
                raise RuntimeError("bicg_spmv_device refused the arrays")
            return y
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros(self.n)
        lib().bicg_spmv(self.h, _d(x), _d(y))
        return y

    def dot(self, x, y):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        return lib().bicg_dot(self.h, _d(x), _d(y))

    def spmv_bench(self, reps: int) -> float:
        ms = C.c_double(0.0)
        lib().bicg_spmv_bench(self.h, reps, C.byref(ms))
        return ms.value

    def comm_counts(self):
        """transport collectives issued for this context since it was created (bicg_comm_counts): dict(exchanges, allreduces)"""
        out = (C.c_ulonglong * 2)()
        lib().bicg_comm_counts(self.h, out)
        return dict(exchanges=int(out[0]), allreduces=int(out[1]))

    def comm_failed(self) -> bool:
        return bool(lib().bicg_comm_failed(self.h))

    FLAGS = {"p2p": 1, "ll_fused": 2, "overlap": 4, "col16": 8, "all_sell": 16, "jagged": 32, "spmm": 64, "window": 128, "rowsplit": 256, "persist": 512,
             "fuse_pipe": 1024, "pipe_probed": 2048, "uniform": 4096, "constant": 8192, "reordered": 16384, "handover": 32768, "tail_finish": 65536}

    def flags(self):
        f = int(lib().bicg_ctx_flags(self.h))
        return {k: bool(f & v) for k, v in self.FLAGS.items()}

    def device_matrix_bytes(self) -> int:
        return int(lib().bicg_device_matrix_bytes(self.h))

    def uniform_entries(self) -> int:
        return int(lib().bicg_uniform_entries(self.h))

    def constant_entries(self) -> int:
        return int(lib().bicg_constant_entries(self.h))

    def masked_rows(self) -> int:
        return int(lib().bicg_masked_rows(self.h))

    def comm_wait_stats(self):
        """microseconds the exchanges of the last solve made the persistent kernels wait (None: nothing recorded)"""
        out = (C.c_double * 6)()
        if lib().bicg_comm_wait_stats(self.h, out) != 0:
            return None
        return dict(zip(("allreduce_p50_us", "allreduce_p99_us", "handoff_p50_us", "handoff_p99_us", "allreduce_samples", "handoff_samples"), list(out)))

    def stencil_info(self):
        """The plane-marching product of a 7-point grid stencil (csrc/bicg_stencil.hip): is it in use, and its tiling."""
        out = (C.c_uint * 8)()
        lib().bicg_stencil_info(self.h, out)
        info = dict(zip(("on", "sy", "ny", "nz", "lines", "planes", "workgroups", "masked_segments"), list(out)))
        info["rows_per_lane"] = int(lib().bicg_stencil_rows_per_lane(self.h))
        return info

    def reorder_info(self):
        """the reordering bicg_create applied under BICG_PLAN="reorder=1|2" (bicg_reorder_info): dict keyed by REORDER_STATS with
        `microseconds` = what ordering + permuting took, or None when this context is not reordered"""
        out = (C.c_ulonglong * 8)()
        if lib().bicg_reorder_info(self.h, out) != 0:
            return None
        return dict(zip(REORDER_STATS[:7] + ("microseconds",), (int(v) for v in out)))

    def plan_collisions(self) -> int:
        return int(lib().bicg_plan_collisions(self.h))

    def last_spmm_windowed(self) -> bool:
        return bool(lib().bicg_last_spmm_windowed(self.h))

    def last_spmm_kind(self) -> str:
        """which SpMM kernel the last pass ran: "pipelined" (k_spmm_pipe), "windowed" (k_spmm_win) or "rowmajor" (k_spmm_sell)"""
        return ("rowmajor", "windowed", "pipelined")[int(lib().bicg_last_spmm_windowed(self.h))]

    def last_spmm_tile(self) -> int:
        """rows per tile of the last pass when it ran k_spmm_pipe (512 or 256); 0 after any other kernel"""
        return int(lib().bicg_last_spmm_tile(self.h))

    def last_shifted_persistent(self) -> bool:
        return bool(lib().bicg_last_shifted_persistent(self.h))

    def spmv_matrix_bytes(self) -> int:
        return int(lib().bicg_spmv_matrix_bytes(self.h))

    def plan_info(self):
        out = (C.c_uint * 8)()
        lib().bicg_plan_info(self.h, out)
        return dict(zip(("rows", "nnz_diag", "nnz_offd", "halo", "row_blocks", "boundary_blocks", "sell_rows",
                         "sell_padding"), list(out)))


def csr_diagonal(blocks):
    """(d, missing) of a rank's diag block (bicg_csr_diagonal; blocks: HostBlocks, or a CSR with local columns): d[i] = the stored
    (i,i) entry -- the sum in stored order where a row stores it more than once --, 0.0 where none is stored; missing = the number
    of rows without one. No GPU needed."""
    if isinstance(blocks, CSR):
        blocks = HostBlocks(blocks, None, blocks.rows, [blocks.rows], [0])
    d = np.zeros(blocks.n_loc)
    missing = int(lib().bicg_csr_diagonal(C.byref(blocks.diag), _d(d) if d.size else None))
    return d, missing


def csr_block_diagonal(blocks, bs: int):
    """(blocks, missing) of a rank's diag block (bicg_csr_block_diagonal; blocks: HostBlocks, or a CSR with local columns): the bs x bs
    diagonal blocks in the layout set_block_diagonal takes, shaped [ceil(n / bs), bs, bs] -- entries stored more than once summed in
    stored order, everything not stored 0.0; missing = the number of rows without a stored (i,i) entry. No GPU needed."""
    bs = int(bs)
    if not 1 <= bs <= 16:
        raise ValueError(f"bs = {bs} is outside 1..16")
    if isinstance(blocks, CSR):
        blocks = HostBlocks(blocks, None, blocks.rows, [blocks.rows], [0])
    out = np.zeros((-(-blocks.n_loc // bs), bs, bs))
    missing = int(lib().bicg_csr_block_diagonal(C.byref(blocks.diag), bs, _d(out) if out.size else None))
    return out, missing


def _installer(method: str) -> str:
    return "set_block_diagonal" if method in ("bicgstab_block", "bicgstab2_block") else "set_diagonal"


def device_allocations() -> int:
    """device allocations of the library's host code not yet freed, in this process (bicg_device_allocations)"""
    return int(lib().bicg_device_allocations())


PRODUCT_KERNELS = {"sell_padded": 1, "sell_jagged": 2, "sell_window_loop": 4, "jagw": 8, "stencil": 16, "csr": 32, "rows": 64, "sell_epilogue": 128,
                   "jagd": 512, "jagw_list": 1024}


def product_kernels(reset: bool = True):
    """names of the product kernels launched since the last reset (bicg_product_kernels)"""
    m = int(lib().bicg_product_kernels(1 if reset else 0))
    return sorted(k for k, v in PRODUCT_KERNELS.items() if m & v)


STREAM_KINDS = {"copy": 0, "triad": 1, "read8": 2, "read16": 3}


def stream_bench(kind: str, bytes_per_array: int = 1 << 30, reps: int = 20) -> float:
    """GB/s of a STREAM-style pass on the current GPU (bicg_stream_bench): copy / triad / read8 / read16"""
    g, ms = C.c_double(0.0), C.c_double(0.0)
    if lib().bicg_stream_bench(STREAM_KINDS[kind], bytes_per_array, reps, C.byref(g), C.byref(ms)) != 0:
        raise RuntimeError("bicg_stream_bench failed")
    return g.value


# ---- host-only helpers (no GPU) ----------------------------------------------------------------
def persist_plan(blocks: HostBlocks, nranks: int, gmax: int):
    """Plan of the persistent iteration (bicg_persist_plan) for one rank's blocks -> dict, or None when the block does not
    qualify. With nranks > 1 the offd block is renumbered to [rows + halo position] through bicg_halo_plan first."""
    L = lib()
    _usp = C.POINTER(C.c_ushort)
    L.bicg_persist_plan.argtypes = [C.POINTER(CSRMatrix), C.POINTER(CSRMatrix), C.c_uint, _up, _up, _usp, _dp, _usp, _usp, _up, _up]
    offd_p, keep = None, None
    halo = 0
    if nranks > 1:
        halo, halo_cols, rc, ren = halo_plan(blocks, nranks)
        nz = int(blocks.offd.ptr[blocks.offd.rows])
        ren = np.ascontiguousarray(ren[:max(nz, 1)], dtype=np.uint32)
        keep = (ren,)
        o = CSRMatrix(blocks.offd.val, ren.ctypes.data_as(_up), blocks.offd.ptr, nz, blocks.offd.rows, blocks.n_loc + halo)
        offd_p = C.byref(o)
    summ = (C.c_uint * 8)()
    if L.bicg_persist_plan(C.byref(blocks.diag), offd_p, gmax, summ, None, None, None, None, None, None, None) != 0:
        return None
    spw, nwg, win_slots, max_runs, max_entries, entries, nruns, rpt = list(summ)      # spw: slices per workgroup; rpt: rows per thread
    n = blocks.n_loc
    nslices = (n + 63) // 64
    pbase = np.zeros(nslices + 1, dtype=np.uint32)
    pslot = np.zeros(max(entries, 1), dtype=np.uint16)
    pval = np.zeros(max(entries, 1))
    rlen = np.zeros(n, dtype=np.uint16)
    rdiag = np.zeros(n, dtype=np.uint16)
    wptr = np.zeros(nwg + 1, dtype=np.uint32)
    runs = np.zeros(2 * max(nruns, 1), dtype=np.uint32)
    rc2 = L.bicg_persist_plan(C.byref(blocks.diag), offd_p, gmax, summ, pbase.ctypes.data_as(_up), pslot.ctypes.data_as(_usp), _d(pval),
                              rlen.ctypes.data_as(_usp), rdiag.ctypes.data_as(_usp), wptr.ctypes.data_as(_up), runs.ctypes.data_as(_up))
    assert rc2 == 0
    return dict(spw=spw, rpt=rpt, nwg=nwg, win_slots=win_slots, max_runs=max_runs, max_entries=max_entries, entries=entries, halo=halo,
                pbase=pbase, pslot=pslot[:entries], pval=pval[:entries], rlen=rlen, rdiag=rdiag, wptr=wptr, runs=runs[:2 * nruns].reshape(-1, 2))


def persist_plan_sources(blocks: HostBlocks, nranks: int, gmax: int, entries: int):
    """Source map of the persistent plan's pval (bicg_persist_plan_sources): `entries` indices into (diag values, then offd values),
    0xFFFFFFFF for padding; None when the block does not qualify. entries: persist_plan(...)["entries"]."""
    offd_p, keep = None, None
    if nranks > 1:
        halo, _, _, ren = halo_plan(blocks, nranks)
        nz = int(blocks.offd.ptr[blocks.offd.rows])
        ren = np.ascontiguousarray(ren[:max(nz, 1)], dtype=np.uint32)
        keep = (ren,)
        o = CSRMatrix(blocks.offd.val, ren.ctypes.data_as(_up), blocks.offd.ptr, nz, blocks.offd.rows, blocks.n_loc + halo)
        offd_p = C.byref(o)
    psrc = np.zeros(max(entries, 1), dtype=np.uint32)
    rc = lib().bicg_persist_plan_sources(C.byref(blocks.diag), offd_p, gmax, psrc.ctypes.data_as(_up))
    del keep
    return None if rc != 0 else psrc[:entries]


def dropin_refreshes() -> int:
    """drop-in calls that updated the resident context's values in place (BICG_DROPIN_CACHE=2; bicg_dropin_refreshes)"""
    return int(lib().bicg_dropin_refreshes())


# bicg_sell_plan_digest (include/bicgstab_hip.h section 5): names of the summary's entries and of the arrays behind the digests
SELL_SUMMARY = ("jag", "c16", "clusters", "window", "retried", "rowsplit", "sell_entries", "sell_nnz", "sell_rows", "uniform_entries",
                "constant_entries", "masked_rows", "nblk", "ng_int", "ng_bnd", "csr16", "win_slots", "win_max_runs", "win_near16",
                "jag_tail16_max", "n_bnd", "lane_info")
SELL_ARRAYS = ("slice_len", "slice_base", "slice_base16", "sval", "scol", "scol16", "perm", "group_is_sell", "gl_int", "gl_bnd", "bint",
               "bbnd", "win_ptr", "win_runs", "list", "lptr", "total", "ubase", "vbase", "mbase", "uoff", "uval", "rmask", "lane_info",
               "dcol16", "fw")


def sell_plan_digest(blocks: HostBlocks, nranks: int = 1, rows_global: int | None = None, nnz_diag_global: int | None = None):
    """The sliced-ELL plan bicg_create would make for this rank's diag block under the BICG_PLAN of the environment, without a
    GPU: (summary dict keyed by SELL_SUMMARY, digest dict keyed by SELL_ARRAYS: 64-bit FNV-1a of each array of the plan).
    rows_global / nnz_diag_global: rows and diag non-zeros of all ranks (default: this block's, i.e. one rank's)."""
    L = lib()
    _ullp = C.POINTER(C.c_ulonglong)
    L.bicg_sell_plan_digest.argtypes = [C.POINTER(CSRMatrix), C.POINTER(CSRMatrix), C.c_int, C.c_uint, C.c_ulonglong, _ullp, _ullp]
    offd_p, keep = None, None
    if nranks > 1:
        halo, _, _, ren = halo_plan(blocks, nranks)
        nz = int(blocks.offd.ptr[blocks.offd.rows])
        ren = np.ascontiguousarray(ren[:max(nz, 1)], dtype=np.uint32)
        keep = (ren,)
        o = CSRMatrix(blocks.offd.val, ren.ctypes.data_as(_up), blocks.offd.ptr, nz, blocks.offd.rows, blocks.n_loc + halo)
        offd_p = C.byref(o)
    rows_global = int(blocks.info.rows) if rows_global is None else rows_global
    nnz_diag_global = int(blocks.diag.ptr[blocks.diag.rows]) if nnz_diag_global is None else nnz_diag_global
    summ, dig = (C.c_ulonglong * len(SELL_SUMMARY))(), (C.c_ulonglong * len(SELL_ARRAYS))()
    if L.bicg_sell_plan_digest(C.byref(blocks.diag), offd_p, nranks, rows_global, nnz_diag_global, summ, dig) != 0:
        raise RuntimeError("bicg_sell_plan_digest failed")
    del keep
    return dict(zip(SELL_SUMMARY, (int(v) for v in summ))), dict(zip(SELL_ARRAYS, (int(v) for v in dig)))


# bicg_spmv_launch_plan (include/bicgstab_hip.h section 5): names of the entries of its four arrays
SPMV_SHAPE = ("ng_int", "ng_bnd", "n_int", "n_bnd", "nblk", "glist_all", "transport", "ll_fused", "has_send", "own_stream", "stencil_ok",
              "stencil_wgs", "sell_gpw", "sell_gpw_dots", "wg_cap")
SPMV_CALL = ("ndot", "epi", "has_shift", "tail", "wave")
SPMV_PLAN = ("error", "groups_per_wg", "stencil", "fused", "merged", "expected", "hand_nsh", "sets_nparts", "tail", "nsteps")
SPMV_STEP = ("family", "list", "nlist", "with_offd", "fused_halo", "slot_base", "after_halo")
SPMV_TRANSPORTS = ("single", "p2p", "hosted")
SPMV_FAMILIES = ("sell", "sell_epi", "stencil", "csr")
SPMV_LISTS = ("all", "int", "bnd", "fused", "blk_int", "blk_bnd")


def spmv_launch_plan(shape: dict, call: dict):
    """The launch plan of one distributed product (bicg_spmv_launch_plan; no GPU, no context): shape keyed by SPMV_SHAPE, call by
    SPMV_CALL (missing entries: 0; sell_gpw / sell_gpw_dots: 1) -> (plan dict keyed by SPMV_PLAN, list of step dicts keyed by
    SPMV_STEP, in launch order)."""
    L = lib()
    _uip = C.POINTER(C.c_uint)
    L.bicg_spmv_launch_plan.argtypes = [_uip, C.POINTER(C.c_int), _uip, _uip]
    L.bicg_spmv_launch_plan.restype = C.c_int
    unknown = (set(shape) - set(SPMV_SHAPE)) | (set(call) - set(SPMV_CALL))
    if unknown:
        raise KeyError(f"not an entry of the shape / the call: {sorted(unknown)}")
    dflt = {"sell_gpw": 1, "sell_gpw_dots": 1}
    sh = (C.c_uint * len(SPMV_SHAPE))(*(int(shape.get(k, dflt.get(k, 0))) for k in SPMV_SHAPE))
    ca = (C.c_int * len(SPMV_CALL))(*(int(call.get(k, 0)) for k in SPMV_CALL))
    pl, st = (C.c_uint * len(SPMV_PLAN))(), (C.c_uint * (4 * len(SPMV_STEP)))()
    if L.bicg_spmv_launch_plan(sh, ca, pl, st) != 0:
        raise RuntimeError("bicg_spmv_launch_plan failed")
    plan = dict(zip(SPMV_PLAN, (int(v) for v in pl)))
    n = len(SPMV_STEP)
    return plan, [dict(zip(SPMV_STEP, (int(v) for v in st[i * n:(i + 1) * n]))) for i in range(plan["nsteps"])]


# bicg_dot_group_plan (include/bicgstab_hip.h section 5): names of the entries of its four arrays, and of their values
DOT_SHAPE = ("transport", "stream_ordered", "overlap", "inline_apply", "tail_finish", "graph_replay", "handover")
DOT_CALL = ("regime", "n", "off", "phase", "apply_single", "event", "open", "by_product")
DOT_PLAN = ("error", "wave", "hand", "apply_now", "n_collect", "tail", "mailbox", "deferred", "nsteps")
DOT_STEP = ("op", "when", "stream", "roles", "n", "off", "phase")
DOT_REGIMES = ("ticket", "wave", "hand")
DOT_EVENTS = ("now", "defer", "force", "consume", "contribute")
DOT_OPEN = ("none", "open", "deferred", "staged")
DOT_OPS = ("nothing", "finish", "allreduce", "apply", "apply_p2p", "record", "wait", "stage", "consumer")
DOT_WHEN = ("at_close", "behind_halo", "after_product", "in_consumer")
DOT_STREAMS = ("compute", "comm")
DOT_ROLES = {"shards": 1, "push": 2, "apply": 4, "block0": 8, "local": 16, "hand": 32}      # FIN_* (csrc/bicg_device.h)


def dot_group_plan(shape: dict, call: dict):
    """Who closes a dot group (bicg_dot_group_plan; no GPU, no context): shape keyed by DOT_SHAPE, call by DOT_CALL (missing
    entries: 0; apply_single: 1) -> (plan dict keyed by DOT_PLAN, list of step dicts keyed by DOT_STEP, in order)."""
    L = lib()
    _ip_ = C.POINTER(C.c_int)
    L.bicg_dot_group_plan.argtypes = [_ip_, _ip_, _ip_, _ip_]
    L.bicg_dot_group_plan.restype = C.c_int
    unknown = (set(shape) - set(DOT_SHAPE)) | (set(call) - set(DOT_CALL))
    if unknown:
        raise KeyError(f"not an entry of the shape / the call: {sorted(unknown)}")
    sh = (C.c_int * len(DOT_SHAPE))(*(int(shape.get(k, 0)) for k in DOT_SHAPE))
    ca = (C.c_int * len(DOT_CALL))(*(int(call.get(k, 1 if k == "apply_single" else 0)) for k in DOT_CALL))
    pl, st = (C.c_int * len(DOT_PLAN))(), (C.c_int * (7 * len(DOT_STEP)))()
    if L.bicg_dot_group_plan(sh, ca, pl, st) != 0:
        raise RuntimeError("bicg_dot_group_plan failed")
    plan = dict(zip(DOT_PLAN, (int(v) for v in pl)))
    n = len(DOT_STEP)
    return plan, [dict(zip(DOT_STEP, (int(v) for v in st[i * n:(i + 1) * n]))) for i in range(plan["nsteps"])]


# bicg_reorder_plan (include/bicgstab_hip.h section 5): names of its stats
REORDER_STATS = ("rows", "components", "bandwidth_given", "bandwidth", "distinct_given", "distinct", "isolated_rows", "reserved")


def reorder_plan(blocks: HostBlocks, method: int = 1):
    """The renumbering bicg_create applies to this diag block under BICG_PLAN="reorder=1|2", without a GPU (bicg_reorder_plan):
    (perm with perm[new] = old, stats dict keyed by REORDER_STATS). method 1: reverse Cuthill-McKee."""
    perm = np.zeros(max(blocks.n_loc, 1), dtype=np.uint32)
    stats = (C.c_ulonglong * 8)()
    if lib().bicg_reorder_plan(C.byref(blocks.diag), method, perm.ctypes.data_as(_up), stats) != 0:
        raise RuntimeError("bicg_reorder_plan failed")
    return perm[:blocks.n_loc], dict(zip(REORDER_STATS, (int(v) for v in stats)))


def permute_block(blocks: HostBlocks, perm) -> CSR:
    """P A P^T of the diag block for perm[new] = old, the entries of every row in their stored order (bicg_permute_block);
    ValueError when perm is not a permutation of 0 .. rows - 1"""
    perm = np.ascontiguousarray(perm, dtype=np.uint32)
    n, nz = blocks.n_loc, int(blocks.diag.ptr[blocks.diag.rows])
    if perm.size != n:
        raise ValueError("perm must have one entry per row")
    ptr = np.zeros(n + 1, dtype=np.uint32)
    col = np.zeros(max(nz, 1), dtype=np.uint32)
    val = np.zeros(max(nz, 1))
    up = lambda a: a.ctypes.data_as(_up)
    if lib().bicg_permute_block(C.byref(blocks.diag), up(perm), up(ptr), up(col), _d(val)) != 0:
        raise ValueError("perm is not a permutation of 0 .. rows - 1")
    return CSR(n, n, ptr, col[:nz], val[:nz])


def partition(n: int, nranks: int):
    cnt = np.zeros(nranks, dtype=np.int32)
    dsp = np.zeros(nranks, dtype=np.int32)
    lib().bicg_partition(n, nranks, cnt.ctypes.data_as(_ip), dsp.ctypes.data_as(_ip))
    return cnt, dsp


def halo_plan(blocks: HostBlocks, nranks: int):
    nz = max(int(blocks.offd.nz), 1)
    cols = np.zeros(nz, dtype=np.uint32)
    ren = np.zeros(nz, dtype=np.uint32)
    rc = np.zeros(nranks, dtype=np.int32)
    h = lib().bicg_halo_plan(C.byref(blocks.offd), C.byref(blocks.info), nranks, blocks.n_loc,
                             cols.ctypes.data_as(_up), rc.ctypes.data_as(_ip), ren.ctypes.data_as(_up))
    return h, cols[:h], rc, ren[:int(blocks.offd.nz)]


def row_blocks(ptr, chunk=2048, max_rows=1024):
    ptr = np.ascontiguousarray(ptr, dtype=np.uint32)
    rows = len(ptr) - 1
    out = np.zeros(rows + 1, dtype=np.uint32)
    nb = lib().bicg_row_blocks(ptr.ctypes.data_as(_up), rows, chunk, max_rows, out.ctypes.data_as(_up))
    return out[:nb + 1]
