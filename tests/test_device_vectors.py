"""Device-resident vectors, the parts that need no GPU.

1. The five entry points (bicg_load_device, bicg_fetch_device, bicg_solve_device, bicg_spmv_device, bicg_solve_multi_device) resolve
   in the cross-compiled library, are listed in hipsolver.EXPORTS and carry the argument types the binding declares.
2. The dispatch of Context.load / solve / spmv / solve_multi decides "device form" from the arguments alone: a CPU tensor, a tensor
   that is not float64 and a mix of tensors and numpy arrays raise TypeError before the library or the context's handle is touched
   -- shown on a Context made with __new__, which has neither a handle nor a row count."""
import ctypes as C

import numpy as np
import pytest
import torch

from mpi_bicgstab_amd import hipsolver as H

SYMBOLS = ("bicg_load_device", "bicg_fetch_device", "bicg_solve_device", "bicg_spmv_device", "bicg_solve_multi_device")


class CudaFloat32:
    """stands for a float32 tensor in device memory where there is no device: what the dispatch looks at, and nothing else"""
    is_cuda = True
    dtype = torch.float32

    def data_ptr(self):
        raise AssertionError("the dispatch must refuse the tensor before it asks for its address")


def test_the_symbols_resolve_and_are_declared():
    L = H.lib()
    for name in SYMBOLS:
        assert name in H.EXPORTS, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int, name
        assert fn.argtypes[0] is C.c_void_p and fn.argtypes[-1] is C.c_void_p, name      # context first, stream last
    assert len(L.bicg_load_device.argtypes) == 4 and len(L.bicg_fetch_device.argtypes) == 4 and len(L.bicg_spmv_device.argtypes) == 4
    assert len(L.bicg_solve_device.argtypes) == 7
    assert L.bicg_solve_multi_device.argtypes[4] is C.c_size_t and len(L.bicg_solve_multi_device.argtypes) == 9


def test_a_null_context_is_refused_without_a_device():
    L = H.lib()
    assert L.bicg_load_device(None, None, None, None) == -1
    assert L.bicg_fetch_device(None, None, None, None) == -1
    assert L.bicg_spmv_device(None, None, None, None) == -1
    assert L.bicg_solve_device(None, 0, None, None, None, None, None) == -1
    assert L.bicg_solve_multi_device(None, 0, None, None, 0, 1, None, None, None) == -1


def _calls(ctx, t):
    return {
        "load": lambda: ctx.load(t, t),
        "load, warm start": lambda: ctx.load(None, t),
        "solve": lambda: ctx.solve("bicgstab", t),
        "solve with x0": lambda: ctx.solve("bicgstab", t, x0=t),
        "spmv": lambda: ctx.spmv(t),
        "solve_multi": lambda: ctx.solve_multi(t),
        "solve_multi with X0": lambda: ctx.solve_multi(t, X0=t),
    }


@pytest.mark.parametrize("what", ["cpu float64", "cpu float32", "cuda float32"])
def test_the_dispatch_refuses_other_tensors_before_any_library_call(what):
    t = {"cpu float64": torch.zeros(8, dtype=torch.float64), "cpu float32": torch.zeros(8), "cuda float32": CudaFloat32()}[what]
    ctx = H.Context.__new__(H.Context)      # no handle, no n: whatever touched either would raise AttributeError, not TypeError
    for name, call in _calls(ctx, t).items():
        with pytest.raises(TypeError):
            call()


def test_a_mix_of_tensors_and_numpy_arrays_is_refused():
    ctx = H.Context.__new__(H.Context)
    t, a = torch.zeros(8, dtype=torch.float64), np.zeros(8)
    for call in (lambda: ctx.load(a, t), lambda: ctx.load(t, a), lambda: ctx.solve("bicgstab", a, x0=t), lambda: ctx.solve_multi(a, X0=t)):
        with pytest.raises(TypeError):
            call()


def test_tensor_form_is_decided_from_the_arguments_alone():
    assert H.tensor_form(np.zeros(3), None) is False and H.tensor_form(None) is False and H.tensor_form([1.0, 2.0]) is False

    class CudaFloat64(CudaFloat32):
        dtype = torch.float64

    assert H.tensor_form(CudaFloat64(), None) is True
    with pytest.raises(TypeError):
        H.tensor_form(CudaFloat64(), CudaFloat32())
