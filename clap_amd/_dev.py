"""The plumbing every host-side mirror shares: a tensor's device address, the current stream, one host-to-device upload."""
import ctypes as C

import numpy as np
import torch

_SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}      # torch has no unsigned 16 / 32 bit types


def ptr(t):
    """Device address of tensor t; 0 (a null pointer) for None."""
    return t.data_ptr() if t is not None else 0


def stream():
    """The current stream, as the library's entry points take it."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def upload(a, dtype, device, shape=None):
    """Contiguous copy of host array `a` on `device`, as `dtype` and, when given, reshaped to `shape`; uint32 / uint16
    arrive as the signed type of the same width with the same bits.  A tensor is taken as it is, made contiguous."""
    if isinstance(a, torch.Tensor):
        return a.contiguous()
    a = np.ascontiguousarray(a, dtype)
    if shape is not None:
        a = a.reshape(shape)
    return torch.from_numpy(a.view(_SIGNED.get(a.dtype, a.dtype))).to(device)
