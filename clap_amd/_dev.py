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


def _new(shape, dtype, device, fill, contents):
    """The one place a mirror's array on `device` is made: a copy of the host array `contents` when that is given (shape
    and dtype are then its own), otherwise `shape` x `dtype` with every element `fill`, uninitialised for fill None.
    device_array and upload look this name up when they are called, so the test suite's guard bands hook it here."""
    if contents is not None:
        return torch.from_numpy(contents).to(device)
    if fill is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if fill == 0:
        return torch.zeros(shape, dtype=dtype, device=device)
    return torch.full(shape, fill, dtype=dtype, device=device)


def device_array(shape, dtype, device, fill=0):
    """A new array of `shape` x `dtype` on `device`, every element `fill`; fill=None leaves it uninitialised."""
    return _new((int(shape),) if isinstance(shape, (int, np.integer)) else tuple(shape), dtype, device, fill, None)


def upload(a, dtype, device, shape=None):
    """Contiguous copy of host array `a` on `device`, as `dtype` and, when given, reshaped to `shape`; uint32 / uint16
    arrive as the signed type of the same width with the same bits.  A tensor is taken as it is, made contiguous."""
    if isinstance(a, torch.Tensor):
        return a.contiguous()
    a = np.ascontiguousarray(a, dtype)
    if shape is not None:
        a = a.reshape(shape)
    return _new(None, None, device, None, a.view(_SIGNED.get(a.dtype, a.dtype)))
