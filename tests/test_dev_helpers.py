"""CPU: the host-to-device upload every mirror class goes through (clap_amd/_dev.py), on device="cpu"."""
import numpy as np
import torch

from clap_amd import _dev
from clap_amd._dev import upload


def test_uint32_keeps_its_bits_as_int32():
    a = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xDEADBEEF, 0xFFFFFFFF], np.uint32)
    t = upload(a, np.uint32, "cpu")
    assert t.dtype == torch.int32 and t.shape == (6,)
    assert t.numpy().tobytes() == a.tobytes()
    assert int(t[4]) == 0xDEADBEEF - (1 << 32)
    # a list of Python ints, as callers pass body indices
    assert upload([3, 0xFFFFFFFE], np.uint32, "cpu").numpy().view(np.uint32).tolist() == [3, 0xFFFFFFFE]


def test_uint16_keeps_its_bits_as_int16():
    a = np.array([[0, 1, 0x7FFF], [0x8000, 0xBEEF, 0xFFFF]], np.uint16)
    t = upload(a, np.uint16, "cpu")
    assert t.dtype == torch.int16 and t.shape == (2, 3)
    assert t.numpy().tobytes() == a.tobytes()


def test_casts_to_the_dtype_asked_for():
    a = np.array([0.1, 1.0 / 3.0, 1e-50, 3e38], np.float64)
    t = upload(a, np.float32, "cpu")
    assert t.dtype == torch.float32
    assert t.numpy().tobytes() == a.astype(np.float32).tobytes()
    assert upload(a, np.float64, "cpu").dtype == torch.float64          # and leaves a matching dtype alone
    assert upload(np.array([1, 0, 1], bool), np.uint8, "cpu").tolist() == [1, 0, 1]


def test_non_contiguous_input_comes_out_contiguous():
    a = np.arange(24, dtype=np.float32).reshape(4, 6)[:, ::2]
    assert not a.flags["C_CONTIGUOUS"]
    t = upload(a, np.float32, "cpu")
    assert t.is_contiguous() and t.shape == (4, 3)
    assert np.array_equal(t.numpy(), a)
    u = upload(np.arange(12, dtype=np.uint32).reshape(3, 4).T, np.uint32, "cpu")
    assert u.is_contiguous() and u.dtype == torch.int32 and np.array_equal(u.numpy(), np.arange(12).reshape(3, 4).T)


def test_shape_reshapes():
    t = upload(np.arange(12.0), np.float32, "cpu", shape=(-1, 3))
    assert t.shape == (4, 3) and t.dtype == torch.float32
    assert np.array_equal(t.numpy(), np.arange(12, dtype=np.float32).reshape(4, 3))
    assert upload([[1.0, 2.0]], np.float64, "cpu", shape=(-1,)).shape == (2,)
    assert upload(np.zeros((0, 3)), np.uint32, "cpu", shape=(-1, 3)).shape == (0, 3)


def test_tensor_comes_back_contiguous_on_its_own_device():
    base = torch.arange(12, dtype=torch.int32).reshape(3, 4)
    t = base.t()
    assert not t.is_contiguous()
    got = upload(t, np.float32, "meta", shape=(-1, 2))      # dtype, device and shape are for host arrays: a tensor keeps its own
    assert got.is_contiguous() and got.device == t.device and got.dtype == torch.int32 and got.shape == (4, 3)
    assert torch.equal(got, t)
    assert upload(base, np.int32, "cpu") is base              # already contiguous: no copy


def test_ptr():
    assert _dev.ptr(None) == 0
    t = torch.zeros(4)
    assert _dev.ptr(t) == t.data_ptr() != 0
