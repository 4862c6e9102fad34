"""CPU: the ray-cast entry points (clapgpu_bp_index, clapgpu_bp_index_status, clapgpu_ray_cast,
clapgpu_bodies_ground_collide) exist and refuse bad arguments before any HIP call."""
import ctypes as C
import os

import pytest

from clap_amd import _lib


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def geoms(n=4):
    return _lib.Geoms(n, 0, 0, 0, 0, 0, 0, 0, 0)


def test_bp_index_needs_a_bp(L):
    assert L.clapgpu_bp_index(None, None, 0, None) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_bp_index(None, None, 3, C.c_void_p(16)) == _lib.ERR_INVALID_ARGUMENTS
    st = C.c_uint32(7)
    assert L.clapgpu_bp_index_status(None, None, C.byref(st)) == _lib.ERR_INVALID_ARGUMENTS


def test_ray_cast_refuses_null_descriptors_and_arrays(L):
    g, s = geoms(), geoms()
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    assert L.clapgpu_ray_cast(None, None, None, C.byref(s), None, 1, ptr, None, ptr, ptr, None, None) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_ray_cast(None, None, C.byref(g), None, None, 1, ptr, None, ptr, ptr, None, None) == _lib.ERR_INVALID_ARGUMENTS
    for ray, dist, hit in ((None, ptr, ptr), (ptr, None, ptr), (ptr, ptr, None)):
        assert L.clapgpu_ray_cast(None, None, C.byref(g), C.byref(s), None, 2, ray, None, dist, hit, None, None) == \
            _lib.ERR_INVALID_ARGUMENTS
    # nothing to do: no launch, OK
    assert L.clapgpu_ray_cast(None, None, C.byref(g), C.byref(s), None, 0, None, None, None, None, None, None) == _lib.OK


def test_ground_collide_refuses_null_descriptors_and_arrays(L):
    s = geoms()
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    b = _lib.Bodies(4, 1, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr)
    args = [ptr] * 9                       # body, ray_off, grounded, grounded_out, normal, dist, hit, flags, scratch
    assert L.clapgpu_bodies_ground_collide(None, None, None, C.byref(s), None, 1, *args) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_bodies_ground_collide(None, None, C.byref(b), None, None, 1, *args) == _lib.ERR_INVALID_ARGUMENTS
    for k in range(9):
        a = list(args)
        a[k] = None
        assert L.clapgpu_bodies_ground_collide(None, None, C.byref(b), C.byref(s), None, 2, *a) == _lib.ERR_INVALID_ARGUMENTS, k


def test_ray_flags_match_header():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "clapgpu.h")).read()
    for name, v in (("INVALID", _lib.RAY_INVALID), ("UNRESOLVED", _lib.RAY_UNRESOLVED), ("MOVED_TARGET", _lib.RAY_MOVED_TARGET)):
        assert f"#define CLAPGPU_RAY_{name}" in src
        line = [l for l in src.splitlines() if l.startswith(f"#define CLAPGPU_RAY_{name} ")][0]
        assert int(line.split()[2].rstrip("u")) == v
