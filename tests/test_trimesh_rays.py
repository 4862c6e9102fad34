"""CPU: the static-mesh entry points (clapgpu_trimesh_*) exist and refuse bad arguments before any HIP call (the ray casts
that take the set: tests/test_rays.py); the loader writes the collision meshes of trimesh bodies."""
import base64
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from clap_amd import _lib, snapshot
from helpers import build_test_load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "scene_fixture")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_trimesh_create_refuses_bad_descriptors(L):
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p).value
    out = C.c_void_p(123)
    assert L.clapgpu_trimesh_create(None, C.byref(out), None) == _lib.ERR_INVALID_ARGUMENTS
    full = dict(static_index=ptr, vx_first=ptr, tri_first=ptr, vx=ptr, idx=ptr, scale=ptr, pos=ptr, quat=ptr)
    d = _lib.TrimeshDesc(1, 4, **full)
    assert L.clapgpu_trimesh_create(None, None, C.byref(d)) == _lib.ERR_INVALID_ARGUMENTS
    for k in full:                                           # n_meshes > 0 with an array missing
        a = dict(full)
        a[k] = None
        d = _lib.TrimeshDesc(2, 4, **a)
        assert L.clapgpu_trimesh_create(None, C.byref(out), C.byref(d)) == _lib.ERR_INVALID_ARGUMENTS, k
        assert not out.value
        e = _lib.TrimeshDesc(0, 4, **{k: ptr})               # n_meshes == 0 with an array given
        assert L.clapgpu_trimesh_create(None, C.byref(out), C.byref(e)) == _lib.ERR_INVALID_ARGUMENTS, k
    d = _lib.TrimeshDesc(3, 0, **full)                       # no statics: every static_index is out of range
    assert L.clapgpu_trimesh_create(None, C.byref(out), C.byref(d)) == _lib.ERR_INVALID_ARGUMENTS


def test_trimesh_pose_and_status_refuse_null(L):
    buf = (C.c_double * 8)()
    ptr = C.cast(buf, C.c_void_p)
    dep, nt = C.c_uint32(), C.c_uint32()
    assert L.clapgpu_trimesh_pose(None, None, ptr, ptr) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_trimesh_status(None, None, C.byref(dep), C.byref(nt)) == _lib.ERR_INVALID_ARGUMENTS
    L.clapgpu_trimesh_destroy(None)                          # a no-op


def gltf_accessor(g, i, dtype, comps):
    """An accessor of a .gltf with a base64 data: buffer, decoded here independently of the loader."""
    acc = g["accessors"][i]
    bv = g["bufferViews"][acc["bufferView"]]
    uri = g["buffers"][bv["buffer"]]["uri"]
    raw = base64.b64decode(uri.split(",", 1)[1])
    off = bv.get("byteOffset", 0) + acc.get("byteOffset", 0)
    n = acc["count"] * comps
    return np.frombuffer(raw, dtype, n, off).reshape(acc["count"], comps)


def test_loader_writes_the_crate_collision_mesh(tmp_path):
    out = str(tmp_path / "scene.clps")
    snapshot.load_scene_json(os.path.join(FIX, "scene.json"), out)
    comps = snapshot.load_scene(out)
    col = comps["collision"]
    scene = json.load(open(os.path.join(FIX, "scene.json")))
    names = [m["name"] for m in scene["model"]]
    k = names.index("crate")
    g = json.load(open(os.path.join(FIX, "crate.gltf")))
    prim = g["meshes"][0]["primitives"][0]
    pos = gltf_accessor(g, prim["attributes"]["POSITION"], np.float32, 3)
    idx = gltf_accessor(g, prim["indices"], np.uint16, 1).reshape(-1, 3)
    lo, hi = pos.min(0), pos.max(0)                          # fix_origin: centre in x / z, bottom at 0 (util.c:77-92)
    c = np.array([(lo[0] + hi[0]) / np.float32(2), lo[1], (lo[2] + hi[2]) / np.float32(2)], np.float32)
    fixed = pos - c
    vf, tf = col["vx_first"], col["tri_first"]
    assert len(vf) == len(tf) == len(names) + 1
    for j in range(len(names)):                              # only the trimesh model has a range
        has = scene["model"][j].get("physics", {}).get("geom") == "trimesh"
        assert (vf[j + 1] > vf[j]) == has and (tf[j + 1] > tf[j]) == has
    assert vf[k + 1] - vf[k] == len(pos) and tf[k + 1] - tf[k] == len(idx)
    vx, ix = col["vx"][vf[k]:vf[k + 1]], col["idx"][tf[k]:tf[k + 1]]
    assert np.array_equal(vx.view(np.uint32), fixed.view(np.uint32))
    for t in (0, len(idx) - 1):                              # first and last triangles, vertex for vertex
        assert np.array_equal(ix[t], idx[t])
        assert np.array_equal(vx[ix[t]], fixed[idx[t]])


def test_loader_collision_meshes_under_sanitizers(tmp_path):
    """The loader built with AddressSanitizer + UBSan (host code) over the fixture, writing the collision keys."""
    exe = str(tmp_path / "test_load_c")
    build_test_load(exe, sanitize=True)
    r = subprocess.run([exe, FIX, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout
    snaps = [f for f in os.listdir(tmp_path) if f.endswith(".clps")]
    assert snaps, os.listdir(tmp_path)
    found = False
    for f in snaps:
        comps = snapshot.load_scene(str(tmp_path / f))
        if "collision" in comps and len(comps["collision"]["idx"]):
            found = True
    assert found
