"""CPU: the mesh set in parts (ABI 47) -- the binding, the refusals that need no device, the top tree's split rule and
height, the height bound's arithmetic, and the image checker of tests/trimeshpartsref.py on images made by hand, good and
broken (the GPU tests hold the device's images to the same checker: tests/test_trimesh_parts_gpu.py)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from clap_amd import _lib
import trimeshpartsref as pr

NEW = ("clapgpu_trimesh_create_parts", "clapgpu_trimesh_pose_meshes", "clapgpu_trimesh_parts_status", "clapgpu_trimesh_read")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_abi_and_symbols(L):
    assert _lib.ABI_VERSION >= 47
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(L, name) is not None, name


def test_refusals_without_a_device(L):
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    # A plain set that needs no device to exist: clapgpu_trimesh_create makes its object with calloc, so zeroed memory
    # is the plain set of no meshes -- and "in parts" is a non-zero mark in it.
    plain = C.cast((C.c_uint64 * 128)(), C.c_void_p)
    inv = _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_trimesh_pose_meshes(None, None, 1, ptr, ptr, ptr) == inv          # a NULL set
    assert L.clapgpu_trimesh_pose_meshes(None, None, 0, None, None, None) == inv
    assert L.clapgpu_trimesh_pose_meshes(None, plain, 1, ptr, ptr, ptr) == inv         # a plain set
    assert L.clapgpu_trimesh_pose_meshes(None, plain, 0, None, None, None) == inv
    out = (C.c_uint32 * 4)()
    assert L.clapgpu_trimesh_parts_status(None, None, out) == inv
    assert L.clapgpu_trimesh_parts_status(None, plain, None) == inv
    assert L.clapgpu_trimesh_read(None, None, None, None, None, None) == inv
    root = (C.c_uint32 * 4)()
    assert L.clapgpu_trimesh_read(None, plain, None, None, None, C.cast(root, C.c_void_p)) == inv   # part_root of a plain set
    o = C.c_void_p(123)
    assert L.clapgpu_trimesh_create_parts(None, C.byref(o), None) == inv               # the checks of clapgpu_trimesh_create
    full = dict(static_index=ptr.value, vx_first=ptr.value, tri_first=ptr.value, vx=ptr.value, idx=ptr.value, scale=ptr.value,
                pos=ptr.value, quat=ptr.value)
    d = _lib.TrimeshDesc(1, 4, **full)
    assert L.clapgpu_trimesh_create_parts(None, None, C.byref(d)) == inv
    for k in full:
        a = dict(full)
        a[k] = None
        d = _lib.TrimeshDesc(2, 4, **a)
        assert L.clapgpu_trimesh_create_parts(None, C.byref(o), C.byref(d)) == inv, k
        assert not o.value
        e = _lib.TrimeshDesc(0, 4, **{k: ptr.value})
        assert L.clapgpu_trimesh_create_parts(None, C.byref(o), C.byref(e)) == inv, k
    d = _lib.TrimeshDesc(3, 0, **full)
    assert L.clapgpu_trimesh_create_parts(None, C.byref(o), C.byref(d)) == inv


# ------------------------------------------------------------------------------------------------- the top tree
def test_split_rule_and_height():
    assert [pr.split(0, n) for n in (2, 3, 4, 5, 65)] == [1, 2, 2, 3, 33]
    for P in list(range(0, 70)) + [127, 128, 129, 1000, 2049, 4097]:
        want = 0 if P <= 1 else math.ceil(math.log2(P))
        assert pr.top_height(P) == want == pr.top_height_by_rule(P), P
        shape = pr.top_shape(P)
        assert len(shape) == max(P - 1, 0)
        parts = sorted(c[1] for n in shape for c in n[2:] if c[0] == "part")
        inner = sorted(c[1] for n in shape for c in n[2:] if c[0] == "node")
        if P >= 2:
            assert parts == list(range(P)) and inner == list(range(1, P - 1)), P    # every part once, every node but 0 once


def test_height_bound_arithmetic():
    # the walk's stack drops pushes beyond 64 entries: 62 edges is the plain set's bound and this one's
    assert pr.HEIGHT_MAX == 62
    assert pr.height_allowed(2049, 12) and pr.height_allowed(1, 62) and pr.height_allowed(2, 61)
    assert not pr.height_allowed(2, 62)
    assert pr.height_allowed(1 << 20, 42) and not pr.height_allowed((1 << 20) + 1, 42)   # 2^20 parts over a deep part
    # a part's own height is at most 62 (distinct 62-bit keys); a set of test size cannot be refused: 4 096 identical
    # centroids make a part 12 or so high under a top of a few levels
    assert pr.height_allowed(65, 62 - 7) and not pr.height_allowed(65, 62 - 6)


def test_part_roots_layout():
    root, P = pr.part_roots([0, 0, 1, 3, 3, 68])             # meshes of 0, 1, 2, 0 and 65 triangles
    assert P == 3
    assert list(root) == [pr.NONE, pr.LEAF | 0, 2 + 1 - 1, pr.NONE, 2 + 3 - 2]
    root, P = pr.part_roots([0, 0, 5])
    assert P == 1 and list(root) == [pr.NONE, 0]            # one part: node 0 is its root
    root, P = pr.part_roots([0, 1])
    assert P == 1 and list(root) == [pr.LEAF]


# ------------------------------------------------------------------------------------------------- the checker
def tris(R, k, at=0.0):
    return R.uniform(-1, 1, (k, 9)) + at


def good_image(sizes=(0, 1, 2, 3, 65), seed=1, order=None):
    R = np.random.Generator(np.random.PCG64(seed))
    meshes = [tris(R, k, 10.0 * m) for m, k in enumerate(sizes)]
    st = 7 + 2 * np.arange(len(sizes))
    return pr.make_image(meshes, st, order), st


def run(img, st):
    return pr.check_image(img["nodes"], img["key"], img["tri"], img["part_root"], img["tri_first"], st)


def test_checker_accepts_good_images():
    img, st = good_image()
    assert run(img, st) == (2, 7, 9)                        # 4 parts; 65 leaves balanced: 7; the big part on a long branch
    img, st = good_image(order=[4, 2, 1, 3])                # any order of the parts under the top
    top, deep, total = run(img, st)
    assert (top, deep) == (2, 7) and total in (8, 9)
    for sizes, want in (((0, 0), (0, 0, 0)), ((1,), (0, 1, 1)), ((0, 5), (0, 3, 3)), ((4, 4), (1, 2, 3)), ((1, 1, 1), (2, 0, 2)),
                        ((1,) * 64, (6, 0, 6)), ((2,) * 65, (7, 1, 8))):
        img, st = good_image(sizes)
        got = run(img, st)
        assert got[:2] == want[:2] and want[2] - 1 <= got[2] <= want[2], (sizes, got)
    img, st = good_image((3, 2))                            # NaN triangles: a NaN box equals a NaN box, unions skip it
    img["tri"][1] = np.nan
    img2 = pr.make_image([img["tri"][:3], img["tri"][3:]], st)
    run(img2, st)


def broken(change, sizes=(0, 1, 2, 3, 65)):
    img, st = good_image(sizes)
    change(img)
    with pytest.raises(pr.Broken) as e:
        run(img, st)
    return str(e.value)


def test_checker_refuses_broken_images():
    def box(img):
        img["nodes"][5]["box"][1][4] = np.nextafter(img["nodes"][5]["box"][1][4], np.float32(np.inf))
    assert "box" in broken(box)

    def inward(img):                                        # a leaf box rounded to nearest instead of outward
        n = img["nodes"][img["part_root"][2]]
        s = int(n["child"][0]) & ~pr.LEAF
        lo = img["tri"][s].reshape(3, 3).min(0)
        f = np.float32(lo[0])
        n["box"][0][0] = f if float(f) > lo[0] else np.nextafter(f, np.float32(np.inf))
    assert "box" in broken(inward)

    def twice(img):                                         # one leaf linked twice, its sibling lost
        n = img["nodes"][img["part_root"][4]]
        while not int(n["child"][0]) & pr.LEAF:
            n = img["nodes"][n["child"][0]]
        n["child"][1] = n["child"][0]
    assert "twice" in broken(twice)

    def foreign(img):                                       # two parts swap a leaf: every slot still reached once
        a, b = img["nodes"][img["part_root"][2]], img["nodes"][img["part_root"][3]]
        ia = 0 if int(a["child"][0]) & pr.LEAF else 1
        ib = 0 if int(b["child"][0]) & pr.LEAF else 1
        ca, cb = a["child"][ia], b["child"][ib]
        a["child"][ia], b["child"][ib] = cb, ca
        ba, bb = a["box"][ia].copy(), b["box"][ib].copy()
        a["box"][ia], b["box"][ib] = bb, ba
    assert "below the root of mesh" in broken(foreign)

    def root(img):
        img["part_root"][2] += 1
    assert "part_root" in broken(root)

    def key_static(img):
        img["key"][3, 0] += 1
    assert "static" in broken(key_static)

    def key_tri(img):
        img["key"][4, 1] = img["key"][5, 1]
    assert "triangles" in broken(key_tri)

    def top_into_part(img):                                 # a top node links into the middle of a part
        img["nodes"][0]["child"][1] = img["part_root"][4] + 1
    msg = broken(top_into_part)
    assert "wrong side" in msg or "top node" in msg, msg

    img, st = good_image((1, 1, 1, 1))                      # a top that is a chain: no balanced tree's height
    n = img["nodes"]
    # chain: node 0 -> (part 0, node 1), node 1 -> (part 1, node 2), node 2 -> (part 2, part 3)
    lb = pr.leaf_boxes(img["tri"])
    n[2]["child"][:] = [pr.LEAF | 2, pr.LEAF | 3]
    n[2]["box"][:] = [lb[2], lb[3]]
    n[1]["child"][:] = [pr.LEAF | 1, 2]
    n[1]["box"][:] = [lb[1], pr.union(lb[2], lb[3])]
    n[0]["child"][:] = [pr.LEAF | 0, 1]
    n[0]["box"][:] = [lb[0], pr.union(lb[1], pr.union(lb[2], lb[3]))]
    with pytest.raises(pr.Broken) as e:
        run(img, st)
    assert "top height" in str(e.value)

    def one_leaf(img):
        img["nodes"][0]["child"][1] = 0
    assert "one leaf" in broken(one_leaf, (1,))
