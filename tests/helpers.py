"""Shared helpers of the parity tests."""
import os
import subprocess

import numpy as np

from clap_amd import synth

SCENE_KEYS = ("pos_scale", "rot", "parent", "model", "model_aabb", "model_skip", "flags", "level_start")
CAM_KEYS = ("cam_pos", "cam_quat", "persp", "ndc_z_zero_one")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "clap_amd", "host")
LOADER_SRCS = [os.path.join(HOST, f) for f in ("clapgpu_load.c", "clapgpu_load_json.c", "clapgpu_load_gltf.c", "clapgpu_load_model.c",
                                               "clapgpu_snapshot.c")]
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build_test_load(exe, sanitize):
    """tests/c/test_load.c.  sanitize: with the loader's sources under AddressSanitizer + UBSan and without the GPU
    part (host code only); otherwise against the built libraries and the oracle's, which the caller has built."""
    cc = ["gcc", "-O1", "-std=gnu11", "-Wall", "-I", os.path.join(ROOT, "include")]
    src = os.path.join(ROOT, "tests", "c", "test_load.c")
    if sanitize:
        cmd = cc + SANITIZE + ["-DTEST_LOAD_NO_GPU", src] + LOADER_SRCS + ["-o", exe, "-lm"]
    else:
        libdir, odir = os.path.join(ROOT, "clap_amd", "lib"), os.path.join(ROOT, "oracle", "_build")
        cmd = cc + ["-I", os.path.join(ROOT, "oracle"), src, "-o", exe, "-L", libdir, "-lclapgpu_scene", "-lclapgpu",
                    "-L", odir, "-lclap_oracle", "-lm", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{odir}"]
    subprocess.run(cmd, check=True)


def bits_equal(a, b):
    """Bit-exact comparison of float arrays (distinguishes -0.0 from 0.0, compares NaN payloads)."""
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_bits_equal(a, b, what):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    bad = np.flatnonzero(a.view(np.uint32).ravel() != b.view(np.uint32).ravel())
    assert bad.size == 0, (f"{what}: {bad.size} of {a.size} floats differ bitwise; first at flat index "
                           f"{bad[0]}: {a.ravel()[bad[0]]!r} vs {b.ravel()[bad[0]]!r}")


def load_golden(path):
    z = np.load(path)
    scene = {k: z["in_" + k] for k in SCENE_KEYS}
    scene["n"] = scene["parent"].shape[0]
    scene["seqs"] = np.zeros(scene["n"], np.uint32)
    cam = {k: z["in_" + k] for k in CAM_KEYS}
    ref = {k[4:]: z[k] for k in z.files if k.startswith("ref_")}
    frames = None
    if "in_frames_pos_scale" in z.files:
        frames = list(zip(z["in_frames_pos_scale"], z["in_frames_rot"], z["in_frames_dirty"]))
    return scene, cam, ref, frames


def apply_frame(scene, st, frame):
    """Host-side mutation a game would do between frames: write TRS of dirty entities, set dirty."""
    ps, rot, dirty = frame
    idx = np.flatnonzero(dirty)
    scene["pos_scale"][idx] = ps[idx]
    scene["rot"][idx] = rot[idx]
    st["flags"][idx] |= synth.E_DIRTY
    return idx


# ---- the floating-point rows of the pose path: EXACT since round 4 ----
# north_star asks for "within 1e-5 relative for float transforms/positions".  Round 3 held that per object with a clause
# for cancelled sums (objects whose error exceeded 1e-5 of their own magnitude passed on 64 fp32 ulps of their TERMS): the
# kernel's arithmetic differed from the reference's (FMA contraction, polynomial slerp, a re-associated hierarchy), and
# no tolerance relative to the result survives a cancellation.  Round 4's kernel performs the reference's operations in
# the reference's order (clap_amd/csrc/pose.hip), so the clause is gone and the comparison is equality of BIT PATTERNS,
# element by element: T / R / S, the palette, joint positions, skinned positions and normals.  (-0.0 is not +0.0: the
# "0.f +" that opens every sum of mat4x4_mul, linmath.h:506-516, turns a -0 sum into +0, and the kernel performs it.
# A NaN must meet a NaN.)  What is recorded per quantity: the worst per-object relative difference (0.0 when the
# test passes) and the number of objects compared.
RTOL = 1e-5                                      # north_star's bar, for the rows that are still held to it (body state after N steps)
MAT3_IDX = (0, 1, 2, 4, 5, 6, 8, 9, 10)          # column-major mat4: the linear block
TCOL_IDX = (12, 13, 14)                          # its translation column
PARITY_BOUNDS = {}                               # worst case seen per quantity; conftest dumps it at session end


def _rel_objects(got, exp, idx=None):
    g = np.asarray(got, np.float64)
    e = np.asarray(exp, np.float64)
    assert g.shape == e.shape, (g.shape, e.shape)
    if idx is not None:
        g, e = g[..., list(idx)], e[..., list(idx)]
    d = np.abs(g - e).max(axis=-1)
    s = np.abs(e).max(axis=-1)
    r = d / np.maximum(s, 1e-30)
    r[~np.isfinite(d)] = np.inf                  # a NaN / inf on either side is settled by the value comparison below
    return r


def assert_values_equal(got, exp, what, key=None, idx=None):
    """(..., k) float arrays of k-component objects (vectors, quaternions, matrix blocks): the same bit patterns
    (a NaN for a NaN)."""
    g = np.ascontiguousarray(got, np.float32)
    e = np.ascontiguousarray(exp, np.float32)
    assert g.shape == e.shape, f"{what}: shape {g.shape} != {e.shape}"
    if idx is not None:
        g, e = g[..., list(idx)], e[..., list(idx)]
    same = (g.view(np.uint32) == e.view(np.uint32)) | (np.isnan(g) & np.isnan(e))          # the same BITS: -0 is not +0
    key = what if key is None else key
    n_obj = int(np.prod(g.shape[:-1])) if g.ndim > 1 else g.size
    PARITY_BOUNDS[key + " | objects compared"] = PARITY_BOUNDS.get(key + " | objects compared", 0) + n_obj
    if same.all():
        PARITY_BOUNDS[key] = max(PARITY_BOUNDS.get(key, 0.0), 0.0)
        return 0.0
    r = _rel_objects(g, e)
    bad_obj = ~same.all(axis=-1) if g.ndim > 1 else ~same
    worst = float(np.nanmax(np.where(np.isfinite(r), r, 0.0))) if r.size else 0.0
    PARITY_BOUNDS[key] = max(PARITY_BOUNDS.get(key, 0.0), worst if worst > 0 else float("inf"))
    at = np.unravel_index(int(np.argmax(bad_obj)), bad_obj.shape)
    raise AssertionError(f"{what}: {int(bad_obj.sum())} of {bad_obj.size} objects differ from the reference's values (first at {at}: "
                         f"{g[at]!r} vs {e[at]!r}; worst relative difference {worst:.3e})")


def assert_vec_equal(got, exp, what, key=None):
    """(..., k) arrays of k-vectors (positions, normals, quaternions)."""
    return assert_values_equal(got, exp, what, key)


def assert_mat4_equal(got, exp, what, key=None):
    """(..., 16) column-major matrices: linear block, translation column and bottom row, recorded separately."""
    key = what if key is None else key
    assert_values_equal(got, exp, f"{what} [3x3 block]", key + " [3x3 block]", MAT3_IDX)
    assert_values_equal(got, exp, f"{what} [translation]", key + " [translation]", TCOL_IDX)
    assert_values_equal(got, exp, f"{what} [bottom row]", key + " [bottom row]", (3, 7, 11, 15))
    return 0.0


def assert_trs_equal(got, exp, what, key=None):
    """(..., 10) joint T(3) R(4, xyzw) S(3)."""
    key = what if key is None else key
    assert_values_equal(got, exp, what + " [T]", key + " [T]", (0, 1, 2))
    assert_values_equal(got, exp, what + " [R]", key + " [R]", (3, 4, 5, 6))
    assert_values_equal(got, exp, what + " [S]", key + " [S]", (7, 8, 9))
    return 0.0
