"""CPU: the camera controller on the device (include/clapgpu.h, "The camera controller on the device", ABI 50) -- the
version and the symbols, the block's layout against the Python mirror's dtype, the host twins and tests/cameraref.py
against a trace of the reference's own camera_update, the refusals every entry point owes before any HIP call, and
that the named cases of tests/test_camera_gpu.py do what they are named for.  No GPU is touched.

tests/golden/camera_trace.npz was recorded by a harness that is not part of the repository: the reference's
core/camera.c and core/model.c included into one translation unit with core/transform.c beside it (the build recipe of
SURVEY.md, Appendix A), `phys_ray_cast` replaced by the harness's own analytic answer (a horizontal plane y = plane_y
and a vertical wall x = wall_x, either absent as NaN), run over 64 seeded cameras.  Per camera it holds the inputs; per
cast iteration the four corners (c->frustum_corner), the four rays as phys_ray_cast received them and the stub's (hit,
depth) answers; and the final target, dist, position and frustum_corner.  Two columns are the harness's own
bookkeeping, because camera.c keeps them in locals: min_scale (fmin over depth / distance, camera.c:101-109) and
dist_after (camera.c:112, 235); a slip in either would show in the next iteration's corners, which are the
reference's.  `updated` is that bookkeeping too (dist != camera_target's dist, camera.c:238): transform_orbit sets the
transform's own flag on every path.  With has_physics == 0 the reference's phys_ray_cast returns before the stub
records anything: such a camera has no iteration rows, only its final state.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from clap_amd import _lib, camera as cam_mod
import cameraref as cr
import camerascene as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("clapgpu_camera_calc", "clapgpu_camera_target", "clapgpu_camera_rays", "clapgpu_camera_decide",
               "clapgpu_camera_update_host")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def trace(golden_dir):
    t = dict(np.load(os.path.join(golden_dir, "camera_trace.npz")))
    assert len(t["quat"]) == 64
    return t


# ---- ABI ---------------------------------------------------------------------------------------------
def test_abi_version_and_symbols(L):
    assert _lib.ABI_VERSION >= 50 and L.clapgpu_abi_version() == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    fields = dict(_lib.FrameDesc._fields_)
    assert fields["camera"] is C.c_void_p and fields["camera_bp"] is C.c_void_p
    assert [f for f, _t in _lib.FrameDesc._fields_][-2:] == ["camera", "camera_bp"]          # at the end of the descriptor


def test_cap_constant():
    assert _lib.CAMERA_ITER_MAX == 16384 and cr.ITER_MAX == 16384


def test_block_size_and_offsets_equal_the_dtype(tmp_path):
    names = [n for n in cam_mod.CAMERA.names]
    src, exe = tmp_path / "cam.c", tmp_path / "cam"
    prints = "".join(f'printf("%zu %zu\\n", offsetof(clapgpu_camera, {n}), sizeof(((clapgpu_camera *)0)->{n}));' for n in names)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "clapgpu.h"\nint main(void) { '
                   'printf("%zu %d %d\\n", sizeof(clapgpu_camera), CLAPGPU_CAMERA_BYTES, (int)CLAPGPU_CAMERA_ITER_MAX);' + prints +
                   ' return 0; }\n')
    p = subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [[int(v) for v in l.split()] for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert rows[0] == [cam_mod.CAMERA.itemsize, _lib.CAMERA_BYTES, 16384] and rows[0][0] % 16 == 0
    for n, (off, size) in zip(names, rows[1:]):
        dt, at = cam_mod.CAMERA.fields[n][:2]
        assert (at, dt.itemsize) == (off, size), n
    assert C.sizeof(_lib.Camera) == cam_mod.CAMERA.itemsize
    for f, _t in _lib.Camera._fields_:
        assert getattr(_lib.Camera, f).offset == cam_mod.CAMERA.fields[f][1], f


# ---- the trace ---------------------------------------------------------------------------------------
def _replay(t, i):
    """cast(ray) that hands out the trace's scripted answers of camera i, checking the rays it is asked for"""
    state = dict(it=0)

    def cast(ray):
        k = state["it"]
        assert k < t["iterations"][i], "more iterations than the reference ran"
        assert same(np.asarray(ray, np.float64), t["ray"][i, k]), f"camera {i}, iteration {k}: the rays"
        state["it"] = k + 1
        return t["hit"][i, k], t["depth"][i, k], [0, 0, 0, 0]
    return cast, state


def _target(fn, t, i):
    return fn(int(t["flags"][i]), t["pos_scale"][i], t["lo"][i], t["hi"][i], t["center"][i], t["head"][i], t["far_plane"][i])


def test_trace_covers_what_it_must(trace):
    t = trace
    moved, phys = t["moved"] == 1, t["has_physics"] == 1
    chars, heads = (t["flags"] & 1) == 1, (t["flags"] & 2) == 2
    assert (moved & ~chars).any() and (moved & chars & heads).any() and (moved & chars & ~heads).any()
    assert (~moved).any() and (moved & ~phys).any()
    far_binds = moved & (bits(t["target_dist"]) == bits((t["far_plane"] - np.float32(10.0)).astype(np.float32)))
    assert far_binds.any()                                                         # far_plane - 10 binds
    assert (moved & (t["target_dist"] == 10.0)).any()                              # dist_cap = 10 binds
    assert (moved & (t["target_dist"] > 10.0)).any()                               # dist_cap = avg_edge binds
    assert (moved & phys & (t["iterations"] == 0)).any()                           # dist <= 0.1 from the start
    assert (moved & (t["iterations"] > 0) & (t["dist"] < 0.1)).any()               # a pull-in to below 0.1
    assert (t["iterations"] >= 3).sum() >= 4                                       # successive pull-ins


@pytest.mark.parametrize("which", ["twins", "cameraref"])
def test_trace_every_iteration_and_the_end(L, trace, which):
    t = trace
    for i in range(len(t["quat"])):
        if not t["moved"][i]:
            continue
        tgt, d0 = _target(cam_mod.target if which == "twins" else cr.camera_target, t, i)
        assert same(tgt, t["target"][i]) and same(np.float32(d0), t["target_dist"][i]), f"camera {i}: camera_target"
        dist = np.float64(d0)
        for k in range(int(t["iterations"][i])):
            f = (cam_mod.rays if which == "twins" else cr.rays)
            corner, ray = f(t["quat"][i], tgt, np.float32(dist), t["near_plane"][i], t["aspect"][i])
            assert same(corner, t["corner"][i, k]) and same(ray, t["ray"][i, k]), f"camera {i}, iteration {k}: corners and rays"
            g = (cam_mod.decide if which == "twins" else cr.decide)
            good, ms, nxt = g(np.float32(dist), t["hit"][i, k], t["depth"][i, k], ray)
            assert same(np.float64(ms), t["min_scale"][i, k]), f"camera {i}, iteration {k}: min_scale"
            assert good == (k + 1 == t["iterations"][i]) or (not good and nxt <= 0.1), f"camera {i}, iteration {k}: the decision"
            if not good:
                dist = np.float64(nxt)
            assert same(dist, t["dist_after"][i, k]), f"camera {i}, iteration {k}: dist"


@pytest.mark.parametrize("which", ["twins", "cameraref"])
def test_trace_whole_update(L, trace, which):
    t = trace
    for i in range(len(t["quat"])):
        cast, state = _replay(t, i)
        phys = bool(t["has_physics"][i])
        if which == "twins":
            rec = np.zeros(1, cam_mod.CAMERA)[0]
            rec["quat"], rec["pos"], rec["dist"] = t["quat"][i], t["cam_pos_in"][i], t["cam_dist_in"][i]
            rec["near_plane"], rec["far_plane"], rec["aspect"] = t["near_plane"][i], t["far_plane"][i], t["aspect"][i]
            rec["moved"], rec["ctl_skip"], rec["flags"] = t["moved"][i], (0 if phys else -1), t["flags"][i]
            if t["moved"][i]:
                rec["target"], rec["dist"] = _target(cam_mod.target, t, i)
            out = cam_mod.update_host(rec, cast)
            got = dict(pos=out["pos"], dist=out["dist"], updated=int(out["updated"]), iterations=int(out["iterations"]),
                       status=int(out["status"]), corner=out["corner"], target=out["target"])
        elif t["moved"][i]:
            tgt, d0 = _target(cr.camera_target, t, i)
            got = cr.update(t["quat"][i], tgt, d0, t["near_plane"][i], t["aspect"][i], phys, cast)
            got["target"] = tgt
        else:
            continue
        if not t["moved"][i]:                                    # nothing but status and iterations
            assert got["iterations"] == 0 and got["status"] == 0
            assert same(got["pos"], t["pos"][i]) and same(np.float32(got["dist"]), t["dist"][i]), f"camera {i}: not moved"
            continue
        assert state["it"] == t["iterations"][i], f"camera {i}: iterations"
        assert got["iterations"] == (t["iterations"][i] if phys else 1) and got["status"] == 0, f"camera {i}"
        assert same(got["target"], t["target"][i]) and same(np.float32(got["dist"]), t["dist"][i]), f"camera {i}: target, dist"
        assert same(got["pos"], t["pos"][i]) and got["updated"] == t["updated"][i], f"camera {i}: pos, updated"
        if got["iterations"]:
            assert same(np.asarray(got["corner"], np.float32), t["corner_final"][i]), f"camera {i}: frustum_corner"


# ---- the named cases of the GPU test ------------------------------------------------------------------
def _run_case(c, meshes):
    sc = cs.brute_scene(meshes)
    ei = cs.entity_inputs(c)
    tgt, d0 = cr.camera_target(ei["flags"], ei["pos_scale"], ei["lo"], ei["hi"], ei["center"], ei["head"], c["far"])
    log = []

    def cast(ray):
        h, dep, f, what = cr.brute_cast(sc, ray, c["skip"])
        log.append(dict(hit=h, flags=f, what=what, scale=[dep[k] / ray[k][6] if h[k] != -1 else np.inf for k in range(4)]))
        return [x != -1 for x in h], dep, f
    out = cr.update(c["quat"], tgt, d0, c["near"], c["aspect"], c["skip"] != -1, cast)
    return out, log


def test_cases_do_what_they_are_named_for():
    """by cameraref and a brute-force fp64 caster; margins keep a last-bit difference of clapgpu_ray_cast from moving them"""
    by = {c["name"]: c for c in cs.CASES}
    assert len(by) == len(cs.CASES) == 10
    out, log = _run_case(by["no_hit"], True)
    assert out["iterations"] == 1 and not any(h != -1 for h in log[0]["hit"]) and out["status"] == 0
    out, log = _run_case(by["one_pull_in"], True)
    assert out["iterations"] == 2 and out["updated"] == 1 and out["trace"][0]["min_scale"] < 0.9 < 0.995 < out["trace"][1]["min_scale"]
    out, log = _run_case(by["three_pull_ins"], True)
    pulls = [k for k, tr in enumerate(out["trace"]) if tr["min_scale"] < 0.99]
    assert len(pulls) >= 3 and pulls == list(range(len(pulls))) and out["iterations"] == len(pulls) + 1
    winners = [int(np.argmin(log[k]["scale"])) for k in pulls]
    assert len(set(winners)) >= 2, winners
    for k in pulls:                                              # decided by a margin, not by rounding
        s = sorted(log[k]["scale"])
        assert s[1] - s[0] > 2e-3 and abs(out["trace"][k]["min_scale"] - 0.99) > 2e-3
    assert {w for l in log for w in l["what"] if w} == {"body", "static"}
    out, log = _run_case(by["triangle_wins"], True)
    assert out["iterations"] >= 2 and log[0]["what"][int(np.argmin(log[0]["scale"]))] == "tri" and out["status"] == 0
    without, _ = _run_case(by["triangle_wins"], False)
    assert without["iterations"] == 1 and without["status"] == cr.UNRESOLVED
    out, log = _run_case(by["body_static_tie"], True)
    ray = out["trace"][0]["ray"]
    sc = cs.brute_scene(True)
    body_only = cr.brute_cast(dict(sc, statics=[]), ray, 0)
    static_only = cr.brute_cast(dict(sc, bodies=[]), ray, 0)
    assert body_only[0] == [1] * 4 and static_only[0] == [-2 - 3] * 4 and body_only[1] == static_only[1]      # equal depths
    assert log[0]["hit"] == [1] * 4                              # bodies before statics
    out, log = _run_case(by["collapse_inside_a_box"], True)
    assert out["iterations"] == 1 and out["dist"] <= 0.1 and out["updated"] == 1 and log[0]["hit"] == [-2 - 2] * 4
    out, log = _run_case(by["unresolved"], True)
    assert out["status"] == cr.UNRESOLVED and out["iterations"] == 1 and all(f & cr.RAY_UNRESOLVED for f in log[0]["flags"])
    pulled, _ = _run_case(by["one_pull_in"], True)
    out, log = _run_case(by["no_physics"], True)
    assert out["iterations"] == 1 and not log and out["updated"] == 0 and pulled["updated"] == 1
    assert by["not_moved"]["moved"] == 0
    out, log = _run_case(by["nan_quaternion"], True)
    assert out["iterations"] == 1 and not (out["status"] & cr.CAPPED) and all(f & cr.RAY_INVALID for f in log[0]["flags"])


def test_host_loop_ends_on_non_finite_input(L):
    """NaN and infinite poses leave clapgpu_camera_update_host's loop by the rule, not by the cap"""
    calls = []

    def cast(ray):
        calls.append(ray.copy())
        return [0] * 4, [0.0] * 4, [_lib.RAY_INVALID if not np.isfinite(ray[k, 3:7]).all() else 0 for k in range(4)]
    for quat, dist, want in (([np.nan, 0, 0, 1], 6.0, 1), ([0, 0, 0, 1], np.nan, 0), ([0, 0, 0, 1], np.inf, 1), ([np.inf, 0, 0, 1], 6.0, 1)):
        rec = np.zeros(1, cam_mod.CAMERA)[0]
        rec["quat"], rec["dist"], rec["near_plane"], rec["aspect"], rec["moved"], rec["ctl_skip"] = quat, dist, 0.1, 1.5, 1, 0
        out = cam_mod.update_host(rec, cast)
        assert out["iterations"] == want and not (out["status"] & _lib.CAMERA_CAPPED), (quat, dist)
    assert all(not np.isfinite(r[:, 3:7]).all() for r in calls)


# ---- the refusals --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mem():
    raw = C.create_string_buffer(8192 + 256)
    at = (C.addressof(raw) + 255) & ~255

    def filled(cls):
        d = cls()
        for name, t in cls._fields_:
            if t is C.c_void_p:
                setattr(d, name, at)
        return d
    ent, geoms = filled(_lib.Entities), _lib.Geoms()
    ent.n = 64
    return dict(raw=raw, ok=at, odd=at + 4, ent=ent, geoms=geoms)


def test_camera_calc_refuses_before_any_hip_call(L, mem):
    """No device exists here: a call that got as far as a launch would fail with another code."""
    ok, odd, bad = mem["ok"], mem["odd"], _lib.ERR_INVALID_ARGUMENTS
    e, g = C.byref(mem["ent"]), C.byref(mem["geoms"])
    call = L.clapgpu_camera_calc
    assert call(None, None, e, None, None, g, g, None, ok) == bad               # a NULL block
    assert call(None, odd, e, None, None, g, g, None, ok) == bad                # a misaligned block
    assert call(None, ok, e, None, None, g, g, None, None) == bad               # a NULL source
    assert call(None, ok, e, None, None, g, g, None, odd) == bad                # a misaligned source
    assert call(None, ok, None, None, None, g, g, None, ok) == bad              # no entities
    assert call(None, ok, e, None, None, None, g, None, ok) == bad              # no bodies
    assert call(None, ok, e, None, None, g, None, None, ok) == bad              # no statics
    for name in ("pos_scale", "model", "model_table", "center"):                # what camera_target reads
        ent = _lib.Entities.from_buffer_copy(mem["ent"])
        setattr(ent, name, None)
        assert call(None, ok, C.byref(ent), None, None, g, g, None, ok) == bad, name


def test_frame_refuses_a_camera_without_its_views(L, mem):
    ok, bad = mem["ok"], _lib.ERR_INVALID_ARGUMENTS
    fr = _lib.Frustum()

    def issue(camera, views=True, frustum=False, camera_bp=None):
        f = _lib.FrameDesc()
        f.entities = C.pointer(mem["ent"])
        if frustum:
            f.frustum = C.pointer(fr)
        if views:
            f.views_source = f.views_state = ok
        f.camera, f.camera_bp = camera, camera_bp
        return L.clapgpu_frame_issue(None, C.byref(f), 0.0, 0)
    assert issue(ok, views=False) == bad                         # no view block to write
    assert issue(ok, views=False, frustum=True) == bad           # host views
    assert issue(mem["odd"]) == bad                              # a misaligned block
    assert issue(ok, camera_bp=ok) == bad                        # an index without bodies to index
