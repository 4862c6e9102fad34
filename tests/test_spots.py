"""CPU: the tracked lights on the device (include/clapgpu.h, "Spotlights on the device", ABI 52) -- the version, the
symbols and the descriptor's layout, the refusals the entry points owe before any HIP call, the host twin and
tests/spotsref.py against a trace of the reference's own light_update as bits, the loader's load-time values, and the list
rules on the cases of tests/spotscases.py.  No GPU is touched.

tests/golden/lights_trace.npz (README beside it) was recorded by a harness that is not part of the repository: the
reference's core/light.c and core/view.c included into one translation unit, transform.c linked as oracle/ref/Makefile
links it, renderer_mat4x4_perspective doubled by linmath's own _ndc_z_1 / _2, run over 128 seeded carriers.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from clap_amd import _lib, cascades as cm, entities, lights as lm
import spotscases as sc
import spotsref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("clapgpu_lights_update", "clapgpu_lights_update_host", "clapgpu_spot_persp")
_F = C.POINTER(C.c_float)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def as_bytes(a):
    return np.ascontiguousarray(np.atleast_1d(a)).view(np.uint8).reshape(-1)


run_host = sc.run_host


def same_outputs(a, b):
    return (same(a[0], b[0]) and same(a[1], b[1]) and a[2] == b[2] and
            ((a[3] is None and b[3] is None) or np.array_equal(as_bytes(a[3]), as_bytes(b[3]))))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def trace(golden_dir):
    t = dict(np.load(os.path.join(golden_dir, "lights_trace.npz")))
    assert len(t["light"]) >= 120
    return t


# ---- ABI ---------------------------------------------------------------------------------------------
def test_abi_version_symbols_and_exports(L):
    assert _lib.ABI_VERSION >= 52 and L.clapgpu_abi_version() == _lib.ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {l.split()[-1] for l in out.stdout.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "clapgpu.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name) and name in exported and name + "(" in header, name
    assert "spotlights' views stay" not in header


def test_descriptor_size_and_fields_equal_gcc(tmp_path):
    names = [f for f, _t in _lib.Spots._fields_]
    prints = "".join(f'printf("%zu %zu\\n", offsetof(clapgpu_spots, {n}), sizeof(((clapgpu_spots *)0)->{n}));' for n in names)
    prints += "".join(f'printf("%zu %zu\\n", offsetof(clapgpu_frame, {n}), sizeof(((clapgpu_frame *)0)->{n}));'
                      for n in ("spots", "view_visible", "view_visible_count"))
    src, exe = tmp_path / "spots.c", tmp_path / "spots"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "clapgpu.h"\nint main(void) { '
                   'printf("%zu %d %d\\n", sizeof(clapgpu_spots), CLAPGPU_SPOTS_BYTES, (int)CLAPGPU_SPOTS_INVALID);' + prints +
                   ' return 0; }\n')
    p = subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [[int(v) for v in l.split()] for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert rows[0] == [C.sizeof(_lib.Spots), _lib.SPOTS_BYTES, _lib.SPOTS_INVALID]
    for n, row in zip(names, rows[1:]):
        assert [getattr(_lib.Spots, n).offset, getattr(_lib.Spots, n).size] == row, n
    for n, row in zip(("spots", "view_visible", "view_visible_count"), rows[1 + len(names):]):
        assert [getattr(_lib.FrameDesc, n).offset, getattr(_lib.FrameDesc, n).size] == row, n
    f = _lib.FrameDesc()                                         # zeroed: the frame as before
    assert not f.spots and not any(f.view_visible) and not any(f.view_visible_count)


# ---- the refusals ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mem():
    raw = C.create_string_buffer(16384 + 256)
    at = (C.addressof(raw) + 255) & ~255

    def filled(cls):
        d = cls()
        for name, t in cls._fields_:
            if t is C.c_void_p:
                setattr(d, name, at)
        return d
    ent = filled(_lib.Entities)
    ent.n = 64
    lights = filled(_lib.Lights)
    lights.nr_lights = 4
    spots = filled(_lib.Spots)
    spots.n = 2
    views = _lib.Views()
    views.n = 2
    for v in range(2):
        views.vis_mask[v] = views.vis_row_pop[v] = at
    return dict(raw=raw, ok=at, odd=at + 4, ent=ent, lights=lights, spots=spots, views=views)


def test_lights_update_refuses_before_any_hip_call(L, mem, monkeypatch):
    """No device exists here, and the launch check is set to fail: a call that got as far as a launch would return
    another code."""
    monkeypatch.setenv("CLAPGPU_TEST_HOOKS", "1")                # read by the library's first clapgpu_test_fail_after
    ok, odd, bad = mem["ok"], mem["odd"], _lib.ERR_INVALID_ARGUMENTS
    call = L.clapgpu_lights_update
    e, s, l = C.byref(mem["ent"]), C.byref(mem["spots"]), C.byref(mem["lights"])
    L.clapgpu_test_fail_after(0)
    try:
        assert call(None, None, 0, s, l, ok) == bad                  # NULL e / s / lights
        assert call(None, e, 0, None, l, ok) == bad
        assert call(None, e, 0, s, None, ok) == bad
        for name in ("pos_scale", "rot", "flags"):
            ent = _lib.Entities.from_buffer_copy(mem["ent"])
            setattr(ent, name, None)
            assert call(None, C.byref(ent), 0, s, l, ok) == bad, name
        for name in ("carrier_entity", "carrier_light", "carrier_off", "dir", "cutoff", "status"):
            sp = _lib.Spots.from_buffer_copy(mem["spots"])
            setattr(sp, name, None)
            assert call(None, e, 0, C.byref(sp), l, ok) == bad, name
        for name in ("pos", "color", "attenuation", "is_dir", "active"):
            li = _lib.Lights.from_buffer_copy(mem["lights"])
            setattr(li, name, None)
            assert call(None, e, 0, s, C.byref(li), ok) == bad, name
        assert call(None, e, 0, s, l, None) == bad                   # a carrier_view_slot and no source
        assert call(None, e, 0, s, l, odd) == bad                    # ... or a misaligned one
        li = _lib.Lights.from_buffer_copy(mem["lights"])
        li.nr_lights = 129
        assert call(None, e, 0, s, C.byref(li), ok) == _lib.ERR_TOO_LARGE
        # nothing to do: nothing launched
        sp = _lib.Spots.from_buffer_copy(mem["spots"])
        sp.n = 0
        sp.carrier_entity = sp.carrier_light = sp.carrier_off = None
        assert call(None, e, 0, C.byref(sp), l, ok) == _lib.OK
        li.nr_lights = 0
        assert call(None, e, 0, s, C.byref(li), ok) == _lib.OK
        sp = _lib.Spots.from_buffer_copy(mem["spots"])               # no view slots: no source needed
        sp.n, sp.carrier_view_slot = 0, None
        assert call(None, e, 0, C.byref(sp), l, None) == _lib.OK
    finally:
        L.clapgpu_test_fail_after(-1)


def test_frame_refuses_spots_and_view_lists_before_any_launch(L, mem, monkeypatch):
    monkeypatch.setenv("CLAPGPU_TEST_HOOKS", "1")
    ok, bad = mem["ok"], _lib.ERR_INVALID_ARGUMENTS
    fr = _lib.Frustum()

    def issue(spots=True, lights=True, block=True, view_slots=True, view_visible=None, count=True, frustum=False, views=True,
              scratch=True):
        ent = _lib.Entities.from_buffer_copy(mem["ent"])
        v = _lib.Views.from_buffer_copy(mem["views"])
        ent.views = C.pointer(v) if views else None
        sp = _lib.Spots.from_buffer_copy(mem["spots"])
        if not view_slots:
            sp.carrier_view_slot = None
        li = _lib.Lights.from_buffer_copy(mem["lights"])
        f = _lib.FrameDesc()
        f.entities = C.pointer(ent)
        if frustum:
            f.frustum = C.pointer(fr)
        if block:
            f.views_source = f.views_state = ok
        if spots:
            f.spots = C.pointer(sp)
        if lights:
            f.lights = C.pointer(li)
        if view_visible is not None:
            f.view_visible[view_visible] = ok
            if count:
                f.view_visible_count[view_visible] = ok
        if scratch:
            f.visible_scratch = ok
        return L.clapgpu_frame_issue(None, C.byref(f), 0.0, 0)
    L.clapgpu_test_fail_after(0)
    try:
        assert issue(lights=False) == bad                            # spots without lights
        assert issue(block=False) == bad                             # a carrier_view_slot without the view block
        assert issue(block=False, frustum=True) == bad
        assert issue(spots=False, lights=False, block=False, view_visible=0) == bad      # a list and no main view
        assert issue(spots=False, view_visible=2) == bad             # v >= entities->views->n
        assert issue(spots=False, view_visible=0, views=False) == bad
        assert issue(spots=False, view_visible=1, count=False) == bad
        assert issue(spots=False, view_visible=1, scratch=False) == bad
    finally:
        L.clapgpu_test_fail_after(-1)


# ---- the trace -----------------------------------------------------------------------------------------
def test_trace_covers_what_it_must(trace):
    t = trace
    q, c = t["quat"], t["cutoff"]
    ran = (t["active"] == 1) & (t["updated"] == 1)
    spotl = ran & (t["is_dir"] != 0) & (c.astype(np.float64) > 0.0)
    assert ((q == [0, 0, 0, 1]).all(1)).any()                                          # identity
    for ax in range(3):                                                                  # half turns about each axis
        h = np.zeros(4, np.float32)
        h[ax] = 1
        assert ((q == h).all(1) & spotl).any(), ax
    pz = (bits(t["light_dir"]) == 0) & (np.abs(q[:, :3]).sum(1) == 1)[:, None] & spotl[:, None]
    assert pz.any(), "a half turn whose dir has a +0 where a negation gives -0"
    assert (q == 0).all(1).any() and (np.abs(np.linalg.norm(q[np.isfinite(q).all(1)].astype(np.float64), axis=1) - 1) > 0.5).any()
    assert np.isinf(q).any() and np.isnan(q).any() and np.isinf(t["pos"]).any() and np.isnan(t["pos"]).any()
    for v in (0.0, -1.0, 1e-30, np.pi):
        assert (c == np.float32(v)).any(), v
    assert np.isnan(c).any()
    assert ((t["is_dir"] != 0) & (c == 0) & ran).any() and ((t["is_dir"] == 0) & ran).any()
    assert (t["active"] == 0).any() and (t["updated"] == 0).any() and (t["z01"] == 1).any() and (t["z01"] == 0).any()
    assert spotl.sum() >= 64


def _view_of(L, pose_pos, pose_quat):
    out = np.zeros(16, np.float32)
    L.clapgpu_view_matrix(np.ascontiguousarray(pose_pos, np.float32).ctypes.data_as(_F),
                          np.ascontiguousarray(pose_quat, np.float32).ctypes.data_as(_F), out.ctypes.data_as(_F))
    return out


def test_twin_and_restatement_reproduce_the_trace_as_bits(L, trace):
    t, nn = trace, ref.one_nan
    views = 0
    for i in range(len(t["light"])):
        for slot in (1, 4):
            case, l = sc.from_trace_row(t, i, slot)
            got = run_host(case)
            assert same_outputs(got, ref.update(case)), f"row {i}: the twin against spotsref"
            pos, dr, status, src = got
            assert status == 0
            assert same(pos[l], t["light_pos"][i]), f"row {i}: pos"
            assert same(dr[l], nn(t["light_dir"][i])), f"row {i}: dir"
            assert (bits(dr)[np.isnan(dr)] == 0x7fc00000).all()
            # what the row does not name keeps its bytes
            keep_p, keep_d = case["lights"]["pos"].copy(), case["dir"].copy()
            keep_p[l], keep_d[l] = pos[l], dr[l]
            assert same(pos, keep_p) and same(dr, keep_d)
            ran = bool(t["active"][i] and t["updated"][i])
            is_spot = ran and ref.is_spotlight(t["is_dir"][i], t["cutoff"][i])
            assert is_spot == bool(t["proj_mx"][i].any() or t["view_mx"][i].any()), f"row {i}: the callback reached its view"
            want = case["source"].copy()
            if is_spot:
                bits(want["slot"][slot]["pos"])[:] = bits(t["pos"][i])
                bits(want["slot"][slot]["quat"])[:] = bits(t["quat"][i])
            assert np.array_equal(as_bytes(src), as_bytes(want)), f"row {i}: the source"
            if not is_spot:
                if ran:
                    assert same(dr[l], t["dir_before"]), f"row {i}: no spotlight, no direction"
                else:
                    assert same(pos[l], t["pos_before"]), f"row {i}: the callback did not run"
                continue
            views += 1
            z01 = int(t["z01"][i])
            view = _view_of(L, src["slot"][slot]["pos"], src["slot"][slot]["quat"])
            assert same(view, nn(t["view_mx"][i])), f"row {i}: the view matrix of the written pose"
            proj = lm.spot_persp(t["cutoff"][i], z01)
            assert same(nn(proj), nn(t["proj_mx"][i])), f"row {i}: the projection"
            planes, corners = entities.frustum_arrays(entities.frustum_from_matrices(view, proj, z01))
            assert same(np.asarray(planes, np.float32).reshape(6, 4), nn(t["planes"][i])), f"row {i}: the planes"
            assert same(np.asarray(corners, np.float32).reshape(8, 4), nn(t["corners"][i])), f"row {i}: the corners"
    assert views >= 128


def test_loader_values_equal_the_twin(L, golden_dir, tmp_path):
    """clapgpu_load.c:274-280 computes pos and dir once at load; the twin over the loaded carriers, every entity counted
    as dirty, gives the same bits"""
    from clap_amd import snapshot
    p = str(tmp_path / "fixture.clps")
    snapshot.load_scene_json(os.path.join(golden_dir, "scene_fixture", "scene.json"), p)
    comps = snapshot.load_scene(p)
    li, car, ents = comps["lights"], comps["carriers"], comps["entities"]
    ce, cl, co = car["entity"], car["light"], car["offset"]
    assert len(ce) >= 3 and len(set(int(v) for v in cl)) == len(cl)
    M = _lib.LIGHTS_MAX

    def full(a, shape, dtype):
        out = np.zeros(shape, dtype)
        out[:len(a)] = a
        return out
    lights = dict(nr_lights=int(li["nr_lights"]), pos=sc.pattern((M, 3)), is_dir=full(li["is_dir"], M, np.int32),
                  active=full(li["active"], M, np.uint32))
    cutoff = full(li["cutoff"], M, np.float32)
    pos, dr, status, _src = lm.update_host(ents["pos_scale"], ents["rot"], ents["flags"], (ce, cl, co, None), lights,
                                           -sc.pattern((M, 3)), cutoff, None, _lib.UPDATE_ALL_DIRTY)
    assert status == 0
    spots = 0
    for k in range(len(ce)):
        l = int(cl[k])
        assert same(pos[l], np.asarray(li["pos"][l], np.float32)), k
        if ref.is_spotlight(lights["is_dir"][l], cutoff[l]):
            spots += 1
            assert same(dr[l], np.asarray(li["dir"][l], np.float32)), k
        else:
            assert same(dr[l], -sc.pattern((M, 3))[l]), k
    assert spots >= 1


# ---- the list rules ------------------------------------------------------------------------------------
def test_list_cases_equal_the_brute_force_loop_and_do_what_they_are_named_for(L):
    cases = sc.list_cases()
    for name, case in cases.items():
        got = run_host(case)
        assert same_outputs(got, ref.update(case)), name
        pos, dr, status, src = got
        p0, d0, s0 = case["lights"]["pos"], case["dir"], case["source"]
        ps, rot = case["pos_scale"], case["rot"]

        def pose(v):
            return np.concatenate([src["slot"][v]["pos"], src["slot"][v]["quat"]])

        def pose_of(e):
            return np.concatenate([ps[e, :3], rot[e]])
        if name == "last_wins_light":
            assert status == 0 and same(pos[2], ps[20, :3] + np.float32([0, 0, 1])) and same(dr[2], ref.direction(rot[20]))
        elif name == "last_wins_view":
            assert status == 0 and same(pose(1), pose_of(5)) and same(dr[1], ref.direction(rot[6]))
        elif name == "last_applying_wins_view":
            assert status == 0 and same(pose(4), pose_of(6)) and same(pos[0], p0[0])
        elif name in ("parent_applies", "all_dirty"):
            assert status == 0 and same(pos[3], ps[40, :3] + np.float32(0.5)) and same(pose(2), pose_of(40))
            assert same(dr[3], ref.direction(rot[40]))
        elif name in ("clean_skipped", "out_of_range", "inactive"):
            assert status == 0 and same(pos, p0) and same(dr, d0) and np.array_equal(as_bytes(src), as_bytes(s0)), name
        elif name == "no_spotlight_no_view":
            assert status == 0 and same(pos[1], ps[9, :3] + np.float32([1, 2, 3])) and same(pos[2], ps[11, :3] + np.float32([3, 2, 1]))
            assert same(dr, d0) and np.array_equal(as_bytes(src), as_bytes(s0))
        elif name == "no_view_slots":
            assert status == 0 and src is None and same(dr[1], ref.direction(rot[9])) and same(dr[2], d0[2])
        else:
            assert name in ("invalid_slot_5", "invalid_slot_huge", "slot_without_from_pose")
            assert status == _lib.SPOTS_INVALID and same(pos, p0) and same(dr, d0) and np.array_equal(as_bytes(src), as_bytes(s0)), name
    assert len(cases) >= 12


def test_trace_scenes_equal_the_brute_force_loop(L, trace):
    """the many-carrier scenes of the GPU test: the twin against the loop, and that they exercise what they are built for"""
    for count in sc.COUNTS:
        for mode in (0, _lib.UPDATE_ALL_DIRTY):
            for slot, view in ((1, True), (4, True), (0, False)):
                case = sc.from_trace(trace, count, slot, mode, view)
                got = run_host(case)
                assert same_outputs(got, ref.update(case)), (count, mode, slot)
                assert got[2] == (0 if count else ref.STATUS_BEFORE)
                if count >= 64:
                    assert not same(got[0], case["lights"]["pos"]) and not same(got[1], case["dir"])
                if count >= 64 and view:
                    assert not np.array_equal(as_bytes(got[3]), as_bytes(case["source"]))
    a = run_host(sc.from_trace(trace, 128, 1, 0, True))
    b = run_host(sc.from_trace(trace, 300, 1, 0, True))
    assert not same(a[0], b[0]), "past 128 carriers a slot's later carrier wins"


def test_the_graph_tests_masks_differ_between_replays(L):
    """the condition that keeps the captured-graph test from passing on a frozen view, checked with the host's frustum
    functions: the six replays' masks of the ring are pairwise different and none is empty or full"""
    masks = [sc.ring_mask_host(k) for k in range(1, sc.RING_REPLAYS + 1)]
    for i, a in enumerate(masks):
        assert 0 < a.sum() < sc.RING_N, i
        for b in masks[i + 1:]:
            assert not np.array_equal(a, b)
