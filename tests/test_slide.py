"""CPU: the restatement of character_sweep_delta / character_apply_velocity (tests/slideref.py) behaves on hand cases and
its random scenes exercise every branch of the loop; the new entry points refuse bad arguments before any HIP call.
(A clapgpu_bp or a mesh set cannot be created without a device: the refusals that need one are in test_slide_gpu.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

from clap_amd import _lib, synth
import slideref as sr

f32 = np.float32


def little_world(statics, sphere=False):
    """one body at the origin (a sphere or a capsule of synth.capsule_bodies), seven far away; -> (OracleSweep, body)"""
    b = synth.capsule_bodies(8, box=1.0, seed=1)
    L = b["length"]
    i = int(np.flatnonzero(L == 0)[0] if sphere else np.flatnonzero(L > 0)[0])
    b["pos"][:] = [-500.0, -500.0, -500.0]
    b["pos"][:, 0] -= 10.0 * np.arange(8)
    b["pos"][i] = 0.0
    return sr.OracleSweep(b, np.asarray(statics, float).reshape(-1, 6)), i


def box_of(w, i, pos):
    L = float(w.b["length"][i])
    return sr.capsule_box(pos, w.st["axis"][i], w.b["radius"][i], L)


def test_drop_onto_a_slab_stops_and_zeroes_the_fall():
    w, i = little_world([[-10, 10, -4, -3, -10, 10]])
    res = sr.run_mover(w, i, [0, -150, 0], 1, 1.0 / 30.0)             # 5 units down, the slab's top 3 below the centre
    lo, _hi = box_of(w, i, res["pos"])
    assert res["first_frac"][0] < 1 and res["velocity"][1] == 0 and res["zeroed"]
    assert -3.0 - 1e-6 <= lo[1] < -3.0 + 0.2, lo                        # rests on the slab, within the back-up
    assert res["pos"][0] == 0 and res["pos"][2] == 0


def test_grounded_walk_into_a_wall_slides_along_it():
    w, i = little_world([[2, 3, -10, 10, -50, 50]])
    res = sr.run_mover(w, i, [60, 0, 60], 0, 1.0 / 30.0)               # (2, 0, 2) a frame, the wall's face at x = 2
    _lo, hi = box_of(w, i, res["pos"])
    assert res["first_frac"][0] < 1 and len(res["calls"][0]) >= 2
    assert hi[0] <= 2.0 + 1e-6, hi                                      # nothing of the move goes into the wall
    assert res["pos"][2] > 1.5 and res["pos"][1] == 0                   # ... and the rest went along it
    assert res["velocity"][1] == 0 and not res["zeroed"]                 # grounded: the velocity is not touched
    assert "slid" in sr.groups(res)


def test_falling_past_a_wall_edge_is_not_stopped_by_the_vertical_sweep():
    w, i = little_world([[0, 0, 0, 0, 0, 0]], sphere=True)
    r = float(w.b["radius"][i])
    w, i = little_world([[0.9 * r, 5, -9, -1, -5, 5]], sphere=True)      # the top edge beside the path: normal y 0.44
    res = sr.run_mover(w, i, [0, -90, 0], 1, 1.0 / 30.0)
    first = res["calls"][0][0]
    assert first["filtered"] and first["hit"] == -2 and res["first_frac"][0] == 1
    assert res["pos"][1] == np.float64(f32(np.float64(f32(-90)) * (1.0 / 30.0))) and res["velocity"][1] == f32(-90)


def test_tiny_dt_changes_nothing_and_long_dt_is_clamped():
    w, i = little_world([[-10, 10, -4, -3, -10, 10]])
    res = sr.run_mover(w, i, [3, -150, 1], 1, 0.9e-6)
    assert not res["changed"] and not res["calls"] and np.all(res["pos"] == 0) and res["velocity"][1] == f32(-150)
    a = sr.run_mover(w, i, [3, -150, 1], 1, 1.0)
    b = sr.run_mover(w, i, [3, -150, 1], 1, 1.0 / 30.0)
    assert a["pos"].tobytes() == b["pos"].tobytes() and a["first_frac"].tobytes() == b["first_frac"].tobytes()
    assert a["changed"] and a["first_frac"][0] < 1


def count_groups(world, movers, v, air):
    tally = {}
    for k, m in enumerate(movers):
        for g in sr.groups(sr.run_mover(world, m, v[k], air[k], 1.0 / 30.0)):
            tally[g] = tally.get(g, 0) + 1
    return tally


def test_random_scenes_exercise_the_loop():
    """scene A through the oracle's sweep, scene B (the terrain and the bodies over it) through meshcontactref.sweep joined
    with the oracle's: in EACH scene every branch of the loop is taken by at least 20 of the 300 movers the GPU tests
    use, and bodies are pushed"""
    b, statics = sr.scene_a()
    movers, v, air = sr.movers_a(b["n"])
    ta = count_groups(sr.OracleSweep(b, statics), movers, v, air)
    import trimeshref as tr
    bb, meshes = sr.scene_b()
    mv, vb, ab = sr.movers_b(bb)
    tb = count_groups(sr.SceneBSweep(bb, tr.bake(*meshes[0]), 0), mv, vb, ab)
    print("scene A", ta, "scene B", tb)
    for name, t in (("A", ta), ("B", tb)):
        for g in ("free", "blocked", "slid", "filtered", "zeroed"):
            assert t.get(g, 0) >= 20, (name, g, t)
        assert t.get("pushed", 0) >= 5, (name, t)


# ------------------------------------------------------------------------------------------------- refusals
@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def descs():
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    b = _lib.Bodies(4, 1, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr)
    return b, _lib.Geoms(4, 0, 0, 0, 0, 0, 0, 0, 0), ptr, buf


def test_sweep_grid_refuses_null_descriptors_and_arrays(L):
    b, s, ptr, _keep = descs()
    a = [ptr] * 5                                                        # sweep_body, delta, frac, normal, hit
    assert L.clapgpu_sweep_capsules_grid(None, None, None, C.byref(s), None, 1, *a, None) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_sweep_capsules_grid(None, None, C.byref(b), None, None, 1, *a, None) == _lib.ERR_INVALID_ARGUMENTS
    for k in range(5):
        x = list(a)
        x[k] = None
        assert L.clapgpu_sweep_capsules_grid(None, None, C.byref(b), C.byref(s), None, 2, *x, None) == _lib.ERR_INVALID_ARGUMENTS, k
    assert L.clapgpu_sweep_capsules_grid(None, None, C.byref(b), C.byref(s), None, 0, None, None, None, None, None, None) == _lib.OK


def test_slide_refuses_null_descriptors_and_arrays(L):
    b, s, ptr, _keep = descs()
    p = ptr.value
    full = lambda n=2: _lib.Slide(n, p, p, p, p, p, p)
    sl = full()
    assert L.clapgpu_characters_slide(None, None, None, C.byref(s), None, 0.01, C.byref(sl), ptr) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_characters_slide(None, None, C.byref(b), None, None, 0.01, C.byref(sl), ptr) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_characters_slide(None, None, C.byref(b), C.byref(s), None, 0.01, None, ptr) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_characters_slide(None, None, C.byref(b), C.byref(s), None, 0.01, C.byref(sl), None) == _lib.ERR_INVALID_ARGUMENTS
    for name in ("body", "velocity", "airborne", "first_frac", "push_hit", "flags"):
        sl = full()
        setattr(sl, name, None)
        assert L.clapgpu_characters_slide(None, None, C.byref(b), C.byref(s), None, 0.01, C.byref(sl), ptr) == \
            _lib.ERR_INVALID_ARGUMENTS, name
    empty = _lib.Slide(0, None, None, None, None, None, None)
    assert L.clapgpu_characters_slide(None, None, C.byref(b), C.byref(s), None, 0.01, C.byref(empty), None) == _lib.OK


def test_slide_flags_and_struct_match_header():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "clapgpu.h")).read()
    for name, v in (("INVALID", _lib.SLIDE_INVALID), ("UNRESOLVED", _lib.SLIDE_UNRESOLVED), ("MOVED_TARGET", _lib.SLIDE_MOVED_TARGET)):
        line = [l for l in src.splitlines() if l.startswith(f"#define CLAPGPU_SLIDE_{name} ")][0]
        assert int(line.split()[2].rstrip("u")) == v
