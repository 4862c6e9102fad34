"""Cases of clapgpu_lights_update (include/clapgpu.h, "Spotlights on the device") for tests/test_spots.py and
tests/test_spots_gpu.py: the rows of tests/golden/lights_trace.npz as carriers of one scene, and the list rules by name.

A case is a dict of host arrays: pos_scale [n, 4], rot [n, 4], flags [n], parent [n] (the call does not read it), carriers
(entity, light, off [k, 3], view_slot or None), lights (nr_lights, pos, is_dir, active: LIGHTS_MAX rows), dir, cutoff,
source (a cascades.VIEWS_SOURCE record, or None) and mode.  Whatever the call may write starts from a pattern, so a byte it
should have left alone shows.
"""
import numpy as np

import ctypes as C

from clap_amd import _lib, cascades as cm, entities, lights as lm
import spotsref

M = _lib.LIGHTS_MAX
N_ENTITIES = 300
SENTINEL = 0xC0FFEE01
COUNTS = (0, 1, 3, 64, 128, 129, 300)                       # the stride loop runs past one pass at 129 and above


def pattern(shape):
    """finite, distinct floats a rule would not produce"""
    n = int(np.prod(shape))
    return (np.float32(1000.0) + np.arange(n, dtype=np.float32) * np.float32(0.5)).reshape(shape)


def blank_source(pose_slots=(1, 2, 3, 4), z01=False):
    s = np.zeros((), cm.VIEWS_SOURCE)
    s.reshape(1).view(np.uint32)[:] = SENTINEL
    for v in range(_lib.VIEW_SLOTS):
        s["slot"][v]["flags"] = (_lib.VIEW_FROM_POSE if v in pose_slots else 0) | (_lib.VIEW_NDC_Z_ZERO_ONE if z01 else 0)
    return s


def blank(n=N_ENTITIES, nr_lights=8, source=True):
    rng = np.random.default_rng(n * 131 + nr_lights)
    q = rng.normal(size=(n, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
    ps = np.concatenate([rng.uniform(-40, 40, (n, 3)), np.ones((n, 1))], 1).astype(np.float32)
    lights = dict(nr_lights=nr_lights, pos=pattern((M, 3)), is_dir=np.zeros(M, np.int32), active=np.zeros(M, np.uint32))
    return dict(pos_scale=ps, rot=q, flags=np.full(n, _lib.E_ALIVE, np.uint32), parent=np.full(n, -1, np.int32),
                carriers=(np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros((0, 3), np.float32), None), lights=lights,
                dir=-pattern((M, 3)), cutoff=np.zeros(M, np.float32), source=blank_source() if source else None, mode=0)


def carriers(case, rows, view=True):
    """rows: (entity, light, off, view_slot)"""
    case["carriers"] = (np.asarray([r[0] for r in rows], np.uint32), np.asarray([r[1] for r in rows], np.int32),
                        np.asarray([r[2] for r in rows], np.float32).reshape(-1, 3),
                        np.asarray([r[3] for r in rows], np.uint32) if view else None)
    return case


def spot(case, l, cutoff=0.6, is_dir=1, active=1):
    case["lights"]["is_dir"][l], case["lights"]["active"][l], case["cutoff"][l] = is_dir, active, cutoff


def dirty(case, *entities):
    for e in entities:
        case["flags"][e] |= _lib.E_DIRTY


def from_trace_row(t, i, slot=2):
    """row i of the trace as one carrier: entity 1 of three, the row's light slot, its view in `slot`"""
    c = blank(3, int(t["light"][i]) + 1)
    l = int(t["light"][i])
    c["lights"]["pos"][:] = t["pos_before"]
    c["dir"][:] = t["dir_before"]
    c["source"] = blank_source(z01=bool(t["z01"][i]))
    c["pos_scale"][1, :3], c["rot"][1] = t["pos"][i], t["quat"][i]
    spot(c, l, t["cutoff"][i], t["is_dir"][i], t["active"][i])
    if t["updated"][i]:
        dirty(c, 1)
    return carriers(c, [(1, l, t["light_off"][i], slot)]), l


def from_trace(t, count, slot=1, mode=0, view=True):
    """`count` carriers over N_ENTITIES entities from the trace's rows: carrier k rides entity (7 k + 3) % 300 and holds
    light k % 128, whose kind is row (k % 128)'s; past 128 a slot has a second and a third carrier with another row's
    transform; every 16th carrier names the view slot, so the slot has several claimants."""
    rows_n = len(t["light"])
    c = blank(N_ENTITIES, min(max(count, 4), M))
    c["mode"] = mode
    rows = []
    for k in range(count):
        e, l = (7 * k + 3) % N_ENTITIES, k % M
        r = (k + (k // M) * 37) % rows_n
        c["pos_scale"][e, :3], c["rot"][e] = t["pos"][r], t["quat"][r]
        if t["updated"][r]:
            dirty(c, e)
        if k < M:
            spot(c, l, t["cutoff"][l % rows_n], t["is_dir"][l % rows_n], t["active"][l % rows_n])
        rows.append((e, l, t["light_off"][r], slot if k % 16 == 0 else 0))
    return carriers(c, rows, view)


def list_cases():
    """name -> case; what each is named for is asserted in tests/test_spots.py"""
    out = {}
    c = blank()                                              # three carriers of one slot: the last in list order writes it
    spot(c, 2)
    dirty(c, 10, 20, 30)
    out["last_wins_light"] = carriers(c, [(10, 2, (1, 0, 0), 0), (30, 2, (0, 1, 0), 0), (20, 2, (0, 0, 1), 0)])
    c = blank()                                              # two spotlights, one view slot: the later carrier's pose
    spot(c, 0), spot(c, 1, 1.2)
    dirty(c, 5, 6)
    out["last_wins_view"] = carriers(c, [(6, 1, (0, 0, 0), 1), (5, 0, (0, 0, 0), 1)])
    c = blank()                                              # ... and an earlier one keeps it when the later one is clean
    spot(c, 0), spot(c, 1, 1.2)
    dirty(c, 6)
    out["last_applying_wins_view"] = carriers(c, [(6, 1, (0, 0, 0), 4), (5, 0, (0, 0, 0), 4)])
    c = blank()                                              # light_update has no parent test
    spot(c, 3)
    c["parent"][40] = 7
    dirty(c, 40)
    out["parent_applies"] = carriers(c, [(40, 3, (0.5, 0.5, 0.5), 2)])
    c = blank()                                              # transform_is_updated is false
    spot(c, 3)
    out["clean_skipped"] = carriers(c, [(40, 3, (0.5, 0.5, 0.5), 2)])
    c = blank()                                              # ... unless every entity counts as dirty
    spot(c, 3)
    c["mode"] = _lib.UPDATE_ALL_DIRTY
    out["all_dirty"] = carriers(c, [(40, 3, (0.5, 0.5, 0.5), 2)])
    c = blank()                                              # indices out of range are skipped silently
    for l in range(8):
        spot(c, l)
    dirty(c, *range(N_ENTITIES))
    out["out_of_range"] = carriers(c, [(1, -1, (0, 0, 0), 1), (2, 8, (0, 0, 0), 1), (3, 200, (0, 0, 0), 1), (N_ENTITIES, 0, (0, 0, 0), 1),
                                       (0xFFFFFFFF, 1, (0, 0, 0), 1), (4, -2 ** 31, (0, 0, 0), 1)])
    c = blank()                                              # a released slot
    spot(c, 1, active=0)
    dirty(c, 9)
    out["inactive"] = carriers(c, [(9, 1, (0, 0, 0), 1)])
    c = blank()                                              # a point light and a directional one: position, no dir, no view
    spot(c, 1, 0.7, is_dir=0), spot(c, 2, 0.0)
    dirty(c, 9, 11)
    out["no_spotlight_no_view"] = carriers(c, [(9, 1, (1, 2, 3), 1), (11, 2, (3, 2, 1), 3)])
    c = blank(source=False)                                  # no views at all
    spot(c, 1), spot(c, 2, 0.0)
    dirty(c, 9, 11)
    out["no_view_slots"] = carriers(c, [(9, 1, (1, 2, 3), 0), (11, 2, (3, 2, 1), 0)], view=False)
    c = blank()                                              # one invalid view slot anywhere voids the whole call ...
    spot(c, 1)
    dirty(c, 9)
    out["invalid_slot_5"] = carriers(c, [(9, 1, (1, 2, 3), 1), (11, 7, (0, 0, 0), 5)])          # (its carrier is clean)
    c = blank()
    spot(c, 1)
    dirty(c, 9)
    out["invalid_slot_huge"] = carriers(c, [(9, 1, (1, 2, 3), 1), (N_ENTITIES + 5, -1, (0, 0, 0), 0xFFFFFFFF)])
    c = blank()                                              # ... and so does a slot that is no pose
    spot(c, 1)
    dirty(c, 9)
    c["source"] = blank_source(pose_slots=(1, 2, 4))
    out["slot_without_from_pose"] = carriers(c, [(9, 1, (1, 2, 3), 1), (11, 1, (0, 0, 0), 3)])
    return out


# ---- the captured-graph test's scene: 256 entities on a ring around a carrier whose spot turns -----------------------
RING_N, RING_R, RING_CUTOFF, RING_STEP, RING_REPLAYS = 256, 20.0, 0.5, 0.7, 6


def ring_positions():
    a = np.arange(RING_N, dtype=np.float64) * (2.0 * np.pi / RING_N)
    return np.stack([RING_R * np.sin(a), np.zeros(RING_N), RING_R * np.cos(a)], 1).astype(np.float32)


def ring_quat(k):
    """the carrier's rotation at replay k: k * 0.7 rad about Y"""
    h = 0.5 * RING_STEP * k
    return np.float32([0.0, np.sin(h), 0.0, np.cos(h)])


def ring_scene():
    """the scene dict of the ring: entities 0 .. 255 on the circle, entity 256 the carrier at its centre; every model box
    is the cube of edge 1, nobody is rotated or scaled, so entity i's world box is pos[i] +- 0.5 exactly"""
    n = RING_N + 1
    pos = np.concatenate([ring_positions(), np.zeros((1, 3), np.float32)])
    return dict(n=n, pos_scale=np.concatenate([pos, np.ones((n, 1), np.float32)], 1), rot=np.tile(np.float32([0, 0, 0, 1]), (n, 1)),
                parent=np.full(n, -1, np.int32), model=np.zeros(n, np.int32),
                flags=np.full(n, _lib.E_ALIVE | _lib.E_VISIBLE | _lib.E_DIRTY, np.uint32), seqs=np.zeros(n, np.uint32),
                level_start=np.asarray([0, n], np.uint32), model_aabb=np.float32([[-0.5, -0.5, -0.5, 0.5, 0.5, 0.5]]),
                model_skip=np.zeros(1, np.uint8))


def ring_mask_host(k):
    """which entities of the ring the spot sees at replay k, by the host's own functions: clapgpu_view_matrix of the
    carrier's pose, clapgpu_spot_persp, clapgpu_frustum_calc, and view_entity_in_frustum's two tests (view.c:296-337)
    over the boxes pos +- 0.5 in float32"""
    F = C.POINTER(C.c_float)
    view, pos, quat = np.zeros(16, np.float32), np.zeros(3, np.float32), ring_quat(k)
    _lib.lib().clapgpu_view_matrix(pos.ctypes.data_as(F), quat.ctypes.data_as(F), view.ctypes.data_as(F))
    planes, corners = entities.frustum_arrays(entities.frustum_from_matrices(view, lm.spot_persp(RING_CUTOFF), False))
    p = ring_positions()
    lo, hi = p - np.float32(0.5), p + np.float32(0.5)
    seen = np.ones(RING_N, bool)
    for pl in planes:
        out = np.zeros(RING_N, np.int32)
        for cx in (lo[:, 0], hi[:, 0]):
            for cy in (lo[:, 1], hi[:, 1]):
                for cz in (lo[:, 2], hi[:, 2]):
                    d = np.float32(0) + pl[0] * cx
                    d = d + pl[1] * cy
                    d = d + pl[2] * cz
                    d = d + pl[3] * np.float32(1)
                    out += d < 0
        seen &= out != 8
    for ax in range(3):
        seen &= ~((corners[:, ax][None, :] > hi[:, ax][:, None]).all(1)) & ~((corners[:, ax][None, :] < lo[:, ax][:, None]).all(1))
    return seen


def run_host(case):
    """the host twin over a case: (pos, dir, status, source)"""
    return lm.update_host(case["pos_scale"], case["rot"], case["flags"], case["carriers"], case["lights"], case["dir"],
                          case["cutoff"], case["source"], case["mode"], status=spotsref.STATUS_BEFORE)
