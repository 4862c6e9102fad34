"""GPU: the entity kernels with the world box taken from its extreme corners (lmd::world_aabb, clap_amd/csrc/lm_dev.h)
against the oracle, on small forests laid out by hand so that every kind of row meets the box: rows that are all roots,
rows of same-lane chains, rows whose parents sit in other lanes, rows mixing roots and children, and lanes whose
position, scale, rotation or model box carry -0.0, inverted (lo > hi), zero, negative, denormal and overflowing values --
so one wavefront holds lanes of the extreme-corner path and lanes of the literal fallback together.

Bar: the same bits in mx / inverse_mx / aabb / aabb_center (a NaN of the inverse against a NaN: assert_same_floats), the
same vis_mask and visible list, over two frames, in the tile and the level layout, all dirty and with a partly dirty
second frame."""
import numpy as np
import pytest

from clap_amd import synth, tiler
from oracle import binding as ob
from helpers import apply_frame, assert_bits_equal

pytestmark = pytest.mark.gpu

WAVE = 64
F32 = np.float32
ROOTS = np.full(WAVE, -1)
SAME = np.arange(WAVE)
HUGE_MODEL = 2                                                   # 3e38 * a scale of 1.5 overflows to +inf: a literal-path lane

MODEL_AABB = np.asarray([[-1, -2, -3, 1, 2, 3],
                         [1, 2, 3, -1, -2, -3],                  # lo > hi
                         [-1, -1, -1, 3e38, 1, 1],               # HUGE_MODEL
                         [-0.0, 0.0, -0.0, 0.0, -0.0, 0.0],      # signed zeros
                         [-1e-42, -1e-42, -1e-42, 1e-42, 1e-42, 1e-42],
                         [-0.5, -0.25, -4, 0.5, 2.5, 0.125]], F32)


def tile_rows(kind, rng):
    """Parent lane (in the previous row, or -1) of the 64 lanes of each row of a tile."""
    branch = lambda: rng.integers(0, WAVE, WAVE)                 # several children per parent, parents in other lanes
    mixed = lambda: np.where(rng.uniform(0, 1, WAVE) < 0.5, -1, rng.integers(0, WAVE, WAVE))
    if kind == 2:
        return [ROOTS, SAME]
    if kind == 3:
        return [ROOTS, branch(), mixed()]
    if kind == 4:
        return [ROOTS, SAME, SAME[::-1].copy(), SAME]
    rows = [ROOTS]                                               # one deep tile
    for r in range(1, kind):
        rows.append(mixed() if r % 13 == 0 else branch() if r % 7 == 0 else SAME)
    return rows


def slot_scene(tiles, seed):
    """A forest written directly in slot order (row r = slots [64 r, 64 r + 64), every slot an entity), with its tile
    and its level boundaries: each row is one hierarchy level of its tile, and one launch of the level layout."""
    rng = np.random.Generator(np.random.PCG64(seed))
    parent, trs = [], [0]
    for kind in tiles:
        for lanes in tile_rows(kind, rng):
            row0 = len(parent) * WAVE
            parent.append(np.where(lanes >= 0, row0 - WAVE + lanes, -1))
        trs.append(len(parent))
    parent = np.concatenate(parent)
    n = parent.size
    root = parent < 0
    pos = np.where(root[:, None], rng.uniform(-120, 120, (n, 3)), rng.uniform(-2, 2, (n, 3))).astype(F32)
    scale = np.where(root, rng.uniform(0.5, 1.5, n), rng.uniform(0.93, 1.07, n)).astype(F32)
    ang = rng.uniform(-np.pi, np.pi, (n, 3))
    rot = synth.quat_from_euler_xyz(ang[:, 0], ang[:, 1], ang[:, 2])
    model = rng.integers(0, len(MODEL_AABB), n)
    model[model == HUGE_MODEL] = 0
    u = rng.uniform(0, 1, n)
    pos[u < 0.05] = -0.0
    pos[root & (u >= 0.05) & (u < 0.15), 1] = 3e38              # roots only: a child's 3e38 overflows in its parent's frame
    scale[(u >= 0.10) & (u < 0.14)] *= -1.0
    last_lanes = np.arange(n) % WAVE >= 56                       # a zero scale empties the whole subtree's matrices: a few lanes only
    scale[last_lanes & (u >= 0.14) & (u < 0.22)] = 0.0
    scale[last_lanes & (u >= 0.22) & (u < 0.26)] = -0.0
    rot[(u >= 0.20) & (u < 0.26)] = (0, 0, 0, 1)                 # unrotated: exact zeros off the diagonal
    rot[(u >= 0.26) & (u < 0.28)] = (0, 0, 0, -1)
    rot[(u >= 0.28) & (u < 0.30)] = (-0.0, 0, 1, -0.0)
    huge = root & (u >= 0.40) & (u < 0.50)                       # unrotated roots, scale 1.5: the only products that overflow
    model[huge], scale[huge], rot[huge], pos[huge] = HUGE_MODEL, 1.5, (0, 0, 0, 1), rng.uniform(-50, 50, (int(huge.sum()), 3))
    d = synth._pack(pos, scale, rot, parent, model=model)
    d["model_aabb"], d["model_skip"] = MODEL_AABB.copy(), np.zeros(len(MODEL_AABB), np.uint8)
    d["orig_of"], d["n_real"] = np.arange(n), n
    d["tile_row_start"] = np.asarray(trs, np.uint32)
    d["level_start"] = np.arange(0, n + 1, WAVE, dtype=np.uint32)
    return d


def chains_scene(n_chains, seed):
    """n_chains roots with one child each, through the project's own layouts (padding slots, a last partial row)."""
    d = synth.entities_chains(n_chains, 2, seed) if n_chains > 1 else synth.entities_flat(1, seed)
    n = d["n"]
    rng = np.random.Generator(np.random.PCG64(seed))
    d["model_aabb"], d["model_skip"] = MODEL_AABB.copy(), np.zeros(len(MODEL_AABB), np.uint8)
    d["model"] = rng.integers(0, len(MODEL_AABB), n).astype(np.int32)
    d["model"][d["model"] == HUGE_MODEL] = 1
    u = rng.uniform(0, 1, n)
    d["pos_scale"][u < 0.1, 3] *= -1.0
    d["pos_scale"][(u >= 0.1) & (u < 0.15), 3] = 0.0
    d["pos_scale"][(u >= 0.15) & (u < 0.2), :3] = -0.0
    huge = (d["parent"] < 0) & (u >= 0.5) & (u < 0.6)
    d["model"][huge], d["pos_scale"][huge, 3], d["rot"][huge] = HUGE_MODEL, 1.5, (0, 0, 0, 1)
    return d


SCENES = {
    "tiles_2_3_4_rows": lambda: slot_scene([2, 3, 4], 11),
    "one_70_row_tile": lambda: slot_scene([70], 12),
    "n1": lambda: chains_scene(1, 13),
    "n130": lambda: chains_scene(65, 14),
}


def lay_out(name, layout):
    scene = SCENES[name]()
    if "tile_row_start" in scene:                                # laid out by hand: the same slots either way
        scene.pop("level_start" if layout == "tiles" else "tile_row_start")
        return scene
    return synth.pad_levels(scene) if layout == "levels" else tiler.tiled_scene(scene)[0]


def test_scenes_hold_every_kind_of_row():
    s = SCENES["tiles_2_3_4_rows"]()
    p = s["parent"].reshape(-1, WAVE)
    lane_of_parent = np.where(p >= 0, p % WAVE, -1)
    child = p >= 0
    all_roots = (~child).all(axis=1)
    same_lane = child.all(axis=1) & (lane_of_parent == SAME).all(axis=1)
    branching = child.all(axis=1) & (lane_of_parent != SAME).any(axis=1)
    mixing = child.any(axis=1) & (~child).any(axis=1)
    assert all_roots.sum() == 3 and same_lane.any() and branching.any() and mixing.any()
    assert list(np.diff(s["tile_row_start"])) == [2, 3, 4]
    deep = SCENES["one_70_row_tile"]()
    assert list(deep["tile_row_start"]) == [0, 70] and deep["n"] == 70 * WAVE
    assert SCENES["n1"]()["n"] == 1 and SCENES["n130"]()["n"] == 130
    for sc in (s, deep):
        ps, m = sc["pos_scale"], sc["model"]
        assert (ps[:, 3] < 0).any() and (ps[:, 3] == 0).any() and np.signbit(ps[:, :3]).all(axis=1).any()
        assert (m == HUGE_MODEL).any() and (m == 1).any() and (ps[:, 1] == F32(3e38)).any()


def oracle_frame(scene, st, fr_o, all_dirty):
    if all_dirty:
        st["flags"] |= np.where(st["flags"] & synth.E_ALIVE, synth.E_DIRTY, 0).astype(np.uint32)
    ob.entities_update(scene, st)
    return ob.entities_cull(scene["n"], st["flags"], st["aabb"], fr_o)


def assert_same_floats(got, exp, what):
    """The same bits, float by float.  One thing is left open, by IEEE 754 itself (6.3): the sign of a NaN an operation
    produces.  The oracle's x86 code yields 0xffc00000 from 0 * inf, and either sign after one of mat4x4_invert's
    negations, as its compiler places them; the scenes' only NaNs are those, in the inverse of a matrix scaled by zero.
    So a NaN must meet a NaN, and every other float its own bits (-0.0 is not 0.0)."""
    g, e = np.ascontiguousarray(got, F32), np.ascontiguousarray(exp, F32)
    assert g.shape == e.shape, f"{what}: shape {g.shape} != {e.shape}"
    differ = g.view(np.uint32) != e.view(np.uint32)
    nan_pair = np.isnan(g) & np.isnan(e)
    print(f"{what}: {int(differ.sum())} of {g.size} floats differ bitwise, {int((differ & nan_pair).sum())} of them NaN against NaN")
    assert_bits_equal(np.where(nan_pair, F32(0), g), np.where(nan_pair, F32(0), e), what)


def check_against(out, st, vis, mask, what):
    assert not np.isnan(st["mx"]).any() and not np.isnan(st["aabb"]).any() and not np.isnan(st["center"]).any()
    assert_bits_equal(out["mx"], st["mx"], what + " mx")
    assert_same_floats(out["inv_mx"], st["inv_mx"], what + " inverse_mx")
    assert_bits_equal(out["aabb"], st["aabb"], what + " aabb")
    assert_bits_equal(out["center"], st["center"], what + " aabb_center")
    assert np.array_equal(out["vis_mask"][:mask.size], mask), what + " vis_mask"
    assert out["visible_count"] == vis.size and np.array_equal(out["visible"], vis), what + " visible list"


@pytest.mark.parametrize("all_dirty", [True, False], ids=["all_dirty", "partly_dirty_second_frame"])
@pytest.mark.parametrize("layout", ["tiles", "levels"])
@pytest.mark.parametrize("name", list(SCENES))
def test_world_box_matches_oracle(name, layout, all_dirty, cuda_device):
    from clap_amd import entities
    scene = lay_out(name, layout)
    n = scene["n"]
    rng = np.random.Generator(np.random.PCG64(n))
    cam = synth.camera(pos=(0, 0, 150))
    fr, _v, _p = entities.view_calc_frustum(cam)
    fr_o, _vo, _po = ob.frustum_from_camera(cam)
    st = ob.entity_state(scene)
    batch = entities.EntityBatch(scene, cuda_device)
    for frame in range(2):
        vis, mask = oracle_frame(scene, st, fr_o, all_dirty)
        batch.mq_update(fr, all_dirty=all_dirty)
        batch.compact_visible()
        check_against(batch.download(), st, vis, mask, f"{name} {layout} frame {frame}")
        if frame == 0:
            aabb = st["aabb"]
            if scene["n_real"] > 1:                              # one wavefront, both paths: an overflowed box among finite ones
                rows = aabb[:n // WAVE * WAVE].reshape(-1, WAVE, 6)
                assert (np.isinf(rows).any(axis=2).any(axis=1) & np.isfinite(rows).all(axis=2).any(axis=1)).any()
            assert 0 < vis.size or scene["n_real"] == 1
        moved = (scene["orig_of"] >= 0) & ((rng.uniform(0, 1, n) < 0.15) | all_dirty)
        ps = scene["pos_scale"].copy()
        ps[moved, :3] += rng.uniform(-1, 1, (int(moved.sum()), 3)).astype(F32)
        apply_frame(scene, st, (ps, scene["rot"], moved))
        idx = np.flatnonzero(moved)
        batch.set_transforms(idx, ps[idx], scene["rot"][idx])
