"""GPU: the multi-level broadphase grid (clapgpu_bp_create_levels; clap_amd/csrc/bp_levels.hip).  Both pair lists of
clapgpu_bp_collide against a brute-force all-pairs overlap in numpy (tests/bplevelref.py), compared with np.array_equal:
no tolerance anywhere.  The scenes are built around the three places a leveled search goes wrong -- a slot shared across
levels by boxes that overlap, a partner list that overflows towards finer and towards coarser levels, and the inclusive
edge of the cells a finer body looks up."""
import ctypes as C

import numpy as np
import pytest
import torch

import bplevelref as ref
from clap_amd import _lib, physics, synth

pytestmark = pytest.mark.gpu

CELL0 = 0.25                                                # a power of two: every level's cell and every bound below is exact


class Grid:
    """A clapgpu_bp made directly through the C ABI (levels=None: clapgpu_bp_create)."""

    def __init__(self, dev, n_max, cell, levels, statics=None):
        self.dev, self.bp, self.L = dev, C.c_void_p(), _lib.lib()
        st = None if statics is None or not len(statics) else np.ascontiguousarray(statics, np.float64)
        self.ns = 0 if st is None else len(st)
        ptr = None if st is None else st.ctypes.data
        if levels is None:
            _lib.check(self.L.clapgpu_bp_create(C.byref(self.bp), n_max, cell, self.ns, ptr), "clapgpu_bp_create")
        else:
            _lib.check(self.L.clapgpu_bp_create_levels(C.byref(self.bp), n_max, cell, levels, self.ns, ptr), "clapgpu_bp_create_levels")
            assert self.L.clapgpu_bp_levels(self.bp) == levels

    def __del__(self):
        if getattr(self, "bp", None):
            self.L.clapgpu_bp_destroy(self.bp)
            self.bp = None

    def collide(self, aabb, cap=None, scap=None):
        """-> (pairs written [min(total, cap), 2], total, static pairs written, static total, status)"""
        n = len(aabb)
        cap = 64 * n if cap is None else cap
        scap = 64 * n if scap is None else scap
        box = torch.from_numpy(np.ascontiguousarray(aabb, np.float64)).to(self.dev)
        i32 = lambda *s: torch.full(s, -1, dtype=torch.int32, device=self.dev)
        pairs, spairs, tot = i32(max(cap, 1), 2), i32(max(scap, 1), 2), i32(2)
        p = lambda t: C.c_void_p(t.data_ptr())
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(self.L.clapgpu_bp_collide(s, self.bp, n, p(box), p(pairs), cap, p(tot), p(spairs) if self.ns else None,
                                             scap if self.ns else 0, C.c_void_p(tot.data_ptr() + 4) if self.ns else None), "clapgpu_bp_collide")
        st = C.c_uint32(0)
        _lib.check(self.L.clapgpu_bp_status(s, self.bp, C.byref(st)), "clapgpu_bp_status")
        t, ts = int(tot[0].item()), int(tot[1].item()) if self.ns else 0
        assert (pairs[min(t, cap):max(cap, 1)] == -1).all().item() or cap == 0, "written past the total or the capacity"
        return (pairs[:min(t, cap)].cpu().numpy().astype(np.int64), t, spairs[:min(ts, scap)].cpu().numpy().astype(np.int64), ts, st.value)


def assert_exact(grid, aabb, statics=None, what="", runs=1):
    want, swant = ref.brute_pairs(aabb), ref.brute_static_pairs(aabb, statics)
    for run in range(runs):
        pairs, total, spairs, stotal, status = grid.collide(aabb)
        assert status == 0, (what, run, status)
        assert total == len(want) and stotal == len(swant), (what, run, total, len(want), stotal, len(swant))
        assert len(np.unique(pairs, axis=0)) == len(pairs), (what, run, "a pair appears twice")
        assert np.array_equal(pairs, want), (what, run, "body pairs")
        assert np.array_equal(spairs, swant), (what, run, "static pairs")
    return want, swant


def mixed_statics(n, box):
    st = synth.static_boxes(n, box, seed=5)                 # [0] is a ground slab 2000 wide: larger than any top-level block
    st[1] = [-40.0, 70.0, 3.0, 5.0, -40.0, 70.0]            # ... and a second one through the middle of the scene
    return st


# ------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("with_statics", [False, True], ids=["bodies", "bodies+statics"])
def test_mixed_scene_is_exact(cuda_device, with_statics):
    levels = 6
    aabb = ref.sphere_aabb(synth.mixed_bodies(3000, box=24.0, cell0=CELL0, seed=4))
    statics = mixed_statics(60, 24.0) if with_statics else None
    grid = Grid(cuda_device, len(aabb), CELL0, levels, statics)
    want, swant = assert_exact(grid, aabb, statics, "mixed", runs=2)     # twice: the counters are left clean
    # the scene reaches what it is meant to reach
    level, over = ref.box_level(aabb, CELL0, levels)
    assert not over.any() and np.count_nonzero(np.bincount(level, minlength=levels)) >= 5
    cross = level[want[:, 0]] != level[want[:, 1]]
    assert cross.sum() > (~cross).sum() > 0
    larger = np.bincount(want[:, 0], minlength=len(aabb))   # partners of larger index: what lands in a body's own list
    assert np.any((larger > 16) & (level >= levels - 3)), "no coarse body overflows its partner list"
    if with_statics:
        top_block = 4 * CELL0 * 2.0 ** (levels - 1)
        assert np.any((statics[:, 1] - statics[:, 0]) > top_block) and len(swant) > 500


# ------------------------------------------------------------------------------------------------- 2
def boundary_scene(levels):
    top = levels - 1
    cl = CELL0 * 2.0 ** top
    rows = []
    slot = 0
    for gap in sorted({1, top}):
        e = CELL0 * 2.0 ** (top - gap)                      # the fine body's edge: its level's cell, exactly
        for axis in range(3):
            for side in (0, 1):
                org = np.array([16.0 + 8.0 * cl * slot, 0.0, 0.0])
                slot += 1
                k = np.array([3.0, 2.0, 5.0]) * cl + org    # the coarse centre: a cell corner of its level
                rows.append(np.stack([k - cl / 2, k + cl / 2], 1).reshape(6))
                lo = k + 0.25 * e                           # inside the coarse box on the other two axes
                lo[axis] = k[axis] + cl / 2 if side else k[axis] - cl / 2 - e       # its face ON the coarse body's far face
                rows.append(np.stack([lo, lo + e], 1).reshape(6))
                lo2 = lo.copy()                             # ... and one a hair outside: no pair
                lo2[axis] = np.nextafter(k[axis] + cl / 2, np.inf) if side else np.nextafter(k[axis] - cl / 2, -np.inf) - e
                lo2[(axis + 1) % 3] += 1.25 * e
                rows.append(np.stack([lo2, lo2 + e], 1).reshape(6))
    n_touch = len(rows) // 3
    # edges of exactly cell0 * 2^l and the doubles next to it, from x = 0 so that the edge is the upper bound itself
    q = 0
    for l in range(levels):
        c = CELL0 * 2.0 ** l
        for e in (c, np.nextafter(c, 0.0)) + ((np.nextafter(c, np.inf),) if l < top else ()):
            rows.append([0.0, e, 0.0625 * q, 0.0625 * q + 0.125, 0.0, 0.125])
            q += 1
    return np.array(rows), n_touch


@pytest.mark.parametrize("levels", [2, 5])
def test_level_boundaries_and_the_edge_of_the_lookup(cuda_device, levels):
    aabb, n_touch = boundary_scene(levels)
    want = ref.brute_pairs(aabb)
    level, over = ref.box_level(aabb, CELL0, levels)
    assert not over.any()
    coarse, fine, outside = np.arange(n_touch) * 3, np.arange(n_touch) * 3 + 1, np.arange(n_touch) * 3 + 2
    assert np.all(level[coarse] == levels - 1) and set(levels - 1 - level[fine]) == {1, levels - 1}
    have = {tuple(p) for p in want}
    assert all((c, f) in have for c, f in zip(coarse, fine)) and not any((c, o) in have for c, o in zip(coarse, outside))
    edge = aabb[3 * n_touch:, 1]
    assert np.all(edge[0::3][:levels - 1] == CELL0 * 2.0 ** np.arange(levels - 1)) and len(np.unique(level[3 * n_touch:])) == levels
    assert_exact(Grid(cuda_device, len(aabb), CELL0, levels), aabb, None, f"boundaries, {levels} levels")
    # the same in another index order: the fine body in front of the coarse one
    perm = np.arange(len(aabb))[::-1]
    assert_exact(Grid(cuda_device, len(aabb), CELL0, levels), aabb[perm], None, f"boundaries reversed, {levels} levels")


# ------------------------------------------------------------------------------------------------- 3
def _slots(level, cell, mask):
    """bp_levels.h's level_slot in numpy, to SEARCH with; what it finds is confirmed through clapgpu_bp_cell_slot"""
    c = np.asarray(cell, np.int64)
    b = (c >> 2).astype(np.uint32)
    h = (b[..., 0] * np.uint32(73856093)) ^ (b[..., 1] * np.uint32(19349663)) ^ (b[..., 2] * np.uint32(83492791)) ^ np.uint32((level * 2654435761) & 0xffffffff)
    h = (h ^ (h >> np.uint32(15))) & np.uint32(mask)
    return (h.astype(np.int64) << 6) | (c[..., 0] & 3) | ((c[..., 1] & 3) << 2) | ((c[..., 2] & 3) << 4)


def test_a_shared_slot_that_overlaps(cuda_device):
    levels, c2 = 3, CELL0 * 4.0
    cluster = np.array([[0.3125, 0.4375] * 3,                            # a: level 0, index 0
                        [0.4375, 0.5625] + [0.3125, 0.4375] * 2,         # b: level 0, touches a
                        [0.4, 1.3, 0.4, 1.3, 0.4, 1.3]])                 # c: level 2, overlaps both
    grid = Grid(cuda_device, 16, CELL0, levels)
    # translate by whole level-2 cells until b's level-0 cell shares its slot with a level-2 cell that a looks up
    t = np.stack(np.meshgrid(np.arange(128), np.arange(128), np.arange(64), indexing="ij"), -1).reshape(-1, 3)     # 2^20
    b_cell = np.floor((cluster[1, 0::2] + cluster[1, 1::2]) * 0.5 / CELL0).astype(np.int64) + 4 * t
    b_slot = _slots(0, b_cell, 1023)
    first = [int(ref.coarse_lookup(cluster[0, 2 * a], cluster[0, 2 * a + 1], c2)[0]) for a in range(3)]
    last = [int(ref.coarse_lookup(cluster[0, 2 * a], cluster[0, 2 * a + 1], c2)[1]) for a in range(3)]
    assert [l - f for f, l in zip(first, last)] == [1, 1, 1]             # a looks up 2 x 2 x 2 cells of level 2
    found = None
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                cand = np.flatnonzero(_slots(2, np.array([first[0] + dx, first[1] + dy, first[2] + dz]) + t, 1023) == b_slot)
                for idx in cand:
                    cj = [int(v) for v in b_cell[idx]]
                    cc = [int(first[0] + dx + t[idx, 0]), int(first[1] + dy + t[idx, 1]), int(first[2] + dz + t[idx, 2])]
                    if found is None and grid.L.clapgpu_bp_cell_slot(grid.bp, 0, *cj) == grid.L.clapgpu_bp_cell_slot(grid.bp, 2, *cc):
                        found = t[idx]
    assert found is not None, "no translation in 2^20 makes a level-0 cell share its slot with a level-2 cell looked up"
    aabb = cluster + np.repeat(found * c2, 2)[None, :]
    assert len(ref.brute_pairs(aabb)) == 3
    assert_exact(grid, aabb, None, f"shared slot at translation {found}", runs=2)


# ------------------------------------------------------------------------------------------------- 4, 5, 6
def overflow_scene(big_first):
    rng = np.random.Generator(np.random.PCG64(11))
    lo = rng.uniform(0.0, 3.8, (70, 3))
    small = np.stack([lo, lo + rng.uniform(0.05, 0.2, (70, 3))], 2).reshape(70, 6)
    big = np.array([[0.0, 4.0] * 3])                                     # level 4 of 0.25: cell 4
    far = small[:8] + 40.0
    aabb = np.concatenate([big, small, far] if big_first else [small, far, big])
    nested = np.array([[-0.5 - k, 4.5 + k] * 3 for k in range(20)])      # 20 statics around the big body
    return aabb, nested


@pytest.mark.parametrize("big_first", [True, False], ids=["largest-first", "largest-last"])
def test_overflow_both_ways(cuda_device, big_first):
    aabb, nested = overflow_scene(big_first)
    grid = Grid(cuda_device, len(aabb), CELL0, 6, nested)
    want, swant = assert_exact(grid, aabb, nested, "overflow", runs=2)
    big = 0 if big_first else len(aabb) - 1
    assert np.count_nonzero((want == big).any(1)) >= 40
    assert (np.bincount(want[:, 0]).max() > 16) == big_first             # its own list overflows / the small bodies' lists take the pairs
    assert np.count_nonzero(swant[:, 0] == big) == 20 > 16


def test_capacity_cuts_inside_an_overflowing_list(cuda_device):
    aabb, nested = overflow_scene(True)
    grid = Grid(cuda_device, len(aabb), CELL0, 6, nested)
    want, swant = ref.brute_pairs(aabb), ref.brute_static_pairs(aabb, nested)
    assert np.count_nonzero(want[:, 0] == 0) > 25 and np.count_nonzero(swant[:, 0] == 0) > 10
    for cap, scap in ((25, 10), (0, 0), (len(want), len(swant)), (len(want) - 1, 17)):
        pairs, total, spairs, stotal, status = grid.collide(aabb, cap, scap)
        assert (total, stotal, status) == (len(want), len(swant), 0), (cap, scap)
        assert np.array_equal(pairs, want[:cap]) and np.array_equal(spairs, swant[:scap]), (cap, scap)


def test_a_body_above_the_top_level(cuda_device):
    aabb, nested = overflow_scene(True)                                  # the big body's edge is 4 = cell0 * 2^4
    short = Grid(cuda_device, len(aabb), CELL0, 4, nested)               # top cell 2
    assert short.collide(aabb)[4] & 1
    assert_exact(Grid(cuda_device, len(aabb), CELL0, 5, nested), aabb, nested, "one more level")


# ------------------------------------------------------------------------------------------------- 7
def test_one_level_is_todays_object(cuda_device):
    b = synth.sphere_bodies(3000, box=14.0, seed=4)
    aabb, statics = ref.sphere_aabb(b), synth.static_boxes(40, 14.0)
    one, old = Grid(cuda_device, 3000, b["cell"], 1, statics), Grid(cuda_device, 3000, b["cell"], None, statics)
    assert old.L.clapgpu_bp_levels(old.bp) == 1
    got, exp = one.collide(aabb), old.collide(aabb)
    assert got[1] > 3000 and got[3] > 500
    for g, e in zip(got, exp):
        assert np.array_equal(g, e)
    assert np.array_equal(got[0], ref.brute_pairs(aabb)) and np.array_equal(got[2], ref.brute_static_pairs(aabb, statics))
    for k in range(4):                                                   # and a one-level object's slots are today's
        assert one.L.clapgpu_bp_cell_slot(one.bp, 0, 5 * k, -3, 7) == old.L.clapgpu_bp_cell_slot(old.bp, 0, 5 * k, -3, 7)
    assert one.L.clapgpu_bp_cell_slot(one.bp, 1, 0, 0, 0) == 0xffffffff


# ------------------------------------------------------------------------------------------------- 8
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def e2e_bodies():
    b = synth.mixed_bodies(1000, box=20.0, cell0=CELL0, seed=6)
    b["lvel"] = b["lvel"] * 0.2
    r = np.minimum(b["radius"], 3.9)                                     # a moved box's edge rounds: keep it off the top cell (8)
    b.update(radius=r, yoffset=r.copy(), mass=4.0 / 3.0 * np.pi * r ** 3)
    rng = np.random.Generator(np.random.PCG64(8))
    mat = np.stack([rng.choice([0.0, 0.3, 0.8], 1000), rng.uniform(0, 0.2, 1000), rng.uniform(0.1, 1.5, 1000),
                    rng.choice([0.0, 0.02, 0.2], 1000), rng.choice([0.0, 0.005, 0.05], 1000)], 1)
    return b, mixed_statics(30, 20.0), mat


def e2e_world(dev, leveled):
    b, statics, mat = e2e_bodies()
    if not leveled:
        b["cell"] = float(2.0 * b["radius"].max()) * (1.0 + 1e-9)        # the one exact one-level choice: the largest edge
    w = physics.PhysWorld(b, statics, pair_capacity=64_000, device=dev, bp_levels=6 if leveled else 1)
    w.set_materials(mat)
    assert w.bp_levels == (6 if leveled else 1)
    return w


def assert_same_world(a, z, what):
    da, dz = a.download(), z.download()
    assert da["pair_total"] > 100 and da["static_pair_total"] > 100, what
    for k in dz:
        assert same_bits(np.asarray(da[k]), np.asarray(dz[k])), (what, k)


def test_end_to_end_phys_step(cuda_device):
    lev, one = e2e_world(cuda_device, True), e2e_world(cuda_device, False)
    for step in range(12):
        for w in (lev, one):
            assert w.phys_step(1.0 / 120.0, broadphase=True, islands=True, solve=True) == 1
        for name in ("pairs", "static_pairs", "pair_total", "static_pair_total"):
            assert torch.equal(getattr(lev, name), getattr(one, name)), (step, name)
    assert lev.broadphase_status() == 0 and one.broadphase_status() == 0
    assert_same_world(lev, one, "12 substeps")


def frame_loop(dev, leveled):
    from clap_amd import entities, frame, tiler
    raw = synth.entities_flat(1200, seed=5)
    scene, tl = tiler.tiled_scene(raw)
    roots = tl["slot_of"][np.flatnonzero(raw["parent"] < 0)]
    scene["model_lod"] = np.asarray([[0, 3]], np.uint8)
    w = e2e_world(dev, leveled)
    w.body_entity.copy_(torch.from_numpy(roots[:w.n].astype(np.int32)))
    batch = entities.EntityBatch(scene, dev)
    return w, frame.FrameLoop(batch, synth.camera(pos=(0, 10, 60)), world=w, contacts=True, islands=True, solve=True, prebin=True)


def test_end_to_end_frame_with_prebin_and_a_captured_replay(cuda_device):
    (lev, lloop), (one, oloop) = frame_loop(cuda_device, True), frame_loop(cuda_device, False)
    for loop in (lloop, oloop):
        loop._issue(0.0, 12)
    assert_same_world(lev, one, "a frame of 12 substeps, prebin")
    for loop in (lloop, oloop):
        loop.capture(1.0 / 120.0)
        loop.clap_frame_replay(0.0)
    assert_same_world(lev, one, "one replay of a captured frame")
    assert lev.broadphase_status() == 0


# ------------------------------------------------------------------------------------------------- 9
def test_queries_through_a_leveled_object_scan(cuda_device):
    w = e2e_world(cuda_device, True)
    w.bp_index()
    assert w.bp_index_status() & 4
    R = np.random.Generator(np.random.PCG64(3))
    nr = 512
    s, d, L = R.uniform(-2.0, 22.0, (nr, 3)), R.normal(size=(nr, 3)), R.choice([2.0, 10.0, 40.0], nr)
    fetch = lambda out: [t.cpu().numpy() for t in out]
    g, f = fetch(w.ray_cast(s, d, L, grid=True)), fetch(w.ray_cast(s, d, L, grid=False))
    for name, x, y in zip(("dist", "hit", "contact", "flags"), g, f):
        assert same_bits(x, y), name
    assert (g[1] >= 0).any() and (g[1] <= -2).any()
    movers, delta = R.integers(0, w.n, nr).astype(np.uint32), R.normal(0, 0.7, (nr, 3)).astype(np.float32)
    sg, sf = fetch(w.sweep_capsules_grid(movers, delta, grid=True)), fetch(w.sweep_capsules_grid(movers, delta, grid=False))
    for name, x, y in zip(("frac", "normal", "hit", "flags"), sg, sf):
        assert same_bits(x, y), name
    assert (sg[2] != -1).any()
    one = e2e_world(cuda_device, False)
    one.bp_index()
    assert not one.bp_index_status() & 4
