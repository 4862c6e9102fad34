"""GPU: queries through the leveled index of a multi-level broadphase object (clapgpu_bp_leveled_index;
clap_amd/csrc/grid_query_dev.h).  Rays, sweeps, the characters' move, the ordered move and the frame's move stage through
the index against the scan of every geom -- the same object with its switch off, or grid=False -- bit for bit, no
tolerance anywhere; and that the index, not a scan, is what a query reads once the switch is on.

A ray's visit looks up at most 3 x 3 x 3 cells and 2 x 2 x 2 blocks per piece, so its lookup loop goes round once a
piece whatever the scene; a range of more than 64 lookups on one level is met here as the sum over a ray's pieces.  The
record loop goes round more than once at the clump (100 records in one cell)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bplevelref as ref
from clap_amd import _lib, physics, synth
from meshscene import fetch, rng, same_bits
from test_bp_levels_gpu import _slots
from test_move_gpu import assert_same, body_state, make, movers, restore, run_call, sleepy, snapshot
from test_order_gpu import run_ordered

pytestmark = pytest.mark.gpu

CELL0, LEVELS, BOX = 0.25, 6, 24.0
TOP = CELL0 * 2.0 ** (LEVELS - 1)
CLUMP_CELL = np.array([41, 43, 38])                         # the level-0 cell that holds the clump


def mixed(n=500, seed=12, clump=100):
    """n sphere bodies with radii log-uniform in 0.025 .. 3.9 (an edge stays under the top cell, 8) in a BOX cube, and
    `clump` spheres of radius 0.03 with their centres in one level-0 cell"""
    R = rng(seed)
    b = synth.sphere_bodies(n + clump, box=BOX, seed=seed)
    r = np.exp(R.uniform(np.log(0.025), np.log(3.9), n + clump))
    r[n:] = 0.03
    b["pos"][n:] = (CLUMP_CELL + R.uniform(0.1, 0.9, (clump, 3))) * CELL0
    b["lvel"] = b["lvel"] * 0.2
    b.update(radius=r, yoffset=r.copy(), mass=4.0 / 3.0 * np.pi * r ** 3, cell=CELL0)
    return b


def statics():
    return synth.static_boxes(40, BOX, seed=5)              # [0]: a ground slab 2 000 wide, in the large list of every level


def world(dev, leveled_index, b=None, **kw):
    w = physics.PhysWorld(mixed() if b is None else b, statics(), pair_capacity=1 << 16, device=dev, bp_levels=LEVELS,
                          leveled_index=leveled_index, **kw)
    assert w.bp_levels == LEVELS
    return w


def one_level_world(dev, b=None, **kw):
    b = mixed() if b is None else b
    b["cell"] = float(2.0 * b["radius"].max()) * (1.0 + 1e-9)
    return physics.PhysWorld(b, statics(), pair_capacity=1 << 16, device=dev, **kw)


def levels_of(w):
    torch.cuda.synchronize()
    level, over = ref.box_level(w.aabb.cpu().numpy()[:w.n], CELL0, LEVELS)
    return level, over


@pytest.fixture(scope="module")
def scene(cuda_device):
    w = world(cuda_device, True)
    level, over = levels_of(w)
    assert not over.any() and np.count_nonzero(np.bincount(level, minlength=LEVELS)) == LEVELS
    return w, mixed(), level


def assert_same_out(got, want, names, what):
    for name, x, y in zip(names, got, want):
        assert same_bits(x, y), (what, name, np.flatnonzero((np.atleast_2d(x.T) != np.atleast_2d(y.T)).any(0))[:8])


RAY_OUT = ("dist", "hit", "contact", "flags")
SWEEP_OUT = ("frac", "normal", "hit", "flags")


# ------------------------------------------------------------------------------------------------- 1
def test_switch_and_status(cuda_device):
    w = world(cuda_device, False)
    w.bp_index()
    assert w.bp_index_status() & 4                          # as created: nothing is built, queries scan
    w.bp_leveled_index(True)
    with pytest.raises(_lib.ClapGpuError):
        w.bp_index_status()                                 # the switch drops the index
    w.bp_index()
    assert w.bp_index_status() == 0
    w.bp_leveled_index(False)
    with pytest.raises(_lib.ClapGpuError):
        w.bp_index_status()
    w.bp_index()
    assert w.bp_index_status() & 4
    one = one_level_world(cuda_device)
    one.bp_index()
    one.bp_leveled_index(True)                              # accepted, and the index stays
    assert one.bp_index_status() == 0
    assert _lib.lib().clapgpu_bp_leveled_index(None, 1) == _lib.ERR_INVALID_ARGUMENTS


# ------------------------------------------------------------------------------------------------- 2
def aimed_rays(b, level, R, per_level=80):
    """per occupied level, short rays from outside bodies of that level towards their centres"""
    s, d, L = [], [], []
    for l in range(LEVELS):
        ids = np.flatnonzero(level == l)
        ids = ids[R.permutation(len(ids))[:per_level]]
        u = R.normal(size=(len(ids), 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        r = b["radius"][ids, None]
        s.append(b["pos"][ids] + u * (1.5 * r + 0.02))
        d.append(-u)
        L.append(np.full(len(ids), 1.0) * (r[:, 0] + 0.05))
    return np.concatenate(s), np.concatenate(d), np.concatenate(L)


def scene_rays(b, level):
    R = rng(31)
    n = 2048
    s, d, L = R.uniform(-4.0, BOX + 4.0, (n, 3)), R.normal(size=(n, 3)), R.choice([1.0, 3.0, 6.0, 40.0], n)
    k = 0
    for l in range(LEVELS):                                 # in the cell-boundary planes of every level
        c = CELL0 * 2.0 ** l
        for axis in range(3):
            q = slice(k, k + 16)
            s[q, axis] = np.round(s[q, axis] / c) * c
            d[q, axis] = 0.0
            k += 16
    s[k:k + 32, 0] = -30.0                                  # from outside the bounds, into the scene
    d[k:k + 32] = np.abs(d[k:k + 32]) * [1.0, 0.1, 0.1]
    L[k:k + 32] = 36.0
    k += 32
    L[k:k + 32] = R.choice([200.0, 1e6], 32)                # longer than the scene
    k += 32
    # through the clump, along x: more than 64 lookups on level 0 over its pieces, and a cell of 100 records
    s[k:k + 16] = (CLUMP_CELL + [-2.0, 0.5, 0.5]) * CELL0 + np.concatenate([np.zeros((16, 1)), R.uniform(-0.1, 0.1, (16, 2))], 1)
    d[k:k + 16] = [1.0, 0.0, 0.0]
    L[k:k + 16] = 6.0
    k += 16
    d[k:k + 10] = 0.0                                       # zero direction
    d[k + 10:k + 20, 1] = np.nan                            # NaN direction
    L[k + 20:k + 24] = -1.0
    a = aimed_rays(b, level, R)
    return np.concatenate([s, a[0]]), np.concatenate([d, a[1]]), np.concatenate([L, a[2]])


def test_rays_equal_the_scan(scene):
    w, b, level = scene
    s, d, L = scene_rays(b, level)
    skip = np.where(np.arange(len(L)) % 5 == 0, np.arange(len(L)) % w.n, -1).astype(np.int32)
    w.bp_leveled_index(True)
    w.bp_index()
    assert w.bp_index_status() == 0
    g = fetch(w.ray_cast(s, d, L, skip=skip, grid=True))
    f = fetch(w.ray_cast(s, d, L, skip=skip, grid=False))
    # what the scan alone says the rays reach
    hit, flags = f[1], f[3].view(np.uint32)
    per_level = np.bincount(level[hit[hit >= 0]], minlength=LEVELS)
    print("hits per level", per_level, "statics", (hit <= -2).sum(), "misses", (hit == -1).sum())
    assert (per_level >= 20).all(), per_level
    assert (hit <= -2).sum() > 5 and (hit == -1).sum() > 20
    assert (flags & _lib.RAY_INVALID).sum() == 24
    assert (hit >= w.n - 100).sum() >= 4, "the clump is hit"
    assert_same_out(g, f, RAY_OUT, "rays")


# ------------------------------------------------------------------------------------------------- 3
def moved_body_is_missed(w, grid_hits_when_off):
    """after the index, body i's pos moves by +1000 in x (no new box, no new index): a ray through the new place"""
    torch.cuda.synchronize()
    pos, r = w.pos.cpu().numpy(), w.radius.cpu().numpy()
    i = int(np.flatnonzero((pos[:, 1] - r > 3.0) & (r > 0.3) & (r < 1.0))[0])         # its ray ends above the ground slab
    w.bp_index()
    w.pos[i, 0] += 1000.0
    s = pos[i] + [1000.0, r[i] + 0.5, 0.0]
    ray = (s[None], np.array([[0.0, -1.0, 0.0]]), np.array([r[i] + 1.0]))
    assert int(w.ray_cast(*ray, grid=False)[1][0]) == i
    assert int(w.ray_cast(*ray, grid=True)[1][0]) == -1     # the index holds it where it was
    if grid_hits_when_off:
        w.bp_leveled_index(False)
        w.bp_index()
        assert int(w.ray_cast(*ray, grid=True)[1][0]) == i  # the scan
        w.bp_leveled_index(True)


def test_the_index_is_what_is_read(cuda_device):
    moved_body_is_missed(world(cuda_device, True, geom_records=False), True)
    moved_body_is_missed(one_level_world(cuda_device, geom_records=False), False)     # the control of the observable


# ------------------------------------------------------------------------------------------------- 4
def test_a_slot_shared_across_levels(cuda_device):
    b = mixed(n=3, clump=0)
    w = world(cuda_device, True, b=b)                       # only for its object: the slots of this bucket count
    L = _lib.lib()
    big_cell = np.array([2, 3, 2])                          # a level-2 cell (size 1)
    cells = np.stack(np.meshgrid(np.arange(96), np.arange(96), np.arange(96), indexing="ij"), -1).reshape(-1, 3)
    want = L.clapgpu_bp_cell_slot(w._bp, 2, *[int(v) for v in big_cell])
    assert want == int(_slots(2, big_cell, 1023))
    cand = cells[_slots(0, cells, 1023) == want]
    cand = cand[(np.abs((cand + 0.5) * CELL0 - (big_cell + 0.5)) > 2.0).any(1)]         # away from the big body
    assert len(cand), "no level-0 cell in the scene shares the level-2 cell's slot"
    small_cell = cand[0]
    assert L.clapgpu_bp_cell_slot(w._bp, 0, *[int(v) for v in small_cell]) == want
    b["pos"][0], b["radius"][0] = (small_cell + 0.5) * CELL0, 0.1          # level 0
    b["pos"][1], b["radius"][1] = big_cell + 0.5, 0.4                      # level 2: an edge of 0.8
    b["pos"][2], b["radius"][2] = b["pos"][0] + [0.15, 0.0, 0.0], 0.1      # a level-0 neighbour that overlaps body 0
    b["yoffset"] = b["radius"].copy()
    w = world(cuda_device, True, b=b)
    level, _ = levels_of(w)
    assert list(level) == [0, 2, 0]
    w.bp_index()
    assert w.bp_index_status() == 0
    R = rng(5)
    ids = np.repeat(np.arange(3), 32)
    u = R.normal(size=(96, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    s = b["pos"][ids] + u * (b["radius"][ids, None] * 2.0 + 0.1)
    length = np.where(np.arange(96) % 2 == 0, 0.5, 3.0) + b["radius"][ids]
    g, f = fetch(w.ray_cast(s, -u, length, grid=True)), fetch(w.ray_cast(s, -u, length, grid=False))
    assert all((f[1] == i).sum() > 10 for i in range(3))
    assert_same_out(g, f, RAY_OUT, "shared slot, rays")
    sweep_ids = np.tile(np.arange(3), 16).astype(np.uint32)
    delta = R.normal(0, 0.3, (48, 3)).astype(np.float32)
    delta[0] = [0.3, 0.0, 0.0]                              # body 0 into its neighbour
    delta[2] = [-0.3, 0.0, 0.0]
    w.bp_index()
    sg = fetch(w.sweep_capsules_grid(sweep_ids, delta, grid=True))
    sf = fetch(w.sweep_capsules_grid(sweep_ids, delta, grid=False))
    assert (sf[2] >= 0).sum() >= 2
    assert_same_out(sg, sf, SWEEP_OUT, "shared slot, sweeps")


# ------------------------------------------------------------------------------------------------- 5
def test_a_body_above_the_top_level(cuda_device):
    b = mixed()
    b["radius"][7] = 0.9 * TOP                              # an edge of 1.8 top cells, above the rest, its centre at 0.95 of a cell in x
    b["pos"][7] = [1.95 * TOP, 100.0, 10.0]
    w = world(cuda_device, True, b=b)
    w.bp_index()
    assert w.bp_index_status() == 1
    # straight down through its rim, 0.85 of a top cell from its centre in x: the top level's cells of the ray start past
    # the centre's cell, so only the scan of every geom finds it
    s = b["pos"][7] + np.stack([np.full(16, 0.85 * TOP), np.full(16, 3.0), np.linspace(-0.2, 0.2, 16) * TOP], 1)
    d, L = np.tile([0.0, -1.0, 0.0], (16, 1)), np.full(16, 5.0)
    assert np.floor((s[0, 0] - 0.5 * TOP * (1 + 1e-9)) / TOP) > np.floor(b["pos"][7][0] / TOP)
    g, f = fetch(w.ray_cast(s, d, L, grid=True)), fetch(w.ray_cast(s, d, L, grid=False))
    assert (f[1] == 7).all()
    assert_same_out(g, f, RAY_OUT, "oversized")
    w.radius[7] = 0.1
    w.bodies_aabb()
    w.broadphase()
    w.bp_index()
    assert w.bp_index_status() == 0


# ------------------------------------------------------------------------------------------------- 6
def test_a_stale_or_missing_index_is_refused(cuda_device):
    w = world(cuda_device, True)
    ray = (np.zeros((4, 3)), np.tile([0, -1.0, 0], (4, 1)), np.ones(4))
    with pytest.raises(_lib.ClapGpuError):
        w.ray_cast(*ray, grid=True)                         # never indexed
    w.bp_index()
    w.ray_cast(*ray, grid=True)
    w.broadphase()
    with pytest.raises(_lib.ClapGpuError):
        w.ray_cast(*ray, grid=True)                         # a collide since
    w.bp_index()
    w.bp_invalidate()
    with pytest.raises(_lib.ClapGpuError):
        w.ray_cast(*ray, grid=True)
    w.bp_index()
    n = w.n
    w.n = n - 1
    with pytest.raises(_lib.ClapGpuError):
        w.ray_cast(*ray, grid=True)                         # another body count
    w.n = n
    w.ray_cast(*ray, grid=True)


# ------------------------------------------------------------------------------------------------- 7
def test_sweeps_equal_the_scan(scene):
    w, b, level = scene
    R = rng(41)
    per = 512 // LEVELS + 1
    ids = np.concatenate([R.choice(np.flatnonzero(level == l), per) for l in range(LEVELS)])[:512].astype(np.uint32)
    delta = (R.normal(0, 0.7, (512, 3)) * np.maximum(b["radius"][ids, None], 0.3)).astype(np.float32)
    # a level-4 mover's swept box covers (edge / 0.25 + 1)^3 > 700 cells of level 0: over the cap, it scans
    assert (level[ids] == 4).sum() > 50 and 64 + (w.n + w.n_static) / 64 < 100
    w.bp_leveled_index(True)
    w.bp_index()
    sg = fetch(w.sweep_capsules_grid(ids, delta, grid=True))
    sf = fetch(w.sweep_capsules_grid(ids, delta, grid=False))
    print("sweep hits per mover level", np.bincount(level[ids][sf[2] != -1], minlength=LEVELS))
    assert (sf[2] >= 0).sum() > 20                          # some sweeps hit
    assert_same_out(sg, sf, SWEEP_OUT, "sweeps")


# ------------------------------------------------------------------------------------------------- 8
@pytest.fixture(scope="module")
def movers_world(cuda_device):
    b = mixed()
    w = world(cuda_device, False, b=b, forces=True)
    sleepy(w, 7)
    w.bodies_aabb()
    return w, b, snapshot(w)


def test_characters_move_is_the_scans(movers_world):
    w, b, snap = movers_world
    mv = movers(b, rng(3).choice(w.n, 256, replace=False), 9, speed=2.0)
    res = []
    for on in (False, True):
        restore(w, snap)
        w.bp_leveled_index(on)
        res.append(run_call(w, mv))
    assert_same(res[1], res[0], "characters_move, switch on against off")
    out = res[0][0]
    assert (out["applied"] != 0).sum() > 10


def test_ordered_move_is_the_scans(movers_world):
    w, b, snap = movers_world
    mv = movers(b, rng(4).choice(w.n, 32, replace=False), 10, speed=2.0)
    res = []
    for on in (False, True):
        restore(w, snap)
        w.bp_leveled_index(on)
        res.append(run_ordered(w, mv))
    assert_same(res[1][:2], res[0][:2], "characters_move_ordered, switch on against off")
    assert same_bits(res[1][2], res[0][2]) and res[1][3] == res[0][3]


# ------------------------------------------------------------------------------------------------- 9
def frame_setup(dev, on):
    from clap_amd import entities, frame, tiler
    raw = synth.entities_flat(900, seed=5)
    scene, tl = tiler.tiled_scene(raw)
    roots = tl["slot_of"][np.flatnonzero(raw["parent"] < 0)]
    scene["model_lod"] = np.asarray([[0, 3]], np.uint8)
    b = mixed()
    chars = rng(7).choice(b["n"], 100, replace=False).astype(np.uint32)
    b["body_entity"][:] = -1
    dyn = np.setdiff1d(np.arange(b["n"]), chars)[:300]
    b["body_entity"][dyn] = roots[:300]
    batch = entities.EntityBatch(scene, dev)
    w = world(dev, on, b=b, forces=True)
    m = make(w, movers(b, chars, 15, speed=2.0), entity=roots[300:400].astype(np.uint32), entity_batch=batch)
    m.set(yaw_quat=rng(16).normal(0, 1, (100, 4)).astype(np.float32))
    return w, batch, m, frame.FrameLoop(batch, synth.camera(pos=(0, 10, 60)), world=w, contacts=True, move=m)


def test_frames_with_the_move_stage(cuda_device):
    (wa, ba, ma, loop_a), (wb, bb, mb, loop_b) = frame_setup(cuda_device, True), frame_setup(cuda_device, False)
    now = 3.0
    for f, dt in enumerate((1 / 60, 1 / 120, 0.03)):
        now += dt
        for loop in (loop_a, loop_b):
            loop.clap_frame(now, dt)
        sa, sb = body_state(wa), body_state(wb)
        sa.update({"move_" + k: t.cpu().numpy() for k, t in ma.outputs().items()})
        sb.update({"move_" + k: t.cpu().numpy() for k, t in mb.outputs().items()})
        sa.update({"e_" + k: v for k, v in ba.download().items() if isinstance(v, np.ndarray)})
        sb.update({"e_" + k: v for k, v in bb.download().items() if isinstance(v, np.ndarray)})
        for k in sa:
            assert same_bits(sa[k], sb[k]), (f, k)
    assert (sa["move_applied"] != 0).sum() > 10
    # an index between two collides leaves the pair lists as they are without it
    def lists(w):
        d = w.download()
        return d["pairs"], d["static_pairs"], d["pair_total"], d["static_pair_total"]
    wa.bodies_aabb()
    wa.broadphase()
    before = lists(wa)
    wa.bp_index()
    assert wa.bp_index_status() == 0
    wa.broadphase()
    after = lists(wa)
    assert before[2] > 100 and before[3] > 100
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert wa.broadphase_status() == 0


# ------------------------------------------------------------------------------------------------- 10
def test_no_bodies(cuda_device):
    L = _lib.lib()
    st = np.ascontiguousarray(statics())
    bp = C.c_void_p()
    _lib.check(L.clapgpu_bp_create_levels(C.byref(bp), 0, CELL0, LEVELS, len(st), st.ctypes.data), "clapgpu_bp_create_levels")
    try:
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(L.clapgpu_bp_leveled_index(bp, 1), "clapgpu_bp_leveled_index")
        _lib.check(L.clapgpu_bp_index(stream, bp, 0, None), "clapgpu_bp_index")
        status = C.c_uint32(9)
        _lib.check(L.clapgpu_bp_index_status(stream, bp, C.byref(status)), "clapgpu_bp_index_status")
        assert status.value == 0
        R = rng(6)
        n = 512
        ray = np.zeros((n, 8))
        ray[:, 0:3], ray[:, 3:6], ray[:, 6] = R.uniform(-2.0, BOX + 8.0, (n, 3)), R.normal(size=(n, 3)), R.choice([2.0, 6.0, 60.0], n)
        ray[:64, 3:6] = [0.0, -1.0, 0.0]                    # onto the ground slab (the large list), unless a box is in the way
        ray[:64, 1], ray[:64, 6] = np.abs(ray[:64, 1]) + 1.0, 60.0
        ray_d = torch.from_numpy(ray).to(cuda_device)
        kind = torch.full((len(st),), _lib.GEOM_BOX, dtype=torch.uint8, device=cuda_device)
        bodies = _lib.Geoms(0, 0, 0, 0, 0, 0, 0, 0, 0)
        sg = _lib.Geoms(len(st), 0, 0, 0, 0, 0, kind.data_ptr(), L.clapgpu_bp_static_aabb(bp), 0)
        out = []
        for grid in (True, False):
            dist = torch.full((n,), float("nan"), dtype=torch.float64, device=cuda_device)
            contact = torch.full((n, 6), float("nan"), dtype=torch.float64, device=cuda_device)
            hit, flags = torch.zeros(n, dtype=torch.int32, device=cuda_device), torch.zeros(n, dtype=torch.int32, device=cuda_device)
            _lib.check(L.clapgpu_ray_cast(stream, bp if grid else None, C.byref(bodies), C.byref(sg), None, n, ray_d.data_ptr(), None,
                                          dist.data_ptr(), hit.data_ptr(), contact.data_ptr(), flags.data_ptr()), "clapgpu_ray_cast")
            out.append(fetch((dist, hit, contact, flags)))
        assert (out[1][1] == -2).sum() >= 8 and (out[1][1] < -2).sum() > 20 and (out[1][1] == -1).sum() > 20
        assert_same_out(out[0], out[1], RAY_OUT, "no bodies")
    finally:
        L.clapgpu_bp_destroy(bp)
