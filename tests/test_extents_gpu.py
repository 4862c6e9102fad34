"""GPU: WHERE every kernel family writes.  Each test installs tests/guards.py's hook, so that every device array the
host mirrors allocate (outputs, scratch and uploaded inputs) sits between two 4096-byte bands of 0xA5, builds its scene
at the counts where tails go wrong (1, 63, 65, 257: around a wavefront and a 256-thread workgroup; list capacities total,
total - 1 and 0), runs the calls, and asserts both what the family's own test asserts about the values (same oracle,
same strictness, imported from that test, not restated) and that no band was touched.

Where a descriptor was once re-pointed by hand, held() asserts that the mirror's array is under guard and that the
descriptor holds its address.  Not covered: tensors a test builds itself unless it guards them (guard_like), the .clone()
snapshots of the imported helpers (host comparison only), upload of what is already a tensor, and the arrays the library
allocates for itself (broadphase objects, mesh sets, the stream-ordered array between the two ray passes).
One test, and only one, passes a wrong extent on purpose, to show that the instrument sees one pair past the end."""
import ctypes as C

import numpy as np
import pytest
import torch

import guards
from clap_amd import _lib, entities, synth, tiler
from clap_amd._dev import upload
from oracle import binding as ob
from helpers import apply_frame, assert_bits_equal

pytestmark = pytest.mark.gpu

COUNTS = [1, 63, 65, 257]


@pytest.fixture
def g(cuda_device, monkeypatch):
    """The registry of the test, with the hook installed under the mirrors."""
    reg = guards.Guards(cuda_device)
    guards.install(monkeypatch, reg)
    return reg


def held(g, obj, names, desc=None, desc_names=None):
    """obj.<name> is an array under guard and desc.<field> holds its address.  The field must be one of the descriptor's:
    a ctypes structure takes any attribute name without a word.  Returns obj."""
    fields = None if desc is None else {f[0] for f in type(desc)._fields_}
    for k, name in enumerate(names):
        t = getattr(obj, name)
        if t is None:
            continue
        assert g.owns(t), f"{type(obj).__name__}.{name} is not under guard"
        if desc is not None:
            field = (desc_names or names)[k]
            assert field in fields, f"{type(desc).__name__} has no field {field!r}"
            assert getattr(desc, field) == t.data_ptr(), f"{type(desc).__name__}.{field} does not hold {name}"
    return obj


def held_entities(g, batch):
    """held() for an EntityBatch's inputs."""
    return held(g, held(g, batch, batch.IN_KEYS + ("model_table",), batch._desc), ("tile_row_start",) if batch.tiled else ())


def untouched(t, fill, what):
    """A whole array still holds `fill` (entry points that return early)."""
    assert bool((t == fill).all().item()), f"{what}: written by a call that had nothing to do"


# ------------------------------------------------------------------------------------------------------ entities
from test_entities_gpu import EXTRA_CAMS, check_against, lay_out, oracle_frame      # noqa: E402

ENTITY_SCENES = {"rows1": lambda: synth.entities_flat(1, 5), "rows2": lambda: synth.entities_flat(65, 7),
                 "rows5": lambda: synth.entities_flat(257, 8), "rows5_deep": lambda: synth.entities_chains(13, 5, 9)}


@pytest.mark.parametrize("n_extra", [1, 4], ids=["views1", "views4"])
@pytest.mark.parametrize("layout", ["levels", "tiles"])
@pytest.mark.parametrize("name", list(ENTITY_SCENES))
def test_entity_update_cull_compact_and_lod(name, layout, n_extra, g, cuda_device):
    scene = lay_out(ENTITY_SCENES[name](), layout)
    scene["model_lod"] = np.tile(np.asarray([[0, 3]], np.uint8), (int(scene["model"].max()) + 1, 1))
    n = scene["n"]
    assert (n + 63) // 64 == int(name[4]), "the scene's rows of 64"
    cam = synth.camera()
    cams = [synth.camera(**kw) for kw in EXTRA_CAMS[:n_extra]]
    fr = entities.view_calc_frustum(cam)[0]
    fr_o = ob.frustum_from_camera(cam)[0]
    frs_o = [ob.frustum_from_camera(c)[0] for c in cams]
    st = ob.entity_state(scene)
    batch = held_entities(g, entities.EntityBatch(scene, cuda_device))
    batch.set_views([entities.view_calc_frustum(c)[0] for c in cams])
    alive = np.flatnonzero(scene["flags"] & synth.E_ALIVE)
    last_row = alive[alive >= (alive.max() // 64) * 64]
    rng = np.random.Generator(np.random.PCG64(3))
    cur = np.zeros(n, np.int32)
    for frame in range(3):
        if frame:                                   # frame 1: only the last row is dirty; frame 2: a subset ending in it
            idx = last_row if frame == 1 else np.union1d(alive[::3], last_row[-1:])
            ps = scene["pos_scale"].copy()
            ps[idx, :3] += rng.uniform(-3, 3, (idx.size, 3)).astype(np.float32)
            dirty = np.zeros(n, bool)
            dirty[idx] = True
            apply_frame(scene, st, (ps, scene["rot"], dirty))
            batch.set_transforms(idx, ps[idx], scene["rot"][idx])
        vis, mask = oracle_frame(scene, st, fr_o)
        batch.mq_update(fr)
        batch.compact_visible()
        what = f"{name} {layout} frame {frame}"
        check_against(batch.download(), st, vis, mask, what)
        g.check(what + " update + compact")
        for v, fo in enumerate(frs_o):
            vis_v, mask_v = ob.entities_cull(n, st["flags"], st["aabb"], fo)
            assert np.array_equal(batch.view_masks[v].cpu().numpy().view(np.uint64)[:mask_v.size], mask_v), f"{what} view {v} mask"
            batch.compact_view(v)
            assert np.array_equal(batch.download()["visible"], vis_v), f"{what} view {v} list"
        batch.compact_visible(index_base=7, two_pass=True)
        out = batch.download()
        assert np.array_equal(out["visible"], vis + 7) and out["visible_count"] == vis.size, what + " two-pass list"
        draw = ob.entities_lod(scene, st, vis, cam["cam_pos"], scene["model_lod"], np.full(n, -1, np.int32), cur)
        batch.visible.fill_(-1)
        batch.compact_visible_lod(cam["cam_pos"])
        torch.cuda.synchronize()
        assert int(batch.visible_count.item()) == len(vis)
        assert np.array_equal(batch.visible[:len(vis)].cpu().numpy().view(np.uint32), vis), what + " fused list"
        assert bool((batch.visible[len(vis):] == -1).all().item()), what + " fused list: written past the count"
        assert np.array_equal(batch.draw_lod[:len(vis)].cpu().numpy(), draw), what + " draw LODs"
        assert np.array_equal(batch.cur_lod.cpu().numpy()[:n], cur), what + " cur_lod"
        g.check(what + " views, two-pass, lod")
    # the stand-alone cull pass and the all-dirty mode
    batch.cull(fr)
    st["flags"] |= np.where(st["flags"] & synth.E_ALIVE, synth.E_DIRTY, 0).astype(np.uint32)
    vis, mask = oracle_frame(scene, st, fr_o)
    batch.mq_update(fr, all_dirty=True)
    batch.compact_visible()
    check_against(batch.download(), st, vis, mask, f"{name} {layout} all dirty", check_flags=False)
    g.check(f"{name} {layout} cull + all dirty")


# ------------------------------------------------------------------------------------------------------ pose and skin
from test_pose_skin_gpu import assert_pose_equal, oracle_pose                        # noqa: E402
from helpers import assert_vec_equal                                                 # noqa: E402


@pytest.mark.parametrize("n", [1, 3, 5], ids=["1char", "3chars", "5chars"])
@pytest.mark.parametrize("J", [1, 40, 64, 100, 200])
def test_pose_palette_joint_positions_and_skin(J, n, g, cuda_device):
    """A block takes 4 characters; rows of J joints are clipped by buffer descriptors; vertex counts are ragged, one
    character has 1 vertex and the total is 1 mod 4 (float4 stores into [total][3] arrays)."""
    from clap_amd import animation
    sk = synth.skeleton(J, min(8, J), seed=31)
    an0 = synth.animation(J, 30, 2.0, seed=31, ragged=True)
    an1 = synth.animation(J, 2, 1.0, seed=32)
    ch = synth.characters(n, J, seed=31)
    sk["bind"] = ob.skeleton_bind(sk)
    vc = np.asarray([1, 70, 130, 63, 65][:n], np.uint32)
    vc[-1] += (1 - int(vc.sum())) % 4
    assert int(vc.sum()) % 4 == 1 and vc[0] == 1
    mesh = synth.skinned_mesh(int(vc.sum()), J, seed=3)
    vf = np.concatenate([[0], np.cumsum(vc[:-1])]).astype(np.uint32)
    rng = np.random.default_rng(5)
    perm = rng.permutation(n + 7).astype(np.uint32)[:n]
    ent_mx = rng.standard_normal((n + 7, 16)).astype(np.float32)
    model = animation.SkinnedModel(sk, [an0, an1], mesh=mesh, bind=sk["bind"], device=cuda_device)
    batch = animation.CharacterBatch(model, n, ch["trs0"], ent_mx, entity_index=perm, vert_first=vf, vert_count=vc)
    which = (np.arange(n) % 4 == 1).astype(np.int32)
    t = ((ch["phase"] * 1.3) - 0.2).astype(np.float32)
    trs = np.tile(ch["trs0"], (n, 1, 1))
    jt, _gl, jp = oracle_pose(sk, (an0, an1), which, t, ent_mx[perm], trs)
    batch.set_frame_times(t, which)
    reach = sk["order"]
    what = f"J={J} n={n}"
    for trs_on, pos_on in ((True, True), (False, False)):
        batch.trs.copy_(torch.from_numpy(np.tile(ch["trs0"], (n, 1, 1))))
        batch.set_outputs(trs=trs_on, joint_pos=pos_on)
        batch.pose_update()
        assert_pose_equal(batch.download(), trs, jt, jp, reach, what, trs_on=trs_on, pos_on=pos_on)
        g.check(f"{what} pose_update trs={trs_on} pos={pos_on}")
    # the pose stops at model space, joint_pos_world finishes (model.c:1400)
    fused = batch.download()["joint_pos"]
    batch.set_outputs()
    batch.set_joint_pos_model_space(True)
    batch.pose_update()
    batch.joint_pos_world()
    torch.cuda.synchronize()
    assert np.array_equal(batch.download()["joint_pos"][:, reach], fused[:, reach]), what + " joint_pos_world"
    g.check(what + " joint_pos_world")
    # skin, without and with out_w
    exp = ob.skin(mesh, vf, vc, jt, with_w=True)
    batch.skin()
    out = batch.download()
    assert_vec_equal(out["out_position"], exp[0], what + " skinned positions", key="pose -> skin position")
    assert_vec_equal(out["out_normal"], exp[1], what + " skinned normals", key="pose -> skin normal")
    g.check(what + " skin")
    batch.set_skin_w(True)
    batch.skin()
    out = batch.download()
    assert_bits_equal(out["out_position"], exp[0], what + " positions (w on)")
    assert_bits_equal(out["out_normal"], exp[1], what + " normals (w on)")
    assert_bits_equal(out["out_w"], exp[2], what + " total_local_pos.w")
    g.check(what + " skin with out_w")


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_animation_clock(n, g, cuda_device):
    from clap_amd import animation
    sk = synth.skeleton(16, 4, seed=5)
    an = synth.animation(16, 6, 1.5, seed=5)
    ch = synth.characters(n, 16, seed=5)
    sk["bind"] = ob.skeleton_bind(sk)
    model = animation.SkinnedModel(sk, [an], bind=sk["bind"], device=cuda_device)
    batch = animation.CharacterBatch(model, n, ch["trs0"], ch["char_mx"])
    repeat = (np.arange(n) % 2).astype(np.uint8)
    start = np.linspace(0, 1, n)
    speed = np.full(n, 1.25, np.float32)
    batch.start_clock(ani_time=start, speed=speed, repeat=repeat)
    held(g, batch, ("repeat_dev", "time_end_dev"), batch._clock, ("restart", "time_end"))
    ani = start.copy()
    te = np.asarray(model.time_end, np.float32)
    trs = np.tile(ch["trs0"], (n, 1, 1))
    for now in (1.0, 1.7, 2.9):
        ft, ended = ob.animation_time(np.zeros(n, np.uint32), te, ani, speed, repeat, now)
        batch.animated_update(now)
        clk = batch.download_clock()
        assert np.array_equal(clk["ani_time"], ani) and np.array_equal(clk["ended"], ended)
        assert np.array_equal(clk["frame_time"].view(np.uint32), ft.view(np.uint32)), f"n={n} now={now} frame_time"
        jt, _gl, jp = ob.pose(sk, an, ft, ch["char_mx"], trs)
        assert_pose_equal(batch.download(), trs, jt, jp, sk["order"], f"n={n} now={now}")
        g.check(f"clock n={n} now={now}")


# ------------------------------------------------------------------------------------------------------ particles
@pytest.mark.parametrize("kw", [
    dict(n_sys=1, count=1, radius=1.0, velocity=2.0),
    dict(n_sys=3, count=65, radius=2.0, velocity=0.7),
    dict(n_sys=5, count=257, radius=3.0, velocity=0.9, ragged=True, seed=9),
    dict(n_sys=3, count=65, radius=1e-3, velocity=1.0),
], ids=["1x1", "3x65", "ragged", "all_respawn"])
@pytest.mark.parametrize("groups", [True, False], ids=["group_counts", "no_group_counts"])
def test_particles(kw, groups, g, cuda_device):
    from clap_amd import particles
    ps = synth.particle_systems(**kw)
    pos, vel, st = ob.particles_spawn(ps, 0x00C0FFEE1234)
    view = np.asarray(ob.frustum_from_camera(synth.camera(pos=(4, 5, 6)))[1])
    batch = particles.ParticleBatch(ps, pos, vel, st, cuda_device)
    held(g, batch, ("sys", "rng_state"), batch._desc)
    if not groups:
        batch._desc.respawn_groups = None
    total = 0
    for f in range(4):
        k, st = ob.particles_update(ps, pos, vel, st)
        total += k
        batch.particles_update(view)
        out = batch.download()
        assert out["respawned"] == k, f"frame {f} respawn count"
        assert_bits_equal(out["pos"], pos, f"frame {f} pos_array")
        assert_bits_equal(out["vel"], vel, f"frame {f} velocity")
        assert out["rng_state"] == st, f"frame {f} drand48 state"
        for s in range(batch.n_sys):
            assert_bits_equal(out["billboard_mx"][s], ob.particles_billboard(view, ps["sys"]["center"][s]), f"frame {f} billboard {s}")
        g.check(f"particles frame {f}")
    assert total > 0
    if kw["radius"] < 1e-2:
        assert total >= 3 * ps["n_real"], "everything respawns every frame"


# ------------------------------------------------------------------------------------------------------ lights
@pytest.mark.parametrize("nl", [1, 128], ids=["1light", "128lights"])
@pytest.mark.parametrize("w,h,cell", [(1, 1, 64), (65, 1, 64), (2599, 1499, 8)], ids=["1x1", "65x1", "2599x1499c8"])
def test_light_grid(w, h, cell, nl, g, cuda_device):
    from clap_amd import lights as gl
    src = synth.lights(nl, seed=31, inactive_frac=0.0)
    _fr, vm, pm = ob.frustum_from_camera(synth.camera(pos=(0, 3, 10)))
    ls = gl.LightSet(cuda_device, w, h, cell)
    ls.load(src)
    exp = ob.light_grid_compute(src, vm, pm, w, h, cell)
    assert exp.shape[:2] == {(1, 1): (1, 1), (65, 1): (1, 2)}.get((w, h), ((h + cell - 1) // cell, (w + cell - 1) // cell))
    for _ in range(2):
        ls.grid_compute(vm, pm)
        assert ls.tiles.shape == exp.shape and np.array_equal(ls.download_tiles(), exp)
        g.check(f"light grid {w}x{h} cell {cell}, {nl} lights")
    assert exp.any()


@pytest.mark.parametrize("nc", COUNTS)
def test_lights_from_entities(nc, g, cuda_device):
    from clap_amd import lights as gl
    scene = synth.pad_levels(synth.entities_chains(300, 2, seed=5))
    L = synth.lights(128, seed=3, inactive_frac=0.0)
    L["active"][5] = 0
    R = np.random.Generator(np.random.PCG64(nc))
    roots, kids = np.flatnonzero(scene["parent"] < 0), np.flatnonzero(scene["parent"] >= 0)
    ent = np.sort(np.concatenate([R.choice(roots, nc - nc // 8, replace=False), R.choice(kids, nc // 8, replace=False)]))
    carriers = dict(entity=ent.astype(np.uint32), light=R.integers(-1, 130, nc).astype(np.int32),       # bad slots are skipped
                    off=R.normal(size=(nc, 3)).astype(np.float32))
    scene["flags"] = scene["flags"].copy()
    scene["flags"][roots[::3]] &= ~np.uint32(_lib.E_DIRTY)
    dirty = ((scene["flags"] & _lib.E_DIRTY) != 0).astype(np.uint8)
    batch = held_entities(g, entities.EntityBatch(scene, cuda_device))
    ls = gl.LightSet(cuda_device, 640, 360, 64)
    ls.set_carriers(carriers["entity"], carriers["light"], carriers["off"])
    for all_dirty in (False, True):
        ls.load(L)
        ls.from_entities(batch, all_dirty=all_dirty)
        exp = ob.lights_from_entities(carriers, scene["pos_scale"], scene["parent"], np.ones_like(dirty) if all_dirty else dirty, L)
        assert np.array_equal(ls.download_pos()[:128], exp), (nc, all_dirty)
        g.check(f"lights_from_entities, {nc} carriers, all_dirty={all_dirty}")


# ------------------------------------------------------------------------------------------------------ broadphase
from test_physics_gpu import _assert_state_equal, _materials, _oracle_body_geoms, oracle_aabbs      # noqa: E402

H = 1.0 / 120.0


def dense_bodies(n, kind="spheres", seed=6):
    """n bodies crowded into a small cube: more partners than a body's fixed list slot holds (BP_LIST = 16)"""
    side = max(1.0, (n / 40.0) ** (1.0 / 3.0))
    return synth.sphere_bodies(n, box=side, seed=seed) if kind == "spheres" else synth.capsule_bodies(n, box=1.6 * side, seed=seed)


def nested_statics():
    statics = synth.static_boxes(45, 8.0, seed=2)
    for s_ in range(40):                                    # 40 nested boxes around the bodies: more hits than the kept list
        statics[s_] = [-1.0, 3.0 + 0.05 * s_, -1.0, 3.0 + 0.05 * s_, -1.0, 3.0 + 0.05 * s_]
    return statics


def capacities(total):
    return sorted({total, max(total - 1, 0), 0}, reverse=True)


@pytest.mark.parametrize("levels", [1, 3], ids=["one_level", "three_levels"])
@pytest.mark.parametrize("n", COUNTS)
def test_broadphase_lists_at_the_three_capacities(n, levels, g, cuda_device):
    from clap_amd import physics
    b = dense_bodies(n)
    if levels > 1:
        b["cell"] = b["cell"] / 2.0 ** (levels - 1)         # the level-0 cell; the top level's is the one-level cell
    statics = nested_statics()
    bb = oracle_aabbs(b)
    exp = ob.broadphase_aabb_pairs(bb, max_pairs=1 << 20)
    exp_s = ob.broadphase_aabb_static_pairs(statics, bb, max_pairs=1 << 20)
    per_static = np.bincount(exp_s[:, 0], minlength=n)
    assert per_static.max() > 16, "no static list overflows the kept list"
    if n > 1:
        assert np.bincount(exp[:, 0], minlength=n).max() > 16 and len(exp) > 2 * n, "no body list overflows the kept list"
    for cap, scap in zip(capacities(len(exp)) + [0] * 2, capacities(len(exp_s))):
        world = physics.PhysWorld(b, statics, pair_capacity=cap, static_pair_capacity=scap, device=cuda_device, bp_levels=levels)
        assert world.pairs.shape == (cap, 2) and world.static_pairs.shape == (scap, 2)
        for run in range(2):                                # twice: the counters the kernels leave behind are clean
            world.broadphase()
            out = world.download()
            what = f"n={n} levels={levels} cap=({cap}, {scap}) run {run}"
            assert np.array_equal(out["aabb"].view(np.uint64), bb.view(np.uint64)), what + " geom AABBs"
            assert out["pair_total"] == len(exp) and out["static_pair_total"] == len(exp_s), what
            assert np.array_equal(out["pairs"], exp[:cap]), what + ": the head of the ascending list"
            assert np.array_equal(out["static_pairs"], exp_s[:scap]), what + ": the head of the ascending static list"
            assert world.broadphase_status() == 0
            g.check(what)


@pytest.mark.parametrize("levels", [1, 3], ids=["one_level", "three_levels"])
@pytest.mark.parametrize("n", COUNTS)
def test_step_prebin_and_bp_index(n, levels, g, cuda_device):
    from clap_amd import physics
    b = dense_bodies(n, "capsules")
    one_level_cell = b["cell"] * 1.25                       # moved boxes of turned capsules stay under the cell
    b["cell"] = one_level_cell / 2.0 ** (levels - 1)
    statics = nested_statics()
    world = physics.PhysWorld(b, statics, pair_capacity=64 * n + 64, static_pair_capacity=64 * n, device=cuda_device, bp_levels=levels)
    st = ob.bodies_state(b)
    ob.bodies_aabb(b, st)
    for step in range(3):
        ob.bodies_step(b, st, H)
        world.world_step(H, prebin=True)
        world.broadphase()
        out = world.download()
        _assert_state_equal(out, st)
        exp = ob.broadphase_aabb_pairs(st["aabb"], max_pairs=1 << 20)
        exp_s = ob.broadphase_aabb_static_pairs(statics, st["aabb"], max_pairs=1 << 20)
        assert out["pair_total"] == len(exp) and np.array_equal(out["pairs"], exp), (n, levels, step)
        assert out["static_pair_total"] == len(exp_s) and np.array_equal(out["static_pairs"], exp_s), (n, levels, step)
        assert world.broadphase_status() == 0
        g.check(f"prebin n={n} levels={levels} step {step}")
    world.bp_index()
    R = np.random.Generator(np.random.PCG64(3))
    nr = 65
    s, d, L = R.uniform(-1.0, 4.0, (nr, 3)), R.normal(size=(nr, 3)), R.choice([2.0, 10.0], nr)
    a, z = world.ray_cast(s, d, L, grid=True), world.ray_cast(s, d, L, grid=False)
    for name, x, y in zip(("dist", "hit", "contact", "flags"), a, z):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (n, levels, name)
    assert bool((a[1] != -1).any().item())
    g.check(f"bp_index + rays n={n} levels={levels}")


def test_the_instrument_sees_one_pair_past_the_end(g, cuda_device):
    """The one place a wrong extent is passed on purpose: clapgpu_bp_collide told capacity + 1 for a list of `capacity`
    pairs, in a scene with more pairs than that.  The pair written behind the array lands in the test's own band."""
    from clap_amd import physics
    n = 120                                                 # indices below 0xA5: no byte of the stray pair equals the poison
    b = dense_bodies(n)
    exp = ob.broadphase_aabb_pairs(oracle_aabbs(b), max_pairs=1 << 20)
    cap = 65
    assert len(exp) > cap + 1
    world = physics.PhysWorld(b, None, pair_capacity=cap, device=cuda_device)
    world.broadphase()
    assert np.array_equal(world.download()["pairs"], exp[:cap])
    g.check("the honest call")
    pairs_at = next(k for k, e in enumerate(g.entries) if e.view.data_ptr() == world.pairs.data_ptr() and e.nbytes == 8 * cap)
    label = g.entries[pairs_at].label
    _lib.check(_lib.lib().clapgpu_bp_collide(physics._stream(), world._bp, n, world.aabb.data_ptr(), world.pairs.data_ptr(), cap + 1,
                                             world.pair_total.data_ptr(), None, 0, None), "clapgpu_bp_collide")
    torch.cuda.synchronize()
    assert g.dirty() == [(label, "after", [0, 1, 2, 3, 4, 5, 6, 7])], "one pair, eight bytes, right behind the pair list"
    assert label.startswith("clap_amd.physics:") and label.endswith(f"int32 [{cap}, 2]")
    stray = g.bands(pairs_at)[1][:8].cpu().numpy().view(np.uint32)
    assert np.array_equal(stray, exp[cap]), "the stray pair is the next of the ascending list"
    with pytest.raises(AssertionError, match="8 bytes after"):
        g.check("the dishonest call")


# ------------------------------------------------------------------------------------------------------ narrowphase
def write_pairs(world, pairs, static_pairs):
    """Pair lists written into the world as a broadphase would have left them (totals above the capacity included)."""
    for name, p in (("pairs", pairs), ("static_pairs", static_pairs)):
        t = getattr(world, name)
        k = min(len(p), t.shape[0])
        if k:
            t[:k] = torch.from_numpy(np.ascontiguousarray(p[:k]).view(np.int32)).to(world.device)
    world.pair_total[0] = len(pairs)
    world.static_pair_total[0] = len(static_pairs)


@pytest.fixture(scope="module")
def contact_scene():
    """300 crowded capsules and spheres among 48 static boxes, both candidate lists (the oracle's) and the materials"""
    n = 300
    b = synth.capsule_bodies(n, box=4.0, seed=33)
    statics = synth.static_boxes(48, 4.0)
    st = ob.bodies_state(b)
    ob.bodies_aabb(b, st)
    pairs = ob.broadphase_aabb_pairs(st["aabb"], max_pairs=1 << 20)
    spairs = ob.broadphase_aabb_static_pairs(statics, st["aabb"], max_pairs=1 << 20)
    assert len(pairs) > 500 and len(spairs) > 500
    R = np.random.Generator(np.random.PCG64(1))             # not the head of the list: bodies from all over the scene
    pick = lambda p: p[np.sort(R.choice(len(p), 300, replace=False))]
    return b, statics, st, pick(pairs), pick(spairs), _materials(n, 4), _materials(48, 5)


@pytest.mark.parametrize("both", [False, True], ids=["two_calls", "one_launch"])
@pytest.mark.parametrize("k", COUNTS)
def test_contacts_geoms_records_at_the_three_capacities(k, both, g, cuda_device, contact_scene):
    from clap_amd import physics
    b, statics, st, pairs, spairs, mat, smat = contact_scene
    n = b["n"]
    A = _oracle_body_geoms(b, st, mat)
    S = ob.geoms(48, kind=np.full(48, 2, np.uint8), aabb=statics, material=smat)
    for cap in capacities(k):
        world = physics.PhysWorld(b, statics, pair_capacity=cap, static_pair_capacity=cap, device=cuda_device)
        world.set_materials(mat)
        world.static_material = upload(smat, np.float64, cuda_device)
        held(g, world, ("static_material",))
        write_pairs(world, pairs[:k], spairs[:k])
        world.alloc_contacts()
        assert world.contact2_buf.shape == (cap, 160)
        if cap:                                              # (the mirror gives the static buffer one row when there is no static)
            assert world.static_contact2_buf.shape == (cap, 160)
        world.contact2_buf.fill_(0xEE)
        world.static_contact2_buf.fill_(0xEE)
        (world.contacts_geoms_both if both else world.contacts_geoms)()
        got = world.download_contacts2(ob.CONTACT2_DTYPE)
        what = f"{k} pairs, capacity {cap}, both={both}"
        exp, exp_total = ob.contacts_geoms(pairs[:min(k, cap)], A, A)
        exp_s, exp_s_total = ob.contacts_geoms(spairs[:min(k, cap)], A, S)
        assert got["body"][1] == exp_total and got["body"][0].tobytes() == exp.tobytes(), what + " body x body records"
        assert got["static"][1] == exp_s_total and got["static"][0].tobytes() == exp_s.tobytes(), what + " body x static records"
        hit = np.zeros(n, bool)
        hit[pairs[:min(k, cap)][np.isin(exp["nc"], (1, 2))].ravel()] = True
        hit[spairs[:min(k, cap)][np.isin(exp_s["nc"], (1, 2))][:, 0]] = True
        assert np.array_equal((world.download()["bflags"] & 16) != 0, hit), what + " CLAPGPU_BODY_HAS_JOINT"
        g.check(what)
        if cap == k and k > 1:
            assert exp_total > 0 and exp_s_total > 0, "nothing touches: the records test nothing"


@pytest.mark.parametrize("k", COUNTS)
def test_sphere_and_sphere_box_records_at_the_three_capacities(k, g, cuda_device):
    from clap_amd import physics
    n = 300
    b = synth.sphere_bodies(n, box=3.0, seed=41)
    statics = synth.static_boxes(48, 6.0)
    bb = oracle_aabbs(b)
    pairs = ob.broadphase_aabb_pairs(bb, max_pairs=1 << 20)[5::3][:k]
    spairs = ob.broadphase_aabb_static_pairs(statics, bb, max_pairs=1 << 20)[5:][:k]
    assert len(pairs) == k and len(spairs) == k
    mat, smat = _materials(n, 4), _materials(48, 5)
    for cap in capacities(k):
        world = physics.PhysWorld(b, statics, pair_capacity=cap, static_pair_capacity=cap, device=cuda_device)
        world.set_materials(mat)
        write_pairs(world, pairs, spairs)
        world.contacts()
        world.contacts_static(smat)
        kept = min(k, cap)
        got, total = world.download_contacts(ob.CONTACT_DTYPE)
        exp, exp_total = ob.contacts_spheres(pairs[:kept], b["pos"], b["radius"], mat)
        assert len(got) == kept and total == exp_total and got.tobytes() == exp.tobytes(), (k, cap, "sphere records")
        got, total = world.download_static_contacts(ob.CONTACT_DTYPE)
        exp, exp_total = ob.contacts_sphere_box(spairs[:kept], b["pos"], b["radius"], statics, mat, smat)
        assert len(got) == kept and total == exp_total and got.tobytes() == exp.tobytes(), (k, cap, "sphere-box records")
        g.check(f"sphere contacts, {k} pairs, capacity {cap}")


# ------------------------------------------------------------------------------------------------------ mesh contacts
import test_mesh_contacts_gpu as mcg                                                   # noqa: E402


def mesh_scene(dev, k):
    """k static pairs against meshes: 1 -- a sphere sunk into a fine heightfield, its contacts capped at 16; 65 -- bodies
    scattered over a terrain, each in the terrain's box"""
    from clap_amd.synth import heightfield
    if k == 1:
        vx, idx = heightfield(65, 4.0, amp=0.05)
        b = synth.sphere_bodies(1, box=1.0, seed=2)
        b["pos"][:] = [[2.0, 0.3, 2.0]]
        b["radius"][:] = [0.6]
        b["lvel"][:] = 0
        b["cell"] = 4.0
        return mcg.meshscene.Scene(dev, b, [(vx, idx, 1.0, [0.0, 0.0, 0.0], mcg.IDENT)], cap=(64, 1), grow=1e-6)
    vx, idx = heightfield(33, 32.0)
    b = mcg.bodies_over(k, 11, 0.0, 32.0, lambda x, z: np.sin(x * 0.37) * np.cos(z * 0.29))
    b["pos"][:, 1] = np.sin(b["pos"][:, 0] * 0.37) * np.cos(b["pos"][:, 2] * 0.29) + mcg.rng(5).uniform(-0.3, 0.5, k)
    return mcg.meshscene.Scene(dev, b, [(vx, idx, 1.0, [0.0, 0.0, 0.0], mcg.IDENT)], cap=(64 * k, k), grow=1.0)


@pytest.mark.parametrize("k", [1, 65])
def test_mesh_contacts_at_the_three_capacities(k, g, cuda_device):
    sc = mesh_scene(cuda_device, k)
    w = sc.w
    assert w.static_pairs.shape == (k, 2)
    full = sc.run()                                          # the mirror's default capacity: everything fits
    rec, ref, total, capped = full
    assert int(w.static_pair_total.item()) == k, "every body is in the mesh's box: the static list is exactly full"
    assert w.mesh_scratch.numel() == _lib.mesh_contact_scratch(k) and total > 1
    compared, tcapped = mcg.check(sc, rec, ref, total)
    assert capped == tcapped == (1 if k == 1 else capped) and compared >= 1
    if k == 1:
        assert int(rec["nc"].sum()) <= 16
    g.check(f"mesh contacts, {k} static pairs, default capacity")
    for cap in capacities(total):
        w.mesh_contact_buf = None                            # another capacity: every array anew, exactly that long
        part = sc.run(capacity=cap)
        assert w.mesh_contact_buf.shape == (max(cap, 1), 160) and w.mesh_ref.shape == (max(cap, 1), 2)
        assert part[2] == total and part[3] == capped and len(part[0]) == cap, (k, cap)
        assert np.array_equal(part[0].view(mcg.RAW), rec[:cap].view(mcg.RAW)) and np.array_equal(part[1], ref[:cap]), (k, cap)
        g.check(f"mesh contacts, {k} static pairs, capacity {cap}")
    # capacity 0: the one row the mirror allocates is not the library's to write
    w.mesh_contact_buf.fill_(0xEE)
    w.mesh_ref.fill_(-7)
    sc.run(capacity=0)
    untouched(w.mesh_contact_buf, 0xEE, "mesh_contacts at capacity 0")
    untouched(w.mesh_ref, -7, "mesh_ref at capacity 0")
    g.check("mesh contacts, capacity 0 again")


# ------------------------------------------------------------------------------------------------------ islands, solve, step
import islandref as ir                                                                  # noqa: E402
import pushref as pr                                                                    # noqa: E402
import test_islands_gpu as tig                                                          # noqa: E402
import test_solve_gpu as tsg                                                            # noqa: E402
import test_solve_wide_gpu as tsw                                                       # noqa: E402
from test_push_gpu import assert_step_equal                                             # noqa: E402


@pytest.mark.parametrize("n", COUNTS)
def test_islands(n, g, cuda_device):
    from clap_amd import physics
    b = synth.capsule_bodies(n, box=8.0, seed=14)
    w = physics.PhysWorld(b, None, pair_capacity=max(n - 1, 1), device=cuda_device)
    w.alloc_islands()
    w.island_scratch = g.scratch(_lib.bodies_islands_scratch_bytes(n))       # exactly what the library asks for
    perm = tig.rng(7).permutation(n)
    pairs = tig.chain_pairs(perm) if n > 1 else np.array([[0, 0]], np.uint32)
    nc = np.where(np.arange(len(pairs)) % 3 == 0, 2, 1).astype(np.uint32)
    assert len(pairs) == w.capacity
    for awake in ([int(perm[-1])], []):
        island, woken = tig.run_against_ref(w, b, tig.sleepers(b, awake), pairs, nc, (n, awake))
        assert woken == (n - 1 if awake else 0)
        g.check(f"islands n={n} awake={awake}")
    st = tig.sleepers(b, [int(perm[0])])                     # NULL outputs: nothing of them is written
    tig.put_state(w, st)
    tig.put_pairs(w, pairs, nc)
    w.island.fill_(-1)
    w.island_woken.fill_(-1)
    assert w.islands(tig.H, want_island=False, want_woken=False) == (None, None)
    ir.islands(st, pairs, nc, h=tig.H)
    tig.assert_islands(w, st, None, None, None, None, "NULL outputs")
    untouched(w.island, -1, "island")
    untouched(w.island_woken, -1, "island_woken")
    g.check(f"islands n={n} without outputs")


@pytest.mark.parametrize("n", COUNTS)
def test_solve_on_the_lane_and_the_workgroup_path(n, g, cuda_device):
    """n spheres in a square on the floor, each touching its neighbours: one island; rows_capacity = rows and rows - 1"""
    side = int(np.ceil(np.sqrt(n)))
    w = tsw.spheres(tsw.grid_positions(n, side), cuda_device)
    held(g, w, ("static_material",))
    case = tsw.Case(w)
    k = case.rows
    assert len(case.per_island) == 1 and k >= 3 * n
    case.both()                                              # wide_rows 1 and 0 against the sequential sweep, bit for bit
    g.check(f"solve n={n}, {k} rows, default capacity")
    for wide_rows in (1, 0):
        need = _lib.bodies_solve_scratch_bytes(w.n, k)
        got = case.run(wide_rows, capacity=k, scratch=g.scratch(need))      # exactly enough rows, exactly the scratch asked for
        case.check(got, wide_rows)
        assert w.row_lambda.shape == w.row_key.shape == w.row_level.shape == (k,)
        g.check(f"solve n={n}, capacity = rows = {k}, wide_rows {wide_rows}")
        w.solve_scratch = None
        got = case.run(wide_rows, capacity=k - 1, scratch=g.scratch(_lib.bodies_solve_scratch_bytes(w.n, k - 1)))
        assert got["status"] & 1 and got["rows_total"] == k and got["wide_total"] == 0 and not (got["row_level"] != 0).any()
        before = case.snap
        assert tsw.same_bits(got["lvel"], before["lvel"].cpu().numpy()[:w.n]) and tsw.same_bits(got["avel"], before["avel"].cpu().numpy()[:w.n])
        g.check(f"solve n={n}, capacity = rows - 1, wide_rows {wide_rows}")
        w.solve_scratch = None


@pytest.mark.parametrize("forces", [False, True], ids=["plain", "forces"])
@pytest.mark.parametrize("n", COUNTS)
def test_body_step_and_read_back(n, forces, g, cuda_device):
    from clap_amd import physics
    b = synth.capsule_bodies(n, box=20.0, seed=8, resting_frac=0.3)
    R = tig.rng(17)
    b["adis_steps_left"][R.random(n) < 0.3] = 2              # some fall asleep inside the run
    scene = synth.pad_levels(synth.entities_flat(n + 3, seed=3))
    b["body_entity"] = R.permutation(n + 3)[:n].astype(np.int32)
    if n > 2:
        b["body_entity"][1] = -1                             # a character's body: no entity of its own
    if forces and n > 4:
        b["bflags"][3] |= pr.KINEMATIC
    w = physics.PhysWorld(b, None, device=cuda_device, forces=forces)
    batch = held_entities(g, entities.EntityBatch(scene, cuda_device))
    moving = g.array((max(n, 1),), torch.uint8, 0xEE, "moving")
    joint = torch.from_numpy(np.arange(n) % 2 == 0).to(cuda_device)
    if forces:
        st = pr.step_state(b)
        for s in range(4):
            f = R.normal(0, 40.0, (n, 3)) * (R.random((n, 1)) < 0.5)
            st["facc"] += f
            w.facc += torch.from_numpy(f).to(w.device)
            st["bflags"][::2] |= 16
            w.bflags[joint] |= 16
            w.world_step(tig.H, prebin=bool(s % 2))
            pr.step_forces(b, st, tig.H)
            assert_step_equal(w, st, (n, s))
            g.check(f"step with forces n={n} substep {s}")
        geo = dict(st, aabb=np.zeros((n, 6)), axis=np.zeros((n, 3)))
        ob.bodies_aabb(b, geo)
        d = w.download()
        assert tsw.same_bits(d["aabb"], geo["aabb"]) and tsw.same_bits(d["axis"], geo["axis"]), "the geoms of the final state"
        rec = w.geom_records.cpu().numpy()
        assert np.array_equal(rec[:, 0:3], d["pos"]) and np.array_equal(rec[:, 3:6], d["axis"])
    else:
        st = ob.bodies_state(b)
        ob.bodies_aabb(b, st)
        for s in range(4):
            st["bflags"][::2] |= 16
            w.bflags[joint] |= 16
            ob.bodies_step(b, st, tig.H)
            w.world_step(tig.H, prebin=bool(s % 2))
            _assert_state_equal(w.download(), st)
            g.check(f"step n={n} substep {s}")
        # phys_body_update: entity TRS <- body pose, entities marked dirty
        ps, rot, fl = scene["pos_scale"].copy(), scene["rot"].copy(), scene["flags"].copy()
        mv = ob.phys_body_update(b, st, ps, rot, fl)
        w.phys_body_update(batch, moving)
        torch.cuda.synchronize()
        assert_bits_equal(batch.pos_scale.cpu().numpy(), ps, "entity pos_scale")
        assert_bits_equal(batch.rot.cpu().numpy(), rot, "entity rot")
        assert np.array_equal(batch.flags.cpu().numpy().view(np.uint32), fl), "entity flags"
        assert np.array_equal(moving.cpu().numpy()[:n] != 0, np.asarray(mv) != 0), "moving"
        g.check(f"phys_body_update n={n}")


@pytest.mark.parametrize("n", COUNTS)
def test_rotate_from_entities(n, g, cuda_device):
    from clap_amd import physics
    scene = synth.pad_levels(synth.entities_chains(n + 5, 2, seed=6))
    scene["flags"] = scene["flags"].copy()
    roots, kids = np.flatnonzero(scene["parent"] < 0), np.flatnonzero(scene["parent"] >= 0)
    scene["flags"][roots[::3]] &= ~np.uint32(_lib.E_DIRTY)
    b = synth.sphere_bodies(n, box=10.0, seed=6)
    m = n - n // 5
    link_entity = np.concatenate([roots[:m], kids[:n - m]]).astype(np.uint32)
    link_body = tig.rng(2).permutation(n).astype(np.uint32)                  # every body linked, each once
    batch = held_entities(g, entities.EntityBatch(scene, cuda_device))
    world = physics.PhysWorld(b, None, device=cuda_device)
    dirty = ((scene["flags"] & _lib.E_DIRTY) != 0).astype(np.uint8)
    for all_dirty in (False, True):
        exp = b["quat"].copy()
        ob.bodies_rotate_from_entities(link_body, link_entity, scene["rot"], scene["parent"],
                                       np.ones_like(dirty) if all_dirty else dirty, exp)
        world.quat.copy_(torch.from_numpy(b["quat"]))
        world.rotate_from_entities(batch, link_body, link_entity, all_dirty=all_dirty)
        got = world.download()["quat"]
        assert np.array_equal(got.view(np.uint64), exp.view(np.uint64)), (n, all_dirty)
        g.check(f"rotate_from_entities n={n} all_dirty={all_dirty}")
    assert (got != b["quat"]).any()


# ------------------------------------------------------------------------------------------------------ queries and movers
import slideref as slr                                                                  # noqa: E402
import test_move_gpu as tmg                                                             # noqa: E402
import test_rays_gpu as trg                                                             # noqa: E402
import test_slide_gpu as tsl                                                            # noqa: E402
from meshscene import fetch, same_bits                                                  # noqa: E402
from test_push_gpu import assert_push_equal, sleepy_start                               # noqa: E402

N_WORLD = 65


def query_world(dev, n=N_WORLD, **kw):
    """n capsules and spheres crowded over a ground slab (its top at y = 0.5) among a dozen static boxes; every other
    body stands on the slab"""
    from clap_amd import physics
    box = 4.0 if n <= N_WORLD else 7.0
    b = synth.capsule_bodies(n, box=box, seed=19)
    stand = np.arange(0, n, 2)
    b["pos"][stand, 1] = 0.5 + b["yoffset"][stand] + tig.rng(30).uniform(-0.04, 0.04, len(stand))
    statics = synth.static_boxes(12, box)
    return physics.PhysWorld(b, statics, device=dev, **kw), b, statics


def mover_inputs(q, seed):
    """(velocity [q, 3] float32, airborne [q]) in the mix of slideref.movers_a: walkers, risers, fallers, some that do not move"""
    R = tig.rng(seed)
    v = R.normal(0, 8.0, (q, 3)).astype(np.float32)
    air = (np.arange(q) % 3 != 0).astype(np.uint8)
    v[air == 1, 1] = (np.where(np.arange(q) % 2, 1.0, -1.0)[air == 1] * (np.abs(v[air == 1, 1]) + 1.0)).astype(np.float32)
    v[::11] = 0
    return v, air


@pytest.mark.parametrize("q", COUNTS)
def test_rays_sweeps_and_pushes_of_q_queries(q, g, cuda_device):
    w, b, statics = query_world(cuda_device, forces=True)
    n = w.n
    R = tig.rng(100 + q)
    # ---- rays: through the index and by brute force, and a ray's answer does not depend on the batch it is in
    w.bp_index()
    assert w.bp_index_status() == 0
    s, d, L = R.uniform(-1.0, 5.0, (257, 3)), R.normal(size=(257, 3)), R.choice([0.5, 2.0, 10.0], 257)
    d[::7] = [0.0, -1.0, 0.0]
    skip = np.where(np.arange(257) % 5 == 0, np.arange(257) % n, -1).astype(np.int32)
    got = fetch(w.ray_cast(s[:q], d[:q], L[:q], skip=skip[:q], grid=True))
    brute = fetch(w.ray_cast(s[:q], d[:q], L[:q], skip=skip[:q], grid=False))
    g.check(f"{q} rays")
    whole = fetch(w.ray_cast(s, d, L, skip=skip, grid=False))
    for name, a, c, e in zip(("dist", "hit", "contact", "flags"), got, brute, whole):
        assert same_bits(a, c), (q, name, "grid against brute force")
        assert same_bits(a, e[:q]), (q, name, "alone against inside a batch of 257")
    assert (whole[1] >= 0).any() and (whole[1] <= -2).any() and (whole[1] == -1).any()
    # ---- sweeps: index, brute force and host lists give the same bytes; and the oracle's sweep, per mover
    movers = R.integers(0, n, q).astype(np.uint32)
    delta = tsl.sweep_deltas(max(q, 64), 21)[-q:] if q < 64 else tsl.sweep_deltas(q, 21)
    frac, normal, hit, flags = tsl.three_ways(w, statics, movers, delta)
    g.check(f"{q} sweeps")
    assert not flags.any()
    st = ob.bodies_state(b)
    ob.bodies_aabb(b, st)
    A = _oracle_body_geoms(b, st)
    S = ob.geoms(len(statics), kind=np.full(len(statics), 2, np.uint8), aabb=statics)
    first, cand = tsl.host_lists(st["aabb"], statics, movers, delta)
    for k, m in enumerate(movers):
        f, nrm, h = ob.sweep_capsule(A, m, delta[k], S, cand[first[k]:first[k + 1]])
        assert np.float32(f).tobytes() == frac[k].tobytes() and nrm.tobytes() == normal[k].tobytes() and h == hit[k], (q, k)
    # ---- pushes: any body may be named any number of times; the sums in the reference's order
    state = sleepy_start(w, b, 9)
    pusher = R.integers(0, n + 2, q).astype(np.uint32)                          # two past the set: no such body
    v = R.normal(0, 5, (q, 3)).astype(np.float32)
    ph = R.integers(-2, n + 2, (q, 6)).astype(np.int32)
    w._push_scratch_buf = g.scratch(_lib.bodies_push_scratch_bytes(q))          # exactly what the library asks for
    for call in range(2):                                                       # the second adds to the first's sums
        want = pr.push(state, b["mass"], pusher, v, ph)
        assert_push_equal(w, state, w.bodies_push(pusher, v, ph), want, (q, call))
        g.check(f"{q} pushers, call {call}")
    assert want.sum() > 0


@pytest.mark.parametrize("n,q", [(N_WORLD, 1), (N_WORLD, 63), (N_WORLD, 65), (300, 257)], ids=["q1", "q63", "q65", "q257_of_300"])
def test_ground_collide_slide_and_move_of_q_bodies(n, q, g, cuda_device):
    """The calls that move the bodies they are given take each body once, so 257 of them need a larger world than 65."""
    R = tig.rng(200 + q)
    # ---- ground collide against the brute-force ray and the reference's arithmetic on it
    w, b, statics = query_world(cuda_device, n)
    sel = np.sort(R.choice(n, q, replace=False)).astype(np.uint32)
    ray_off = np.asarray(b["yoffset"], float) * R.uniform(0.7, 1.0, n)
    grounded = R.uniform(0, 1, n) < 0.5
    pos0 = w.pos.cpu().numpy().copy()
    roff = ray_off[sel] - 0.05
    ray_len = b["yoffset"][sel] - roff + 1e-3
    start = np.stack([pos0[sel, 0].astype(np.float32), (pos0[sel, 1] - roff).astype(np.float32),
                      pos0[sel, 2].astype(np.float32)], 1).astype(np.float64)
    rd, rh, rc, rf = fetch(w.ray_cast(start, np.tile([0, -1.0, 0], (q, 1)), ray_len * 2, skip=sel.astype(np.int32), grid=False))
    w.bp_index()
    out, normal, dist, hit, flags = fetch(w.ground_collide(sel, ray_off[sel], grounded[sel], grid=True))
    g.check(f"ground collide of {q}")
    assert np.array_equal(hit, rh) and np.array_equal((flags & 3), rf)
    h = hit != -1
    assert same_bits(dist[h], rd[h]) and np.array_equal(normal[h], rc[h, 3:].astype(np.float32))
    res, dy, branch = trg.ground_reference(pos0[sel], b["yoffset"][sel], ray_off[sel], grounded[sel], rd, rh)
    assert np.array_equal(out.astype(bool), res)
    exp = pos0.copy()
    moved = (branch == 0) | (branch == 1)
    exp[sel[moved], 1] = pos0[sel[moved], 1] + dy[moved].astype(np.float64)
    assert same_bits(w.pos.cpu().numpy(), exp)
    tsl.check_geoms_current(w)
    if q > 1:
        assert h.any() and moved.any()
    # ---- slide against the restatement, mover by mover
    w, b, statics = query_world(cuda_device, n)
    w.lvel.normal_()
    movers = R.choice(n, q, replace=False).astype(np.uint32)
    v, air = mover_inputs(q, 300 + q)
    before = tsl.snapshot(w)
    out = tsl.slide_and_fetch(w, movers, v, air)
    g.check(f"slide of {q}")
    moved_n, _flagged = tsl.compare_with(slr.OracleSweep(b, statics), out, before, movers, v, air)
    tsl.check_geoms_current(w)
    tsl.restore(w, before)
    brute = tsl.slide_and_fetch(w, movers, v, air, grid=False)
    for k in out:
        assert same_bits(out[k], brute[k]), (q, k)
    g.check(f"slide of {q}, brute force")
    if q > 1:
        assert moved_n > q // 4
    # ---- characters_move: the call is its parts (ground ray, decision, slide, push)
    w, b, statics = query_world(cuda_device, n)
    tmg.sleepy(w, 7)
    w.bodies_aabb()
    snap = tmg.snapshot(w)
    mv = tmg.movers(b, R.choice(n, q, replace=False), 11)
    for grid in (True, False):
        tmg.restore(w, snap)
        got = tmg.run_call(w, mv, grid=grid)
        g.check(f"characters_move of {q}, grid={grid}")
        tmg.restore(w, snap)
        want = tmg.composed(w, mv, grid=grid)
        tmg.assert_same(got, want, (q, grid))
        g.check(f"characters_move of {q} from its parts, grid={grid}")
    if q > 1:
        assert got[0]["applied"].any() and (got[0]["collision"] != -1).any()


def test_calls_with_nothing_to_do_write_nothing(g, cuda_device):
    """n == 0 through the mirrors: every output is the one row the mirror allocates so that no address is null, and it
    comes back as it was filled, in every byte"""
    w, b, statics = query_world(cuda_device, forces=True)
    w.bp_index()
    torch.cuda.synchronize()
    state = {k: getattr(w, k).clone() for k in tmg.KEYS}
    none3, none = np.zeros((0, 3)), np.zeros(0)
    u32 = np.zeros(0, np.uint32)
    calls = {"ray_cast": lambda: w.ray_cast(none3, none3, none),
             "ground_collide": lambda: w.ground_collide(u32, none, none),
             "sweep_capsules": lambda: w.sweep_capsules(u32, none3.astype(np.float32), np.zeros(1, np.uint32), u32),
             "sweep_capsules_grid": lambda: w.sweep_capsules_grid(u32, none3.astype(np.float32)),
             "slide": lambda: w.slide(u32, none3.astype(np.float32), np.zeros(0, np.uint8), 1 / 30),
             "bodies_push": lambda: w.bodies_push(u32, none3.astype(np.float32), np.zeros((0, 6), np.int32)),
             "characters_move": lambda: w.characters_move(tmg.make(w, {k: v[:0] for k, v in tmg.movers(b, [5, 6], 1).items()}), 1 / 60)}
    for name, call in calls.items():
        start = len(g)
        call()
        torch.cuda.synchronize()
        assert len(g) > start, name + ": the mirror allocated nothing under guard"
        assert g.rewritten(start) == [], name
        g.check(name + " of nothing")
    for k, t in state.items():
        assert same_bits(getattr(w, k).cpu().numpy(), t.cpu().numpy()), k
    # zero carriers, through the C entry point (the mirror does not make this call)
    from clap_amd import lights as gl
    batch = held_entities(g, entities.EntityBatch(synth.pad_levels(synth.entities_flat(5, 1)), cuda_device))
    ls = gl.LightSet(cuda_device, 64, 64, 64)
    ls.load(synth.lights(4, seed=3, inactive_frac=0.0))
    ls._upload()
    before = ls._d["pos"].clone()
    one = g.array((1, 3), torch.float32, 7.0, "carrier_off")
    desc = ls._desc()
    rc = _lib.lib().clapgpu_lights_from_entities(None, C.byref(batch._desc), 0, 0, one.data_ptr(), one.data_ptr(), one.data_ptr(),
                                                 C.byref(desc))
    torch.cuda.synchronize()
    assert rc == _lib.OK and torch.equal(ls._d["pos"], before)
    g.check("no carriers")


# ------------------------------------------------------------------------------------------------------ characters_update
from test_characters import _chars, _entity_scene                                       # noqa: E402


@pytest.mark.parametrize("with_bodies", [False, True], ids=["no_bodies", "bodies"])
@pytest.mark.parametrize("n", [1, 63, 65])
def test_characters_update(n, with_bodies, g, cuda_device):
    from clap_amd import characters, physics
    feed = synth.character_feed(n, seed=21, with_bodies=with_bodies)
    scene = _entity_scene(n, feed["pos"])
    batch = held_entities(g, entities.EntityBatch(scene, cuda_device))
    cf = characters.CharacterFeed(feed, cuda_device)
    world, bodies = None, None
    if with_bodies:
        bodies = synth.sphere_bodies(n, box=50.0, seed=21)
        bodies["lvel"][::4] = 0.0
        bodies["pos"] = np.ascontiguousarray(feed["pos"].astype(np.float64))
        bodies["pos"][:, 1] += bodies["yoffset"]
        world = physics.PhysWorld(bodies, None, device=cuda_device)
    chars = _chars(feed)
    ps, fl = scene["pos_scale"].copy(), scene["flags"].copy()
    for f in range(4):
        moved = ob.characters_update(chars, feed["limbo_height"], ps, fl, bodies)
        cf.character_update(batch, world)
        out = cf.download()
        assert np.array_equal(batch.pos_scale.cpu().numpy().view(np.uint32), ps.view(np.uint32)), f"frame {f} entity pos"
        assert np.array_equal(batch.flags.cpu().numpy().view(np.uint32), fl), f"frame {f} dirty flags"
        assert np.array_equal(out["hist_pos"].view(np.uint32), chars["hist_pos"].view(np.uint32))
        assert np.array_equal(out["hist_head"], chars["hist_head"]) and np.array_equal(out["hist_wrapped"], chars["hist_wrapped"])
        assert np.array_equal(out["moved"], moved)
        g.check(f"characters_update n={n} frame {f}")
        if with_bodies:
            assert np.array_equal(world.pos.cpu().numpy().view(np.uint64), bodies["pos"].view(np.uint64)), "body positions"
            bodies["pos"][:, 1] -= 40.0
            world.pos.copy_(torch.from_numpy(bodies["pos"]))
        else:
            ps[:n, 1] -= np.float32(40.0)
            batch.pos_scale.copy_(torch.from_numpy(ps))



def guarded_clock(g, n, seed):
    """(clapgpu_anim_clock over guarded arrays for n characters playing two animations, its tensors, its host state)"""
    R = tig.rng(seed)
    host = dict(anim=R.integers(0, 2, n).astype(np.uint32), time_end=np.asarray([1.5, 0.7], np.float32),
                ani=np.linspace(0.0, 1.0, n), speed=R.choice([0.5, 1.25, 2.0], n).astype(np.float32),
                restart=(np.arange(n) % 2).astype(np.uint8))
    dev = g.device
    t = dict(anim=guards.guard_like(g, torch.from_numpy(host["anim"].view(np.int32)), "clock.anim"),
             time_end=guards.guard_like(g, torch.from_numpy(host["time_end"]), "clock.time_end"),
             ani_time=guards.guard_like(g, torch.from_numpy(host["ani"]), "clock.ani_time"),
             speed=guards.guard_like(g, torch.from_numpy(host["speed"]), "clock.speed"),
             restart=guards.guard_like(g, torch.from_numpy(host["restart"]), "clock.restart"),
             frame_time=g.array((n,), torch.float32, -3.0, "clock.frame_time"),
             ended=g.array((n,), torch.uint8, 0xEE, "clock.ended"))
    assert all(v.device == dev for v in t.values())
    clk = _lib.AnimClock(n, 2, *[t[k].data_ptr() for k in ("anim", "time_end", "ani_time", "speed", "restart", "frame_time", "ended")])
    return clk, t, host


@pytest.mark.parametrize("with_bodies", [False, True], ids=["no_bodies", "bodies"])
@pytest.mark.parametrize("n,n_clock", [(1, 257), (63, 65), (65, 1), (257, 63)])
def test_characters_update_with_the_clock_in_the_same_launch(n, n_clock, with_bodies, g, cuda_device):
    """clapgpu_characters_update_clock: blocks [0, ceil(n / 256)) run the character hooks, the rest the clock of n_clock
    characters -- two hand-clipped tails in one grid, the parts of unequal size and on either side of a block boundary.
    The mirrors do not make this call (the frame does): it goes through the C entry point, the clock arrays under guard;
    the host's `now` and the device's (now_dev) in turn."""
    from clap_amd import characters, physics
    feed = synth.character_feed(n, seed=21, with_bodies=with_bodies)
    scene = _entity_scene(n, feed["pos"])
    batch = held_entities(g, entities.EntityBatch(scene, cuda_device))
    cf = characters.CharacterFeed(feed, cuda_device)
    world, bodies = None, None
    if with_bodies:
        bodies = synth.sphere_bodies(n, box=50.0, seed=21)
        bodies["lvel"][::4] = 0.0
        bodies["pos"] = np.ascontiguousarray(feed["pos"].astype(np.float64))
        bodies["pos"][:, 1] += bodies["yoffset"]
        world = physics.PhysWorld(bodies, None, device=cuda_device)
    clk, ct, ch = guarded_clock(g, n_clock, 5)
    now_dev = g.array((1,), torch.float64, 0.0, "now_dev")
    chars = _chars(feed)
    ps, fl = scene["pos_scale"].copy(), scene["flags"].copy()
    L = _lib.lib()
    for f, now in enumerate((0.9, 1.6, 2.9, 3.0)):
        moved = ob.characters_update(chars, feed["limbo_height"], ps, fl, bodies)
        ft, ended = ob.animation_time(ch["anim"], ch["time_end"], ch["ani"], ch["speed"], ch["restart"], now)
        now_dev[0] = now
        rc = L.clapgpu_characters_update_clock(physics._stream(), C.byref(cf._desc), C.byref(batch._desc),
                                               C.byref(world._desc) if world is not None else None, C.byref(clk),
                                               -1.0 if f % 2 else now, now_dev.data_ptr() if f % 2 else None)
        _lib.check(rc, "clapgpu_characters_update_clock")
        out = cf.download()
        what = f"n={n} clock={n_clock} frame {f}"
        assert np.array_equal(batch.pos_scale.cpu().numpy().view(np.uint32), ps.view(np.uint32)), what + " entity pos"
        assert np.array_equal(batch.flags.cpu().numpy().view(np.uint32), fl), what + " dirty flags"
        assert np.array_equal(out["hist_pos"].view(np.uint32), chars["hist_pos"].view(np.uint32)), what
        assert np.array_equal(out["hist_head"], chars["hist_head"]) and np.array_equal(out["hist_wrapped"], chars["hist_wrapped"]), what
        assert np.array_equal(out["moved"], moved), what
        assert np.array_equal(ct["ani_time"].cpu().numpy().view(np.uint64), ch["ani"].view(np.uint64)), what + " ani_time"
        assert np.array_equal(ct["frame_time"].cpu().numpy().view(np.uint32), ft.view(np.uint32)), what + " frame_time"
        assert np.array_equal(ct["ended"].cpu().numpy(), ended), what + " ended"
        g.check(what)
        if with_bodies:
            assert np.array_equal(world.pos.cpu().numpy().view(np.uint64), bodies["pos"].view(np.uint64)), "body positions"
            bodies["pos"][:, 1] -= 40.0
            world.pos.copy_(torch.from_numpy(bodies["pos"]))
        else:
            ps[:n, 1] -= np.float32(40.0)
            batch.pos_scale.copy_(torch.from_numpy(ps))
    if n_clock > 1:
        assert ended.any() and not ended.all(), "some animations ran out, some did not"


def test_entry_points_with_no_body_or_no_character_write_nothing(g, cuda_device):
    """b->n == 0 for clapgpu_bodies_islands and clapgpu_bodies_solve (the header: "returns CLAPGPU_OK and launches
    nothing"), c->n == 0 for clapgpu_characters_update and n_chars == 0 for clapgpu_animation_time and for both parts of
    clapgpu_characters_update_clock: through the C entry points, every array one guarded row that keeps its fill."""
    from clap_amd import physics
    w, b, statics = query_world(cuda_device)
    w.alloc_contacts()
    w.solver = _lib.Solver()
    _lib.lib().clapgpu_solver_defaults(C.byref(w.solver))
    L = _lib.lib()
    nobody = _lib.Bodies.from_buffer_copy(w._desc)
    nobody.n = 0
    start = len(g)
    i32 = lambda what, fill=-7: g.array((1,), torch.int32, fill, what)
    island, woken, total = i32("island"), i32("island_woken"), i32("pair_total", 1)
    scratch = g.array((256,), torch.uint8, 0xEE, "scratch")
    pairs = g.array((1, 2), torch.int32, 0, "pairs")
    rec = g.array((1, 160), torch.uint8, 0, "contacts")
    rc = L.clapgpu_bodies_islands(physics._stream(), C.byref(nobody), C.byref(w.world), H, pairs.data_ptr(), total.data_ptr(), 1,
                                  rec.data_ptr(), scratch.data_ptr(), island.data_ptr(), woken.data_ptr())
    assert rc == _lib.OK
    lam, key = g.array((1,), torch.float64, -1.0, "row_lambda"), g.array((1,), torch.int64, -1, "row_key")
    rows, status, level, wide = i32("rows_total"), i32("status"), i32("row_level"), i32("wide_total")
    rc = L.clapgpu_bodies_solve(physics._stream(), C.byref(nobody), C.byref(w.world), C.byref(w.solver), H, island.data_ptr(),
                                None, None, 0, None, None, None, None, 0, pairs.data_ptr(), total.data_ptr(), 1, rec.data_ptr(),
                                1, scratch.data_ptr(), lam.data_ptr(), key.data_ptr(), rows.data_ptr(), status.data_ptr(),
                                level.data_ptr(), wide.data_ptr())
    assert rc == _lib.OK
    # no character, no clocked character
    batch = held_entities(g, entities.EntityBatch(synth.pad_levels(synth.entities_flat(5, 1)), cuda_device))
    before = {k: getattr(batch, k).clone() for k in ("pos_scale", "flags")}
    u8 = lambda what: g.array((1,), torch.uint8, 0xEE, what)
    ent, body, head = i32("entity", 0), i32("body", 0), i32("hist_head")
    hist = g.array((1, 8, 3), torch.float32, 7.5, "hist_pos")
    wrapped, air, moved = u8("hist_wrapped"), u8("airborne"), u8("moved")
    nochar = _lib.Characters(0, 70.0, ent.data_ptr(), body.data_ptr(), hist.data_ptr(), head.data_ptr(), wrapped.data_ptr(),
                             air.data_ptr(), moved.data_ptr())
    assert L.clapgpu_characters_update(physics._stream(), C.byref(nochar), C.byref(batch._desc), C.byref(w._desc)) == _lib.OK
    f32 = lambda what: g.array((1,), torch.float32, 2.5, what)
    anim, te, speed, ft = i32("anim", 0), f32("time_end"), f32("speed"), f32("frame_time")
    ani, restart, ended = g.array((1,), torch.float64, 0.25, "ani_time"), u8("restart"), u8("ended")
    noclock = _lib.AnimClock(0, 1, anim.data_ptr(), te.data_ptr(), ani.data_ptr(), speed.data_ptr(), restart.data_ptr(),
                             ft.data_ptr(), ended.data_ptr())
    assert L.clapgpu_animation_time(physics._stream(), C.byref(noclock), 9.0) == _lib.OK
    assert L.clapgpu_characters_update_clock(physics._stream(), C.byref(nochar), C.byref(batch._desc), None, C.byref(noclock), 9.0,
                                             None) == _lib.OK
    torch.cuda.synchronize()
    assert g.rewritten(start) == []
    for k, t in before.items():
        assert torch.equal(getattr(batch, k), t), k
    g.check("no body, no character")


# ------------------------------------------------------------------------------------------------------ one whole frame
def whole_frame(g, dev):
    """A FrameLoop with every stage on, at the 65-sized scenes: 65 bodies (40 drive entities, 25 belong to characters that
    are fed, moved and linked) among static boxes and one static mesh, 65 posed and skinned characters, 3 x 65 particles,
    lights with carriers, contacts, islands, solve and the pre-binning step."""
    from clap_amd import animation, characters, frame, lights, particles
    from clap_amd.synth import box_mesh
    raw = synth.entities_flat(257, seed=5)
    scene, tl = tiler.tiled_scene(raw)
    roots = tl["slot_of"][np.flatnonzero(raw["parent"] < 0)]
    scene["model_lod"] = np.asarray([[0, 3]], np.uint8)
    batch = held_entities(g, entities.EntityBatch(scene, dev))
    nb, nd, J, vpc = N_WORLD, 40, 24, 65
    nc = nb - nd
    b = synth.capsule_bodies(nb, box=4.0, seed=19)
    stand = np.arange(0, nb, 2)
    b["pos"][stand, 1] = 0.5 + b["yoffset"][stand] + tig.rng(30).uniform(-0.04, 0.04, len(stand))
    b["body_entity"] = np.concatenate([roots[:nd], np.full(nc, -1)]).astype(np.int32)
    bv, bi = box_mesh()
    sc = mcg.meshscene.Scene(dev, b, [(bv, bi, 2.0, [2.0, 1.0, 2.0], mcg.IDENT)], bb=synth.static_boxes(6, 4.0),
                             material=_materials(nb, 4), static_material=_materials(7, 5), cap=(2048, 2048), grow=1e-6)
    w = sc.w
    held(g, w, ("static_material",))
    w.enable_forces()
    char_bodies = np.arange(nd, nb).astype(np.uint32)
    char_e = roots[nd:nb].astype(np.uint32)
    mv = tmg.movers(b, char_bodies, 15)
    m = tmg.make(w, mv, entity=char_e, entity_batch=batch)
    m.set(yaw_quat=tig.rng(16).normal(0, 1, (nc, 4)).astype(np.float32))
    feed = synth.character_feed(nc, seed=5, with_bodies=True, body_base=nd)
    feed["entity"] = char_e
    cf = characters.CharacterFeed(feed, dev)
    ls = lights.LightSet(dev, 65, 1, 64)
    ls.load(synth.lights(12, seed=5))
    ls.set_carriers(roots[-4:].astype(np.uint32), np.arange(4, dtype=np.int32), np.ones((4, 3), np.float32))
    sk, an = synth.skeleton(J, 5, seed=5), synth.animation(J, 8, 0.05, seed=5)
    ch = synth.characters(N_WORLD, J, seed=5)
    model = animation.SkinnedModel(sk, [an], mesh=synth.skinned_mesh(vpc, J, seed=5), device=dev)
    cb = animation.CharacterBatch(model, N_WORLD, ch["trs0"], batch.mx, entity_index=roots[100:100 + N_WORLD].astype(np.uint32),
                                  vert_first=np.zeros(N_WORLD, np.uint32), vert_count=np.full(N_WORLD, vpc, np.uint32))
    cb.start_clock(ani_time=np.zeros(N_WORLD), speed=np.ones(N_WORLD, np.float32))
    held(g, cb, ("repeat_dev", "time_end_dev"), cb._clock, ("restart", "time_end"))
    ps = synth.particle_systems(n_sys=3, count=65, radius=2.0, velocity=0.5, seed=5)
    ppos, pvel, pst = ob.particles_spawn(ps, 0x1234ABCD330E)
    pb = particles.ParticleBatch(ps, ppos, pvel, pst, dev)
    held(g, pb, ("sys", "rng_state"), pb._desc)
    return frame.FrameLoop(batch, synth.camera(pos=(0, 10, 60)), world=w, feed=cf, body_links=(char_bodies, char_e), lights=ls,
                           characters=cb, particles=pb, contacts=True, prebin=True, islands=True, solve=True, move=m)


def frame_state(loop):
    torch.cuda.synchronize()
    e, c, p, w = loop.batch.download(), loop.characters.download(), loop.particles.download(), loop.world.download()
    out = dict(mx=e["mx"], inv_mx=e["inv_mx"], aabb=e["aabb"], e_flags=e["flags"], visible=e["visible"],
               lod=loop.batch.draw_lod[:len(e["visible"])].cpu().numpy(), jt=c["joint_transforms"], jpos=c["joint_pos"],
               skinned=c["out_position"], normals=c["out_normal"], ani=loop.characters.download_clock()["ani_time"], ppos=p["pos"],
               pvel=p["vel"], rng=np.asarray([p["rng_state"]], np.uint64), tiles=loop.lights.download_tiles(),
               lpos=loop.lights._d["pos"].cpu().numpy(), island=loop.world.island.cpu().numpy(),
               facc=loop.world.facc.cpu().numpy(), mesh_total=loop.world.mesh_contact_total.cpu().numpy())
    out.update({"w_" + k: np.asarray(v) for k, v in w.items()})
    out.update({"move_" + k: t.cpu().numpy() for k, t in loop.move.outputs().items()})
    out.update({"feed_" + k: v for k, v in loop.feed.download().items()})
    return out


def test_one_frame_with_everything_on_eager_and_replayed(g, cuda_device):
    """What this test is for is g.check(): every stage of the frame at once, all arrays under guard, launch by launch and
    replayed from a graph.  Its value comparisons are weaker than the families' own above and say so: two builds of the
    same frame give the same bytes (the frame is deterministic whatever order its atomics took; no wrong kernel fails
    that), the replay gives the bytes of the launches one by one (the comparison of the existing capture test), and of the
    frame's outputs only the visible list and the light grid are held to the oracle, from the boxes and light positions
    the frame itself left.  The stages against their oracles, and the frame against the separate calls: the tests above,
    test_frame_gpu.py, test_solve_gpu.py and test_move_gpu.py."""
    dt = 1.0 / 120.0
    eager, graph = whole_frame(g, cuda_device), whole_frame(g, cuda_device)
    for loop in (eager, graph):                              # a frame of two substeps, issued launch by launch
        loop.move_dt = dt
        loop._issue(0.01, 2)                                 # (now, substeps)
    a, z = frame_state(eager), frame_state(graph)
    g.check("a frame of two substeps")
    for k in a:
        assert same_bits(a[k], z[k]), ("two builds of the same frame", k)
    cam = eager.cam
    vis, _mask = ob.entities_cull(eager.batch.n, a["e_flags"], a["aabb"], ob.frustum_from_camera(cam)[0])
    assert np.array_equal(a["visible"], vis), "the visible list against the oracle's cull of the frame's own boxes"
    _fr, oview, oproj = ob.frustum_from_camera(cam)
    src = dict(synth.lights(12, seed=5))
    src["pos"] = a["lpos"][:12].copy()
    assert np.array_equal(a["tiles"], ob.light_grid_compute(src, oview, oproj, 65, 1, 64)), "the light grid against the oracle"
    assert a["w_pair_total"] > 10 and a["w_static_pair_total"] > 10 and len(a["visible"]) > 10
    assert int(eager.world.solve_status.item()) == 0
    eager.clap_frame(0.03, dt)
    graph.capture(dt, warmup_now=0.03)                       # issues this frame eagerly, then records one
    g.check("capture")
    eager.clap_frame(0.06, dt)                               # the clock is past the end of the 0.05 s animation
    graph.clap_frame_replay(0.06)
    a, z = frame_state(eager), frame_state(graph)
    g.check("one replay of the captured frame")
    for k in a:
        assert same_bits(a[k], z[k]), ("graph replay against the launches one by one", k)
    assert (a["ani"] != 0).any(), "the 0.05 s animation restarted"


# ------------------------------------------------------------------------------------------------------ shard, world 1
from test_exchange_gpu import _oracle_visible                                           # noqa: E402


@pytest.mark.parametrize("route", ["rccl", "c10d"])
@pytest.mark.parametrize("n", [65, 257])
def test_shard_world_1(n, route, g, cuda_device, process_group):
    from clap_amd import shard
    scene, _tl = tiler.tiled_scene(synth.entities_flat(n, seed=77))
    cams = [synth.camera(pos=(0, 5, 60)), synth.camera(pos=(30, 0, -20))]
    batch = held_entities(g, entities.EntityBatch(scene, cuda_device))
    xch = shard.VisibleExchange(batch, 0, 1, cuda_device, route=route)
    assert (xch.direct is not None) == (route == "rccl")
    assert xch.g_vis[0].shape == (scene["n"],) and xch.g_mask[0].shape == (scene["n"] // 64,)
    try:
        for f, cam in enumerate(cams * 2):                   # four frames: both mask buffers used twice
            fr = entities.view_calc_frustum(cam)[0]
            xch.begin()
            batch.mq_update(fr, all_dirty=True)
            xch.submit()
            torch.cuda.synchronize()
            cnt, ids = xch.last()
            vis, mask = _oracle_visible(scene, cam)
            assert np.array_equal(ids[:int(cnt.item())].cpu().numpy().view(np.uint32), vis), (n, route, f)
            assert np.array_equal(xch.g_mask[(xch.frame - 1) & 1].cpu().numpy().view(np.uint64)[:len(mask)], mask)
            g.check(f"shard n={n} {route} frame {f}")
    finally:
        xch.destroy()
