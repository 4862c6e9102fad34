"""GPU: the frame's views in device memory (include/clapgpu.h, "Views in device memory", ABI 49).

(1) clapgpu_views_calc leaves the bits of the host's clapgpu_view_matrix / clapgpu_frustum_calc, non-finite inputs
    included; (2) every *_views twin leaves the bits of its original called with those host values; (3) a frame with
    views_dev is the same frame; (4) a replayed graph follows the camera written into the block before the replay.
Everything is compared as bit patterns or as integer arrays; nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import guards
from clap_amd import _lib, entities, synth
from clap_amd.views import ViewBlock
from helpers import load_golden
from oracle import binding as ob

pytestmark = pytest.mark.gpu
F32P = C.POINTER(C.c_float)
QNAN = np.uint32(0x7FC00000)


# --------------------------------------------------------------------------------------------------------- host side
def fp(a):
    return a.ctypes.data_as(F32P)


def host_view(pos, quat):
    pos, quat, out = np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(quat, np.float32), np.zeros(16, np.float32)
    _lib.lib().clapgpu_view_matrix(fp(pos), fp(quat), fp(out))
    return out


def host_proj(cam):
    out = np.zeros(16, np.float32)
    fov, aspect, near, far = (float(v) for v in cam["persp"])
    _lib.lib().clapgpu_perspective(fov, aspect, near, far, int(cam["ndc_z_zero_one"][0]), fp(out))
    return out


def host_frustum(view, proj, z01):
    return entities.frustum_from_matrices(view, proj, z01)


def host_mvp(view, proj):
    """proj * view in linmath.h's order (506-516), in float32, with the view functions' one quiet NaN"""
    a, b = np.asarray(proj, np.float32).reshape(4, 4), np.asarray(view, np.float32).reshape(4, 4)      # [col][row]
    out = np.zeros((4, 4), np.float32)
    with np.errstate(all="ignore"):
        for c in range(4):
            for r in range(4):
                s = np.float32(0.0)
                for k in range(4):
                    s = np.float32(s + np.float32(a[k, r] * b[c, k]))
                out[c, r] = s
    bits = out.view(np.uint32)
    bits[np.isnan(out)] = QNAN
    return out.ravel()


def pose_source(pos, quat, proj, z01=False):
    return dict(pos=np.asarray(pos, np.float32), quat=np.asarray(quat, np.float32), proj=np.asarray(proj, np.float32),
                view=None, z01=bool(z01))


def matrix_source(view, proj, pos=(1.0, 2.0, 3.0), z01=False):
    return dict(pos=np.asarray(pos, np.float32), quat=None, proj=np.asarray(proj, np.float32),
                view=np.asarray(view, np.float32), z01=bool(z01))


def cam_source(cam):
    return pose_source(cam["cam_pos"], cam["cam_quat"], host_proj(cam), int(cam["ndc_z_zero_one"][0]))


def put(block, slot, s):
    if s["view"] is None:
        block.set_pose(slot, s["pos"], s["quat"], s["proj"], s["z01"])
    else:
        block.set_matrices(slot, s["view"], s["proj"], s["pos"], s["z01"])
    # a NaN / inf position must arrive with its bits: write the words themselves
    words = block.host.numpy().view(np.uint32)
    at = slot * (C.sizeof(_lib.ViewSource) // 4) + 32
    words[at:at + 3] = s["pos"].view(np.uint32)


def expected(s):
    view = host_view(s["pos"], s["quat"]) if s["view"] is None else s["view"]
    fr = host_frustum(view, s["proj"], s["z01"])
    planes, corners = entities.frustum_arrays(fr)
    return dict(planes=planes.ravel(), corners=corners.ravel(), view_mx=view, proj_mx=s["proj"], mvp=host_mvp(view, s["proj"]),
                cam_pos=s["pos"])


def got(state, slot):
    v = state.slot[slot]
    arr = lambda f: np.ctypeslib.as_array(f).astype(np.float32).ravel().copy()    # noqa: E731
    return dict(planes=arr(v.frustum.planes), corners=arr(v.frustum.corners), view_mx=arr(v.view_mx), proj_mx=arr(v.proj_mx),
                mvp=arr(v.mvp), cam_pos=arr(v.cam_pos), cull=np.ctypeslib.as_array(v.cull).copy())


def assert_slot(state, slot, s, what):
    g, e = got(state, slot), expected(s)
    for k, ev in e.items():
        gb, eb = g[k].view(np.uint32), np.ascontiguousarray(ev, np.float32).view(np.uint32)
        bad = np.flatnonzero(gb != eb)
        assert bad.size == 0, f"{what}: {k}[{bad[0]}] is {gb[bad[0]]:#010x}, the host gives {eb[bad[0]]:#010x} ({bad.size} words differ)"
    # the cull's constants: per-axis extremes of the corners (NaN when any is), every plane component finite
    c = e["corners"].reshape(8, 4)
    cull = g["cull"].view(np.float32)
    for ax in range(3):
        if np.isnan(c[:, ax]).any():
            assert g["cull"][ax] == QNAN and g["cull"][3 + ax] == QNAN, f"{what}: extremes of axis {ax} with a NaN corner"
        else:
            assert cull[ax] == c[:, ax].min() and cull[3 + ax] == c[:, ax].max(), f"{what}: extremes of axis {ax}"
    assert g["cull"][6] == int(np.isfinite(e["planes"]).all()) and g["cull"][7] == 0, f"{what}: the finite flag"


def random_quat(rng):
    q = rng.normal(size=4)
    return (q / np.linalg.norm(q)).astype(np.float32)


def sources(golden_dir):
    rng = np.random.Generator(np.random.PCG64(49))
    out = []
    for name in ("entities_chains", "entities_forest_frames", "entities_flat_c1", "entities_flat_euler"):
        _scene, cam, _ref, _frames = load_golden(f"{golden_dir}/{name}.npz")
        out.append((name, cam_source(cam)))
    for k in range(8):
        cam = synth.camera(pos=rng.uniform(-80, 80, 3), quat=random_quat(rng), fov_deg=float(rng.uniform(40, 100)),
                           near=float(rng.uniform(0.05, 1.0)), far=float(rng.uniform(100, 900)), ndc_z_zero_one=k & 1)
        out.append((f"random pose {k}", cam_source(cam)))
    base = synth.camera(pos=(3, 4, 50), quat=random_quat(rng))
    proj = host_proj(base)
    out.append(("zero quaternion", pose_source((3, 4, 50), (0, 0, 0, 0), proj)))
    out.append(("NaN position", pose_source((np.nan, 4, 50), base["cam_quat"], proj)))
    out.append(("inf position", pose_source((3, -np.inf, 50), base["cam_quat"], proj)))
    out.append(("projection of zeros (singular mvp)", pose_source((3, 4, 50), base["cam_quat"], np.zeros(16, np.float32))))
    for z01 in (0, 1):
        cam = synth.camera(pos=(3, 4, 50), quat=base["cam_quat"], ndc_z_zero_one=z01)
        out.append((f"NDC z convention {z01}", cam_source(cam)))
    view = host_view(base["cam_pos"], base["cam_quat"])
    out.append(("a slot given as view_mx", matrix_source(view, proj, base["cam_pos"])))
    out.append(("the same slot FROM_POSE", pose_source(base["cam_pos"], base["cam_quat"], proj)))
    return out


# ------------------------------------------------------------------------------------------------ (1) block == host
def test_view_block_equals_the_host_functions(cuda_device, golden_dir, monkeypatch):
    g = guards.Guards(cuda_device)
    guards.install(monkeypatch, g)
    block = ViewBlock(cuda_device)
    src = sources(golden_dir)
    assert len(src) == 20
    for first in range(0, len(src), 5):                      # all five slots at once
        for slot in range(5):
            put(block, slot, src[first + slot][1])
        block.upload()
        block.calc(5)
        st = block.download()
        for slot in range(5):
            assert_slot(st, slot, src[first + slot][1], f"{src[first + slot][0]} in slot {slot}")
    assert src[18][0].startswith("a slot given") and first == 15      # the last group's slots 3 and 4: one view, given two ways
    a, b = got(st, 3), got(st, 4)
    for k in ("planes", "corners", "view_mx", "mvp"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), f"view_mx against FROM_POSE: {k}"
    g.check("clapgpu_views_calc, five slots")

    # n_views = 1: slots 1 .. 4 keep whatever they held
    for name, s in src:
        pattern = np.arange(_lib.VIEWS_STATE_BYTES // 4, dtype=np.int64) * 2654435761 % (1 << 31)
        block.state.copy_(torch.from_numpy(pattern.astype(np.int32)))
        put(block, 0, s)
        block.upload()
        block.calc(1)
        st = block.download()
        assert_slot(st, 0, s, f"{name}, n_views = 1")
        words = np.frombuffer(bytes(st), np.int32)
        per = C.sizeof(_lib.ViewState) // 4
        assert np.array_equal(words[per:], pattern.astype(np.int32)[per:]), f"{name}: n_views = 1 wrote past slot 0"
    g.check("clapgpu_views_calc, one slot")


# ------------------------------------------------------------------------------------------------- (2) the twins
E_ALIVE, E_VISIBLE, E_SKIP = _lib.E_ALIVE, _lib.E_VISIBLE, _lib.E_SKIP_CULLING
SENT8, SENT64 = 0x5A, 0x5A5A5A5A5A5A5A5A


def cull_inputs(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    lo = rng.uniform(-120, 120, (n, 3)).astype(np.float32)
    lo[:, 2] -= np.float32(40.0)
    hi = (lo + rng.uniform(0.1, 25, (n, 3))).astype(np.float32)
    aabb = np.concatenate([lo, hi], 1)
    flags = np.full(n, E_ALIVE | E_VISIBLE, np.uint32)
    kind = rng.integers(0, 16, n)
    flags[kind == 0] &= ~np.uint32(E_ALIVE)                  # dead
    flags[kind == 1] &= ~np.uint32(E_VISIBLE)                # hidden
    flags[kind == 2] |= np.uint32(E_SKIP)
    if n > 2:
        aabb[n // 3, 1] = np.nan                             # a NaN box
        aabb[n // 2, 3:] = aabb[n // 2, :3] - np.float32(2.0)  # max < min
        flags[[n // 3, n // 2]] = E_ALIVE | E_VISIBLE
    return flags, aabb


def view_cams(n_extra):
    rng = np.random.Generator(np.random.PCG64(7))
    cams = [synth.camera(pos=(0, 10, 60))]
    for v in range(n_extra):
        cams.append(synth.camera(pos=rng.uniform(-60, 60, 3), quat=random_quat(rng), fov_deg=float(rng.uniform(50, 95)),
                                 ndc_z_zero_one=v & 1))
    out = [cam_source(c) for c in cams]
    if n_extra == 4:
        out[3] = pose_source((np.inf, 0, 0), cams[3]["cam_quat"], host_proj(cams[3]))      # planes not finite: the literal test
    return out


class CullOut:
    def __init__(self, g, n, n_extra):
        rows = (n + 63) // 64
        self.mask = [g.array((rows,), torch.int64, SENT64) for _ in range(1 + n_extra)]
        self.pop = [g.array(((rows + 15) // 16 * 16,), torch.uint8, SENT8) for _ in range(1 + n_extra)]

    def host(self):
        return [m.cpu().numpy() for m in self.mask] + [p.cpu().numpy() for p in self.pop]


def cull_desc(flags_t, aabb_t, n, out, frusta, keep):
    e = _lib.Entities()
    e.n, e.flags, e.aabb = n, flags_t.data_ptr(), aabb_t.data_ptr()
    e.vis_mask, e.vis_row_pop = out.mask[0].data_ptr(), out.pop[0].data_ptr()
    if len(out.mask) > 1:
        v = _lib.Views()
        v.n = len(out.mask) - 1
        for k in range(v.n):
            v.vis_mask[k], v.vis_row_pop[k] = out.mask[1 + k].data_ptr(), out.pop[1 + k].data_ptr()
            if frusta is not None:
                C.memmove(C.byref(v.frustum[k]), C.byref(frusta[1 + k]), C.sizeof(_lib.Frustum))
        keep.append(v)
        e.views = C.pointer(v)
    return e


@pytest.fixture(scope="module")
def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("n_extra", [2, 4], ids=["main+2", "main+4"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 4097])
def test_cull_twin_equals_the_original(cuda_device, stream, n, n_extra):
    L = _lib.lib()
    g = guards.Guards(cuda_device)
    flags, aabb = cull_inputs(n, 100 + n)
    flags_t = g.array((n,), torch.int32, contents=torch.from_numpy(flags.view(np.int32)))
    aabb_t = g.array((n, 6), torch.float32, contents=torch.from_numpy(aabb))
    srcs = view_cams(n_extra)
    frusta = [host_frustum(host_view(s["pos"], s["quat"]), s["proj"], s["z01"]) for s in srcs]
    keep = []
    a, b = CullOut(g, n, n_extra), CullOut(g, n, n_extra)
    ea = cull_desc(flags_t, aabb_t, n, a, frusta, keep)
    eb = cull_desc(flags_t, aabb_t, n, b, None, keep)        # e->views->frustum[] all zeros: the twin must not read it
    block = ViewBlock(cuda_device)
    for slot, s in enumerate(srcs):
        put(block, slot, s)
    block.upload()
    block.calc(1 + n_extra)
    _lib.check(L.clapgpu_entities_cull(stream, C.byref(ea), C.byref(frusta[0])), "clapgpu_entities_cull")
    _lib.check(L.clapgpu_entities_cull_views(stream, C.byref(eb), block.state.data_ptr()), "clapgpu_entities_cull_views")
    torch.cuda.synchronize()
    ha, hb = a.host(), b.host()
    for k, (x, y) in enumerate(zip(ha, hb)):
        assert np.array_equal(x, y), f"n {n}: {'mask' if k <= n_extra else 'row pop'} of plane {k % (1 + n_extra)}"
    rows = (n + 63) // 64
    assert all((p[rows:] == SENT8).all() for p in ha[1 + n_extra:]), "the bytes past ceil(n / 64) are the caller's"
    main = ha[0].view(np.uint64)
    assert n < 64 or 0 < sum(bin(int(w)).count("1") for w in main) < n, "the case culls something and keeps something"
    g.check(f"cull, n {n}, {n_extra} further views")


def test_lod_twins_equal_the_originals(cuda_device, stream):
    """On the visible list of the 4097-entity case; force_lod set and NULL; the two-call and the one-call form."""
    L = _lib.lib()
    n = 4097
    g = guards.Guards(cuda_device)
    rng = np.random.Generator(np.random.PCG64(11))
    flags, aabb = cull_inputs(n, 100 + n)
    aabb[n // 3, 1] = aabb[n // 3, 4] - np.float32(1.0)      # the pick reads finite boxes
    center = ((aabb[:, 3:] - aabb[:, :3]) * np.float32(0.5) + aabb[:, :3]).astype(np.float32)
    up = lambda a, dt: g.array(a.shape, dt, contents=torch.from_numpy(a))     # noqa: E731
    table = np.zeros((3, 8), np.float32)
    table[:, 0:3], table[:, 4:7] = [[-1, -2, -3], [-4, -1, -2], [-0.5, -0.5, -0.5]], [[1, 2, 3], [4, 1, 2], [0.5, 0.5, 0.5]]
    table.view(np.uint32)[:, 7] = np.asarray([0 | 3 << 8, 1 | 6 << 8, 0 | 0 << 8], np.uint32)
    ps = np.concatenate([center, rng.uniform(0.5, 3.0, (n, 1)).astype(np.float32)], 1).astype(np.float32)
    t = dict(flags=up(flags.view(np.int32), torch.int32), aabb=up(aabb, torch.float32), center=up(center, torch.float32),
             pos_scale=up(ps, torch.float32), model=up(rng.integers(0, 3, n).astype(np.int32), torch.int32),
             table=up(table, torch.float32))
    rows = (n + 63) // 64
    mask, pop = g.array((rows,), torch.int64), g.array(((rows + 15) // 16 * 16,), torch.uint8)
    e = _lib.Entities()
    e.n, e.n_models = n, 3
    e.flags, e.aabb, e.center, e.pos_scale = t["flags"].data_ptr(), t["aabb"].data_ptr(), t["center"].data_ptr(), t["pos_scale"].data_ptr()
    e.model, e.model_table, e.vis_mask, e.vis_row_pop = t["model"].data_ptr(), t["table"].data_ptr(), mask.data_ptr(), pop.data_ptr()
    cam = synth.camera(pos=(0, 10, 60))
    s = cam_source(cam)
    block = ViewBlock(cuda_device)
    put(block, 0, s)
    block.upload()
    block.calc(1)
    _lib.check(L.clapgpu_entities_cull_views(stream, C.byref(e), block.state.data_ptr()), "cull")
    cam_pos = (C.c_float * 3)(*[float(v) for v in cam["cam_pos"]])
    forced = rng.integers(-1, 4, n).astype(np.int32)
    scratch = g.array((max(L.clapgpu_visible_scratch_bytes(n) // 4, 1),), torch.int32)
    cur0 = rng.integers(0, 4, n).astype(np.int32)
    for force in (forced, None):
        f_t = up(force, torch.int32) if force is not None else None
        res = []
        for twin in (False, True):
            for one_call in (False, True):
                vis, cnt = g.array((n,), torch.int32, -1), g.array((1,), torch.int32)
                cur, draw = up(cur0, torch.int32), g.array((n,), torch.int32, -7)
                fp_ = f_t.data_ptr() if f_t is not None else None
                view_arg = block.state.data_ptr() if twin else cam_pos
                if one_call:
                    fn = L.clapgpu_visible_compact_lod_views if twin else L.clapgpu_visible_compact_lod
                    rc = fn(stream, C.byref(e), 0, view_arg, fp_, cur.data_ptr(), vis.data_ptr(), cnt.data_ptr(), draw.data_ptr(),
                            scratch.data_ptr())
                else:
                    _lib.check(L.clapgpu_visible_compact(stream, mask.data_ptr(), pop.data_ptr(), n, 0, vis.data_ptr(), cnt.data_ptr(),
                                                         scratch.data_ptr()), "compact")
                    fn = L.clapgpu_entities_lod_views if twin else L.clapgpu_entities_lod
                    rc = fn(stream, C.byref(e), vis.data_ptr(), cnt.data_ptr(), 0, view_arg, fp_, cur.data_ptr(), draw.data_ptr())
                _lib.check(rc, fn.__name__)
                torch.cuda.synchronize()
                res.append([x.cpu().numpy() for x in (vis, cnt, cur, draw)])
        assert 100 < int(res[0][1][0]) < n - 100, "the list holds a part of the entities"
        assert len(np.unique(res[0][3][:int(res[0][1][0])])) >= 3, "the pick gives several LODs"
        for r in res[1:]:
            for name, x, y in zip(("visible", "count", "cur_lod", "draw_lod"), res[0], r):
                assert np.array_equal(x, y), f"force_lod {'set' if force is not None else 'NULL'}: {name}"
    g.check("LOD twins")


def test_light_grid_twin_equals_the_original(cuda_device, monkeypatch):
    from clap_amd import lights
    g = guards.Guards(cuda_device)
    guards.install(monkeypatch, g)
    cam = synth.camera(pos=(5, 8, 40), quat=(0.0, 0.2588190451, 0.0, 0.9659258263))
    s = cam_source(cam)
    view = host_view(s["pos"], s["quat"])
    block = ViewBlock(cuda_device)
    put(block, 0, s)
    block.upload()
    block.calc(1)
    ls = lights.LightSet(cuda_device, 1280, 720, 64)
    ls.load(synth.lights(12, seed=5))
    ls.grid_compute(view, s["proj"])
    a = ls.download_tiles().copy()
    ls.tiles.fill_(-1)
    ls.grid_compute_views(block)
    b = ls.download_tiles().copy()
    assert np.array_equal(a, b) and a.any() and (a != a.ravel()[0]).any(), "the tile masks, and they are not all one value"
    g.check("light grid twin")


def test_particles_twin_equals_the_original(cuda_device, monkeypatch):
    from clap_amd import particles
    g = guards.Guards(cuda_device)
    guards.install(monkeypatch, g)
    cam = synth.camera(pos=(5, 8, 40), quat=(0.0, 0.2588190451, 0.0, 0.9659258263))
    s = cam_source(cam)
    view = host_view(s["pos"], s["quat"])
    block = ViewBlock(cuda_device)
    put(block, 0, s)
    block.upload()
    block.calc(1)
    ps = synth.particle_systems(n_sys=3, count=256, radius=2.0, velocity=0.5, seed=5)
    ppos, pvel, pst = ob.particles_spawn(ps, 0x1234ABCD330E)
    a = particles.ParticleBatch(ps, ppos.copy(), pvel.copy(), pst, cuda_device)
    b = particles.ParticleBatch(ps, ppos.copy(), pvel.copy(), pst, cuda_device)
    a.billboard_mx.fill_(-3.0)
    b.billboard_mx.fill_(-3.0)
    for f in range(4):
        a.particles_update(view)
        b.particles_update_views(block)
        torch.cuda.synchronize()
        da, db = a.download(), b.download()
        assert np.array_equal(a.billboard_mx.cpu().numpy().view(np.uint32), b.billboard_mx.cpu().numpy().view(np.uint32)), f"frame {f}: billboards"
        assert np.array_equal(da["pos"].view(np.uint32), db["pos"].view(np.uint32)), f"frame {f}: positions"
        assert np.array_equal(a.vel.cpu().numpy().view(np.uint32), b.vel.cpu().numpy().view(np.uint32)), f"frame {f}: velocities"
        assert da["rng_state"] == db["rng_state"] and a.stream_state() == b.stream_state(), f"frame {f}: rng state"
    assert da["rng_state"] != pst, "particles respawned during the frames"
    assert not (a.billboard_mx.cpu().numpy() == -3.0).any(), "every system's billboard was written"
    g.check("particles twin")


# ------------------------------------------------------------------------------------------- (3), (4) the frame
def light_view():
    """One further view: a light looking down on the scene, as (view_mx, proj_mx, ndc_z_zero_one)"""
    cam = synth.camera(pos=(10, 80, 20), quat=(-0.6427876097, 0.0, 0.0, 0.7660444431), fov_deg=60.0, near=1.0, far=300.0)
    return host_view(cam["cam_pos"], cam["cam_quat"]), host_proj(cam), False


def build_loop(device, views_dev, cam):
    """The scene of test_captured_frame_graph_replays_the_same_frames (tests/test_frame_gpu.py) + one further view"""
    from clap_amd import animation, characters, frame, lights, particles, physics, tiler
    raw = synth.entities_flat(3000, seed=5)
    scene, tl = tiler.tiled_scene(raw)
    roots = tl["slot_of"][np.flatnonzero(raw["parent"] < 0)]
    scene["model_lod"] = np.asarray([[0, 3]], np.uint8)
    batch = entities.EntityBatch(scene, device)
    batch.set_views(None, matrices=[light_view()])
    nb, nc, J, vpc = 200, 12, 24, 90
    b = synth.sphere_bodies(nb, box=10.0, seed=5)
    b["body_entity"] = roots[:nb].astype(np.int32)
    world = physics.PhysWorld(b, synth.static_boxes(6, 10.0), pair_capacity=8192, device=device)
    feed = synth.character_feed(nc, seed=5, with_bodies=False)
    feed["entity"] = roots[nb:nb + nc].astype(np.uint32)
    cf = characters.CharacterFeed(feed, device)
    ls = lights.LightSet(device, 1280, 720, 64)
    ls.load(synth.lights(12, seed=5))
    ls.set_carriers(roots[-4:].astype(np.uint32), np.arange(4, dtype=np.int32), np.ones((4, 3), np.float32))
    sk, an = synth.skeleton(J, 5, seed=5), synth.animation(J, 8, 0.05, seed=5)
    ch = synth.characters(nc, J, seed=5)
    model = animation.SkinnedModel(sk, [an], mesh=synth.skinned_mesh(vpc, J, seed=5), device=device)
    cb = animation.CharacterBatch(model, nc, ch["trs0"], batch.mx, entity_index=feed["entity"],
                                  vert_first=np.zeros(nc, np.uint32), vert_count=np.full(nc, vpc, np.uint32))
    cb.start_clock(ani_time=np.zeros(nc), speed=np.ones(nc, np.float32))
    ps = synth.particle_systems(n_sys=3, count=256, radius=2.0, velocity=0.5, seed=5)
    ppos, pvel, pst = ob.particles_spawn(ps, 0x1234ABCD330E)
    pb = particles.ParticleBatch(ps, ppos, pvel, pst, device)
    return frame.FrameLoop(batch, cam, world=world, feed=cf, lights=ls, characters=cb, particles=pb, contacts=True,
                           views_dev=views_dev)


def frame_state(loop):
    torch.cuda.synchronize()
    e, c, p, w = loop.batch.download(), loop.characters.download(), loop.particles.download(), loop.world.download()
    return dict(mx=e["mx"], vis_mask=e["vis_mask"], visible=e["visible"], lod=loop.batch.draw_lod[:len(e["visible"])].cpu().numpy(),
                cur_lod=loop.batch.cur_lod.cpu().numpy(), view1_mask=loop.batch.view_masks[0].cpu().numpy(),
                jt=c["joint_transforms"], jpos=c["joint_pos"], skinned=c["out_position"],
                ani=loop.characters.download_clock()["ani_time"], ppos=p["pos"], rng=np.asarray([p["rng_state"]], np.uint64),
                bill=loop.particles.billboard_mx.cpu().numpy(), bpos=w["pos"], pairs=w["pairs"], spairs=w["static_pairs"],
                tiles=loop.lights.download_tiles())


CAM_A = dict(pos=(0.0, 10.0, 60.0), yaw=0.0)


def cam_at(pos, yaw):
    return synth.camera(pos=pos, quat=(0.0, float(np.sin(yaw / 2)), 0.0, float(np.cos(yaw / 2))))


def camera_path(frames=10):
    """A quarter turn of yaw and a move of tens of units, from a fixed seed: frame f's camera"""
    rng = np.random.Generator(np.random.PCG64(2049))
    out = []
    for f in range(1, frames + 1):
        t = f / frames
        jitter = rng.uniform(-1.0, 1.0, 3)
        out.append(cam_at((40.0 * t + jitter[0], 10.0 + 6.0 * t + jitter[1], 60.0 - 35.0 * t + jitter[2]), -(np.pi / 2) * t))
    return out


def same(a, b, what):
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype.kind == "f":
            x, y = x.view(np.uint32 if x.itemsize == 4 else np.uint64), y.view(np.uint32 if y.itemsize == 4 else np.uint64)
        assert x.shape == y.shape and np.array_equal(x, y), f"{what}: {k}"


def test_frame_with_views_in_device_memory_is_the_same_frame(cuda_device):
    cam_a = cam_at(**CAM_A)
    host, dev = build_loop(cuda_device, False, cam_a), build_loop(cuda_device, True, cam_a)
    dt = 1.0 / 120.0
    for f, cam in enumerate(camera_path(), 1):
        for loop in (host, dev):
            loop.set_camera(cam)
            loop.clap_frame(f * dt, dt)
        same(frame_state(host), frame_state(dev), f"frame {f}")
    st = frame_state(dev)
    assert 0 < len(st["visible"]) < 3000 and st["view1_mask"].any(), "the main view and the further view both draw something"


def test_replayed_graph_follows_the_camera(cuda_device):
    """The one-stream frame captured at camera A, replayed for ten frames with set_camera before each replay, against an
    eager loop with host views given the same cameras -- and against what camera A would have given, which the frames
    must NOT equal (a replay that kept camera A would pass every other assertion of a weaker test)."""
    cam_a = cam_at(**CAM_A)
    graph, ref, frozen = (build_loop(cuda_device, True, cam_a), build_loop(cuda_device, False, cam_a),
                          build_loop(cuda_device, False, cam_a))
    dt = 1.0 / 120.0
    ref.clap_frame(dt, dt)
    frozen.clap_frame(dt, dt)
    graph.capture(dt, warmup_now=dt)                          # issues frame 1 eagerly, then records at camera A
    same(frame_state(ref), frame_state(graph), "frame 1 (camera A)")
    moved = dict(vis_mask=0, visible=0, lod=0, tiles=0, bill=0)
    for f, cam in enumerate(camera_path(), 2):
        ref.set_camera(cam)
        ref.clap_frame(f * dt, dt)
        frozen.clap_frame(f * dt, dt)
        graph.set_camera(cam)
        graph.clap_frame_replay(f * dt)
        r, a = frame_state(ref), frame_state(frozen)
        same(r, frame_state(graph), f"frame {f} (replay)")
        for k in moved:
            moved[k] += int(r[k].shape != a[k].shape or not np.array_equal(r[k], a[k]))
    assert all(v >= 8 for v in moved.values()), f"frames (of 10) whose outputs differ from camera A's: {moved}"
