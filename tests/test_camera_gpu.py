"""GPU: clapgpu_camera_calc (include/clapgpu.h, "The camera controller on the device", ABI 50) against the host loop it
replaces -- clapgpu_camera_target, then clapgpu_camera_update_host with one clapgpu_ray_cast of four rays, a
synchronisation and a download per iteration -- AS BYTES: the whole 160-byte block and the whole view source.  The scene
and the ten named cases are tests/camerascene.py's (tests/test_camera.py shows on the CPU that each does what it is named
for); every case runs by scan, through a one-level index and through a leveled index, each with and without the mesh
set.  Then the frame: with `camera` it is the frame without it followed by camera_calc, views_calc, cull, list and LOD
as separate calls, on one stream and on three; and a captured graph of a frame with move, aniq and camera replays what
the eager frame computes while the control character walks.  Every array of the mirrors lies between the guard bands of
tests/guards.py."""
import numpy as np
import pytest
import torch

from clap_amd import _dev, _lib, camera as cam_mod, physics, synth, views as views_mod
import camerascene as cs
import guards

pytestmark = pytest.mark.gpu
SENTINEL = 0x7a7a7a7a                                       # what the outputs hold before a call


def as_bytes(a):
    return np.ascontiguousarray(np.atleast_1d(a)).view(np.uint8).reshape(-1)


def bodies():
    b = synth.capsule_bodies(3, box=1.0, seed=1)
    b["pos"][:] = cs.BODY_POS
    b["quat"][:] = [1.0, 0.0, 0.0, 0.0]                      # upright
    b["radius"][:], b["length"][:] = cs.BODY_RADIUS, cs.BODY_LENGTH
    b["yoffset"][:] = cs.BODY_RADIUS + cs.BODY_LENGTH / 2
    b["lvel"][:], b["avel"][:] = 0.0, 0.0
    return b


class Ents:
    """what clapgpu_camera_calc reads of a clapgpu_entities, and nothing else"""

    def __init__(self, dev):
        self.keep = [_dev.upload(cs.ENT_POS_SCALE, np.float32, dev), _dev.upload(cs.ENT_MODEL, np.int32, dev),
                     _dev.upload(cs.MODEL_TABLE.reshape(-1, 4), np.float32, dev), _dev.upload(cs.ENT_CENTER, np.float32, dev)]
        d = _lib.Entities()
        d.n, d.n_models = len(cs.ENT_MODEL), len(cs.MODEL_TABLE)
        d.pos_scale, d.model, d.model_table, d.center = [t.data_ptr() for t in self.keep]
        self._desc = d


class Rig:
    """one world (scan / one_level / leveled) with the scene's colliders, the entities, the joints, a view block and a
    camera block"""

    def __init__(self, dev, index):
        b = bodies()
        b["cell"] = 0.5 if index == "leveled" else cs.CELL       # leveled: three levels, the top cell 2.0
        kw = dict(bp_levels=3, leveled_index=True) if index == "leveled" else {}
        self.index, self.grid = index, index != "scan"
        self.w = w = physics.PhysWorld(b, cs.static_boxes(), device=dev, **kw)
        w.set_static_geoms(cs.STATIC_KIND, *cs.static_geo())
        vx, idx = cs.terrain()
        w.set_static_meshes([cs.MESH_STATIC], [vx], [idx], [1.0], [cs.TERRAIN_POS], [[0.0, 0.0, 0.0, 1.0]])
        if self.grid:
            w.bp_index()
            assert w.bp_index_status() == 0, "an indexed box larger than a cell, or no index: the rays would scan"
        self.ents = Ents(dev)
        self.joint_pos = _dev.upload(cs.JOINT_POS, np.float32, dev)
        self.views = views_mod.ViewBlock(dev)
        self.block = cam_mod.CameraBlock(dev)

    def ray_cast(self, ray, skip, meshes):
        dist, hit, _contact, flags = self.w.ray_cast(ray[:, 0:3], ray[:, 3:6], ray[:, 6], skip=np.full(4, skip, np.int32),
                                                     grid=self.grid, meshes=meshes)
        torch.cuda.synchronize()
        return dist.cpu().numpy(), hit.cpu().numpy(), flags.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def rigs(cuda_device):
    reg = guards.Guards(cuda_device)
    with pytest.MonkeyPatch.context() as mp:
        guards.install(mp, reg)
        out = {k: Rig(cuda_device, k) for k in ("scan", "one_level", "leveled")}
    yield reg, out
    reg.check("at the end of the module")


def fill_source(views):
    """a source whose every byte is known: slot 0 a pose that the camera must replace, the others matrices it must keep"""
    proj = np.arange(16, dtype=np.float32) + 0.5
    views.set_pose(0, (9.0, 8.0, 7.0), (0.5, 0.5, 0.5, 0.5), proj)
    for s in range(1, _lib.VIEW_SLOTS):
        views.set_matrices(s, np.arange(16, dtype=np.float32) + s, proj * s, pos=(s, s, s))
    views.upload()
    return views.host.numpy().view(np.uint8).copy()


def block_inputs(rig, c):
    rig.block.set(c["quat"], c["near"], c["far"], c["aspect"], c["entity"], ctl_skip=c["skip"], character=bool(c["flags"] & 1),
                  head_joint=c["head_joint"] if c["flags"] & 2 else None, moved=c["moved"], pos=(-1.0, -2.0, -3.0), dist=77.0)
    h = rig.block.host[0]
    h["target"], h["corner"] = 55.0, 66.0
    for k in ("updated", "iterations", "status"):
        h[k] = SENTINEL
    h["pad"] = SENTINEL
    rig.block.upload()
    return h.copy()


def host_loop(rig, c, start, meshes):
    """what a host does today: camera_target on downloaded values, then the loop with a ray cast round trip per
    iteration.  Returns (the block it ends with, the per-iteration (hit, flags) of the casts)"""
    want, log = start.copy(), []
    if c["moved"]:
        ei = cs.entity_inputs(c)
        want["target"], want["dist"] = cam_mod.target(ei["flags"], ei["pos_scale"], ei["lo"], ei["hi"], ei["center"], ei["head"], c["far"])

    def cast(ray):
        dist, hit, flags = rig.ray_cast(ray, c["skip"], meshes)
        log.append((hit.copy(), flags.copy(), dist.copy(), ray.copy()))
        return hit != -1, np.where(hit != -1, dist, 0.0), flags
    return cam_mod.update_host(want, cast), log


@pytest.mark.parametrize("meshes", [False, True], ids=["no_meshes", "meshes"])
@pytest.mark.parametrize("index", ["scan", "one_level", "leveled"])
@pytest.mark.parametrize("c", cs.CASES, ids=[c["name"] for c in cs.CASES])
def test_block_and_source_equal_the_host_loop_as_bytes(rigs, c, index, meshes):
    reg, all_rigs = rigs
    rig = all_rigs[index]
    src0 = fill_source(rig.views)
    start = block_inputs(rig, c)
    rig.block.calc(rig.ents, rig.w, rig.views, joint_pos=rig.joint_pos, grid=rig.grid, meshes=meshes)
    got = rig.block.download()
    src = as_bytes(rig.views.source.cpu().numpy())
    want, log = host_loop(rig, c, start, meshes)
    print(c["name"], index, "meshes" if meshes else "no meshes", "iterations", int(got["iterations"]), "dist", float(got["dist"]),
          "status", int(got["status"]), "hits", [l[0].tolist() for l in log])
    for k in cam_mod.CAMERA.names:
        assert np.array_equal(as_bytes(got[k]), as_bytes(want[k])), (k, got[k], want[k])
    assert np.array_equal(as_bytes(got), as_bytes(want))
    # the source: slot 0's pos and quat are the block's, every other byte is what was uploaded
    want_src = src0.copy()
    if c["moved"]:
        at_pos, at_quat = _lib.ViewSource.pos.offset, _lib.ViewSource.quat.offset
        want_src[at_pos:at_pos + 12] = as_bytes(want["pos"])
        want_src[at_quat:at_quat + 16] = as_bytes(c["quat"])
    assert np.array_equal(src, want_src)
    reg.check(f"{c['name']} {index}")
    # the case is what it is named for, by what clapgpu_ray_cast answered the host loop
    name = c["name"]
    if name == "not_moved":
        keep = start.copy()
        keep["status"], keep["iterations"] = 0, 0
        assert np.array_equal(as_bytes(got), as_bytes(keep)) and np.array_equal(src, src0)
    if name == "no_physics":
        assert not log and got["iterations"] == 1 and got["updated"] == 0
    if name == "one_pull_in":
        assert got["iterations"] == 2 and got["updated"] == 1
    if name == "three_pull_ins":
        assert got["iterations"] >= 4
        win = [int(np.argmin(np.where(h != -1, d / r[:, 6], np.inf))) for h, _f, d, r in log[:-1]]
        assert len(set(win)) >= 2, win
    if name == "triangle_wins":
        if meshes:
            assert (log[0][0] == -2 - cs.MESH_STATIC).all() and got["iterations"] >= 2 and got["status"] == 0
        else:
            assert got["status"] == _lib.CAMERA_UNRESOLVED and got["iterations"] == 1
    if name == "body_static_tie":
        assert (log[0][0] == 1).all()                         # the body wins; without it the static answers the same depth
        d_static = rig.w.ray_cast(log[0][3][:, 0:3], log[0][3][:, 3:6], log[0][3][:, 6], skip=np.full(4, 1, np.int32), grid=rig.grid,
                                  meshes=meshes)
        assert (d_static[1].cpu().numpy() == -2 - 3).all() and np.array_equal(as_bytes(d_static[0].cpu().numpy()), as_bytes(log[0][2]))
    if name == "collapse_inside_a_box":
        assert got["iterations"] == 1 and got["dist"] <= 0.1
    if name == "unresolved":
        assert int(got["status"]) & _lib.CAMERA_UNRESOLVED
    if name == "nan_quaternion":
        assert got["iterations"] == 1 and not (int(got["status"]) & _lib.CAMERA_CAPPED) and (log[0][1] & _lib.RAY_INVALID).all()
    if name == "no_hit":
        assert got["iterations"] == 1 and (log[0][0] == -1).all() and got["status"] == 0


def test_a_control_out_of_range_is_reported_and_nothing_else_is_written(rigs):
    """what the host cannot see before a HIP call (the block lives on the device) the kernel refuses"""
    reg, all_rigs = rigs
    rig = all_rigs["scan"]
    by = {c["name"]: c for c in cs.CASES}
    for bad in ("entity", "head"):
        src0 = fill_source(rig.views)
        block_inputs(rig, by["one_pull_in"] if bad == "entity" else by["triangle_wins"])
        if bad == "entity":
            rig.block.host[0]["ctl_entity"] = len(cs.ENT_MODEL)
            rig.block.upload()
        start = rig.block.host[0].copy()
        rig.block.calc(rig.ents, rig.w, rig.views, joint_pos=rig.joint_pos if bad == "entity" else None, grid=False, meshes=True)
        got = rig.block.download()
        start["status"], start["iterations"] = _lib.CAMERA_INVALID, 0
        assert np.array_equal(as_bytes(got), as_bytes(start)), bad
        assert np.array_equal(as_bytes(rig.views.source.cpu().numpy()), src0)
    reg.check("out of range")


# ------------------------------------------------------------------------------------------------- the frame
NB, NC, J, VPC = 200, 12, 24, 90                            # the smallest scene of test_frame_gpu.py, its bodies capsules
HEAD = 5                                                    # the control character's "head": joint 5 of character 0


def frame_setup(dev, camera=True, index=True):
    """The frame of test_aniq_gpu.py (move, aniq, pose, skinning, contacts) with its views in device memory and the camera
    controller on the device, following character 0."""
    import aniqcases as ac
    import aniqref as ar
    from clap_amd import animation, characters, entities, frame, tiler
    R = ac.rng(31)
    raw = synth.entities_flat(3000, seed=5)
    scene, tl = tiler.tiled_scene(raw)
    roots = tl["slot_of"][np.flatnonzero(raw["parent"] < 0)]
    scene["model_lod"] = np.asarray([[0, 3]], np.uint8)
    batch = entities.EntityBatch(scene, dev)
    b = synth.capsule_bodies(NB, box=10.0, seed=5)
    chars = R.choice(NB, NC, replace=False).astype(np.uint32)
    b["body_entity"][:] = -1
    dyn = np.setdiff1d(np.arange(NB), chars)[:150]
    b["body_entity"][dyn] = roots[:150]
    b["pos"][chars[:NC // 2], 1] = 0.5 + b["yoffset"][chars[:NC // 2]]          # half of them stand on the ground slab
    w = physics.PhysWorld(b, synth.static_boxes(6, 10.0), pair_capacity=8192, device=dev, forces=True)
    char_e = roots[150:150 + NC].astype(np.uint32)
    nrm = np.tile(np.float32([0, 1, 0]), (NC, 1))
    m = physics.CharacterMoves(w, chars, np.asarray(b["yoffset"], float)[chars] * 0.9, entity=char_e, entity_batch=batch,
                               motion=np.zeros((NC, 2), np.float32), state=np.full(NC, ar.CS_IDLE, np.uint8),
                               jump=np.zeros(NC, np.uint8), jump_params=(R.uniform(0.5, 2.0, (NC, 2)) * [1.0, 4.0]).astype(np.float32),
                               velocity=np.zeros((NC, 3), np.float32), normal=nrm, airborne=np.zeros(NC, np.uint8))
    feed = synth.character_feed(NC, seed=5, with_bodies=True)
    feed["entity"], feed["body"] = char_e, chars.astype(np.int32)
    cf = characters.CharacterFeed(feed, dev)
    cf._desc.airborne = m.airborne.data_ptr()
    sk = synth.skeleton(J, 5, seed=5)
    full = ac.models()["all"]
    model = ar.Model(full.name_anim, full.time_end / np.float32(8))
    anims = [synth.animation(J, 6, float(te), seed=40 + i) for i, te in enumerate(model.time_end)]
    sm = animation.SkinnedModel(sk, anims, mesh=synth.skinned_mesh(VPC, J, seed=5), device=dev)
    ch = synth.characters(NC, J, seed=5)
    cb = animation.CharacterBatch(sm, NC, ch["trs0"], batch.mx, entity_index=char_e, vert_first=np.zeros(NC, np.uint32),
                                  vert_count=np.full(NC, VPC, np.uint32))
    start = ac.walk_start(model, NC, 17)
    start["ani_time"][:] = -np.linspace(0.0, 0.1, NC)
    aq = animation.AnimationQueues(NC, model.name_anim, sm.time_end, batch=cb, moves=m,
                                   **{k: start[k] for k in ("queue", "len", "cur", "cleared", "ani_time", "ch_motion")})
    cam = synth.camera(pos=(0, 10, 60), quat=tuple(cs.quat_yaw_pitch(25.0, 25.0)))      # from below: the rays meet the ground slab
    block = cam_mod.CameraBlock(dev)
    fov, aspect, near, far = (float(v) for v in cam["persp"])
    block.set(cam["cam_quat"], near, far, aspect, int(char_e[0]), ctl_skip=int(chars[0]), character=True, head_joint=HEAD)
    block.upload()
    loop = frame.FrameLoop(batch, cam, world=w, feed=cf, characters=cb, contacts=True, move=m, aniq=aq, views_dev=True,
                           camera=block, camera_index=index)
    m.set(motion=np.tile(np.float32([0.0, 2.0]), (NC, 1)), jump=np.zeros(NC, bool), yaw_quat=np.tile(np.float32([0, 0, 0, 1]), (NC, 1)))
    if not camera:                                              # the same frame with the stage and the list taken out
        f = loop._build()
        f.camera = f.camera_bp = None
        f.visible = None
    return loop, dict(w=w, batch=batch, m=m, cb=cb, aq=aq, block=block, views=loop.views)


def frame_state(p):
    torch.cuda.synchronize()
    e, c, wd = p["batch"].download(), p["cb"].download(), p["w"].download()
    out = dict(block=as_bytes(p["block"].download()), source=as_bytes(p["views"].source.cpu().numpy()),
               state=as_bytes(p["views"].state.cpu().numpy()), vis_mask=e["vis_mask"], visible=e["visible"], mx=e["mx"],
               lod=p["batch"].draw_lod[:len(e["visible"])].cpu().numpy(), cur_lod=p["batch"].cur_lod.cpu().numpy(),
               jpos=c["joint_pos"], skinned=c["out_position"], bpos=wd["pos"])
    out.update({"aq_" + k: v for k, v in p["aq"].download().items()})
    return out


def assert_same_state(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and np.array_equal(as_bytes(x), as_bytes(y)), f"{what}: {k}"


@pytest.fixture
def g(cuda_device, monkeypatch):
    reg = guards.Guards(cuda_device)
    guards.install(monkeypatch, reg)
    yield reg
    reg.check("at the end of the test")


@pytest.mark.parametrize("overlap", [False, True], ids=["one_stream", "overlap"])
def test_frame_with_the_camera_is_the_frame_in_pieces(cuda_device, g, overlap):
    dt = 1.0 / 120.0
    whole, pw = frame_setup(cuda_device)
    parts, pp = frame_setup(cuda_device, camera=False)
    whole.overlap = parts.overlap = overlap
    dists = []
    for f in range(1, 5):
        whole.clap_frame(f * dt, dt)
        parts.clap_frame(f * dt, dt)                              # 1. the frame without `camera` (and without its list)
        pp["w"].bp_index()
        pp["block"].calc(pp["batch"], pp["w"], pp["views"], joint_pos=pp["cb"].joint_pos)      # 2. clapgpu_camera_calc
        pp["views"].calc(1)                                       # 3. clapgpu_views_calc
        pp["batch"].cull_views(pp["views"])                       # 4. cull, list, LOD
        pp["batch"].compact_visible_lod_views(pp["views"])
        a, b = frame_state(pw), frame_state(pp)
        assert_same_state(a, b, f"frame {f}")
        blk = pw["block"].download()
        assert blk["iterations"] >= 1 and (int(blk["status"]) & ~_lib.CAMERA_UNRESOLVED) == 0
        dists.append((int(blk["iterations"]), float(blk["dist"]), blk["target"].tolist()))
    print("frame in pieces:", dists, "visible", len(a["visible"]))
    assert 0 < len(a["visible"]) < 3000
    assert max(d[0] for d in dists) >= 2, "the orbit dips under the ground slab: the frame's camera pulls in"


def test_frame_without_a_camera_is_the_frame_before(cuda_device, g):
    """camera NULL: launch for launch the parent's frame -- the same arrays as a FrameLoop that never heard of a camera"""
    dt = 1.0 / 120.0
    a, pa = frame_setup(cuda_device, camera=False)
    fa = a._desc
    fa.visible = pa["batch"].visible.data_ptr()                    # put the list back: only `camera` stays NULL
    from clap_amd import frame
    b, pb = frame_setup(cuda_device)
    plain = frame.FrameLoop(pb["batch"], b.cam, world=pb["w"], feed=b.feed, characters=pb["cb"], contacts=True, move=pb["m"],
                            aniq=pb["aq"], views_dev=True)
    for f in range(1, 4):
        a.clap_frame(f * dt, dt)
        plain.clap_frame(f * dt, dt)
        sa, sb = frame_state(pa), frame_state(dict(pb, views=plain.views))
        for k in ("block",):
            sa.pop(k), sb.pop(k)
        assert_same_state(sa, sb, f"frame {f}")


def test_captured_graph_follows_the_control_character(cuda_device, g):
    """move + aniq + camera captured once; three replays with nothing written from the host but the clock"""
    dt = 1.0 / 120.0
    graph, pg = frame_setup(cuda_device)
    eager, pe = frame_setup(cuda_device)
    eager.clap_frame(dt, dt)
    graph.capture(dt, warmup_now=dt)                              # issues frame 1 eagerly, then records
    assert_same_state(frame_state(pe), frame_state(pg), "frame 1")
    first = pe["block"].download()
    for f in range(2, 5):
        eager.clap_frame(f * dt, dt)
        graph.clap_frame_replay(f * dt)
        assert_same_state(frame_state(pe), frame_state(pg), f"replay {f - 1}")
    last = pg["block"].download()
    print("graph: target", first["target"], "->", last["target"], "dist", first["dist"], "->", last["dist"], "iterations", last["iterations"])
    assert not np.array_equal(first["target"], last["target"]), "the control character walked: the camera's target follows"
