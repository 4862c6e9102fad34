"""GPU: clapgpu_characters_move against the calls it is made of -- ground_collide, tests/moveref.py on the host, bp_index,
slide of the sliding movers, bodies_push -- bit for bit; the batch against movers processed one at a time; the rotation
hand-off; the frame with the move as its first stage; a captured graph; characters that land and walk on a terrain.
Every comparison is == on bit patterns: the call runs the same kernels on the same inputs, and k_move_decide states
moveref's arithmetic in the same order.  (The restatement itself and the refusals: test_move.py.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from clap_amd import _lib, physics, synth
import moveref as mr
import slideref as sr
from meshscene import Scene, fetch, guarded_scratch, same_bits, rng

pytestmark = pytest.mark.gpu
DT = 1.0 / 60.0
N = 200                                                     # three wavefronts and eight lanes of a fourth
KEYS = ("pos", "quat", "lvel", "aabb", "axis", "geom_records", "facc", "bflags", "adis_steps_left", "adis_time_left")
IN = ("motion", "state", "jump", "jump_params", "velocity", "normal", "airborne")
OUT = ("velocity", "normal", "airborne", "request", "applied", "collision", "first_frac", "push_hit", "flags")


def snapshot(w):
    return {k: getattr(w, k).clone() for k in KEYS}


def restore(w, snap):
    for k in KEYS:
        getattr(w, k).copy_(snap[k])
    w.bp_invalidate()


def body_state(w):
    torch.cuda.synchronize()
    return {k: getattr(w, k).cpu().numpy().copy() for k in KEYS}


def sleepy(w, seed):
    """forces on, something in every accumulator, four bodies in ten asleep with spent counters: what the pushes add to,
    wake and reset"""
    R = rng(seed)
    w.enable_forces(R.normal(0, 3.0, (w.n, 3)))
    w.world.adis_time = 0.125
    asleep = torch.from_numpy(R.random(w.n) < 0.4).to(w.device)
    w.bflags[asleep] |= _lib.BODY_DISABLED
    w.adis_steps_left[asleep] = -1
    w.adis_time_left[asleep] = -0.25


def movers(b, bodies, seed, speed=4.0):
    """the per-character state of len(bodies) movers: every state, a quarter airborne, one in six jumping, a third without
    motion, some without a ground normal"""
    R = rng(seed)
    n = len(bodies)
    bodies = np.asarray(bodies, np.uint32)
    nrm = R.normal(0, 1, (n, 3)).astype(np.float32)
    nrm[:, 1] = np.abs(nrm[:, 1]) + 1.0
    nrm[R.random(n) < 0.1] = 0
    return dict(body=bodies, ray_off=np.asarray(b["yoffset"], float)[bodies] * R.uniform(0.7, 1.0, n),
                motion=(R.normal(0, speed, (n, 2)) * (R.integers(0, 3, (n, 1)) > 0)).astype(np.float32),
                state=(np.arange(n) % 7).astype(np.uint8)[R.permutation(n)], jump=(R.integers(0, 6, n) == 0).astype(np.uint8),
                jump_params=R.uniform(0.5, 2.0, (n, 2)).astype(np.float32) * np.float32([1.0, 4.0]),
                velocity=R.normal(0, speed, (n, 3)).astype(np.float32), normal=nrm,
                airborne=(R.integers(0, 4, n) == 0).astype(np.uint8))


def make(w, mv, **kw):
    return physics.CharacterMoves(w, mv["body"], mv["ray_off"], **{k: mv[k] for k in IN}, **kw)


def run_call(w, mv, dt=DT, grid=True, meshes=True, **kw):
    """one clapgpu_characters_move call: (outputs, bodies afterwards)"""
    m = make(w, mv, **kw)
    out = {k: t.cpu().numpy().copy() for k, t in w.characters_move(m, dt, grid=grid, meshes=meshes).items()}
    out["flags"] = out["flags"].view(np.uint32)
    return out, body_state(w)


def composed(w, mv, dt=DT, grid=True, meshes=True):
    """the parent commit's way: ground_collide, read back, moveref on the host, upload, slide and push of the sliding
    movers.  Returns what run_call returns"""
    n = len(mv["body"])
    if grid:
        w.bp_index()
    gout, nrm, _dist, hit, rflags = fetch(w.ground_collide(mv["body"], mv["ray_off"], mv["airborne"] == 0, grid=grid, meshes=meshes))
    rflags = rflags.view(np.uint32)
    wrote = (hit != -1) & ((rflags & (_lib.RAY_INVALID | _lib.RAY_UNRESOLVED)) == 0)      # the normal: only on a hit
    normal = np.where(wrote[:, None], nrm, mv["normal"]).astype(np.float32)
    d = mr.character_move_decide(rflags, gout, mv["state"], mv["jump"], mv["motion"], mv["jump_params"], mv["velocity"], normal,
                                 mv["airborne"], np.float32(w.world.gravity[1]), dt)
    out = dict(velocity=d["velocity"].copy(), normal=normal, airborne=d["airborne"], request=d["request"], applied=d["applied"],
               collision=hit, first_frac=np.ones((n, 2), np.float32), push_hit=np.full((n, 6), -1, np.int32),
               flags=rflags.copy())
    s = np.flatnonzero(d["applied"])
    if not dt < 1e-6 and len(s):
        if grid:
            w.bp_index()
        vel, ff, ph, fl, _pushed = fetch(w.slide_and_push(mv["body"][s], d["velocity"][s], d["airborne"][s], dt, grid=grid,
                                                          meshes=meshes))
        out["velocity"][s], out["first_frac"][s], out["push_hit"][s] = vel, ff, ph
        out["flags"][s] |= fl.view(np.uint32) << 8
    return out, body_state(w)


def assert_same(got, want, what):
    (go, gb), (wo, wb) = got, want
    for k in OUT:
        assert same_bits(go[k], wo[k]), (what, k, np.flatnonzero((np.atleast_2d(go[k].T) != np.atleast_2d(wo[k].T)).any(0))[:8])
    for k in KEYS:
        assert same_bits(gb[k], wb[k]), (what, "bodies", k)


def coverage(out, what):
    """the batch took every branch: printed, then asked for"""
    req = np.bincount(out["request"], minlength=256)
    rf, sf = out["flags"] & 0xff, out["flags"] >> 8
    seen = dict(idle=req[mr.CS_IDLE], moving=req[mr.CS_MOVING], jump=req[mr.CS_JUMP_START], falling=req[mr.CS_FALLING],
                applied=int(out["applied"].sum()), hits=int((out["collision"] != -1).sum()),
                misses=int((out["collision"] == -1).sum()), blocked=int((out["first_frac"] < 1).any(1).sum()),
                pushes=int((out["push_hit"] >= 0).any(1).sum()), ray_moved=int(((rf & 4) != 0).sum()),
                slide_moved=int(((sf & 4) != 0).sum()), ended=int(req[mr.CS_NONE]))
    print(what, seen)
    return seen


# ------------------------------------------------------------------------------------------------- scenes
@pytest.fixture(scope="module")
def scene_a(cuda_device):
    b, statics = sr.scene_a()
    # half of the first test's movers stand on the ground slab (its top is at y = 0.5), their feet within the shortest
    # ray's reach of it (ray_len >= 0.051): grounded movers to walk, jump and idle; the others hang in the crowd
    stand = rng(3).choice(b["n"], N, replace=False)[:N // 2]
    b["pos"][stand, 1] = 0.5 + b["yoffset"][stand] + rng(30).uniform(-0.04, 0.04, len(stand))
    w = physics.PhysWorld(b, statics, device=cuda_device)
    sleepy(w, 7)
    w.bodies_aabb()
    return w, b, snapshot(w)


@pytest.fixture(scope="module")
def scene_b(cuda_device):
    b, meshes = sr.scene_b(n=3000)
    sc = Scene(cuda_device, b, meshes, cap=(1 << 20, 1 << 20))
    sleepy(sc.w, 8)
    sc.w.bodies_aabb()
    return sc.w, b, snapshot(sc.w)


def over_terrain(b):
    n = int(b["n"])
    return np.flatnonzero((np.arange(n) >= n // 6) & (np.abs(b["pos"][:, 0] - 16) < 11) & (np.abs(b["pos"][:, 2] - 16) < 11))


# ------------------------------------------------------------------------------------------------- 1. composition
@pytest.mark.parametrize("grid", [True, False], ids=["grid", "bp_null"])
def test_move_is_its_parts_scene_a(scene_a, grid):
    w, b, before = scene_a
    mv = movers(b, rng(3).choice(b["n"], N, replace=False), 11)
    restore(w, before)
    got = run_call(w, mv, grid=grid)
    restore(w, before)
    want = composed(w, mv, grid=grid)
    assert_same(got, want, "scene a")
    seen = coverage(got[0], "scene a")
    for k in ("idle", "moving", "jump", "falling", "applied", "hits", "misses", "blocked", "pushes"):
        assert seen[k] > 0, (k, seen)
    assert not same_bits(got[1]["facc"], before["facc"].cpu().numpy()) and not same_bits(got[1]["pos"], before["pos"].cpu().numpy())
    assert not got[1]["lvel"][mv["body"][got[0]["applied"] != 0]].any()


@pytest.mark.parametrize("grid,meshes", [(True, True), (False, True), (True, False)], ids=["grid", "bp_null", "no_meshes"])
def test_move_is_its_parts_scene_b(scene_b, grid, meshes):
    w, b, before = scene_b
    mv = movers(b, rng(4).choice(over_terrain(b), N, replace=False), 12)
    restore(w, before)
    got = run_call(w, mv, grid=grid, meshes=meshes)
    restore(w, before)
    want = composed(w, mv, grid=grid, meshes=meshes)
    assert_same(got, want, "scene b")
    seen = coverage(got[0], "scene b meshes=%s" % meshes)
    if meshes:
        for k in ("idle", "moving", "jump", "falling", "applied", "hits", "misses", "blocked"):
            assert seen[k] > 0, (k, seen)
        assert (got[0]["collision"] <= -2).any()                              # the terrain
    else:                                                                     # the terrain is an OTHER static nobody resolves
        o = got[0]
        ended = (o["flags"] & _lib.RAY_UNRESOLVED) != 0
        assert ended.sum() > 20 and (o["request"][ended] == mr.CS_NONE).all() and not o["applied"][ended].any()
        for k in ("velocity", "normal", "airborne"):
            assert same_bits(o[k][ended], mv[k][ended]), k
        assert (o["first_frac"][ended] == 1).all() and (o["push_hit"][ended] == -1).all() and not (o["flags"][ended] >> 8).any()


@pytest.mark.parametrize("dt", [0.0, 0.9e-6, 1e-6, 1.0], ids=["zero", "below", "at_1e-6", "long"])
def test_move_is_its_parts_at_the_dt_thresholds(scene_a, dt):
    w, b, before = scene_a
    mv = movers(b, rng(5).choice(b["n"], N, replace=False), 13)
    restore(w, before)
    got = run_call(w, mv, dt=dt)
    restore(w, before)
    assert_same(got, composed(w, mv, dt=dt), dt)
    o = got[0]
    air = o["request"] == mr.CS_FALLING
    if dt < 1e-6:                                                            # no slide, no push: the ground snaps alone
        walkers = (o["request"] == mr.CS_MOVING) & (mv["state"] >= mr.CS_IDLE)
        assert walkers.sum() > 10 and (o["applied"] == walkers).all()
        assert same_bits(got[1]["facc"], before["facc"].cpu().numpy()) and same_bits(got[1]["lvel"], before["lvel"].cpu().numpy())
        assert (o["first_frac"] == 1).all() and (o["push_hit"] == -1).all() and not (o["flags"] >> 8).any()
    elif dt == 1e-6:                                                         # the slide runs, gravity does not (> against <)
        assert air.sum() > 10 and not o["applied"][air].any() and same_bits(o["velocity"][air], mv["velocity"][air])
    else:
        assert o["applied"][air].all()


def test_move_of_none_and_of_one(scene_a):
    w, b, before = scene_a
    restore(w, before)
    empty = {k: v[:0] for k, v in movers(b, [5, 6], 1).items()}
    out, bodies = run_call(w, empty)
    assert all(len(out[k]) == 0 for k in OUT)
    for k in KEYS:
        assert same_bits(bodies[k], before[k].cpu().numpy()), k
    for body in (17, 4021):
        for state, air in ((mr.CS_MOVING, 0), (mr.CS_FALLING, 1)):
            mv = movers(b, [body], 2)
            mv["state"][:], mv["airborne"][:], mv["jump"][:] = state, air, 0
            restore(w, before)
            got = run_call(w, mv)
            restore(w, before)
            assert_same(got, composed(w, mv), ("one", body, state))


# ------------------------------------------------------------------------------------------------- 2. one at a time
def apart_movers(b, bb, cand, mv, want, dt):
    """movers (indices into cand) none of which can reach another: a mover stays within its ground snap and ray plus the
    way its velocity -- as given, after gravity, walking or jumping -- takes it in dt, summed over its calls"""
    yo = np.asarray(b["yoffset"], float)[cand]
    ray = 2 * (yo - (mv["ray_off"] - 0.05) + 1e-3) + mv["ray_off"]
    speed = np.abs(mv["velocity"]).sum(1) + 9.8 * dt + 2 * np.abs(mv["motion"]).sum(1)
    reach = (2 * speed * dt + ray + 2e-3)[:, None]
    lo, hi = bb[cand][:, 0::2] - reach, bb[cand][:, 1::2] + reach
    keep = []
    for k in range(len(cand)):
        if all(not (np.all(lo[j] <= hi[k]) and np.all(hi[j] >= lo[k])) for j in keep):
            keep.append(k)
            if len(keep) == want:
                break
    assert len(keep) == want, len(keep)
    return np.asarray(keep)


def test_batch_is_the_movers_one_at_a_time(scene_a):
    w, b, before = scene_a
    restore(w, before)
    cand = rng(6).choice(b["n"], 1500, replace=False)
    mv = movers(b, cand, 14, speed=2.0)
    mv["jump"][:] = 0                                                        # a jump's velocity is not in the reach
    keep = apart_movers(b, w.download()["aabb"], cand, mv, 70, DT)
    mv = {k: v[keep] for k, v in mv.items()}
    batch, bodies = run_call(w, mv)
    restore(w, before)
    single = {k: [] for k in OUT}
    for k in range(len(keep)):                                               # in list order, on the world the others left
        o, _ = run_call(w, {key: v[k:k + 1] for key, v in mv.items()})
        for key in OUT:
            single[key].append(o[key][0])
    seq = body_state(w)
    flagged = ((batch["flags"] & 4) != 0) | (((batch["flags"] >> 8) & 4) != 0)
    print("apart movers", len(keep), "flagged MOVED_TARGET", int(flagged.sum()), coverage(batch, "apart"))
    assert flagged.sum() <= 0.05 * len(keep)
    ok = ~flagged
    for key in OUT:
        assert same_bits(batch[key][ok], np.asarray(single[key])[ok]), key
    mine = mv["body"][ok]
    for key in ("pos", "lvel", "aabb", "axis", "geom_records"):
        assert same_bits(bodies[key][mine], seq[key][mine]), key
    if not flagged.any():                                                    # then the pushes are the same sums too
        for key in KEYS:
            assert same_bits(bodies[key], seq[key]), key


# ------------------------------------------------------------------------------------------------- 3. rotation
def test_rotation_hand_off_is_for_the_applied_movers(scene_a):
    from clap_amd import entities
    w, b, before = scene_a
    restore(w, before)
    scene = synth.pad_levels(synth.entities_flat(600, seed=3))
    scene["flags"] = (scene["flags"] & ~np.uint32(_lib.E_DIRTY)).astype(np.uint32)
    batch = entities.EntityBatch(scene, w.device)
    rot0, flags0, pos0 = batch.rot.cpu().numpy().copy(), batch.flags.cpu().numpy().copy(), batch.pos_scale.cpu().numpy().copy()
    mv = movers(b, rng(3).choice(b["n"], N, replace=False), 11)
    entity = rng(9).choice(600, N, replace=False).astype(np.uint32)
    q = rng(10).normal(0, 1, (N, 4)).astype(np.float32)
    m = make(w, mv, entity=entity, entity_batch=batch)
    m.set(yaw_quat=q)
    out = {k: t.cpu().numpy() for k, t in w.characters_move(m, DT).items()}
    ap = out["applied"] != 0
    assert 20 < ap.sum() < N - 20
    rot1, flags1 = batch.rot.cpu().numpy(), batch.flags.cpu().numpy()
    want_rot, want_flags = rot0.copy(), flags0.copy()
    want_rot[entity[ap]] = q[ap]
    want_flags[entity[ap]] |= _lib.E_DIRTY
    assert same_bits(rot1, want_rot) and same_bits(flags1, want_flags) and same_bits(batch.pos_scale.cpu().numpy(), pos0)
    # without the pair nothing of the entities changes, and the rest of the call is the same
    batch.rot.copy_(torch.from_numpy(rot0).to(w.device))
    batch.flags.copy_(torch.from_numpy(flags0).to(w.device))
    restore(w, before)
    plain, _ = run_call(w, mv)
    assert same_bits(batch.rot.cpu().numpy(), rot0) and same_bits(batch.flags.cpu().numpy(), flags0)
    for k in OUT:
        assert same_bits(plain[k], out[k].view(plain[k].dtype)), k


# ------------------------------------------------------------------------------------------------- 4. the frame
def frame_setup(dev, move):
    from clap_amd import entities, frame, tiler
    raw = synth.entities_flat(900, seed=5)
    scene, tl = tiler.tiled_scene(raw)
    roots = tl["slot_of"][np.flatnonzero(raw["parent"] < 0)]
    scene["model_lod"] = np.asarray([[0, 3]], np.uint8)
    b = synth.capsule_bodies(1500, box=9.0, seed=23)
    chars = rng(7).choice(1500, 100, replace=False).astype(np.uint32)
    b["body_entity"][:] = -1
    dyn = np.setdiff1d(np.arange(1500), chars)[:300]
    b["body_entity"][dyn] = roots[:300]
    batch = entities.EntityBatch(scene, dev)
    w = physics.PhysWorld(b, synth.static_boxes(20, 9.0), pair_capacity=1 << 16, device=dev, forces=True)
    mv = movers(b, chars, 15)
    m = make(w, mv, entity=roots[300:400].astype(np.uint32), entity_batch=batch)
    m.set(yaw_quat=rng(16).normal(0, 1, (100, 4)).astype(np.float32))
    loop = frame.FrameLoop(batch, synth.camera(pos=(0, 10, 60)), world=w, contacts=True, move=m if move else None)
    return w, batch, m, loop, mv


def frame_state(w, batch, m):
    out = body_state(w)
    out.update({"move_" + k: t.cpu().numpy().copy() for k, t in m.outputs().items()})
    out.update({"e_" + k: v for k, v in batch.download().items() if isinstance(v, np.ndarray)})
    return out


def host_half(m, frame):
    """what the host does between frames: the states the call asked for, fresh input"""
    req = m.request.cpu().numpy()
    state = m.state.cpu().numpy().copy()
    state[req != mr.CS_NONE] = req[req != mr.CS_NONE]
    R = rng(100 + frame)
    m.set(state=state, motion=R.normal(0, 3, (m.n, 2)).astype(np.float32), jump=R.integers(0, 8, m.n) == 0)


def test_frame_with_the_move_is_the_move_then_the_frame(cuda_device):
    wa, ba, ma, loop_a, _ = frame_setup(cuda_device, True)
    wb, bb, mb, loop_b, _ = frame_setup(cuda_device, False)
    now = 3.0
    for f, dt in enumerate((1 / 60, 1 / 120, 0.03)):
        now += dt
        loop_a.clap_frame(now, dt)
        wb.characters_move(mb, dt)
        loop_b.clap_frame(now, dt)
        sa, sb = frame_state(wa, ba, ma), frame_state(wb, bb, mb)
        assert sa.keys() == sb.keys()
        for k in sa:
            assert same_bits(sa[k], sb[k]), (f, k)
        host_half(ma, f)
        host_half(mb, f)
    assert (sa["move_applied"] != 0).sum() > 10 and (sa["move_request"] == mr.CS_FALLING).any()


def test_frame_without_the_move_is_the_frame_before(cuda_device):
    wp, bp, mp, plain, _ = frame_setup(cuda_device, False)
    plain._issue(0.0, 2)
    w, batch, m, loop, _ = frame_setup(cuda_device, True)
    f = loop._build()
    f.move = None                                                            # dt and scratch stay set
    loop.move_dt = DT
    loop._issue(0.0, 2)
    sa, sb = frame_state(w, batch, m), frame_state(wp, bp, mp)
    for k in sa:
        assert same_bits(sa[k], sb[k]), k
    assert not sa["move_request"].any() and not sa["move_applied"].any()      # nothing ran the movers


# ------------------------------------------------------------------------------------------------- 5. captured graph
def test_move_in_a_captured_graph(scene_b):
    """captured with the default queue count, meshes and index included; replayed twice on the restored state: the eager
    call's bytes"""
    w, b, before = scene_b
    mv = movers(b, rng(4).choice(over_terrain(b), N, replace=False), 12)
    restore(w, before)
    eager = run_call(w, mv)
    restore(w, before)
    m = make(w, mv)
    sg = w.static_geoms()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=w.device)
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _lib.check(_lib.lib().clapgpu_characters_move(physics._stream(), w._bp, C.byref(w._desc), C.byref(w.world), C.byref(sg),
                                                          w._meshes, None, DT, C.byref(m._desc), m.scratch.data_ptr()),
                       "clapgpu_characters_move")
    torch.cuda.current_stream().wait_stream(side)
    for trial in range(2):
        restore(w, before)
        m.set(**{k: mv[k] for k in IN})
        g.replay()
        out = {k: t.cpu().numpy().copy() for k, t in m.outputs().items()}
        out["flags"] = out["flags"].view(np.uint32)
        assert_same((out, body_state(w)), eager, ("replay", trial))


# ------------------------------------------------------------------------------------------------- 6. the scratch
@pytest.mark.parametrize("n", [1, 256, 257])
def test_move_stays_inside_the_scratch_it_asks_for(scene_a, n):
    """a scratch of exactly clapgpu_characters_move_scratch_bytes, 0xA5 behind it: the call leaves the tail alone and
    gives the bytes it gives on the wrapper's own scratch.  n = 256 fills the byte-sized grounded arrays' 256-byte part,
    257 starts the next; the push's scratch, sized by its own count, is the last part"""
    w, b, before = scene_a
    mv = movers(b, rng(8).choice(b["n"], n, replace=False), 17)
    restore(w, before)
    want = run_call(w, mv)
    restore(w, before)
    m = make(w, mv)
    need = _lib.characters_move_scratch_bytes(w.n, n)
    m.scratch, tail = guarded_scratch(need, w.device)
    out = {k: t.cpu().numpy().copy() for k, t in w.characters_move(m, DT).items()}
    out["flags"] = out["flags"].view(np.uint32)
    got = (out, body_state(w))
    assert (tail == 0xA5).all().item(), ("written past the scratch", need, torch.nonzero(tail != 0xA5)[:8].flatten().tolist())
    assert_same(got, want, ("guarded scratch", n))


# ------------------------------------------------------------------------------------------------- 7. behaviour
def test_characters_land_and_walk_on_the_terrain(cuda_device):
    """64 characters dropped over scene B's terrain, 120 frames of one clapgpu_characters_move call each and the host's
    half of the state machine: all land, end grounded and walking, their feet (pos.y - yoffset) within a capsule radius
    of the terrain's closed-form height -- the margin and the final check of
    test_characters_fall_walk_and_stay_on_the_terrain -- and no frame leaves a GROUNDED character's feet further below
    that height than the radius.  A character still airborne at the end of a frame is in transit: character_move casts
    the ground ray before it moves, so the frame in which a fall crosses the ground ends up to velocity * dt below it
    (0.105 against a radius of 0.103 at frame 38 of this drop, 6 units a second after 0.63 s) and the next frame's ray
    lifts it; that depth is printed and bounded by one frame of the fastest fall of this drop (3 units: 7.7 a second)."""
    n, pool = 64, 256
    vx, idx = synth.heightfield(33, 32.0)
    bv, bi = synth.box_mesh()
    ident = [0.0, 0.0, 0.0, 1.0]
    meshes = [(vx, idx, 1.0, [0.0, 0.0, 0.0], ident), (bv, bi, 4.0, [40.0, 0.0, 16.0], ident)]
    R = rng(91)
    b = synth.capsule_bodies(pool, box=32.0, seed=91)
    b["quat"][:] = [1.0, 0.0, 0.0, 0.0]                                      # characters do not tumble
    b["pos"][:, 0], b["pos"][:, 2] = R.uniform(8, 24, pool), R.uniform(8, 24, pool)
    b["pos"][:, 1] = sr.ground_b(b["pos"][:, 0], b["pos"][:, 2]) + b["yoffset"] + R.uniform(0.5, 2.5, pool)
    b["lvel"][:] = 0
    b["avel"][:] = 0
    sc = Scene(cuda_device, b, meshes, cap=(1 << 16, 1 << 16))
    w = sc.w
    w.enable_forces()
    # upright characters whose geom ends well above their feet, as test_characters_fall_walk_and_stay_on_the_terrain picks them
    below = w.pos.cpu().numpy()[:, 1] - w.aabb.cpu().numpy()[:, 2]
    bodies = np.flatnonzero(below <= 0.6 * b["yoffset"])[:n].astype(np.uint32)
    assert len(bodies) == n
    away = np.setdiff1d(np.arange(pool), bodies)
    w.pos[torch.from_numpy(away).to(w.device)] = torch.tensor([-500.0, -500.0, -500.0], dtype=torch.float64, device=w.device)
    w.bodies_aabb()
    yoff, radius = b["yoffset"][bodies], b["radius"][bodies]
    motion = np.stack([R.uniform(-1.5, 1.5, n), R.uniform(-1.5, 1.5, n)], 1).astype(np.float32)
    state = np.full(n, mr.CS_FALLING, np.uint8)
    m = physics.CharacterMoves(w, bodies, np.asarray(yoff, float) * 0.8, motion=motion, state=state, airborne=np.ones(n, np.uint8))
    landed = np.zeros(n, bool)
    worst, transit = -1.0, 0.0
    for frame in range(120):
        out = {k: t.cpu().numpy() for k, t in w.characters_move(m, DT).items()}
        flags = out["flags"].view(np.uint32)
        assert not (flags & 0x303).any(), (frame, flags)                      # INVALID / UNRESOLVED of either stage
        landed |= out["airborne"] == 0
        req = out["request"]
        state = np.where(req != mr.CS_NONE, req, state).astype(np.uint8)      # the animations always start: the state is taken
        m.set(state=state)
        pos = w.pos.cpu().numpy()[bodies]
        assert np.isfinite(pos).all(), frame
        under = sr.ground_b(pos[:, 0], pos[:, 2]) - (pos[:, 1] - yoff)
        down = out["airborne"] == 0
        worst = max(worst, float((under - radius)[down].max()) if down.any() else -1.0)
        transit = max(transit, float(under[~down].max()) if (~down).any() else 0.0)
        assert (under[down] <= radius[down]).all(), (frame, under[down].max())
        assert (under[~down] <= np.sqrt(2 * 9.8 * 3.0) * DT + radius[~down]).all(), (frame, under[~down].max())
    print("deepest grounded feet below the terrain, less the radius:", worst, "deepest in transit:", transit)
    assert landed.all() and (out["airborne"] == 0).all() and (state == mr.CS_MOVING).all()
    feet = pos[:, 1] - yoff
    assert (np.abs(feet - sr.ground_b(pos[:, 0], pos[:, 2])) <= radius).all()
