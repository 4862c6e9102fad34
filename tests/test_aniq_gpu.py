"""GPU: clapgpu_characters_state and clapgpu_animation_queue_time against tests/aniqref.py -- the transition table, the
random walks, the quirks by name, host-owned characters, the frame with both calls in it (one stream, three chains, a
captured graph).  Every comparison is == on bit patterns: there is no libm in the rule, the doubles are one subtraction
and one product, the floats one product per velocity component, all without contraction.  Every array of the mirrors
lies between the guard bands of tests/guards.py.  (The restatement itself is held to the reference's own code, and
the inputs to their conditions, in test_aniq.py.)"""
import numpy as np
import pytest
import torch

from clap_amd import _dev, _lib, animation, synth
import aniqcases as ac
import aniqref as ar
import guards

pytestmark = pytest.mark.gpu
FIELDS = ar.Batch.FIELDS
UP = ("queue", "len", "cur", "cleared", "ani_time", "state", "airborne", "velocity", "ch_motion", "jump_params")


class Requests:
    """what clapgpu_characters_state reads of a clapgpu_move: n, request, motion"""

    def __init__(self, n, dev):
        self.n = n
        self.request = _dev.device_array(max(n, 1), torch.uint8, dev, 0xff)
        self.motion = _dev.device_array((max(n, 1), 2), torch.float32, dev)
        self._desc = _lib.CharactersMove(n)
        self._desc.request, self._desc.motion = self.request.data_ptr(), self.motion.data_ptr()

    def set(self, request, motion):
        if self.n:
            self.request[:self.n].copy_(torch.from_numpy(np.ascontiguousarray(request, np.uint8)))
            self.motion[:self.n].copy_(torch.from_numpy(np.ascontiguousarray(motion, np.float32).reshape(-1, 2)))


def queues(model, a, dev, **kw):
    n = len(a["len"])
    aq = animation.AnimationQueues(n, model.name_anim, model.time_end, device=dev, **kw, **{k: a[k] for k in UP})
    if n:                                                   # the outputs start from what the reference batch starts from
        aq.pose_anim[:n].copy_(torch.from_numpy(a["pose_anim"].view(np.int32)))
        aq.frame_time[:n].copy_(torch.from_numpy(a["frame_time"]))
        aq.events[:n].copy_(torch.from_numpy(a["events"].view(np.int32)))
    return aq


def assert_same(got, want, what):
    for k in FIELDS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape[0] == w.shape[0], (what, k)
        if not g.shape[0]:
            continue
        same = g.view(np.uint8).reshape(len(g), -1) == w.view(np.uint8).reshape(len(w), -1)
        assert same.all(), (what, k, np.flatnonzero(~same.all(axis=1))[:8])


@pytest.fixture
def g(cuda_device, monkeypatch):
    reg = guards.Guards(cuda_device)
    guards.install(monkeypatch, reg)
    yield reg
    reg.check("at the end of the test")


def take(a, idx):
    return {k: v[idx] for k, v in a.items()}


# ------------------------------------------------------------------------------------------------- 1. the transition table
@pytest.mark.parametrize("mname", ["all", "part"])
def test_transition_table(cuda_device, g, mname):
    model = ac.models()[mname]
    for past in (False, True):
        a, request, motion, now = ac.transition_table(model, past)
        n = len(request)
        assert n > 1500
        # the state call, then the clock on what it left
        ref, aq, rq = ar.Batch(model, a), queues(model, a, cuda_device), Requests(n, cuda_device)
        rq.set(request, motion)
        ref.characters_state(request, motion, now)
        aq.characters_state(rq, now)
        assert_same(aq.download(), ref.arrays(), ("state", past))
        ev = ref.events >> ar.STATE_SHIFT
        for bit in (ar.STARTED, ar.CB_IDLE, ar.CB_START_MOTION, ar.CB_ANY_TO_JUMP, ar.HOST, ar.OVERFLOW):
            assert (ev & bit).any(), bit
        ref.queue_time(now)
        aq.queue_time(now)
        assert_same(aq.download(), ref.arrays(), ("state, then the clock", past))
        # the clock alone on the table as given
        ref, aq = ar.Batch(model, a), queues(model, a, cuda_device)
        ref.queue_time(now)
        aq.queue_time(now)
        assert_same(aq.download(), ref.arrays(), ("clock", past))
        ev = ref.events & 0xff
        assert bool((ev & ar.ENDED).any()) == past
        if past:
            for bit in (ar.ADVANCED, ar.STARTED, ar.CB_IDLE, ar.CB_START_MOTION, ar.CB_ANY_TO_JUMP, ar.HOST):
                assert (ev & bit).any(), bit
        g.check(("table", past))


@pytest.mark.parametrize("n", [0, 1, 255, 257])
def test_sizes_around_a_block(cuda_device, g, n):
    """256 lanes a block: one short, one over, one alone, none; through a mover table that reverses the movers and
    leaves every seventh character without one"""
    model = ac.models()["all"]
    a, request, motion, now = ac.transition_table(model, True, seed=5)
    pickn = ac.rng(n).choice(len(request), n, replace=False)
    a, request, motion = take(a, pickn), request[pickn], motion[pickn]
    for mover in (None, np.where(np.arange(n) % 7 == 3, -1, n - 1 - np.arange(n)).astype(np.int32)):
        ref = ar.Batch(model, a)
        aq = queues(model, a, cuda_device, mover=mover)
        rq = Requests(n, cuda_device)
        rq.set(request, motion)
        ref.characters_state(request, motion, now, mover=mover)
        aq.characters_state(rq, now)
        assert_same(aq.download(), ref.arrays(), ("state", n))
        ref.queue_time(now)
        aq.queue_time(now)
        assert_same(aq.download(), ref.arrays(), ("clock", n))


# ------------------------------------------------------------------------------------------------- 2. the random walks
@pytest.mark.parametrize("name", list(ac.WALKS))
def test_random_walk(cuda_device, g, name):
    """1 000 characters x 300 frames of state call + queue clock; every array, every frame"""
    model, start, request, airborne, motion = ac.walk(name)
    n, frames = request.shape[1], request.shape[0]
    ref, aq, rq = ar.Batch(model, start), queues(model, start, cuda_device), Requests(n, cuda_device)
    ever = np.zeros(n, bool)
    seen = 0
    for f in range(frames):
        now = ac.WALK_T0 + (f + 1) * ac.DT
        asked = request[f] != ar.CS_NONE
        for c in np.flatnonzero(asked):                      # the move's airborne
            ref.chars[c].airborne = int(airborne[f, c])
        on = torch.from_numpy(asked).to(cuda_device)
        aq.airborne[:n] = torch.where(on, torch.from_numpy(airborne[f]).to(cuda_device), aq.airborne[:n])
        rq.set(request[f], motion[f])
        ref.characters_state(request[f], motion[f], now)
        aq.characters_state(rq, now)
        ref.queue_time(now)
        aq.queue_time(now)
        assert_same(aq.download(), ref.arrays(), (name, f))
        ever |= ref.host_owned()
        seen |= int(np.bitwise_or.reduce(ref.events))
    want = ar.ENDED | ar.STARTED | ar.ADVANCED | ar.CB_IDLE | ar.CB_ANY_TO_JUMP
    if name != "part":                                       # (no motion_start there: nobody installs that callback)
        want |= ar.CB_START_MOTION
    assert seen & want == want and (seen >> ar.STATE_SHIFT) & ar.STARTED, hex(seen)
    assert ever.any() == (name == "part")


# ------------------------------------------------------------------------------------------------- 3. quirks, by name
def one(model, state, entries, dev, cur=0, cleared=0, airborne=0, ani_time=0.0, n=1):
    a = ac.blank(n, 3)
    for i, e in enumerate(entries):
        a["queue"][:, i] = e
    a["len"][:], a["cur"][:], a["cleared"][:], a["state"][:], a["airborne"][:], a["ani_time"][:] = (
        len(entries), cur, cleared, state, airborne, ani_time)
    return a, queues(model, a, dev), Requests(n, dev)


def test_cleared_delays_the_advance_by_exactly_one_frame(cuda_device, g):
    m = ac.models()["all"]
    A = lambda name: m.name_anim[ar.SLOT[name]]
    _a, aq, rq = one(m, ar.CS_MOVING, [(A("motion"), 1, 0, 1.0)], cuda_device)
    rq.set([ar.CS_IDLE], [[0, 0]])
    aq.characters_state(rq, 5.0)
    d = aq.download()
    assert list(d["queue"]["animation"][0, :2]) == [A("motion_stop"), A("idle")] and d["len"][0] == 2
    assert (d["cur"][0], d["cleared"][0], d["state"][0], d["ani_time"][0]) == (0, 1, ar.CS_IDLE, 5.0)
    t = 5.0 + float(m.time_end[A("motion_stop")]) + 0.001
    aq.queue_time(t - 0.002)
    assert aq.download()["events"][0] & 0xff == 0
    aq.queue_time(t)                                         # it ends: held for this frame
    d = aq.download()
    assert (d["cur"][0], d["cleared"][0], d["ani_time"][0], d["events"][0] & 0xff) == (0, 0, 5.0, ar.ENDED)
    assert d["pose_anim"][0] == A("motion_stop") and d["frame_time"][0] == np.float32(t - 5.0)
    aq.queue_time(t + ac.DT)                                 # and advanced in the next
    d = aq.download()
    assert (d["cur"][0], d["ani_time"][0]) == (1, t + ac.DT)
    assert d["events"][0] & 0xff == ar.ENDED | ar.ADVANCED | ar.STARTED and d["pose_anim"][0] == A("motion_stop")
    aq.queue_time(t + 2 * ac.DT)
    d = aq.download()
    assert d["pose_anim"][0] == A("idle") and d["frame_time"][0] == np.float32((t + 2 * ac.DT) - (t + ac.DT))


def test_a_clearing_push_fires_the_interrupted_entry_s_callback(cuda_device, g):
    m = ac.models()["all"]
    A = lambda name: m.name_anim[ar.SLOT[name]]
    _a, aq, rq = one(m, ar.CS_IDLE, [(A("motion_start"), 0, ar.END_START_MOTION, 1.0), (A("motion"), 1, 0, 1.0)], cuda_device)
    rq.set([ar.CS_FALLING], [[0, 0]])
    aq.characters_state(rq, 2.0)
    d = aq.download()
    assert d["events"][0] >> ar.STATE_SHIFT == ar.CB_START_MOTION | ar.STARTED
    assert (d["state"][0], d["len"][0], d["queue"]["animation"][0, 0], d["queue"]["repeat"][0, 0]) == (ar.CS_FALLING, 1, A("fall"), 1)
    # character_idle's own push lands in front of the interrupting one
    _a, aq, rq = one(m, ar.CS_FALLING, [(A("fall_to_idle"), 0, ar.END_IDLE, 1.0)], cuda_device)
    rq.set([ar.CS_MOVING], [[1, 0]])
    aq.characters_state(rq, 2.0)
    d = aq.download()
    assert list(d["queue"]["animation"][0, :3]) == [A("idle"), A("jump_to_motion"), A("motion")] and d["state"][0] == ar.CS_MOVING
    assert d["events"][0] >> ar.STATE_SHIFT == ar.CB_IDLE | ar.STARTED


def test_any_to_jump_uses_the_motion_of_the_jump_frame(cuda_device, g):
    m = ac.models()["all"]
    A = lambda name: m.name_anim[ar.SLOT[name]]
    a, aq, rq = one(m, ar.CS_IDLE, [(A("idle"), 1, 0, 1.0)], cuda_device)
    rq.set([ar.CS_JUMP_START], [[0.5, -2.0]])
    aq.characters_state(rq, 1.0)
    rq.set([ar.CS_FALLING], [[9.0, 9.0]])                    # this frame's motion differs, and FALLING does not store it
    t = 1.0 + float(m.time_end[A("idle_to_jump")]) + 0.001
    aq.characters_state(rq, t)
    aq.queue_time(t)
    d = aq.download()
    jf, ju = a["jump_params"][0]
    assert d["events"][0] & 0xff == ar.ENDED | ar.CB_ANY_TO_JUMP | ar.STARTED
    assert list(d["velocity"][0]) == [np.float32(0.5) * jf, ju, np.float32(-2.0) * jf]
    assert list(d["ch_motion"][0]) == [0.5, -2.0]
    assert (d["state"][0], d["airborne"][0], d["queue"]["animation"][0, 0], d["cleared"][0]) == (ar.CS_JUMPING, 1, A("jump"), 0)


def test_a_missing_jump_leaves_the_character_to_the_host_at_the_next_clock(cuda_device, g):
    p = ac.models()["part"]
    P = lambda name: p.name_anim[ar.SLOT[name]]
    _a, aq, rq = one(p, ar.CS_MOVING, [(P("motion"), 1, 0, 1.0)], cuda_device)
    rq.set([ar.CS_JUMP_START], [[1, 1]])
    aq.characters_state(rq, 1.0)
    aq.queue_time(1.0 + float(p.time_end[P("motion_to_jump")]) + 0.01)
    d = aq.download()
    assert (d["cur"][0], d["len"][0], d["state"][0], d["airborne"][0]) == (-1, 0, ar.CS_JUMP_START, 1)
    assert d["events"][0] & 0xff == ar.ENDED | ar.CB_ANY_TO_JUMP
    aq.queue_time(3.0)
    e = aq.download()
    assert e["events"][0] & 0xff == ar.HOST
    assert all(np.array_equal(d[k], e[k]) for k in FIELDS if k != "events")


# ------------------------------------------------------------------------------------------------- 4. host-owned characters
def test_host_owned_characters_keep_every_byte(cuda_device, g):
    for mname, model in ac.models().items():
        a, request, motion, now = ac.transition_table(model, True, seed=9)
        ref = ar.Batch(model, a)
        ref.characters_state(request, motion, now)
        host_s = (ref.events >> ar.STATE_SHIFT) & ar.HOST != 0
        ref = ar.Batch(model, a)
        ref.queue_time(now)
        host_t = ref.events & ar.HOST != 0
        assert host_s.sum() > 50 and host_t.sum() > 50 and (host_s & ~host_t).any()
        n = len(request)
        aq, rq = queues(model, a, cuda_device), Requests(n, cuda_device)
        rq.set(request, motion)
        before = {k: getattr(aq, k)[:n].clone() for k in UP + ("pose_anim", "frame_time")}
        aq.characters_state(rq, now)
        torch.cuda.synchronize()
        rows = torch.from_numpy(np.flatnonzero(host_s)).to(cuda_device)
        for k, t in before.items():
            assert torch.equal(getattr(aq, k)[:n][rows].view(torch.uint8), t[rows].view(torch.uint8)), (mname, "state", k)
        for k, t in before.items():                          # the clock, on the table as given
            getattr(aq, k)[:n].copy_(t)
        aq.queue_time(now)
        torch.cuda.synchronize()
        rows = torch.from_numpy(np.flatnonzero(host_t)).to(cuda_device)
        for k, t in before.items():
            assert torch.equal(getattr(aq, k)[:n][rows].view(torch.uint8), t[rows].view(torch.uint8)), (mname, "clock", k)
        ev = aq.download()["events"]
        assert ((ev[host_t] & 0xff) & ~np.uint32(ar.OVERFLOW) == ar.HOST).all()


# ------------------------------------------------------------------------------------------------- 5. the frame
NB, NC, J, VPC = 200, 12, 24, 90                            # the smallest scene of test_frame_gpu.py, its bodies capsules


def frame_setup(dev, with_aniq):
    """-> (loop, parts): FrameLoop(move=, aniq=) when with_aniq, else the frame without move, queues and pose, for the
    stand-alone sequence"""
    from clap_amd import characters, entities, frame, physics, tiler
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
    cf._desc.airborne = m.airborne.data_ptr()                                   # the hooks read what the move left
    sk = synth.skeleton(J, 5, seed=5)
    full = ac.models()["all"]
    model = ar.Model(full.name_anim, full.time_end / np.float32(8))            # 3 to 12 frames each: they end within the test
    anims = [synth.animation(J, 6, float(te), seed=40 + i) for i, te in enumerate(model.time_end)]
    sm = animation.SkinnedModel(sk, anims, mesh=synth.skinned_mesh(VPC, J, seed=5), device=dev)
    ch = synth.characters(NC, J, seed=5)
    cb = animation.CharacterBatch(sm, NC, ch["trs0"], batch.mx, entity_index=char_e, vert_first=np.zeros(NC, np.uint32),
                                  vert_count=np.full(NC, VPC, np.uint32))
    cb.set_outputs(trs=True, joint_pos=True)
    start = ac.walk_start(model, NC, 17)
    start["ani_time"][:] = -np.linspace(0.0, 0.1, NC)
    aq = animation.AnimationQueues(NC, model.name_anim, sm.time_end, batch=cb, moves=m,
                                   **{k: start[k] for k in ("queue", "len", "cur", "cleared", "ani_time", "ch_motion")})
    cam = synth.camera(pos=(0, 10, 60))
    if with_aniq:
        loop = frame.FrameLoop(batch, cam, world=w, feed=cf, characters=cb, contacts=True, move=m, aniq=aq)
    else:
        loop = frame.FrameLoop(batch, cam, world=w, feed=cf, contacts=True)
    return loop, dict(w=w, batch=batch, m=m, cf=cf, cb=cb, aq=aq)


def frame_state(p):
    torch.cuda.synchronize()
    out = {"aq_" + k: v for k, v in p["aq"].download().items()}
    out.update({"move_" + k: t.cpu().numpy().copy() for k, t in p["m"].outputs().items()})
    out["move_state"] = p["m"].state.cpu().numpy().copy()
    wd = p["w"].download()
    out.update({"w_" + k: wd[k] for k in ("pos", "quat", "lvel", "pairs")})
    e = p["batch"].download()
    out.update(e_mx=e["mx"], e_visible=e["visible"])
    c = p["cb"].download()
    out.update(jt=c["joint_transforms"], jpos=c["joint_pos"], skinned=c["out_position"])
    out.update({"cf_" + k: v for k, v in p["cf"].download().items()})
    return out


def frame_inputs(p, f):
    """the host between frames: this frame's stick and jump button (the states are the device's now)"""
    R = ac.rng(200 + f)
    n = p["m"].n
    walking = (np.arange(n) + f // 6) % 3 != 0
    p["m"].set(motion=(R.normal(0, 2, (n, 2)) * walking[:, None]).astype(np.float32), jump=R.integers(0, 10, n) == 0,
               yaw_quat=np.tile(np.float32([0, 0, 0, 1]), (n, 1)))


def test_frame_with_the_queues_is_the_stand_alone_sequence(cuda_device, g):
    """move -> state -> substeps -> hooks -> queue clock -> pose, as one frame call on one stream, on three chains and
    replayed from a captured graph, against the same calls made one by one; 20 frames"""
    dt = 1.0 / 120.0                                         # one substep a frame: what a captured frame holds
    loops = {k: frame_setup(cuda_device, True) for k in ("one_stream", "overlap", "graph")}
    alone, pa = frame_setup(cuda_device, False)
    loops["overlap"][0].overlap = True
    for k, (loop, p) in loops.items():                       # frame 1 (capture() issues it eagerly)
        frame_inputs(p, 1)
    frame_inputs(pa, 1)

    def stand_alone(now):
        pa["w"].characters_move(pa["m"], dt)
        pa["aq"].characters_state(pa["m"], now)
        alone.clap_frame(now, dt)
        pa["aq"].queue_time(now)
        pa["cb"].pose_update()
        pa["cb"].skin()

    loops["one_stream"][0].clap_frame(dt, dt)
    loops["overlap"][0].clap_frame(dt, dt)
    loops["graph"][0].capture(dt, warmup_now=dt)
    stand_alone(dt)
    seen = 0
    for f in range(2, 21):
        now = f * dt
        for _loop, p in loops.values():
            frame_inputs(p, f)
        frame_inputs(pa, f)
        loops["one_stream"][0].clap_frame(now, dt)
        loops["overlap"][0].clap_frame(now, dt)
        loops["graph"][0].clap_frame_replay(now)
        stand_alone(now)
        want = frame_state(pa)
        for k, (_loop, p) in loops.items():
            got = frame_state(p)
            assert got.keys() == want.keys()
            for key in want:
                assert np.array_equal(got[key], want[key]), (k, f, key)
        seen |= int(np.bitwise_or.reduce(want["aq_events"]))
    states = set(want["move_state"].tolist())
    print("frame: events seen", hex(seen), "states", sorted(states))
    assert seen & ar.ENDED and seen & (ar.STARTED << ar.STATE_SHIFT) and len(states) > 1     # the device moved the states itself
    assert not (want["aq_events"] & (ar.HOST | ar.HOST << ar.STATE_SHIFT)).any()


def test_frame_without_the_queues_is_the_frame_before(cuda_device, g):
    """aniq NULL: the plain clock, fused with the hooks as before -- the clock's arrays, not the queues', move"""
    loop, p = frame_setup(cuda_device, True)
    f = loop._build()
    f.aniq = None
    before = {k: v.copy() for k, v in p["aq"].download().items()}
    frame_inputs(p, 1)
    loop.clap_frame(0.5, 1.0 / 120.0)
    after = p["aq"].download()
    for k in ("queue", "len", "cur", "cleared", "ani_time", "ch_motion", "events"):
        assert np.array_equal(before[k], after[k]), k
    assert (p["cb"].download_clock()["frame_time"] == np.float32(0.5)).all()      # anim 0 from ani_time 0 at speed 1
