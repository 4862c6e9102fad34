"""CPU: character states and animation queues (ABI 46) -- the binding, the refusals, the conditions the GPU tests' inputs
must meet (asserted on the restatement alone), and the rule of clap_amd/csrc/aniq_dev.h compiled for the host against
tests/aniqref.py: the same header the kernels are made of, one character at a time, == on every array."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from clap_amd import _lib
import aniqcases as ac
import aniqref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ar.Batch.FIELDS


def test_abi_46_binds_both_entry_points():
    assert _lib.ABI_VERSION >= 46
    assert "clapgpu_characters_state" in _lib.SYMBOLS and "clapgpu_animation_queue_time" in _lib.SYMBOLS
    assert C.sizeof(_lib.AniqEntry) == 8 == ar.ENTRY.itemsize
    assert tuple(_lib.ANI_NAME_LIST) == ar.NAMES and _lib.ANI_NAMES == len(ar.NAMES)
    for k in ("ENDED", "STARTED", "ADVANCED", "CB_IDLE", "CB_START_MOTION", "CB_ANY_TO_JUMP", "HOST", "OVERFLOW", "STATE_SHIFT"):
        assert getattr(_lib, "ANIQ_" + k) == getattr(ar, k), k
    for k in ("NONE", "IDLE", "START_MOTION", "ANY_TO_JUMP", "HOST"):
        assert getattr(_lib, "ANI_END_" + k) == getattr(ar, "END_" + k), k
    for name, slot in ar.SLOT.items():
        assert getattr(_lib, "ANI_" + name.upper()) == slot, name


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_refusals_come_before_any_device_call(L):
    """no GPU here: a call that got as far as a launch would not return INVALID_ARGUMENTS or OK"""
    bad, ok = _lib.ERR_INVALID_ARGUMENTS, _lib.OK
    m, q = _lib.CharactersMove(0), _lib.Aniq()
    assert L.clapgpu_characters_state(None, None, C.byref(m), 0.0, None) == bad
    assert L.clapgpu_characters_state(None, C.byref(q), None, 0.0, None) == bad
    assert L.clapgpu_animation_queue_time(None, None, 0.0, None) == bad
    assert L.clapgpu_characters_state(None, C.byref(q), C.byref(m), 0.0, None) == ok          # n == 0: nothing is asked
    assert L.clapgpu_animation_queue_time(None, C.byref(q), 0.0, None) == ok
    names = [f for f, _t in _lib.Aniq._fields_ if f not in ("n", "n_anims")]
    full = lambda: _lib.Aniq(3, 2, *[0x1000] * len(names))
    for f in names:                                                                           # every array but mover
        q = full()
        setattr(q, f, None)
        want_state = ok if f in ("mover", "pose_anim", "frame_time", "time_end") else bad
        want_time = ok if f == "mover" else bad
        if want_state == bad:
            assert L.clapgpu_characters_state(None, C.byref(q), C.byref(_lib.CharactersMove(3)), 0.0, None) == bad, f
        if want_time == bad:
            assert L.clapgpu_animation_queue_time(None, C.byref(q), 0.0, None) == bad, f
    q = full()
    q.queue = 0x1008
    assert L.clapgpu_animation_queue_time(None, C.byref(q), 0.0, None) == bad                 # 16-byte aligned
    q = full()
    q.mover = None
    assert L.clapgpu_characters_state(None, C.byref(q), C.byref(_lib.CharactersMove(2, *[0x1000] * 17)), 0.0, None) == bad
    assert L.clapgpu_characters_state(None, C.byref(full()), C.byref(_lib.CharactersMove(3)), 0.0, None) == bad   # no request


def test_frame_refuses_queues_that_do_not_feed_its_pose(L):
    f, ent = _lib.FrameDesc(), _lib.Entities()
    f.entities = C.pointer(ent)
    q = _lib.Aniq(3, 2, *[0x1000] * 16)
    f.aniq = C.pointer(q)
    assert L.clapgpu_frame_issue(None, C.byref(f), 0.0, 0) == _lib.ERR_INVALID_ARGUMENTS     # no pose at all
    sk, an = _lib.Skeleton(), _lib.Animations()
    f.skeleton, f.animations = C.pointer(sk), C.pointer(an)
    for anim, ft, n in ((0x2000, 0x1000, 3), (0x1000, 0x2000, 3), (0x1000, 0x1000, 4)):
        pb = _lib.PoseBatch(n, 0, anim, ft)
        f.pose = C.pointer(pb)
        assert L.clapgpu_frame_issue(None, C.byref(f), 0.0, 0) == _lib.ERR_INVALID_ARGUMENTS, (anim, ft, n)


# ------------------------------------------------------------------------------------------------ the rule, by name
def one(model, state, entries, cur=0, cleared=0, airborne=0, ani_time=0.0):
    a = ac.blank(1, 3)
    for i, e in enumerate(entries):
        a["queue"][0, i] = e
    a["len"][0], a["cur"][0], a["cleared"][0], a["state"][0], a["airborne"][0], a["ani_time"][0] = (
        len(entries), cur, cleared, state, airborne, ani_time)
    return ar.Batch(model, a)


def test_restatement_quirks():
    M = ac.models()
    m = M["all"]
    A = lambda name: m.name_anim[ar.SLOT[name]]
    te = lambda name: float(m.time_end[A(name)])
    # IDLE -> JUMP_START: a clearing push, cleared holds the finished entry for exactly one more frame, the callback
    # fires at the first end and rebuilds the velocity from the stored motion
    b = one(m, ar.CS_IDLE, [(A("idle"), 1, 0, 1.0)])
    b.characters_state([ar.CS_JUMP_START], [[0.5, -2.0]], 1.0)
    ch = b.chars[0]
    assert [e.key()[:3] for e in ch.aniq] == [(A("idle_to_jump"), 0, ar.END_ANY_TO_JUMP)] and ch.cleared == 1
    assert ch.state == ar.CS_JUMP_START and ch.ani_time == 1.0 and b.events[0] == ar.STARTED << ar.STATE_SHIFT
    b.characters_state([ar.CS_MOVING], [[9.0, 9.0]], 1.1)                   # JUMP_START: fallback to IDLE, which returns
    assert ch.state == ar.CS_JUMP_START and [float(v) for v in ch.motion] == [9.0, 9.0]
    ch.motion = [ar.F32(0.5), ar.F32(-2.0)]
    t = 1.0 + te("idle_to_jump") + 0.001
    b.queue_time(t)
    assert b.events[0] & 0xff == ar.ENDED | ar.CB_ANY_TO_JUMP | ar.STARTED
    assert ch.state == ar.CS_JUMPING and ch.airborne == 1 and ch.cleared == 0 and ch.animation == 0
    assert [e.key()[:3] for e in ch.aniq] == [(A("jump"), 1, 0)] and ch.ani_time == t
    jf, ju = ch.jump_forward, ch.jump_upward
    assert ch.vel == [ar.F32(0.5) * jf, ju, ar.F32(-2.0) * jf]
    assert b.pose_anim[0] == A("idle_to_jump")                              # the pose of this frame is the old entry's
    # cleared: MOVING -> IDLE pushes motion_stop (clearing) and idle; motion_stop ends, stays one frame, then idle
    b = one(m, ar.CS_MOVING, [(A("motion"), 1, 0, 1.0)])
    b.characters_state([ar.CS_IDLE], [[0, 0]], 5.0)
    ch = b.chars[0]
    assert [e.animation for e in ch.aniq] == [A("motion_stop"), A("idle")] and ch.cleared == 1 and ch.state == ar.CS_IDLE
    t = 5.0 + te("motion_stop") + 0.001
    b.queue_time(t)
    assert (ch.animation, ch.cleared, ch.ani_time) == (0, 0, 5.0) and b.events[0] & 0xff == ar.ENDED
    b.queue_time(t + ac.DT)
    assert (ch.animation, ch.ani_time) == (1, t + ac.DT) and b.events[0] & 0xff == ar.ENDED | ar.ADVANCED | ar.STARTED
    # a clearing push fires the interrupted entry's callback: motion_start's character_start_motion
    b = one(m, ar.CS_IDLE, [(A("motion_start"), 0, ar.END_START_MOTION, 1.0), (A("motion"), 1, 0, 1.0)])
    b.characters_state([ar.CS_FALLING], [[0, 0]], 2.0)
    assert b.events[0] >> ar.STATE_SHIFT == ar.CB_START_MOTION | ar.STARTED and b.chars[0].state == ar.CS_FALLING
    # ... and character_idle's own push lands in front of the interrupting one
    b = one(m, ar.CS_FALLING, [(A("fall_to_idle"), 0, ar.END_IDLE, 1.0)])
    b.characters_state([ar.CS_MOVING], [[1, 0]], 2.0)
    assert [e.animation for e in b.chars[0].aniq] == [A("idle"), A("jump_to_motion"), A("motion")]
    # a missing jump: cur = -1, the state unchanged, the host's at the next clock
    p = M["part"]
    P = lambda name: p.name_anim[ar.SLOT[name]]
    b = one(p, ar.CS_MOVING, [(P("motion"), 1, 0, 1.0)])
    b.characters_state([ar.CS_JUMP_START], [[1, 1]], 1.0)
    ch = b.chars[0]
    assert ch.state == ar.CS_JUMP_START and ch.airborne == 1 and ch.aniq[0].end == ar.END_ANY_TO_JUMP
    b.queue_time(1.0 + float(p.time_end[P("motion_to_jump")]) + 0.01)
    assert (ch.animation, len(ch.aniq), ch.state, ch.cleared) == (-1, 0, ar.CS_JUMP_START, 0)
    before = b.arrays()
    b.queue_time(3.0)
    assert b.events[0] & 0xff == ar.HOST
    after = b.arrays()
    assert all(np.array_equal(before[k], after[k]) for k in FIELDS if k != "events")
    # an appending push on four entries: the host's, OVERFLOW, nothing written
    b = one(m, ar.CS_JUMPING, [(A("idle"), 1, 0, 1.0)] * 4, cur=3, airborne=1)
    before = b.arrays()
    b.characters_state([ar.CS_MOVING], [[0, 0]], 1.0)                       # airborne JUMPING -> MOVING: only the append
    assert b.events[0] >> ar.STATE_SHIFT == ar.HOST | ar.OVERFLOW and b.chars[0].state == ar.CS_JUMPING
    after = b.arrays()
    assert all(np.array_equal(before[k], after[k]) for k in FIELDS if k != "events")


# ------------------------------------------------------------------------------------------------ conditions on the inputs
@pytest.fixture(scope="module")
def walks():
    """every walk of the GPU tests on the restatement with a queue of unlimited length: (batch, ever host-owned [n])"""
    out = {}
    for name in ac.WALKS:
        model, start, request, airborne, motion = ac.walk(name)
        b = ar.Batch(model, start, limit=None)
        ever = np.zeros(b.n, bool)

        def each(f, b, ever=ever):
            ever |= b.host_owned()
        ac.run_walk(b, request, airborne, motion, each=each)
        out[name] = (b, ever, request)
    return out


def test_no_input_that_is_not_meant_to_overflow_holds_more_than_four_entries(walks):
    for name, (b, _ever, _r) in walks.items():
        assert 2 <= b.longest <= ar.ANIQ_MAX, (name, b.longest)
    for mname, model in ac.models().items():
        for past in (False, True):
            a, request, motion, now = ac.transition_table(model, past)
            overflow_meant = a["len"] == ar.ANIQ_MAX
            b = ar.Batch(model, a, limit=None)
            b.characters_state(request, motion, now)
            b.queue_time(now)
            longest = np.asarray([len(ch.aniq) for ch in b.chars])
            assert (longest[~overflow_meant] <= ar.ANIQ_MAX).all(), mname
            assert (longest[overflow_meant] > ar.ANIQ_MAX).any(), mname          # and the ones meant to, do


def test_walk_with_every_name_never_needs_the_host(walks):
    for name in ("all", "all_air"):
        b, ever, request = walks[name]
        assert not ever.any(), (name, np.flatnonzero(ever)[:8])
        states = np.bincount([ch.state for ch in b.chars], minlength=7)
        assert (states[ar.CS_IDLE:] > 0).all(), (name, states)                    # the walk ends in every state past WAKING
    assert (walks["all"][2] == ar.CS_NONE).any()


def test_walk_with_missing_names_leaves_half_the_characters_to_the_device(walks):
    b, ever, _r = walks["part"]
    assert 0.5 * b.n <= (~ever).sum() < b.n, (~ever).sum()
    assert ever.sum() > 0.2 * b.n                                                 # and the missing names do bite


# ------------------------------------------------------------------------------------------------ the header, on the host
@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    """clap_amd/csrc/aniq_dev.h through tests/aniq_host.cpp, as a shared object; -ffp-contract=off as the device build"""
    so = tmp_path_factory.mktemp("aniq") / "aniq_host.so"
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "clap_amd", "csrc"),
           os.path.join(ROOT, "tests", "aniq_host.cpp"), "-o", str(so)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return C.CDLL(str(so))


class HostArrays:
    """the arrays of a clapgpu_aniq in host memory, for the host build of the rule"""

    def __init__(self, model, a):
        self.a = {k: np.ascontiguousarray(v).copy() for k, v in a.items()}
        n = len(a["len"])
        raw = np.zeros(n * 32 + 16, np.uint8)                                     # the queue, 16-byte aligned
        off = -raw.ctypes.data % 16
        self.a["queue"] = raw[off:off + n * 32].view(ar.ENTRY).reshape(n, ar.ANIQ_MAX)
        self.a["queue"][:] = a["queue"]
        self._raw = raw
        self.name_anim = np.asarray(model.name_anim, np.int32)
        self.time_end = np.ascontiguousarray(model.time_end, np.float32)
        p = lambda x: x.ctypes.data
        self.desc = _lib.Aniq(n, model.n_anims, p(self.name_anim), p(self.time_end),
                              *[p(self.a[k]) for k in ("queue", "len", "cur", "cleared", "ani_time", "state", "airborne",
                                                       "velocity", "ch_motion", "jump_params")],
                              None, *[p(self.a[k]) for k in ("pose_anim", "frame_time", "events")])

    def state(self, lib, request, motion, now):
        request, motion = np.ascontiguousarray(request, np.uint8), np.ascontiguousarray(motion, np.float32)
        lib.aniq_host_state(C.byref(self.desc), C.c_uint32(len(request)), C.c_void_p(request.ctypes.data),
                            C.c_void_p(motion.ctypes.data), C.c_double(now))

    def time(self, lib, now):
        lib.aniq_host_time(C.byref(self.desc), C.c_double(now))


def assert_same(got, want, what):
    for k in FIELDS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        same = g.view(np.uint8).reshape(len(g), -1) == w.view(np.uint8).reshape(len(w), -1)
        assert same.all(), (what, k, np.flatnonzero(~same.all(axis=1))[:8])


@pytest.mark.parametrize("mname", ["all", "part"])
@pytest.mark.parametrize("past", [False, True], ids=["before_end", "past_end"])
def test_host_build_of_the_rule_on_the_transition_table(host_rule, mname, past):
    model = ac.models()[mname]
    a, request, motion, now = ac.transition_table(model, past)
    ref, h = ar.Batch(model, a), HostArrays(model, a)
    ref.characters_state(request, motion, now)
    h.state(host_rule, request, motion, now)
    assert_same(h.a, ref.arrays(), "state")
    ev = ref.events >> ar.STATE_SHIFT
    assert (ev & ar.HOST).any() and (ev & ar.OVERFLOW).any() and (ev & ar.CB_ANY_TO_JUMP).any() and (ev & ar.CB_IDLE).any()
    ref.queue_time(now)
    h.time(host_rule, now)
    assert_same(h.a, ref.arrays(), "state, then the clock")
    # the clock alone, on the table as given
    ref, h = ar.Batch(model, a), HostArrays(model, a)
    ref.queue_time(now)
    h.time(host_rule, now)
    assert_same(h.a, ref.arrays(), "clock")
    assert bool((ref.events & ar.ENDED).any()) == past


@pytest.mark.parametrize("name", list(ac.WALKS))
def test_host_build_of_the_rule_on_the_walks(host_rule, name):
    model, start, request, airborne, motion = ac.walk(name)
    n, frames = 200, 150                                                           # the GPU test runs all of it
    start = {k: v[:n] for k, v in start.items()}
    ref, h = ar.Batch(model, start), HostArrays(model, start)
    for f in range(frames):
        now = ac.WALK_T0 + (f + 1) * ac.DT
        asked = request[f, :n] != ar.CS_NONE
        h.a["airborne"][asked] = airborne[f, :n][asked]
        for c in np.flatnonzero(asked):
            ref.chars[c].airborne = int(airborne[f, c])
        ref.characters_state(request[f, :n], motion[f, :n], now)
        h.state(host_rule, request[f, :n], motion[f, :n], now)
        ref.queue_time(now)
        h.time(host_rule, now)
        assert_same(h.a, ref.arrays(), (name, f))


# ------------------------------------------------------------------------------------------------ the reference's own code
TRACE = os.path.join(ROOT, "tests", "golden", "aniq_trace.npz")
TRACE_FIELDS = ("state", "airborne", "velocity", "cur", "len", "q_anim", "q_repeat", "q_end", "q_speed", "cleared", "ani_time")


def record_key(t, pfx, at):
    """one record of the trace as a tuple of plain values, floats and doubles by bit pattern"""
    n = min(int(t[pfx + "_len"][at]), ar.ANIQ_MAX)
    q = tuple((int(t[pfx + "_q_anim"][at][i]), int(t[pfx + "_q_repeat"][at][i]), int(t[pfx + "_q_end"][at][i]),
               int(t[pfx + "_q_speed"][at][i].view(np.uint32))) for i in range(n))
    return (int(t[pfx + "_state"][at]), int(t[pfx + "_airborne"][at]), tuple(int(v) for v in t[pfx + "_velocity"][at].view(np.uint32)),
            int(t[pfx + "_cur"][at]), int(t[pfx + "_len"][at]), q, int(t[pfx + "_cleared"][at]),
            int(t[pfx + "_ani_time"][at].view(np.uint64)))


def char_key(ch):
    return (ch.state, ch.airborne, tuple(int(ar.F32(v).view(np.uint32)) for v in ch.vel), ch.animation, len(ch.aniq),
            tuple(e.key() for e in ch.aniq), ch.cleared, int(np.float64(ch.ani_time).view(np.uint64)))


def adopt(ch, t, pfx, at):
    """the host's doing: the character as the reference left it (ch->motion is not part of a record and stays)"""
    ch.state, ch.airborne = int(t[pfx + "_state"][at]), int(t[pfx + "_airborne"][at])
    ch.vel = [ar.F32(v) for v in t[pfx + "_velocity"][at]]
    n = int(t[pfx + "_len"][at])
    assert n <= ar.ANIQ_MAX
    ch.aniq = [ar.Entry(t[pfx + "_q_anim"][at][i], t[pfx + "_q_repeat"][at][i], t[pfx + "_q_end"][at][i], t[pfx + "_q_speed"][at][i])
               for i in range(n)]
    ch.animation, ch.cleared, ch.ani_time = int(t[pfx + "_cur"][at]), int(t[pfx + "_cleared"][at]), float(t[pfx + "_ani_time"][at])
    ch.tail, ch.raw_len = [], None


def test_restatement_replays_the_reference_trace():
    """tests/golden/aniq_trace.npz (see aniq_trace.README.md): the reference's character_set_state, animated_update and
    end callbacks on 32 body-less characters of two models over 240 frames, every field after each of a frame's two
    steps.  The restatement, given the same inputs, gives the same fields, ==; where it declares a step the host's the
    reference's result is adopted (that is what the host would do) and the replay goes on."""
    t = dict(np.load(TRACE))
    frames, n = t["request"].shape
    assert (frames, n) == (240, 32)
    M = [ar.Model(t["name_anim"][0], t["time_end_all"]), ar.Model(t["name_anim"][1], t["time_end_part"])]
    assert (t["name_anim"][0] >= 0).all() and sorted(np.flatnonzero(t["name_anim"][1] < 0)) == sorted(
        ar.SLOT[k] for k in ("motion_start", "idle_to_jump", "jump"))
    chars = []
    for c in range(n):
        ch = ar.Char()
        ch.motion = [ar.F32(0), ar.F32(0)]
        ch.jump_forward, ch.jump_upward = ar.F32(t["jump_params"][c, 0]), ar.F32(t["jump_params"][c, 1])
        adopt(ch, t, "i", c)
        chars.append(ch)
    compared = hosted = 0
    seen = 0
    for f in range(frames):
        now = float(t["now"][f])
        for c, ch in enumerate(chars):
            model, req = M[t["char_model"][c]], int(t["request"][f, c])
            if req != ar.CS_NONE:
                ch.airborne = int(t["airborne"][f, c])
                ev, _ = ar.characters_state_one(ch, model, req, t["motion"][f, c], now)
                if ev & ar.HOST:
                    if req in (ar.CS_JUMP_START, ar.CS_MOVING, ar.CS_IDLE):
                        ch.motion = [ar.F32(t["motion"][f, c, 0]), ar.F32(t["motion"][f, c, 1])]
                    adopt(ch, t, "a", (f, c))
                    hosted += 1
                else:
                    seen |= ev
                    compared += 1
            assert char_key(ch) == record_key(t, "a", (f, c)), ("state step", f, c)
            ev, _out, _ = ar.queue_time_one(ch, model, now)
            if ev & ar.HOST:
                adopt(ch, t, "b", (f, c))
                hosted += 1
            else:
                seen |= ev
                compared += 1
                assert char_key(ch) == record_key(t, "b", (f, c)), ("animated_update", f, c)
    print(f"aniq trace: {compared} steps compared, {hosted} the host's, events seen {seen:#x}")
    assert compared > 0.9 * (compared + hosted) and hosted > 0
    assert seen == ar.ENDED | ar.STARTED | ar.ADVANCED | ar.CB_IDLE | ar.CB_START_MOTION | ar.CB_ANY_TO_JUMP
    assert os.path.getsize(TRACE) <= max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f))
                                         for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f != "aniq_trace.npz"
                                         and os.path.isfile(os.path.join(ROOT, "tests", "golden", f)))
