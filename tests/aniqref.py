"""The character state machine and its animation queue, restated in Python from the reference, line by line.

Nothing here imports the device code.  The functions follow
  character_idle / character_start_motion / character_any_to_jump     character.c:86-121
  character_set_state                                                  character.c:316-426
  animation_start, ani_current, animation_end, animation_next          model.c:1406-1483
  animation_set_end_callback, animation_push_by_name, animated_update  model.c:1485-1592
with the reference's own recursion (a push calls a callback that calls set_state that pushes) and a queue of unlimited
length, so that an overflow of the device's CLAPGPU_ANIQ_MAX entries can be reported rather than suffered.  What the
library adds to the reference is the notion of a HOST-OWNED character (include/clapgpu.h): a step that would need the
host -- an empty or exhausted queue on entry (animation_next would draw drand48), an animation index outside the model,
an end code 0xff, a fifth entry, (cur + 1) % 0 -- leaves the character untouched and says so in its events word.

Left out of set_state's case CS_MOVING: character_apply_velocity and character_set_moved (:350-351), which
clapgpu_characters_move has done.  The joint cursors animation_start resets have no counterpart (the pose brackets a
key time without a cursor); sfx_state is the host's (STARTED tells it when to reset it).

Numbers: ani_time and now are doubles (Python floats), speed, time_end, velocity, motion and jump parameters float32
(numpy scalars): the jump velocity is one float32 product per component, frame_time (float)((now - ani_time) * speed).
"""
import numpy as np

CS_START, CS_WAKING, CS_IDLE, CS_MOVING, CS_JUMP_START, CS_JUMPING, CS_FALLING, CS_NONE = 0, 1, 2, 3, 4, 5, 6, 0xff
END_NONE, END_IDLE, END_START_MOTION, END_ANY_TO_JUMP, END_HOST = 0, 1, 2, 3, 0xff
NAMES = ("idle", "start_to_idle", "motion_stop", "jump_to_idle", "fall_to_idle", "motion", "motion_start",
         "jump_to_motion", "idle_to_jump", "motion_to_jump", "jump", "fall")
SLOT = {name: i for i, name in enumerate(NAMES)}
ENDED, STARTED, ADVANCED, CB_IDLE, CB_START_MOTION, CB_ANY_TO_JUMP, HOST, OVERFLOW = 1, 2, 4, 8, 16, 32, 64, 128
STATE_SHIFT = 8
ANIQ_MAX = 4
ENTRY = np.dtype([("animation", "<u2"), ("repeat", "u1"), ("end", "u1"), ("speed", "<f4")])
F32 = np.float32


class HostOwned(Exception):
    """The step needs the host; overflow: because a push found ANIQ_MAX entries."""

    def __init__(self, overflow=False):
        self.overflow = overflow


class Model:
    """name_anim[12]: animation_by_name of each of NAMES, -1 for none; time_end[n_anims] float32."""

    def __init__(self, name_anim, time_end):
        self.name_anim = [int(v) for v in name_anim]
        assert len(self.name_anim) == len(NAMES)
        self.time_end = np.asarray(time_end, np.float32)
        self.n_anims = len(self.time_end)
        self._te = [float(v) for v in self.time_end]          # (double)an->time_end


class Entry:
    """struct queued_animation (model.h:352-361): animation, repeat, end (a code), speed.  Never changed in place: a
    store into a queued entry replaces the list element (with_end), so that a copy of a queue is a copy of a list."""
    __slots__ = ("animation", "repeat", "end", "speed")

    def __init__(self, animation, repeat, end=END_NONE, speed=F32(1.0)):
        self.animation, self.repeat, self.end, self.speed = int(animation), int(repeat), int(end), F32(speed)

    def with_end(self, end):
        return Entry(self.animation, self.repeat, end, self.speed)

    def key(self):
        return (self.animation, self.repeat, self.end, F32(self.speed).view(np.uint32).item())


class Char:
    """struct character's state, airborne, velocity, motion, jump parameters and its entity's aniq, animation,
    ani_cleared, ani_time.  tail: what the device array holds behind `len` as long as no step has committed."""
    __slots__ = ("state", "airborne", "vel", "motion", "jump_forward", "jump_upward", "aniq", "animation", "cleared",
                 "ani_time", "tail", "raw_len")

    def copy(self):
        c = Char()
        c.state, c.airborne, c.vel, c.motion = self.state, self.airborne, list(self.vel), list(self.motion)
        c.jump_forward, c.jump_upward = self.jump_forward, self.jump_upward
        c.aniq = list(self.aniq)
        c.animation, c.cleared, c.ani_time, c.tail, c.raw_len = self.animation, self.cleared, self.ani_time, [], None
        return c


class Ctx:
    """One step of one character: the model, the frame's clock, the events so far, the queue limit (None: unlimited)."""
    __slots__ = ("model", "now", "events", "limit", "max_len")

    def __init__(self, model, now, limit):
        self.model, self.now, self.events, self.limit, self.max_len = model, float(now), 0, limit, 0


# ------------------------------------------------------------------------------------------------ model.c:1406-1561
def animation_start(ch, cx):
    if not cx.model.n_anims:                                 # :1413-1414
        return
    ch.ani_time = cx.now                                     # :1423
    cx.events |= STARTED


def ani_current(ch):
    if ch.animation < 0 or ch.animation >= len(ch.aniq):     # :1438: an int against a size_t, -1 is "none" too
        return None
    return ch.aniq[ch.animation]


def animation_end(qa, ch, cx, at=None):
    """at: the entry's place in ch.aniq, None for push_by_name's local copy"""
    end = qa.end                                             # :1445
    if not end:
        return
    if at is not None:
        ch.aniq[at] = qa.with_end(END_NONE)                  # :1450 (the copy's is never read again)
    CALLBACKS.get(end, character_host_callback)(ch, cx)      # :1451


def animation_set_end_callback(ch, end):
    if not ch.aniq:                                          # :1489-1490
        return
    ch.aniq[-1] = ch.aniq[-1].with_end(end)


def animation_push_by_name(ch, cx, name, clear, repeat):
    if clear:                                                # :1530-1541
        qa = ani_current(ch)
        _qa = qa                                             # memcpy(&_qa, qa, sizeof(_qa))
        ch.aniq = []
        if qa is not None:
            animation_end(_qa, ch, cx)
    id_ = cx.model.name_anim[SLOT[name]]                     # :1543
    if id_ < 0:
        if clear:
            ch.animation = -1
        return False
    if id_ >= cx.model.n_anims or id_ > 0xffff:
        raise HostOwned()
    if cx.limit is not None and len(ch.aniq) >= cx.limit:
        raise HostOwned(overflow=True)
    ch.aniq.append(Entry(id_, 1 if repeat else 0))           # :1550-1553
    cx.max_len = max(cx.max_len, len(ch.aniq))
    if clear:
        animation_start(ch, cx)
        ch.animation = 0
        ch.cleared = 1
    return True


def animation_next(ch, cx):
    """model.c:1454-1483 for a queue that is not empty, with animation >= 0 (else the character is the host's)"""
    qa = ani_current(ch)                                     # :1471
    if not qa.repeat:
        animation_end(qa, ch, cx, ch.animation)
        if ch.cleared:
            ch.cleared = 0
            return
        if not ch.aniq:
            raise HostOwned()                                # (animation + 1) % 0
        ch.animation = (ch.animation + 1) % len(ch.aniq)
        cx.events |= ADVANCED
        qa = ani_current(ch)
    animation_start(ch, cx)                                  # :1481-1482


def animated_update(ch, cx):
    """model.c:1563-1592 behind its ani_current.  Returns (pose animation, float32 frame time)."""
    qa = ani_current(ch)
    an = qa.animation
    frame_time = (cx.now - ch.ani_time) * float(qa.speed)    # :1578
    out = (an, F32(frame_time))                              # channels_transform(e, an, frame_time), :1582
    if frame_time >= cx.model._te[an]:                       # :1590
        cx.events |= ENDED
        animation_next(ch, cx)
    return out


# ------------------------------------------------------------------------------------------------ character.c:86-121
def character_idle(ch, cx):
    cx.events |= CB_IDLE
    ch.state = CS_IDLE                                       # CS_AWAKE
    animation_push_by_name(ch, cx, "idle", True, True)


def character_start_motion(ch, cx):
    cx.events |= CB_START_MOTION
    ch.state = CS_MOVING


def character_any_to_jump(ch, cx):
    cx.events |= CB_ANY_TO_JUMP
    ch.airborne = 1
    ch.vel = [F32(ch.motion[0]) * F32(ch.jump_forward), F32(ch.jump_upward), F32(ch.motion[1]) * F32(ch.jump_forward)]
    character_set_state(ch, cx, CS_JUMPING)


def character_host_callback(ch, cx):
    raise HostOwned()


CALLBACKS = {END_IDLE: character_idle, END_START_MOTION: character_start_motion, END_ANY_TO_JUMP: character_any_to_jump}


# ------------------------------------------------------------------------------------------------ character.c:316-426
def character_set_state(ch, cx, state):
    push = lambda name, clear, repeat: animation_push_by_name(ch, cx, name, clear, repeat)
    if state != CS_IDLE and ch.state < CS_IDLE:              # :319
        if ch.state == CS_START:
            ch.state = CS_WAKING
            push("start_to_idle", True, False)
            animation_set_end_callback(ch, END_IDLE)
        return
    while True:                                              # fail_fallback:
        if state == CS_IDLE:
            if ch.airborne:
                return
            if ch.state == CS_MOVING:
                push("motion_stop", True, False)
            elif ch.state == CS_JUMPING:
                push("jump_to_idle", True, False)
            elif ch.state == CS_FALLING:
                push("fall_to_idle", True, False)
            elif ch.state <= CS_IDLE or ch.state == CS_JUMP_START:
                return
            push("idle", False, True)
            ch.state = state
            return
        elif state == CS_MOVING:
            # character_apply_velocity, character_set_moved (:350-351): the move's
            if ch.state == CS_IDLE:
                if push("motion_start", True, False):
                    animation_set_end_callback(ch, END_START_MOTION)
                else:
                    state = CS_IDLE
                    continue
            elif ch.state in (CS_FALLING, CS_JUMPING) and not ch.airborne:
                if not push("jump_to_motion", True, False):
                    state = CS_IDLE
                    continue
            elif ch.state == CS_JUMP_START:
                state = CS_IDLE
                continue
            elif ch.state == CS_MOVING:
                return
            if not push("motion", False, True):
                state = CS_IDLE
                continue
            ch.state = state
            return
        elif state == CS_JUMP_START:
            if ch.state == CS_IDLE:
                if push("idle_to_jump", True, False):
                    animation_set_end_callback(ch, END_ANY_TO_JUMP)
                else:
                    state = CS_IDLE
                    continue
            elif ch.state == CS_MOVING:
                ch.airborne = 1                              # :388
                if push("motion_to_jump", True, False):
                    animation_set_end_callback(ch, END_ANY_TO_JUMP)
                else:
                    state = CS_IDLE
                    continue
            elif ch.state in (CS_JUMP_START, CS_JUMPING):
                state = CS_IDLE
                continue
            ch.state = state
            return
        elif state == CS_JUMPING:
            if ch.state == CS_JUMP_START:
                if push("jump", True, True):
                    ch.state = state
                    return
            state = CS_IDLE
            continue
        elif state == CS_FALLING:
            if ch.state in (CS_JUMP_START, CS_JUMPING):
                return
            push("fall", True, True)
            ch.state = state
            return
        else:
            ch.state = state
            return


# ------------------------------------------------------------------------------------------------ the library's two steps
def host_owned_on_entry(ch, model):
    n = len(ch.aniq) if ch.raw_len is None else ch.raw_len
    if n == 0 or n > ANIQ_MAX or ch.animation < 0 or ch.animation >= n:
        return True
    return any(e.animation >= model.n_anims for e in ch.aniq)


def _step(ch, model, now, limit, fn):
    """fn(work, cx) on a copy; committed into ch unless the step turned out the host's.  Returns (events, fn's value,
    the longest queue the step held)."""
    if host_owned_on_entry(ch, model):
        return HOST, None, 0
    work, cx = ch.copy(), Ctx(model, now, limit)
    try:
        out = fn(work, cx)
    except HostOwned as h:
        return HOST | (OVERFLOW if h.overflow else 0), None, cx.max_len
    for k in Char.__slots__:
        setattr(ch, k, getattr(work, k))
    return cx.events, out, cx.max_len


def characters_state_one(ch, model, request, motion, now, limit=ANIQ_MAX):
    """clapgpu_characters_state for one character with a mover; request != CS_NONE.  -> (events, longest queue)"""
    def fn(work, cx):
        if request in (CS_JUMP_START, CS_MOVING, CS_IDLE):   # character.c:499, the grounded path alone
            work.motion = [F32(motion[0]), F32(motion[1])]
        character_set_state(work, cx, int(request))
    ev, _, longest = _step(ch, model, now, limit, fn)
    return ev, longest


def queue_time_one(ch, model, now, limit=ANIQ_MAX):
    """clapgpu_animation_queue_time for one character.  -> (events, (pose animation, frame time) or None, longest queue)"""
    if not host_owned_on_entry(ch, model):                   # a short cut, for speed alone: an entry that has not run out
        qa = ch.aniq[ch.animation]                           # changes nothing (model.c:1578, 1590)
        frame_time = (float(now) - ch.ani_time) * float(qa.speed)
        if not frame_time >= model._te[qa.animation]:
            ch.tail = []                                     # (the step is committed all the same)
            return 0, (qa.animation, F32(frame_time)), 0
    return _step(ch, model, now, limit, animated_update)


class Batch:
    """The characters of one clapgpu_aniq, as objects; arrays() gives what the device arrays must hold."""
    FIELDS = ("queue", "len", "cur", "cleared", "ani_time", "state", "airborne", "velocity", "ch_motion", "pose_anim",
              "frame_time", "events")

    def __init__(self, model, a, limit=ANIQ_MAX):
        """a: dict of the arrays of FIELDS (and jump_params), as uploaded"""
        self.model, self.limit = model, limit
        self.n = n = len(a["len"])
        self.jump_params = np.asarray(a["jump_params"], np.float32).reshape(n, 2)
        self.pose_anim = np.asarray(a.get("pose_anim", np.zeros(n)), np.uint32).copy()
        self.frame_time = np.asarray(a.get("frame_time", np.zeros(n)), np.float32).copy()
        self.events = np.asarray(a.get("events", np.zeros(n)), np.uint32).copy()
        self.longest = 0
        q = np.asarray(a["queue"], ENTRY).reshape(n, ANIQ_MAX)
        self.chars = []
        for c in range(n):
            ch = Char()
            ch.state, ch.airborne = int(a["state"][c]), int(a["airborne"][c])
            ch.vel = [F32(v) for v in a["velocity"][c]]
            ch.motion = [F32(v) for v in a["ch_motion"][c]]
            ch.jump_forward, ch.jump_upward = F32(self.jump_params[c, 0]), F32(self.jump_params[c, 1])
            ln = int(a["len"][c])
            rows = [Entry(int(e["animation"]), int(e["repeat"]), int(e["end"]), e["speed"]) for e in q[c]]
            live = min(ln, ANIQ_MAX)
            ch.aniq, ch.tail, ch.raw_len = rows[:live], rows[live:], (ln if ln > ANIQ_MAX else None)
            ch.animation, ch.cleared, ch.ani_time = int(a["cur"][c]), int(a["cleared"][c]), float(a["ani_time"][c])
            self.chars.append(ch)

    def characters_state(self, request, motion, now, mover=None):
        request, motion = np.asarray(request), np.asarray(motion, np.float32).reshape(-1, 2)
        for c, ch in enumerate(self.chars):
            k = c if mover is None else int(mover[c])
            req = int(request[k]) if 0 <= k < len(request) else CS_NONE
            if req == CS_NONE:
                self.events[c] = 0
                continue
            ev, longest = characters_state_one(ch, self.model, req, motion[k], now, self.limit)
            self.longest = max(self.longest, longest)
            self.events[c] = ev << STATE_SHIFT

    def queue_time(self, now):
        for c, ch in enumerate(self.chars):
            ev, out, longest = queue_time_one(ch, self.model, now, self.limit)
            self.longest = max(self.longest, longest)
            if out is not None:
                self.pose_anim[c], self.frame_time[c] = out
            self.events[c] = (int(self.events[c]) & (0xff << STATE_SHIFT)) | ev

    def host_owned(self):
        """[n] bool: the last step of either kind left the character to the host"""
        return ((self.events & HOST) | ((self.events >> STATE_SHIFT) & HOST)) != 0

    def arrays(self):
        n = self.n
        q = np.zeros((n, ANIQ_MAX), ENTRY)
        out = dict(queue=q, len=np.zeros(n, np.uint8), cur=np.zeros(n, np.int8), cleared=np.zeros(n, np.uint8),
                   ani_time=np.zeros(n, np.float64), state=np.zeros(n, np.uint8), airborne=np.zeros(n, np.uint8),
                   velocity=np.zeros((n, 3), np.float32), ch_motion=np.zeros((n, 2), np.float32),
                   pose_anim=self.pose_anim.copy(), frame_time=self.frame_time.copy(), events=self.events.copy())
        for c, ch in enumerate(self.chars):
            rows = (ch.aniq + ch.tail)[:ANIQ_MAX]              # longer only with limit=None: then nobody compares arrays
            for i, e in enumerate(rows):
                q[c, i] = (e.animation, e.repeat, e.end, e.speed)
            out["len"][c] = len(ch.aniq) if ch.raw_len is None else ch.raw_len
            out["cur"][c], out["cleared"][c], out["ani_time"][c] = ch.animation, ch.cleared, ch.ani_time
            out["state"][c], out["airborne"][c] = ch.state, ch.airborne
            out["velocity"][c], out["ch_motion"][c] = ch.vel, ch.motion
        return out
