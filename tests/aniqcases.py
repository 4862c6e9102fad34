"""Inputs of the character-state / animation-queue tests, shared by test_aniq.py (CPU: the conditions on these inputs,
the host build of the rule) and test_aniq_gpu.py (the kernels).  Nothing here is computed by the code under test.

Two models: ALL has the twelve names character.c pushes (in an order of its own, between two animations nobody asks
for), PART lacks motion_start, idle_to_jump and jump.  Every animation has a time_end of its own.
"""
import itertools

import numpy as np

import aniqref as ar

DT = 1.0 / 60.0


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def models():
    order = [7, 2, 11, 0, 5, 9, 3, 12, 1, 6, 10, 4]                       # names -> animation ids 0 .. 12, 8 is nobody's
    te_all = (0.2 + 0.045 * np.arange(14)).astype(np.float32)
    missing = (ar.SLOT["motion_start"], ar.SLOT["idle_to_jump"], ar.SLOT["jump"])
    kept = [s for s in range(12) if s not in missing]
    part = np.full(12, -1, np.int32)
    part[kept] = np.arange(len(kept))[::-1]
    te_part = (0.15 + 0.06 * np.arange(10)).astype(np.float32)
    return dict(all=ar.Model(order, te_all), part=ar.Model(part, te_part))


def blank(n, seed):
    """n characters with an empty queue and random struct character fields"""
    R = rng(seed)
    return dict(queue=np.zeros((n, ar.ANIQ_MAX), ar.ENTRY), len=np.zeros(n, np.uint8), cur=np.zeros(n, np.int8),
                cleared=np.zeros(n, np.uint8), ani_time=np.zeros(n, np.float64), state=np.zeros(n, np.uint8),
                airborne=np.zeros(n, np.uint8), velocity=R.normal(0, 2, (n, 3)).astype(np.float32),
                ch_motion=R.normal(0, 1, (n, 2)).astype(np.float32),
                jump_params=(R.uniform(0.5, 2.0, (n, 2)) * [1.0, 4.0]).astype(np.float32),
                pose_anim=np.full(n, 0xdead, np.uint32), frame_time=np.full(n, -7.0, np.float32),
                events=np.full(n, 0xa5a5, np.uint32))


# ------------------------------------------------------------------------------------------------ the transition table
def queue_shapes(model):
    """[(entries, cur, cleared)]: entries of (animation, repeat, end, speed)"""
    a = [v for v in model.name_anim if v >= 0]
    idle = model.name_anim[ar.SLOT["idle"]]
    out = [([], 0, 0)]
    for cleared in (0, 1):
        out.append(([(idle, 1, 0, 1.0)], 0, cleared))
        for end in (0, 1, 2, 3, 0xff):
            out.append(([(a[1], 0, end, 1.0), (idle, 1, 0, 1.5)], 0, cleared))
        # four entries: an appending push overflows; the current one is the second, its successor repeats
        out.append(([(a[2], 0, 0, 1.0), (a[3], 0, 2, 0.5), (idle, 1, 0, 1.0), (a[4], 1, 0, 2.0)], 1, cleared))
    out.append(([(a[1], 0, 1, 1.0), (idle, 1, 0, 1.0)], 1, 0))           # the current entry is the repeating second one
    out.append(([(a[1], 0, 3, 1.0), (a[2], 0, 1, 1.0), (idle, 1, 0, 1.0)], 1, 0))
    # the host's on entry: no current entry, an exhausted cursor, an animation the model has not, an unknown end code
    out.append(([(idle, 1, 0, 1.0)], -1, 0))
    out.append(([(idle, 1, 0, 1.0)], 1, 0))
    out.append(([(idle, 1, 0, 1.0), (model.n_anims, 0, 0, 1.0)], 0, 0))
    out.append(([(a[1], 0, 7, 1.0), (idle, 1, 0, 1.0)], 0, 0))
    return out


REQUESTS = (ar.CS_IDLE, ar.CS_MOVING, ar.CS_JUMP_START, ar.CS_JUMPING, ar.CS_FALLING, ar.CS_NONE)


def transition_table(model, past, seed=1):
    """One character per (queue shape, state, request, airborne).  past: the current entry has run past its time_end at
    NOW (else it has not).  -> (arrays, request [n], motion [n, 2], now)"""
    combos = list(itertools.product(queue_shapes(model), range(7), REQUESTS, (0, 1)))
    n = len(combos)
    a = blank(n, seed)
    R = rng(seed + 100)
    now = 12.5
    request = np.zeros(n, np.uint8)
    for c, ((entries, cur, cleared), state, req, air) in enumerate(combos):
        for i, e in enumerate(entries):
            a["queue"][c, i] = e
        for i in range(len(entries), ar.ANIQ_MAX):
            a["queue"][c, i] = (0x1234 + i, 1, 2, -3.0)                    # what lies behind len is nobody's business
        a["len"][c], a["cur"][c], a["cleared"][c] = len(entries), cur, cleared
        a["state"][c], a["airborne"][c], request[c] = state, air, req
        if 0 <= cur < len(entries) and entries[cur][0] < model.n_anims:
            te, speed = float(model.time_end[entries[cur][0]]), entries[cur][3]
            ran = te * (1.0 + R.uniform(0.01, 0.5)) if past else te * R.uniform(0.0, 0.99)
            a["ani_time"][c] = now - ran / speed
        else:
            a["ani_time"][c] = now - 0.1
    motion = R.normal(0, 1, (n, 2)).astype(np.float32)
    return a, request, motion, now


# ------------------------------------------------------------------------------------------------ the random walk
def walk_inputs(n, frames, seed, passive=0.0, independent_air=False):
    """request [frames, n], airborne [frames, n] (what the move leaves in airborne before the state call), motion
    [frames, n, 2].  Each character follows segments of idle / move / jump / fall / no request, paired as
    clapgpu_characters_move pairs them (FALLING with airborne, the grounded requests without); a jump is JUMP_START for
    one frame, its grounded intent for a while (the move keeps asking while the *_to_jump animation plays) and then the
    fall.  The first `passive` of the characters never walk or jump.  independent_air: airborne drawn on its own."""
    R = rng(seed)
    request = np.full((frames, n), ar.CS_NONE, np.uint8)
    airborne = np.zeros((frames, n), np.uint8)
    motion = np.zeros((frames, n, 2), np.float32)
    n_passive = int(round(passive * n))
    for c in range(n):
        f, air = 0, 0
        kinds = ("idle", "fall", "none") if c < n_passive else ("idle", "move", "move", "jump", "fall", "none")
        while f < frames:
            kind = kinds[R.integers(len(kinds))]
            d = int(R.integers(3, 70))
            seg_req, seg_air = [], []
            m = R.normal(0, 1, 2).astype(np.float32)
            if kind == "idle":
                seg_req, seg_air, m = [ar.CS_IDLE] * d, [0] * d, np.zeros(2, np.float32)
            elif kind == "move":
                seg_req, seg_air = [ar.CS_MOVING] * d, [0] * d
            elif kind == "fall":
                seg_req, seg_air = [ar.CS_FALLING] * d, [1] * d
            elif kind == "none":
                d = min(d, 5)
                seg_req, seg_air = [ar.CS_NONE] * d, [air] * d
            else:
                ground = ar.CS_MOVING if R.integers(2) else ar.CS_IDLE
                g, fall = int(R.integers(5, 45)), int(R.integers(5, 40))
                seg_req = [ar.CS_JUMP_START] + [ground] * g + [ar.CS_FALLING] * fall
                seg_air = [0] * (1 + g) + [1] * fall
            for r, a_ in zip(seg_req, seg_air):
                if f >= frames:
                    break
                request[f, c], airborne[f, c], motion[f, c] = r, a_, m
                air = a_
                f += 1
    if independent_air:
        airborne = (R.integers(0, 3, (frames, n)) == 0).astype(np.uint8)
    return request, airborne, motion


def walk_start(model, n, seed):
    """every character at CS_START with the host's idle entry playing at a phase of its own (model.c:1462-1468)"""
    a = blank(n, seed)
    R = rng(seed + 7)
    idle = model.name_anim[ar.SLOT["idle"]]
    a["queue"][:, 0] = (idle, 1, 0, 1.0)
    a["len"][:], a["state"][:] = 1, ar.CS_START
    a["ani_time"][:] = 2.0 - R.uniform(0, float(model.time_end[idle]), n)
    a["velocity"][:] = 0
    return a


WALKS = dict(                                               # name -> (model, seed, passive, independent_air)
    all=("all", 11, 0.0, False),
    part=("part", 12, 0.55, False),
    all_air=("all", 13, 0.0, True),
)
WALK_N, WALK_FRAMES, WALK_T0 = 1000, 300, 2.0


def walk(name):
    """-> (model, start arrays, request, airborne, motion)"""
    mname, seed, passive, indep = WALKS[name]
    model = models()[mname]
    return (model, walk_start(model, WALK_N, seed)) + walk_inputs(WALK_N, WALK_FRAMES, seed, passive, indep)


def run_walk(batch, request, airborne, motion, t0=WALK_T0, dt=DT, each=None):
    """The frames of a walk on an aniqref.Batch: the move's airborne, the state step, the queue clock.  each(f, batch)
    is called after every frame."""
    now = t0
    for f in range(len(request)):
        now = t0 + (f + 1) * dt
        for c, ch in enumerate(batch.chars):
            if request[f, c] != ar.CS_NONE:
                ch.airborne = int(airborne[f, c])
        batch.characters_state(request[f], motion[f], now)
        batch.queue_time(now)
        if each is not None:
            each(f, batch)
    return now
