"""Times the character state call and the queue clock (clapgpu_characters_state, clapgpu_animation_queue_time) at
`--chars` characters, the plain clock (clapgpu_animation_time) at the same size, and a whole frame with the move in it
with and without the queues.

Method: warm; HIP event pairs, launch to launch; [min, median, max] over `--runs` frames.  The
two kernels run the all-names walk of tests/aniqcases.py (its per-character intents, tiled to `--chars`), so a frame
has its share of pushes, ends and callbacks; the plain clock runs one repeating entry per character, what it was made
for.  The frame: `--chars` capsule bodies moved as characters over 64 static boxes, their entities, a pose of 8
joints; FrameLoop(move=, characters=) against FrameLoop(move=, characters=, aniq=), alternated.  A tree without
AnimationQueues (the parent) reports the plain clock and the first frame alone.  One JSON line.
    python tools/aniq_time.py [--chars 65536] [--runs 50] [--no-frame]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from clap_amd import _dev, _lib, animation, entities, frame, physics, synth, tiler  # noqa: E402

HAVE = hasattr(animation, "AnimationQueues")
DEV = "cuda:0"


def tri(v):
    v = sorted(v)
    return [round(v[0], 1), round(v[len(v) // 2], 1), round(v[-1], 1)]


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def plain_clock(n, runs):
    """clapgpu_animation_time over n characters of one repeating animation"""
    te = _dev.upload(np.float32([0.5]), np.float32, DEV)
    anim = _dev.device_array(n, torch.int32, DEV)
    ani = _dev.upload(np.linspace(0, 0.5, n), np.float64, DEV)
    speed, restart = _dev.device_array(n, torch.float32, DEV, 1.0), _dev.device_array(n, torch.uint8, DEV, 1)
    ft, ended = _dev.device_array(n, torch.float32, DEV), _dev.device_array(n, torch.uint8, DEV)
    clk = _lib.AnimClock(n, 1, *[t.data_ptr() for t in (anim, te, ani, speed, restart, ft, ended)])
    L, out = _lib.lib(), []
    for f in range(runs + 5):
        us = event_us(lambda: _lib.check(L.clapgpu_animation_time(_dev.stream(), C.byref(clk), 1.0 + f / 60.0), "clock"))
        if f >= 5:
            out.append(us)
    return tri(out)


def queue_kernels(n, runs):
    import aniqcases as ac
    import aniqref as ar
    model, start, request, airborne, motion = ac.walk("all")
    reps = (n + ac.WALK_N - 1) // ac.WALK_N
    tile = lambda a, axis: np.concatenate([a] * reps, axis)[(slice(None),) * axis + (slice(0, n),)]
    start = {k: tile(v, 0) for k, v in start.items()}
    frames = min(runs + 5, len(request))
    req_d = _dev.upload(tile(request[:frames], 1), np.uint8, DEV)
    mot_d = _dev.upload(tile(motion[:frames], 1), np.float32, DEV)
    air_d = _dev.upload(tile(airborne[:frames], 1), np.uint8, DEV)
    aq = animation.AnimationQueues(n, model.name_anim, model.time_end, device=DEV,
                                   **{k: start[k] for k in ("queue", "len", "cur", "cleared", "ani_time", "state", "airborne",
                                                            "velocity", "ch_motion", "jump_params")})

    class Rq:
        _desc = _lib.CharactersMove(n)
    st, tm, events = [], [], np.zeros(16, np.int64)
    for f in range(frames):
        now = ac.WALK_T0 + (f + 1) * ac.DT
        Rq._desc.request, Rq._desc.motion = req_d[f].data_ptr(), mot_d[f].data_ptr()
        aq.airborne[:n] = torch.where(req_d[f] != 0xff, air_d[f], aq.airborne[:n])          # the move's airborne
        a = event_us(lambda: aq.characters_state(Rq, now))
        b = event_us(lambda: aq.queue_time(now))
        if f >= 5:
            st.append(a)
            tm.append(b)
            ev = aq.events[:n].cpu().numpy().view(np.uint32)
            events += [int(((ev >> bit) & 1).sum()) for bit in range(16)]
    names = ("ended", "started", "advanced", "cb_idle", "cb_start_motion", "cb_any_to_jump", "host", "overflow")
    per = {k: round(events[i] / len(st), 1) for i, k in enumerate(names)}
    per.update({"state_" + k: round(events[8 + i] / len(st), 1) for i, k in enumerate(names) if events[8 + i]})
    return tri(st), tri(tm), per, ar.ANIQ_MAX


def frame_pair(n, runs):
    """-> {without: us, with: us}: a frame with the move, the hooks' clock or the queues, a pose of 8 joints"""
    import aniqcases as ac
    J = 8
    raw = synth.entities_flat(n, seed=5)
    scene, tl = tiler.tiled_scene(raw)
    roots = tl["slot_of"][np.flatnonzero(raw["parent"] < 0)]
    n = min(n, len(roots))
    scene["model_lod"] = np.asarray([[0, 3]], np.uint8)
    R = np.random.Generator(np.random.PCG64(3))
    b = synth.capsule_bodies(n, box=400.0, seed=5)
    b["body_entity"][:] = -1
    b["pos"][:, 1] = 0.5 + b["yoffset"]
    model = ac.models()["all"]
    anims = [synth.animation(J, 6, float(te), seed=40 + i) for i, te in enumerate(model.time_end)]
    sk = synth.skeleton(J, 4, seed=5)
    ch = synth.characters(n, J, seed=5)
    out = {}
    loops = {}
    for key in (("without", "with") if HAVE else ("without",)):
        batch = entities.EntityBatch(scene, DEV)
        w = physics.PhysWorld(b, synth.static_boxes(64, 400.0), pair_capacity=1 << 20, device=DEV, forces=True)
        m = physics.CharacterMoves(w, np.arange(n, dtype=np.uint32), np.asarray(b["yoffset"], float) * 0.9,
                                   entity=roots[:n].astype(np.uint32), entity_batch=batch,
                                   motion=R.normal(0, 2, (n, 2)).astype(np.float32), state=np.full(n, 2, np.uint8),
                                   jump=np.zeros(n, np.uint8), jump_params=np.tile(np.float32([1, 5]), (n, 1)),
                                   velocity=np.zeros((n, 3), np.float32), normal=np.tile(np.float32([0, 1, 0]), (n, 1)),
                                   airborne=np.zeros(n, np.uint8))
        sm = animation.SkinnedModel(sk, anims, device=DEV)
        cb = animation.CharacterBatch(sm, n, ch["trs0"], batch.mx, entity_index=roots[:n].astype(np.uint32))
        kw = {}
        if key == "with":
            start = ac.walk_start(model, n, 17)
            kw["aniq"] = animation.AnimationQueues(n, model.name_anim, sm.time_end, batch=cb, moves=m,
                                                   **{k: start[k] for k in ("queue", "len", "cur", "cleared", "ani_time", "ch_motion")})
        loops[key] = frame.FrameLoop(batch, synth.camera(pos=(0, 10, 60)), world=w, characters=cb, move=m, **kw)
        out[key] = []
    dt = 1.0 / 120.0
    for f in range(runs + 3):                               # alternated
        for key, loop in loops.items():
            us = event_us(lambda: loop.clap_frame(2.0 + f * dt, dt))
            if f >= 3:
                out[key].append(us)
    return {k: tri(v) for k, v in out.items()}, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chars", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--no-frame", action="store_true")
    a = ap.parse_args()
    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    res = dict(chars=a.chars, runs=a.runs, abi=_lib.ABI_VERSION, unit="us [min, median, max]")
    res["animation_time_us"] = plain_clock(a.chars, a.runs)
    if HAVE:
        res["characters_state_us"], res["animation_queue_time_us"], res["events_per_frame"], _ = queue_kernels(a.chars, a.runs)
    if not a.no_frame:
        fr, n = frame_pair(a.chars, min(a.runs, 20))
        res["frame_chars"] = n
        res.update({"frame_" + k + "_aniq_us": v for k, v in fr.items()})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
