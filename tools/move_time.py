"""Times clapgpu_characters_move at workload B of profiles/slide/ (tools/mesh_contact_time.py's scene: 262 144 bodies on a
terrain, 5 000 statics, the mesh set; 65 536 movers), and the yardstick: character_move of the same movers done as
before the call existed -- PhysWorld.ground_collide, its results read back, tests/moveref.py on the host, the velocities
uploaded again, PhysWorld.slide_and_push of the sliding movers.

Method: warm; the two ways alternate, `--runs` times each, on one process and one box.  Every timed
pass starts from the restored bodies.  The one call is timed launch to launch between a HIP event pair (restore included,
the restore alone timed the same way and reported, so it can be taken off).  The yardstick has the host in its middle and
is timed on the wall clock between two device synchronisations; the time tests/moveref.py takes is reported on its own:
it is a Python loop, a host written in C would spend microseconds there, so the figure to compare the call with is
`parent_less_host_decide_us`.  One JSON line.
    python tools/move_time.py [--movers 65536] [--runs 5]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from clap_amd import _lib, physics  # noqa: E402
from mesh_contact_time import scene  # noqa: E402
import moveref as mr  # noqa: E402

f32 = np.float32
KEYS = ("pos", "lvel", "aabb", "axis", "geom_records", "facc", "bflags", "adis_steps_left", "adis_time_left")


def movers_of(w, b, n, seed):
    """walkers for the most part, a fifth airborne, a few jumping or standing: a crowd in motion"""
    R = np.random.Generator(np.random.PCG64(seed))
    body = R.choice(w.n, n, replace=False).astype(np.uint32)
    state = R.choice([mr.CS_IDLE, mr.CS_MOVING, mr.CS_MOVING, mr.CS_MOVING, mr.CS_FALLING], n).astype(np.uint8)
    return dict(body=body, ray_off=np.asarray(b["yoffset"], float)[body] * 0.8,
                motion=(R.uniform(-6, 6, (n, 2)) * (R.random((n, 1)) < 0.9)).astype(f32), state=state,
                jump=(R.random(n) < 0.02).astype(np.uint8), jump_params=np.tile(f32([1.0, 5.0]), (n, 1)),
                velocity=np.stack([R.uniform(-4, 4, n), R.uniform(-6, 0, n), R.uniform(-4, 4, n)], 1).astype(f32),
                normal=np.tile(f32([0, 1, 0]), (n, 1)), airborne=(state == mr.CS_FALLING).astype(np.uint8))


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--movers", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    w, b, _terrain = scene("B")
    w.enable_forces()
    w.bodies_aabb()
    dt = 1.0 / 60.0
    mv = movers_of(w, b, a.movers, 10)
    IN = ("motion", "state", "jump", "jump_params", "velocity", "normal", "airborne")
    m = physics.CharacterMoves(w, mv["body"], mv["ray_off"], **{k: mv[k] for k in IN})
    snap = {k: getattr(w, k).clone() for k in KEYS}
    state0 = {k: getattr(m, k).clone() for k in ("velocity", "normal", "airborne")}

    def restore():
        for k in KEYS:
            getattr(w, k).copy_(snap[k])
        for k, t in state0.items():
            getattr(m, k).copy_(t)
        w.bp_invalidate()

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def one_call():
        restore()
        w.characters_move(m, dt)

    def parent_way():
        """returns (wall us, us of it inside moveref)"""
        restore()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w.bp_index()
        gout, nrm, _dist, hit, rflags = (t.cpu().numpy() for t in w.ground_collide(mv["body"], mv["ray_off"], mv["airborne"] == 0))
        rflags = rflags.view(np.uint32)
        wrote = (hit != -1) & ((rflags & 3) == 0)
        normal = np.where(wrote[:, None], nrm, mv["normal"]).astype(f32)
        h0 = time.perf_counter()
        d = mr.character_move_decide(rflags, gout, mv["state"], mv["jump"], mv["motion"], mv["jump_params"], mv["velocity"], normal,
                                     mv["airborne"], f32(w.world.gravity[1]), dt)
        h1 = time.perf_counter()
        s = np.flatnonzero(d["applied"])
        w.bp_index()
        w.slide_and_push(mv["body"][s], d["velocity"][s], d["airborne"][s], dt)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return (t1 - t0) * 1e6, (h1 - h0) * 1e6, len(s)

    one_call()                                              # warm: both ways once
    parent_way()
    torch.cuda.synchronize()
    rest, call, parent, host, sliding = [], [], [], [], 0
    for _ in range(a.runs):                                 # alternated
        rest.append(event_us(restore))
        call.append(event_us(one_call))
        p, h, sliding = parent_way()
        parent.append(p)
        host.append(h)
    out = m.outputs()
    flags = out["flags"].cpu().numpy().view(np.uint32)
    res = dict(bodies=w.n, statics=w.n_static, movers=a.movers, runs=a.runs, dt=dt, unit="us [min, median, max]",
               sliding=int(sliding), applied=int(out["applied"].sum().item()),
               ray_flags=[int(((flags & bit) != 0).sum()) for bit in (1, 2, 4)],
               slide_flags=[int((((flags >> 8) & bit) != 0).sum()) for bit in (1, 2, 4)],
               scratch_bytes=_lib.characters_move_scratch_bytes(w.n, a.movers))
    tri = lambda v: [round(min(v), 1), round(median(v), 1), round(max(v), 1)]
    res["restore_us"], res["restore_plus_move_us"] = tri(rest), tri(call)
    res["move_call_us"] = round(median(call) - median(rest), 1)
    res["parent_way_wall_us"], res["parent_host_decide_us"] = tri(parent), tri(host)
    res["parent_less_host_decide_us"] = round(median(parent) - median(host), 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
