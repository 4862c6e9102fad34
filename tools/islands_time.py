"""Timing drivers for the island pass (clapgpu_bodies_islands); profiles/islands/README.md holds what they measured.

    python tools/islands_time.py pass [--asleep 0.0|0.1] [--runs 5] [--k 20]
        262 144 capsule-mix bodies (synth.capsule_bodies, bench_extras' physics size), the broadphase's real pair list and
        the narrowphase's records; times the contact launch, the pass and the step launch to launch between HIP events,
        every call on the same restored state: one JSON line.  --asleep: that fraction of the bodies asleep with spent
        counters, each in contact with an awake one where it has a contact at all.  Under rocprofv3 --kernel-trace --stats
        (a run of its own) the same run gives every kernel's time.
    python tools/islands_time.py step <libclapgpu.so | shipped> [iters]
        the step alone, no accumulator: tools/push_time.py's driver (works on a build of the parent commit too)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clap_amd import _lib, physics, synth  # noqa: E402

H = 1.0 / 120.0
STATE = ("pos", "quat", "lvel", "avel", "bflags", "adis_steps_left", "adis_time_left", "aabb", "axis", "geom_records")


def event_us(fn, k, runs, before=None):
    out = []
    for _ in range(runs):
        if before:
            before()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0 / k)
    out.sort()
    return [round(out[0], 2), round(out[len(out) // 2], 2), round(out[-1], 2)]


def run_pass(asleep, runs, k):
    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    n = 262_144
    b = synth.capsule_bodies(n, box=60.0, seed=4)
    w = physics.PhysWorld(b, None, device="cuda:0")
    w.broadphase()
    w.contacts_geoms()
    torch.cuda.synchronize()
    total = int(w.pair_total.item())
    pairs = w.pairs[:total].cpu().numpy().view(np.uint32)
    nc = w.contact2_buf[:total, 100:104].cpu().numpy().copy().view(np.uint32).ravel()
    touching = pairs[(nc & 0x7fffffff) >= 1]
    res = dict(bodies=n, pairs=total, touching_pairs=int(len(touching)), asleep_frac=asleep, k=k, runs=runs,
               unit="us per call [min, median, max]")
    if asleep > 0:                                      # sleepers: one side of touching pairs whose other side stays awake
        R = np.random.Generator(np.random.PCG64(3))
        pick = touching[R.permutation(len(touching))]
        sleeper = np.zeros(n, bool)
        awake_needed = np.zeros(n, bool)
        want = int(asleep * n)
        for a, c in pick:
            if sleeper.sum() >= want:
                break
            if not sleeper[a] and not sleeper[c] and not awake_needed[a]:
                sleeper[a], awake_needed[c] = True, True
        rest = np.flatnonzero(~sleeper & ~awake_needed)
        sleeper[rest[:max(0, want - int(sleeper.sum()))]] = True          # the rest of the tenth sleeps alone
        idx = torch.from_numpy(np.flatnonzero(sleeper)).to(w.device)
        w.bflags[idx] |= 1
        w.adis_steps_left[idx] = 0
        w.lvel[idx] = 0
        w.avel[idx] = 0
        res["sleepers"] = int(sleeper.sum())
        res["sleepers_touching_awake"] = int(awake_needed.sum())
    w.contacts_geoms()                                   # HAS_JOINT as a substep leaves it
    saved = {key: getattr(w, key).clone() for key in STATE}

    def restore():
        for key in STATE:
            getattr(w, key).copy_(saved[key])
    w.islands(H)
    torch.cuda.synchronize()
    res["woken"] = int(w.island_woken.item())
    res["islands"] = int(len(np.unique(w.island.cpu().numpy())))
    restore()
    res["restore_us"] = event_us(restore, k, runs)
    res["contacts_us"] = event_us(w.contacts_geoms, k, runs, restore)
    res["restore_islands_us"] = event_us(lambda: (restore(), w.islands(H)), k, runs)
    res["restore_step_us"] = event_us(lambda: (restore(), w.world_step(H)), k, runs)
    res["restore_islands_step_us"] = event_us(lambda: (restore(), w.islands(H), w.world_step(H)), k, runs)
    res["islands_alone_us"] = round(res["restore_islands_us"][1] - res["restore_us"][1], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "step":
        from push_time import step
        step(sys.argv[2], "null", int(sys.argv[3]) if len(sys.argv) > 3 else 200)
    else:
        import argparse
        ap = argparse.ArgumentParser()
        ap.add_argument("mode")
        ap.add_argument("--asleep", type=float, default=0.0)
        ap.add_argument("--runs", type=int, default=5)
        ap.add_argument("--k", type=int, default=20)
        a = ap.parse_args()
        run_pass(a.asleep, a.runs, a.k)
