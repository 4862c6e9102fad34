"""Times clapgpu_characters_slide and clapgpu_sweep_capsules_grid at the physics scene of tools/mesh_contact_time.py
(262 144 bodies on a terrain, 5 000 statics, mesh set; workload A or B), and the yardstick: the same move done as before
these calls existed -- a host loop over PhysWorld.sweep_capsules with numpy in between and the candidate lists rebuilt
from downloaded boxes after each move (tests/slideref.py's loop is the same arithmetic).

Method: warm, K back-to-back calls between one HIP event pair, several runs, the range reported.
A slide moves its bodies and clears the index, so a timed call is restore (pos, lvel, boxes) + clapgpu_bp_index (grid
path only) + the slide; the restore alone is timed too and subtracted.  The device calls go through ctypes with the
arguments uploaded once.  The host loop is timed on --host-movers movers (it is minutes long at 65 536) and compared
with the device call on the same movers.  One JSON line per workload.
    python tools/slide_bench.py [--workload A|B|both] [--runs 5] [--k 3] [--movers 65536] [--host-movers 512]"""
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
from clap_amd import _lib, physics  # noqa: E402
from mesh_contact_time import scene  # noqa: E402

f32 = np.float32
KEYS = ("pos", "lvel", "aabb", "axis", "geom_records")


def event_us(fn, k, runs):
    """[min, median, max] microseconds per call over `runs` runs of k back-to-back calls"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / k)
    out.sort()
    return [round(out[0], 1), round(out[len(out) // 2], 1), round(out[-1], 1)]


class Slide:
    """clapgpu_characters_slide with its arguments on the device"""

    def __init__(self, w, movers, vel, air):
        dev = w.device
        n = len(movers)
        self.w, self.n = w, n
        self.body = torch.from_numpy(np.ascontiguousarray(movers, np.uint32).view(np.int32)).to(dev)
        self.vel0 = torch.from_numpy(np.ascontiguousarray(vel, f32)).to(dev)
        self.vel = self.vel0.clone()
        self.air = torch.from_numpy(np.ascontiguousarray(air, np.uint8)).to(dev)
        self.first = torch.ones((n, 2), dtype=torch.float32, device=dev)
        self.push = torch.full((n, 6), -1, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(n, dtype=torch.int32, device=dev)
        self.scratch = torch.zeros(w.n, dtype=torch.int32, device=dev)
        self.desc = _lib.Slide(n, self.body.data_ptr(), self.vel.data_ptr(), self.air.data_ptr(), self.first.data_ptr(),
                               self.push.data_ptr(), self.flags.data_ptr())
        self.sg = w.static_geoms()
        self.snap = {k: getattr(w, k).clone() for k in KEYS}

    def restore(self):
        for k in KEYS:
            getattr(self.w, k).copy_(self.snap[k])
        self.vel.copy_(self.vel0)

    def call(self, grid, dt=1.0 / 30.0):
        w = self.w
        self.restore()
        if grid:
            w.bp_index()
        _lib.check(_lib.lib().clapgpu_characters_slide(physics._stream(), w._bp if grid else None, C.byref(w._desc),
                                                       C.byref(self.sg), w._meshes, dt, C.byref(self.desc),
                                                       self.scratch.data_ptr()), "clapgpu_characters_slide")


def mixes(w, n, seed):
    R = np.random.Generator(np.random.PCG64(seed))
    movers = R.choice(w.n, n, replace=False).astype(np.uint32)
    walk = np.stack([R.uniform(-6, 6, n), R.uniform(-1, 0, n), R.uniform(-6, 6, n)], 1).astype(f32)
    fall = np.stack([R.uniform(-4, 4, n), R.uniform(-15, -5, n), R.uniform(-4, 4, n)], 1).astype(f32)
    return movers, dict(walk=(walk, np.zeros(n, np.uint8)), fall=(fall, np.ones(n, np.uint8)))


def host_loop(w, movers, vel, air, dt=1.0 / 30.0):
    """the parent commit's way: per character_sweep_delta iteration one batched PhysWorld.sweep_capsules over the movers
    still sweeping, lists rebuilt in numpy from the downloaded boxes, positions uploaded after each move"""
    n = len(movers)
    bb = w.aabb.cpu().numpy()[:w.n].copy()
    sbb = w._statics_host
    pos = w.pos.cpu().numpy()
    falling = (air != 0) & ~(vel[:, 1] > 0)
    calls = [(np.where(falling[:, None], np.stack([np.zeros(n), (vel[:, 1].astype(np.float64) * dt), np.zeros(n)], 1),
                       vel * f32(dt)).astype(f32), np.where(falling, 0.5, -1.0), ~falling, np.ones(n, bool)),
             (np.stack([vel[:, 0].astype(np.float64) * dt, np.zeros(n), vel[:, 2].astype(np.float64) * dt], 1).astype(f32),
              np.full(n, -1.0), np.ones(n, bool), falling)]
    for delta, min_ny, stop, active in calls:
        delta = delta.copy()
        live = active.copy()
        for _it in range(3):
            live &= np.sqrt((delta * delta).sum(1)) >= 1e-6
            idx = np.flatnonzero(live)
            if not len(idx):
                break
            cand, first = [], [0]
            for k in idx:                                   # lists from the swept box: statics, then bodies
                m = movers[k]
                lo = np.minimum(bb[m, 0::2], bb[m, 0::2] + delta[k]) - 1e-3
                hi = np.maximum(bb[m, 1::2], bb[m, 1::2] + delta[k]) + 1e-3
                s_hit = np.flatnonzero(np.all((sbb[:, 0::2] <= hi) & (sbb[:, 1::2] >= lo), axis=1))
                b_hit = np.flatnonzero(np.all((bb[:, 0::2] <= hi) & (bb[:, 1::2] >= lo), axis=1))
                cand.append(s_hit.astype(np.uint32))
                cand.append(b_hit.astype(np.uint32) | np.uint32(1 << 31))
                first.append(first[-1] + len(s_hit) + len(b_hit))
            frac, nrm, _hit = (x.cpu().numpy() for x in w.sweep_capsules(movers[idx], delta[idx], np.asarray(first, np.uint32),
                                                                          np.concatenate(cand)))
            frac = np.where((frac < 1) & (nrm[:, 1] < min_ny[idx]), f32(1), frac)
            step = delta[idx] * frac[:, None]
            mv = frac > 0
            pos[movers[idx[mv]]] += step[mv].astype(np.float64)
            done = (frac >= 1) | ((frac <= 0) & stop[idx])
            rem = delta[idx] * (f32(1) - frac)[:, None]
            dot = (rem * nrm).sum(1, dtype=f32)
            delta[idx] = rem - nrm * dot[:, None]
            live[idx[done]] = False
            w.pos.copy_(torch.from_numpy(pos))              # the moved bodies go back up, their boxes come back down
            w.bodies_aabb()
            bb = w.aabb.cpu().numpy()[:w.n].copy()
    w.lvel[torch.from_numpy(movers.astype(np.int64)).to(w.device)] = 0
    torch.cuda.synchronize()


def run(workload, a):
    w, _b, terrain = scene(workload)
    res = dict(workload=workload, bodies=w.n, statics=w.n_static, movers=a.movers, k=a.k, runs=a.runs, unit="us per call [min, median, max]")
    w.bodies_aabb()
    movers, mix = mixes(w, a.movers, 10)
    for name, (vel, air) in mix.items():
        s = Slide(w, movers, vel, air)
        res["restore_us"] = event_us(s.restore, a.k, a.runs)

        def index_only():
            s.restore()
            w.bp_index()
        res["restore_index_us"] = event_us(index_only, a.k, a.runs)
        res[f"slide_{name}_grid_us"] = event_us(lambda: s.call(True), a.k, a.runs)
        res[f"slide_{name}_brute_us"] = event_us(lambda: s.call(False), 1, 3)
        torch.cuda.synchronize()
        fl = s.flags.cpu().numpy()
        res[f"slide_{name}_flags"] = [int((fl & b).astype(bool).sum()) for b in (1, 2, 4)]
        res[f"slide_{name}_blocked"] = int((s.first.cpu().numpy()[:, 0] < 1).sum())
        s.restore()
    # the yardstick on a sample of the movers, against the device call on the same sample
    hm = movers[:a.host_movers]
    for name, (vel, air) in mix.items():
        s = Slide(w, hm, vel[:a.host_movers], air[:a.host_movers])
        res[f"sample_{name}_grid_us"] = event_us(lambda: s.call(True), a.k, a.runs)
        times = []
        for _ in range(2):
            s.restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_loop(w, hm, vel[:a.host_movers], air[:a.host_movers])
            times.append((time.perf_counter() - t0) * 1e6)
        res[f"sample_{name}_host_loop_us"] = [round(min(times), 1), round(max(times), 1)]
        s.restore()
    res["host_movers"] = a.host_movers
    # layer 1: the sweep with gathered candidates, and the existing launch fed one-candidate lists (README's row)
    R = np.random.Generator(np.random.PCG64(10))
    n = a.movers
    sb = R.choice(w.n, n, replace=False).astype(np.uint32)
    delta = np.concatenate([R.uniform(-0.3, 0.3, (n, 1)), np.full((n, 1), -0.5), R.uniform(-0.3, 0.3, (n, 1))], 1).astype(f32)
    dev = w.device
    sb_d, dl_d = torch.from_numpy(sb.view(np.int32)).to(dev), torch.from_numpy(delta).to(dev)
    cf_d = torch.arange(n + 1, dtype=torch.int32, device=dev)
    cd_d = torch.full((n,), terrain, dtype=torch.int32, device=dev)
    frac, nrm, hit, fl = (torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros((n, 3), dtype=torch.float32, device=dev),
                          torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
    g, sg = w.body_geoms(), w.static_geoms()
    L = _lib.lib()
    w.bodies_aabb()
    w.bp_index()

    def grid_sweep(bp):
        _lib.check(L.clapgpu_sweep_capsules_grid(physics._stream(), bp, C.byref(w._desc), C.byref(sg), w._meshes, n, sb_d.data_ptr(),
                                                 dl_d.data_ptr(), frac.data_ptr(), nrm.data_ptr(), hit.data_ptr(), fl.data_ptr()), "grid")
    res["sweep_grid_us"] = event_us(lambda: grid_sweep(w._bp), a.k, a.runs)
    res["sweep_brute_us"] = event_us(lambda: grid_sweep(None), 1, 3)
    res["sweep_host_lists_terrain_only_us"] = event_us(
        lambda: _lib.check(L.clapgpu_sweep_capsules(physics._stream(), C.byref(g), C.byref(sg), w._meshes, n, sb_d.data_ptr(),
                                                    dl_d.data_ptr(), cf_d.data_ptr(), cd_d.data_ptr(), frac.data_ptr(),
                                                    nrm.data_ptr(), hit.data_ptr()), "lists"), a.k, a.runs)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="both", choices=["A", "B", "both"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--movers", type=int, default=65536)
    ap.add_argument("--host-movers", type=int, default=512)
    a = ap.parse_args()
    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    for wl in (("A", "B") if a.workload == "both" else (a.workload,)):
        print(json.dumps(run(wl, a)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
