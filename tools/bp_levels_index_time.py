"""Times the queries through a leveled broadphase index (clapgpu_bp_leveled_index) at the mixed workload of
tools/bp_time.py --mixed --levels 6 (262 144 sphere bodies of radius 0.025 .. 4, six levels from cell 0.25) with the
5 000 statics of tools/ray_time.py, and prints one JSON line: 65 536 ground rays and 65 536 capsule sweeps
  * through the leveled index (switch on),
  * through the same object's scan of every geom (switch off: what the object did before it had an index),
  * through the index of the one exact one-level object (cell = the largest edge, 8),
and clapgpu_bp_index of both objects.  Medians of --reps runs (--scan-reps for the scans), CUDA events around one call
each, in microseconds.
    python tools/bp_levels_index_time.py [--reps 10] [--scan-reps 3] [--n 262144] [--queries 65536]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clap_amd import _lib, physics, synth  # noqa: E402

LEVELS, CELL0 = 6, 0.25


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return float(np.median(out))


def statics():
    R = np.random.Generator(np.random.PCG64(5))
    ns = 5000
    lo = R.uniform(-5, 65, (ns, 3))
    bb = np.empty((ns, 6))
    bb[:, 0::2], bb[:, 1::2] = lo, lo + R.uniform(0.1, 3.0, (ns, 3))
    bb[0] = [-1e3, 1e3, -10.0, 0.0, -1e3, 1e3]
    return bb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scan-reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=262_144)
    ap.add_argument("--queries", type=int, default=65536)
    a = ap.parse_args()
    lib = _lib.lib()
    _lib.check(lib.clapgpu_init(0), "clapgpu_init")
    b = synth.mixed_bodies(a.n, box=64.0 * (a.n / 262_144) ** (1 / 3), cell0=CELL0, seed=4)
    one_cell = float(2.0 * b["radius"].max())
    st = statics()
    lev = physics.PhysWorld(b, st, pair_capacity=1024, device="cuda:0", bp_levels=LEVELS, leveled_index=True)
    one = physics.PhysWorld(dict(b, cell=one_cell), st, pair_capacity=1024, device="cuda:0")
    R = np.random.Generator(np.random.PCG64(9))
    n = min(a.queries, a.n)
    sel = R.choice(a.n, n, replace=False).astype(np.uint32)
    # the ground rays as phys_body_ground_collide casts them (tools/ray_time.py): from inside the body, which is skipped
    ray_off = b["yoffset"][sel] * 0.9
    ray_len = b["yoffset"][sel] - (ray_off - 0.05) + 1e-3
    ray = np.zeros((n, 8))
    ray[:, 0:3] = b["pos"][sel] - np.stack([np.zeros(n), ray_off - 0.05, np.zeros(n)], 1)
    ray[:, 4], ray[:, 6] = -1.0, 2 * ray_len
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()
    ray_d, skip_d, body_d = dev(ray, np.float64), dev(sel.view(np.int32), np.int32), dev(sel.view(np.int32), np.int32)
    delta_d = dev(R.normal(0, 0.1, (n, 3)), np.float32)
    f64, i32, f32 = torch.float64, torch.int32, torch.float32
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")
    rout = [new(n, f64), new(n, i32), new((n, 6), f64), new(n, i32)]
    sout = [new(n, f32), new((n, 3), f32), new(n, i32), new(n, i32)]
    stream = physics._stream()

    def rays(w):
        g, sg = w.body_geoms(), w.static_geoms()
        return lambda: _lib.check(lib.clapgpu_ray_cast(stream, w._bp, C.byref(g), C.byref(sg), None, n, ray_d.data_ptr(),
                                                       skip_d.data_ptr(), *[o.data_ptr() for o in rout]), "clapgpu_ray_cast")

    def sweeps(w):
        sg = w.static_geoms()
        return lambda: _lib.check(lib.clapgpu_sweep_capsules_grid(stream, w._bp, C.byref(w._desc), C.byref(sg), None, n,
                                                                  body_d.data_ptr(), delta_d.data_ptr(),
                                                                  *[o.data_ptr() for o in sout]), "clapgpu_sweep_capsules_grid")

    res = dict(bodies=a.n, statics=len(st), levels=LEVELS, cell0=CELL0, one_level_cell=one_cell, queries=n, reps=a.reps,
               scan_reps=a.scan_reps)
    hits = {}
    for name, w, reps in (("leveled_index", lev, a.reps), ("one_level_index", one, a.reps), ("leveled_scan", lev, a.scan_reps)):
        if name == "leveled_scan":
            lev.bp_leveled_index(False)
        else:
            res[f"{name}_bp_index_us"] = timed(w.bp_index, a.reps)
        w.bp_index()
        res[f"{name}_status"] = w.bp_index_status()
        res[f"{name}_ground_rays_us"] = timed(rays(w), reps)
        res[f"{name}_sweeps_us"] = timed(sweeps(w), reps)
        torch.cuda.synchronize()
        hits[name] = [o.clone() for o in rout[:2] + sout[:1] + sout[2:3]]
    res["ray_hits"] = int((hits["leveled_scan"][1] != -1).sum().item())
    res["sweep_hits"] = int((hits["leveled_scan"][3] != -1).sum().item())
    hit_of = lambda h: (torch.where(h[1] != -1, h[0], torch.zeros_like(h[0])), h[1], h[2], h[3])   # dist: unchanged on a miss
    res["same_results"] = all(torch.equal(x, y) for k in ("leveled_index", "one_level_index")
                              for x, y in zip(hit_of(hits[k]), hit_of(hits["leveled_scan"])))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
