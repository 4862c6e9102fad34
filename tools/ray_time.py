"""Times the ray-cast entry points at the full physics scene (262 144 capsule-mix bodies, 5 000 statics of kinds box,
sphere, capsule and other, as in tests/test_physics_gpu.py / tests/test_rays_gpu.py) and prints one JSON line:
clapgpu_bp_index, grid and brute-force clapgpu_ray_cast for ground-length, camera and 10^6-long downward rays, and
clapgpu_bodies_ground_collide.  Times are medians of --reps runs (CUDA events around one call each), in microseconds.
    python tools/ray_time.py [--reps 20] [--brute-rays 65536]"""
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


def scene():
    b = synth.capsule_bodies(262_144, box=60.0, seed=4)
    R = np.random.Generator(np.random.PCG64(5))
    ns = 5000
    lo = R.uniform(-5, 65, (ns, 3))
    bb = np.empty((ns, 6))
    bb[:, 0::2], bb[:, 1::2] = lo, lo + R.uniform(0.1, 3.0, (ns, 3))
    bb[0] = [-1e3, 1e3, -10.0, 0.0, -1e3, 1e3]
    kind = R.choice([0, 1, 2, 3], ns, p=[0.3, 0.3, 0.3, 0.1]).astype(np.uint8)
    kind[0] = 2
    c, axis, r, length = synth.geoms_of_aabbs(bb, kind)
    w = physics.PhysWorld(b, bb, pair_capacity=4_000_000, static_pair_capacity=8_000_000, device="cuda:0")
    w.set_static_geoms(kind, c, axis, r, length)
    return w, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--brute-rays", type=int, default=65536, help="rays of the brute-force ground-ray row")
    a = ap.parse_args()
    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    w, b = scene()
    R = np.random.Generator(np.random.PCG64(9))
    n = 65536
    sel = R.choice(w.n, n, replace=False).astype(np.uint32)
    ray_off = b["yoffset"][sel] * 0.9
    ray_len = b["yoffset"][sel] - (ray_off - 0.05) + 1e-3
    ground = (b["pos"][sel] - np.stack([np.zeros(n), ray_off - 0.05, np.zeros(n)], 1), np.tile([0, -1.0, 0], (n, 1)), 2 * ray_len)
    cam = (R.uniform(0, 60, (4, 3)), R.normal(size=(4, 3)), np.full(4, 20.0))
    down = (np.concatenate([R.uniform(0, 60, (1024, 1)), np.full((1024, 1), 80.0), R.uniform(0, 60, (1024, 1))], 1),
            np.tile([0, -1.0, 0], (1024, 1)), np.full(1024, 1e6))
    res = dict(bodies=w.n, statics=w.n_static, cell=w.cell, reps=a.reps)
    lib = _lib.lib()
    g, sg = w.body_geoms(), w.static_geoms()
    st = physics._stream()

    def caster(s, d, ln, grid, skip=None):
        """the C call alone, on device inputs uploaded once"""
        sk = None if skip is None else torch.from_numpy(np.ascontiguousarray(skip, np.int32)).cuda()
        ray = np.zeros((len(s), 8))
        ray[:, 0:3], ray[:, 3:6], ray[:, 6] = s, d, ln
        rd = torch.from_numpy(ray).cuda()
        m = len(s)
        outs = [torch.empty(m, dtype=torch.float64, device="cuda"), torch.empty(m, dtype=torch.int32, device="cuda"),
                torch.empty((m, 6), dtype=torch.float64, device="cuda"), torch.empty(m, dtype=torch.int32, device="cuda")]
        return lambda: _lib.check(lib.clapgpu_ray_cast(st, w._bp if grid else None, C.byref(g), C.byref(sg), None, m, rd.data_ptr(),
                                                       None if sk is None else sk.data_ptr(), *[o.data_ptr() for o in outs]),
                                  "clapgpu_ray_cast")

    res["bp_index_us"] = timed(w.bp_index, a.reps)
    w.bp_index()
    # the ground rays as phys_body_ground_collide casts them: from inside the body's own capsule, which is skipped
    skip = sel.astype(np.int32)
    for name, (s, d, ln), sk in (("ground_65536", ground, skip), ("camera_4", cam, None), ("down_1e6_1024", down, None)):
        res[f"{name}_grid_us"] = timed(caster(s, d, ln, True, sk), a.reps)
    nb = min(a.brute_rays, n)
    res[f"ground_{nb}_brute_us"] = timed(caster(ground[0][:nb], ground[1][:nb], ground[2][:nb], False, skip[:nb]),
                                         max(1, a.reps // 10))
    res["camera_4_brute_us"] = timed(caster(*cam, False), a.reps)
    res["down_1e6_1024_brute_us"] = timed(caster(*down, False), max(1, a.reps // 10))

    # clapgpu_bodies_ground_collide for 65 536 bodies (grid; it clears the index, so each run indexes first)
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()
    body_d, off_d, gr_d = dev(sel.view(np.int32), np.int32), dev(ray_off, np.float64), dev(R.uniform(0, 1, n) < 0.5, np.uint8)
    o8, nrm = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda")
    dd, hh, ff = (torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
                  torch.empty(n, dtype=torch.int32, device="cuda"))
    scratch = torch.empty(w.n, dtype=torch.int32, device="cuda")

    def gc():
        _lib.check(lib.clapgpu_bodies_ground_collide(st, w._bp, C.byref(w._desc), C.byref(sg), None, n, body_d.data_ptr(),
                                                     off_d.data_ptr(), gr_d.data_ptr(), o8.data_ptr(), nrm.data_ptr(),
                                                     dd.data_ptr(), hh.data_ptr(), ff.data_ptr(), scratch.data_ptr()),
                   "clapgpu_bodies_ground_collide")

    res["index_plus_ground_collide_65536_us"] = timed(lambda: (w.bp_index(), gc()), a.reps)
    res["ground_collide_65536_brute_us"] = timed(lambda: _lib.check(lib.clapgpu_bodies_ground_collide(
        st, None, C.byref(w._desc), C.byref(sg), None, n, body_d.data_ptr(), off_d.data_ptr(), gr_d.data_ptr(), o8.data_ptr(),
        nrm.data_ptr(), dd.data_ptr(), hh.data_ptr(), ff.data_ptr(), scratch.data_ptr()), "ground"), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
