"""Times ray casts against static triangle meshes at the full physics scene of tools/ray_time.py (262 144 bodies, 5 000
statics) plus (A) a 256 x 256 heightfield terrain (130 050 triangles) or (B) that terrain and 2 048 more meshes of 512
triangles each, and prints one JSON line per workload: clapgpu_trimesh_create and _pose (rebuild), the tree height,
and grid clapgpu_ray_cast for 65 536 ground rays, 4 camera rays and 1 024 rays 10^6 long with and without the mesh
set, and clapgpu_bodies_ground_collide with the mesh set for 65 536 bodies.  Medians of --reps runs (CUDA events), microseconds.
    python tools/trimesh_ray_time.py [--reps 20] [--workload A|B|both]"""
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
from clap_amd import _lib, physics, synth  # noqa: E402
from ray_time import scene, timed  # noqa: E402


def terrain(nv, side, origin):
    """(vx, idx, origin) of a mesh: synth's heightfield a unit lower, its place in the world carried separately"""
    return synth.heightfield(nv, side, y0=-1.0) + (np.asarray(origin, float),)


def run(workload, reps):
    w, b = scene()
    R = np.random.Generator(np.random.PCG64(9))
    meshes = [terrain(256, 64.0, [-2.0, 0.0, -2.0])]
    if workload == "B":
        small = terrain(17, 4.0, [0, 0, 0])                                # 16 x 16 x 2 = 512 triangles
        for _ in range(2048):
            meshes.append((small[0], small[1], R.uniform(-5, 60, 3)))
    # the mesh statics: the first OTHER statics of the scene take the meshes (their AABBs are the broadphase's; the mesh
    # is where the rays see them)
    kind = w._static_keep["kind"].cpu().numpy()
    others = np.nonzero(kind == _lib.GEOM_OTHER)[0]
    extra = len(meshes) - len(others)
    if extra > 0:                                                            # B: more meshes than OTHER statics
        kind[np.nonzero(kind != _lib.GEOM_OTHER)[0][-extra:]] = _lib.GEOM_OTHER
        w._static_keep["kind"].copy_(torch.from_numpy(kind))
        others = np.nonzero(kind == _lib.GEOM_OTHER)[0]
    sidx = others[:len(meshes)]
    quats = np.tile(np.float32([0, 0, 0, 1]), (len(meshes), 1))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    w.set_static_meshes(sidx, [m[0] for m in meshes], [m[1] for m in meshes], np.ones(len(meshes)), [m[2] for m in meshes], quats)
    torch.cuda.synchronize()
    res = dict(workload=workload, bodies=w.n, statics=w.n_static, meshes=len(meshes), reps=reps,
               create_ms_incl_upload=(time.perf_counter() - t0) * 1e3)
    depth, ntri = w.static_meshes_status()
    res.update(triangles=ntri, depth=depth)
    pos_d = torch.from_numpy(np.array([m[2] for m in meshes], np.float64)).cuda()
    q_d = torch.from_numpy(quats).cuda()
    lib = _lib.lib()
    st = physics._stream()
    res["pose_rebuild_us"] = timed(lambda: _lib.check(lib.clapgpu_trimesh_pose(st, w._meshes, pos_d.data_ptr(), q_d.data_ptr()),
                                                      "pose"), reps)
    n = 65536
    sel = R.choice(w.n, n, replace=False).astype(np.uint32)
    ray_off = b["yoffset"][sel] * 0.9
    ray_len = b["yoffset"][sel] - (ray_off - 0.05) + 1e-3
    ground = (b["pos"][sel] - np.stack([np.zeros(n), ray_off - 0.05, np.zeros(n)], 1), np.tile([0, -1.0, 0], (n, 1)), 2 * ray_len)
    cam = (R.uniform(0, 60, (4, 3)), R.normal(size=(4, 3)), np.full(4, 20.0))
    down = (np.concatenate([R.uniform(0, 60, (1024, 1)), np.full((1024, 1), 80.0), R.uniform(0, 60, (1024, 1))], 1),
            np.tile([0, -1.0, 0], (1024, 1)), np.full(1024, 1e6))
    g, sg = w.body_geoms(), w.static_geoms()
    w.bp_index()

    def caster(s, d, ln, meshes, skip=None):
        sk = None if skip is None else torch.from_numpy(np.ascontiguousarray(skip, np.int32)).cuda()
        ray = np.zeros((len(s), 8))
        ray[:, 0:3], ray[:, 3:6], ray[:, 6] = s, d, ln
        rd = torch.from_numpy(ray).cuda()
        m = len(s)
        outs = [torch.empty(m, dtype=torch.float64, device="cuda"), torch.empty(m, dtype=torch.int32, device="cuda"),
                torch.empty((m, 6), dtype=torch.float64, device="cuda"), torch.empty(m, dtype=torch.int32, device="cuda")]
        return lambda: _lib.check(lib.clapgpu_ray_cast(st, w._bp, C.byref(g), C.byref(sg), w._meshes if meshes else None,
                                                       m, rd.data_ptr(), None if sk is None else sk.data_ptr(),
                                                       *[o.data_ptr() for o in outs]), "clapgpu_ray_cast")

    skip = sel.astype(np.int32)
    for name, (s, d, ln), sk in (("ground_65536", ground, skip), ("camera_4", cam, None), ("down_1e6_1024", down, None)):
        res[f"{name}_meshes_us"] = timed(caster(s, d, ln, True, sk), reps)
        res[f"{name}_no_meshes_us"] = timed(caster(s, d, ln, False, sk), reps)
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()
    body_d, off_d, gr_d = dev(sel.view(np.int32), np.int32), dev(ray_off, np.float64), dev(R.uniform(0, 1, n) < 0.5, np.uint8)
    o8, nrm = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda")
    dd, hh, ff = (torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
                  torch.empty(n, dtype=torch.int32, device="cuda"))
    scratch = torch.empty(w.n, dtype=torch.int32, device="cuda")

    def gc():
        _lib.check(lib.clapgpu_bodies_ground_collide(st, w._bp, C.byref(w._desc), C.byref(sg), w._meshes, n,
                                                     body_d.data_ptr(), off_d.data_ptr(), gr_d.data_ptr(), o8.data_ptr(),
                                                     nrm.data_ptr(), dd.data_ptr(), hh.data_ptr(), ff.data_ptr(),
                                                     scratch.data_ptr()), "clapgpu_bodies_ground_collide")

    res["index_plus_ground_collide_meshes_65536_us"] = timed(lambda: (w.bp_index(), gc()), reps)
    res["index_us"] = timed(w.bp_index, reps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--workload", default="both", choices=["A", "B", "both"])
    a = ap.parse_args()
    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    for wl in (("A", "B") if a.workload == "both" else (a.workload,)):
        print(json.dumps(run(wl, a.reps)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
