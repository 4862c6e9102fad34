"""Times posing static triangle meshes through both kinds of mesh set -- the plain one (clapgpu_trimesh_create: a pose
rebuilds the tree over every triangle) and the one in parts (clapgpu_trimesh_create_parts: a pose refits) -- at the scene
of tools/mesh_contact_time.py with the meshes of tools/trimesh_ray_time.py: (A) the 130 050-triangle terrain, (B) the
terrain and 2 048 meshes of 512 triangles.  One JSON line per workload, everything in one process: creation of either
kind, the full pose through either, clapgpu_trimesh_pose_meshes of 1, 16 and 256 of the small meshes (B) and of the
terrain alone, and three queries through either set (65 536 ground rays through the grid, index + ground collide of
65 536 bodies, clapgpu_contacts_meshes).  Every figure is [median, min, max] of --reps runs (CUDA events), microseconds.
    python tools/trimesh_pose_time.py [--reps 20] [--workload A|B|both]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clap_amd import _lib, physics  # noqa: E402
from mesh_contact_time import scene  # noqa: E402  (the meshes are trimesh_ray_time's: workloads A and B)


def stats(fn, reps):
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
    return [round(float(np.median(out)), 1), round(float(min(out)), 1), round(float(max(out)), 1)]


def run(workload, reps):
    w, b, _terrain = scene(workload)                                     # the plain set is set
    lib, st = _lib.lib(), physics._stream()
    keep = w._meshes_keep
    M = int(keep["static_index"].shape[0])
    res = dict(workload=workload, bodies=w.n, statics=w.n_static, meshes=M, reps=reps)
    desc = _lib.TrimeshDesc(M, w.n_static, *[keep[k].data_ptr() for k in ("static_index", "vx_first", "tri_first", "vx", "idx", "scale",
                                                                           "pos", "quat")])

    def create(name):
        def go():
            out = C.c_void_p()
            _lib.check(getattr(lib, name)(st, C.byref(out), C.byref(desc)), name)
            lib.clapgpu_trimesh_destroy(out)
        return go
    res["create_us"] = stats(create("clapgpu_trimesh_create"), reps)
    res["create_parts_us"] = stats(create("clapgpu_trimesh_create_parts"), reps)

    pos_d, q_d = keep["pos"].clone(), keep["quat"].clone()
    R = np.random.Generator(np.random.PCG64(11))
    n = 65536
    sel = R.choice(w.n, n, replace=False).astype(np.uint32)
    ray_off = b["yoffset"][sel] * 0.9
    ray_len = b["yoffset"][sel] - (ray_off - 0.05) + 1e-3
    ray = np.zeros((n, 8))
    ray[:, 0:3] = b["pos"][sel] - np.stack([np.zeros(n), ray_off - 0.05, np.zeros(n)], 1)
    ray[:, 3:6], ray[:, 6] = [0, -1.0, 0], 2 * ray_len
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()
    rd, sk = dev(ray, np.float64), dev(sel.view(np.int32), np.int32)
    outs = [torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
            torch.empty((n, 6), dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")]
    body_d, off_d, gr_d = sk, dev(ray_off, np.float64), dev(R.uniform(0, 1, n) < 0.5, np.uint8)
    o8, nrm = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda")
    scratch = torch.empty(w.n, dtype=torch.int32, device="cuda")
    g, sg = w.body_geoms(), w.static_geoms()
    pos0 = w.pos.clone()

    def rays():
        _lib.check(lib.clapgpu_ray_cast(st, w._bp, C.byref(g), C.byref(sg), w._meshes, n, rd.data_ptr(), sk.data_ptr(),
                                        *[o.data_ptr() for o in outs]), "clapgpu_ray_cast")

    def index_ground():
        w.pos.copy_(pos0)                                                # the same bodies in the same place every run
        w.bp_index()
        _lib.check(lib.clapgpu_bodies_ground_collide(st, w._bp, C.byref(w._desc), C.byref(sg), w._meshes, n, body_d.data_ptr(),
                                                     off_d.data_ptr(), gr_d.data_ptr(), o8.data_ptr(), nrm.data_ptr(),
                                                     outs[0].data_ptr(), outs[1].data_ptr(), outs[3].data_ptr(), scratch.data_ptr()),
                   "clapgpu_bodies_ground_collide")

    def some(k, first):                                                  # k meshes from `first` on, moved a little
        idx = dev(np.arange(first, first + k, dtype=np.int32), np.int32)
        p = pos_d[first:first + k].clone() + 0.125
        q = q_d[first:first + k].clone()
        return lambda: _lib.check(lib.clapgpu_trimesh_pose_meshes(st, w._meshes, k, idx.data_ptr(), p.data_ptr(), q.data_ptr()),
                                  "clapgpu_trimesh_pose_meshes")

    for kind in ("plain", "parts"):
        if kind == "parts":
            out = C.c_void_p()
            _lib.check(lib.clapgpu_trimesh_create_parts(st, C.byref(out), C.byref(desc)), "clapgpu_trimesh_create_parts")
            w._free_meshes()
            w._meshes = out
            res["parts_status"] = list(w.static_meshes_parts_status())
        res[f"{kind}_depth"] = w.static_meshes_status()[0]
        res[f"{kind}_pose_all_us"] = stats(lambda: _lib.check(lib.clapgpu_trimesh_pose(st, w._meshes, pos_d.data_ptr(), q_d.data_ptr()),
                                                              "clapgpu_trimesh_pose"), reps)
        if kind == "parts":
            res["parts_pose_terrain_us"] = stats(some(1, 0), reps)
            for k in (1, 16, 256):
                if M > k:
                    res[f"parts_pose_{k}_small_us"] = stats(some(k, 1), reps)
            _lib.check(lib.clapgpu_trimesh_pose(st, w._meshes, pos_d.data_ptr(), q_d.data_ptr()), "clapgpu_trimesh_pose")
        w.pos.copy_(pos0)
        w.bodies_aabb()
        w.bp_index()
        res[f"{kind}_ground_rays_65536_us"] = stats(rays, reps)
        res[f"{kind}_index_ground_collide_65536_us"] = stats(index_ground, reps)
        w.pos.copy_(pos0)
        w.bodies_aabb()
        w.broadphase()
        w.alloc_mesh_contacts(8 * w.n)
        res[f"{kind}_contacts_meshes_us"] = stats(w.contacts_meshes, reps)
        torch.cuda.synchronize()
        res[f"{kind}_mesh_records"] = int(w.mesh_contact_total.item())
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
