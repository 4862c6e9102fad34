"""Times contacts against static triangle meshes at the physics scene of tools/ray_time.py (262 144 bodies, 5 000
statics) with the meshes of tools/trimesh_ray_time.py -- (A) a 256 x 256 heightfield terrain (130 050 triangles) or (B)
that terrain and 2 048 meshes of 512 triangles -- the mesh statics' broadphase boxes holding their meshes, and every body
placed on the terrain (its lowest point about 5 % of its size below the surface).  Prints one JSON line per workload:
clapgpu_contacts_meshes after one broadphase (the records, capped pairs), a batch of 65 536 capsule sweeps against the
terrain static with and without the mesh set, and a captured frame (FrameLoop, 2 000 entities, contacts on) with and
without the mesh pass.  Medians of --reps runs (CUDA events), microseconds.
    python tools/mesh_contact_time.py [--reps 20] [--workload A|B|both]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clap_amd import _lib, entities, frame, physics, synth  # noqa: E402
from ray_time import timed  # noqa: E402
from trimesh_ray_time import terrain  # noqa: E402


def ground(x, z):
    return synth.terrain_y(x + 2.0, z + 2.0, y0=-1.0)                    # the surface of terrain(256, 64, (-2, 0, -2))


def scene(workload):
    R = np.random.Generator(np.random.PCG64(9))
    meshes = [terrain(256, 64.0, [-2.0, 0.0, -2.0])]
    if workload == "B":
        small = terrain(17, 4.0, [0, 0, 0])
        for _ in range(2048):
            meshes.append((small[0], small[1], R.uniform(-5, 60, 3)))
    b = synth.capsule_bodies(262_144, box=60.0, seed=4)
    P = np.random.Generator(np.random.PCG64(6))
    x, z = P.uniform(0, 60, b["n"]), P.uniform(0, 60, b["n"])
    half = b["radius"] + 0.5 * b["length"]
    b["pos"][:, 0], b["pos"][:, 2] = x, z
    b["pos"][:, 1] = ground(x, z) + 0.95 * half
    b["lvel"][:] = 0
    S = np.random.Generator(np.random.PCG64(5))                          # the statics of tools/ray_time.py
    ns = 5000
    lo = S.uniform(-5, 65, (ns, 3))
    bb = np.empty((ns, 6))
    bb[:, 0::2], bb[:, 1::2] = lo, lo + S.uniform(0.1, 3.0, (ns, 3))
    bb[0] = [-1e3, 1e3, -10.0, -3.0, -1e3, 1e3]                          # the floor box lies below the terrain
    kind = S.choice([0, 1, 2, 3], ns, p=[0.3, 0.3, 0.3, 0.1]).astype(np.uint8)
    kind[0] = 2
    sidx = np.arange(1, 1 + len(meshes))                                 # the mesh statics: OTHER, boxes holding the meshes
    kind[sidx] = 3
    for k, (vx, _i, org) in enumerate(meshes):
        v = vx.astype(np.float64) + org
        bb[sidx[k], 0::2], bb[sidx[k], 1::2] = v.min(0) - 1e-3, v.max(0) + 1e-3
    c, axis, r, length = synth.geoms_of_aabbs(bb, kind)
    w = physics.PhysWorld(b, bb, pair_capacity=4_000_000, static_pair_capacity=8_000_000, device="cuda:0")
    w.set_static_geoms(kind, c, axis, r, length)
    quats = np.tile(np.float32([0, 0, 0, 1]), (len(meshes), 1))
    w.set_static_meshes(sidx, [m[0] for m in meshes], [m[1] for m in meshes], np.ones(len(meshes)), [m[2] for m in meshes], quats)
    return w, b, int(sidx[0])


def run(workload, reps):
    w, b, terrain = scene(workload)
    res = dict(workload=workload, bodies=w.n, statics=w.n_static, reps=reps)
    depth, ntri = w.static_meshes_status()
    res.update(triangles=ntri, depth=depth)
    w.broadphase()
    torch.cuda.synchronize()
    res["static_pairs"] = int(w.static_pair_total.item())
    w.alloc_mesh_contacts(8 * w.n)
    res["contacts_meshes_us"] = timed(w.contacts_meshes, reps)
    _rec, _ref, total, capped = w.download_mesh_contacts(np.dtype([("b", np.uint8, 160)]))
    res.update(mesh_records=total, capped_pairs=capped)
    res["contacts_geoms_both_us"] = timed(w.contacts_geoms_both, reps)   # the existing lists of the same step, for scale
    # sweeps: 65 536 characters, each against the terrain static, 0.5 down and up to 0.3 sideways
    R = np.random.Generator(np.random.PCG64(10))
    n = 65536
    sb = R.choice(w.n, n, replace=False).astype(np.uint32)
    delta = np.concatenate([R.uniform(-0.3, 0.3, (n, 1)), np.full((n, 1), -0.5), R.uniform(-0.3, 0.3, (n, 1))], 1).astype(np.float32)
    cf = np.arange(n + 1, dtype=np.uint32)
    cand = np.full(n, terrain, np.uint32)
    for meshes in (True, False):
        res[f"sweep_65536_{'meshes' if meshes else 'no_meshes'}_us"] = timed(lambda: w.sweep_capsules(sb, delta, cf, cand, meshes=meshes), reps)
    # a captured frame with and without the mesh pass
    scn = synth.pad_levels(synth.entities_flat(2000, seed=3))
    dt = 1.0 / 120.0
    for meshes in (True, False):
        saved = w._meshes
        if not meshes:
            w._meshes = None
        loop = frame.FrameLoop(entities.EntityBatch(scn, "cuda:0"), synth.camera(pos=(0, 10, 60)), world=w, contacts=True)
        loop.capture(dt)
        w._meshes = saved
        k = [0]

        def replay():
            k[0] += 1
            loop.clap_frame_replay(k[0] * dt)
        res[f"frame_{'with' if meshes else 'without'}_mesh_pass_us"] = timed(replay, reps)
        del loop
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
