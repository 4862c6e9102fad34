"""Writes every output array of the rigid-body entry points raw into a directory, for a byte-for-byte comparison of two
builds of the library (select one with CLAPGPU_LIB, one process per library; `cmp` the two directories' files):
the full physics scene of tools/ray_time.py (262 144 capsule-mix bodies, 5 000 statics) after 8 substeps with and without
prebin, both pair lists of clapgpu_bp_collide, the 160-byte records of clapgpu_contacts_geoms and _geoms_both,
clapgpu_bp_index + clapgpu_ray_cast, the entity arrays after clapgpu_phys_body_update, and on a sphere scene the
104-byte records of clapgpu_contacts_spheres / _sphere_box with and without materials.
    python tools/physics_dump.py OUTDIR"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clap_amd import _lib, physics, synth  # noqa: E402
import ray_time  # noqa: E402


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    count = [0]

    def save(name, a):
        a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        np.ascontiguousarray(a).tofile(os.path.join(out, name + ".bin"))
        count[0] += 1

    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    for prebin in (False, True):
        tag = "prebin" if prebin else "plain"
        w, b = ray_time.scene()
        for _ in range(8):
            w.world_step(1.0 / 120.0, prebin=prebin)
        torch.cuda.synchronize()
        for k in ("pos", "quat", "lvel", "avel", "aabb", "axis", "geom_records", "bflags", "adis_steps_left", "adis_time_left"):
            save(f"{tag}_step8_{k}", getattr(w, k))
        w.broadphase()                                       # after a prebinning step: without its own bin launch
        torch.cuda.synchronize()
        d = w.download()
        save(f"{tag}_pairs", d["pairs"])
        save(f"{tag}_static_pairs", d["static_pairs"])
        save(f"{tag}_pair_totals", np.array([d["pair_total"], d["static_pair_total"], w.broadphase_status()], np.uint32))
        for both in (False, True):
            name = "geoms_both" if both else "geoms"
            (w.contacts_geoms_both if both else w.contacts_geoms)()
            c = w.download_contacts2(np.uint8)
            save(f"{tag}_{name}_body", c["body"][0])
            save(f"{tag}_{name}_static", c["static"][0])
            save(f"{tag}_{name}_totals", np.array([c["body"][1], c["static"][1]], np.uint32))
        save(f"{tag}_bflags_after_contacts", w.bflags)
        if prebin:
            w.world_step(1.0 / 120.0, prebin=True)           # indexed without using the prebin up, then collided
        w.bp_index()
        R = np.random.Generator(np.random.PCG64(9))
        n = 65536
        sel = R.choice(w.n, n, replace=False).astype(np.uint32)
        pos = w.pos.cpu().numpy()
        start = pos[sel] + np.array([0.0, 0.05, 0.0])
        for rays, (s, dr, ln, skip) in (("ground", (start, np.tile([0, -1.0, 0], (n, 1)), np.full(n, 2.0), sel.astype(np.int32))),
                                        ("down", (np.concatenate([R.uniform(0, 60, (1024, 1)), np.full((1024, 1), 80.0),
                                                                  R.uniform(0, 60, (1024, 1))], 1),
                                                  np.tile([0, -1.0, 0], (1024, 1)), np.full(1024, 1e6), None))):
            res = w.ray_cast(s, dr, ln, skip, grid=True, meshes=False)
            torch.cuda.synchronize()
            for k, t in zip(("dist", "hit", "contact", "flags"), res):
                save(f"{tag}_ray_{rays}_{k}", t)
        save(f"{tag}_index_status", np.array([w.bp_index_status()], np.uint32))
        w.broadphase()
        torch.cuda.synchronize()
        d = w.download()
        save(f"{tag}_pairs_after_index", d["pairs"])
        save(f"{tag}_static_pairs_after_index", d["static_pairs"])
        if not prebin:
            ne = int(b["body_entity"].max()) + 1
            ent = types.SimpleNamespace(n=ne, pos_scale=torch.zeros((ne, 4), dtype=torch.float32, device="cuda"),
                                        rot=torch.zeros((ne, 4), dtype=torch.float32, device="cuda"),
                                        flags=torch.zeros(ne, dtype=torch.int32, device="cuda"))
            moving = torch.zeros(w.n, dtype=torch.uint8, device="cuda")
            w.phys_body_update(ent, moving)
            torch.cuda.synchronize()
            for k in ("pos_scale", "rot", "flags"):
                save(f"body_update_{k}", getattr(ent, k))
            save("body_update_moving", moving)
        del w

    # sphere bodies against each other and against static boxes: the 104-byte records
    n = 262_144
    b = synth.sphere_bodies(n, box=48.0, seed=4)
    R = np.random.Generator(np.random.PCG64(5))
    ns = 5000
    lo = R.uniform(-2, 48, (ns, 3))
    statics = np.empty((ns, 6))
    statics[:, 0::2], statics[:, 1::2] = lo, lo + R.uniform(0.1, 3.0, (ns, 3))
    mat = np.stack([R.uniform(0, 1, n) * (R.uniform(0, 1, n) < 0.5), R.uniform(0, 2, n), R.uniform(0, 2, n),
                    R.uniform(0, 0.5, n) * (R.uniform(0, 1, n) < 0.7), R.uniform(0, 0.1, n) * (R.uniform(0, 1, n) < 0.7)], 1)
    smat = np.stack([R.uniform(0, 1, ns) * (R.uniform(0, 1, ns) < 0.5), R.uniform(0, 2, ns), R.uniform(0, 2, ns),
                     R.uniform(0, 0.5, ns) * (R.uniform(0, 1, ns) < 0.7), R.uniform(0, 0.1, ns) * (R.uniform(0, 1, ns) < 0.7)], 1)
    for tag, material, static_material in (("nomat", None, None), ("mat", mat, smat)):
        w = physics.PhysWorld(b, statics, pair_capacity=8 * n, device="cuda:0")
        if material is not None:
            w.set_materials(material)
        w.broadphase()
        w.contacts()
        w.contacts_static(static_material)
        recs, total = w.download_contacts(np.uint8)
        srecs, stotal = w.download_static_contacts(np.uint8)
        save(f"spheres_{tag}_records", recs)
        save(f"spheres_{tag}_static_records", srecs)
        save(f"spheres_{tag}_totals", np.array([total, stotal, len(recs) // 104, len(srecs) // 104], np.uint32))
        del w
    print(f"{count[0]} files in {out}")


if __name__ == "__main__":
    main()
