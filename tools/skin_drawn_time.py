"""Times clapgpu_skin_drawn against clapgpu_skin at BASELINE configs[2] (50 000 characters x 200 vertices, 64 joints, one
distinct mesh per character), and the FrameLoop frame with and without skin_select.

Workload: the characters' entities are SURVEY 8(d)'s C1 population (synth.entities_flat: U(-500,500) x U(-50,50) x
U(-500,500)) under its camera (synth.camera(): the origin, looking down -Z).  The entity update's cull and the LOD pick
(lod_min 0, lod_max 3) run once on the device and leave the plane and cur_lod the skinning follows; the drawn fraction and
the LOD histogram they give are printed.  LOD lists: a SYNTHETIC thinning -- LOD 0 every vertex (CLAPGPU_SKIN_LOD_ALL),
LOD 1 every 2nd, LOD 2 every 4th, LOD 3 every 8th vertex of the mesh (100 / 50 / 25 / 12.5 %), one row for all; and, as
"prefix" lists, the same counts as the FIRST 100 / 50 / 25 vertices (a vertex buffer ordered coarse-first), which touch
whole cache lines where the strided lists touch 12 bytes of each.

Rows: plain clapgpu_skin; skin_drawn with everything drawn and no lists (the price of the selection); the culled
population without lists; the culled population with the strided lists; the same with the prefix lists.  Per row: us
[min, median, max], the algorithmic bytes of CharacterBatch.skin_algorithmic_bytes / skin_drawn_algorithmic_bytes, and
bytes/s at the median.

Method: one process, warm-up, `--runs` timed calls per row with the rows ALTERNATED, HIP events
around each call, a synchronise before the events are read.  --frame: the same for two FrameLoop frames (1M entities in
chains of 8 with the characters on 50 000 of their roots, pose + skinning; no physics, particles or lights), one with
skin_select.  One JSON line.
    python tools/skin_drawn_time.py [--chars 50000] [--runs 20] [--frame]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clap_amd import _lib, animation, entities, frame, synth, tiler  # noqa: E402

DEV = "cuda:0"
J, VPC = 64, 200


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


def thinning():
    """(lod_first [1, 4], lod_count [1, 4], list): every vertex, every 2nd, 4th, 8th"""
    parts = [np.arange(0, VPC, s, dtype=np.uint32) for s in (2, 4, 8)]
    first = np.asarray([[_lib.SKIN_LOD_ALL, 0, len(parts[0]), len(parts[0]) + len(parts[1])]], np.uint32)
    count = np.asarray([[0] + [len(p) for p in parts]], np.uint32)
    return first, count, np.concatenate(parts)


def prefix():
    """the same counts for a vertex buffer ordered coarse-first: LOD l draws the first 100 / 50 / 25 vertices"""
    parts = [np.arange(0, VPC // s, dtype=np.uint32) for s in (2, 4, 8)]
    first, count, _l = thinning()
    return first, count, np.concatenate(parts)


def character_batch(n, entity_mx, entity_index=None):
    sk = synth.skeleton(J, 8, seed=3)
    an = synth.animation(J, 30, 2.0, seed=3)
    ch = synth.characters(n, J, seed=3)
    mesh = synth.skinned_mesh(VPC, J, seed=3, copies=n)                # what bench.py builds: distinct vertices per character
    vf = (np.arange(n, dtype=np.int64) * VPC).astype(np.uint32)
    model = animation.SkinnedModel(sk, [an], mesh=mesh, device=DEV)
    cb = animation.CharacterBatch(model, n, ch["trs0"], ch["char_mx"] if entity_mx is None else entity_mx, entity_index=entity_index,
                                  vert_first=vf, vert_count=np.full(n, VPC, np.uint32))
    return cb, ch


def culled_population(n):
    """the C1 population under its camera: (plane tensor, cur_lod tensor, entity slots of the characters, n_entities)"""
    scene = synth.pad_levels(synth.entities_flat(n, seed=1234))
    scene["model_lod"] = np.asarray([[0, 3]], np.uint8)
    batch = entities.EntityBatch(scene, DEV)
    cam = synth.camera()
    batch.mq_update(entities.view_calc_frustum(cam)[0])
    batch.compact_visible_lod(cam["cam_pos"])
    torch.cuda.synchronize()
    return batch, scene["slot_of"][:n].astype(np.uint32)


def kernels(n, runs):
    cb, ch = character_batch(n, None)
    cb.set_frame_times(ch["phase"])
    cb.pose_update()
    batch, ent = culled_population(n)
    everything = torch.full_like(batch.vis_mask, -1)
    variants = {
        "skin": (None, cb.skin),
        "drawn_all_no_lists": (dict(planes=[everything], n_entities=batch.n, entity=ent), cb.skin_drawn),
        "drawn_culled_no_lists": (dict(planes=[batch.vis_mask], n_entities=batch.n, entity=ent, cur_lod=batch.cur_lod), cb.skin_drawn),
        "drawn_culled_lists": (dict(planes=[batch.vis_mask], n_entities=batch.n, entity=ent, cur_lod=batch.cur_lod,
                                    lod_lists=thinning()), cb.skin_drawn),
        "drawn_culled_prefix_lists": (dict(planes=[batch.vis_mask], n_entities=batch.n, entity=ent, cur_lod=batch.cur_lod,
                                           lod_lists=prefix()), cb.skin_drawn),
    }
    # one select descriptor per variant, swapped in before its call (set_skin_select allocates: not inside the timed loop)
    descs, info = {}, {}
    for name, (kw, _fn) in variants.items():
        if kw is None:
            continue
        cb.set_skin_select(**kw)
        descs[name] = (cb._sel_desc, cb._sel_lists_host, cb._sel_row_host,
                       [cb.skinned, cb.sel_chars, cb.sel_count, cb.sel_status, cb._sel_scratch, cb._sel_lists, cb._sel_entity])
        cb.skin_drawn()
        out = cb.download()
        sk = out["skinned"]
        hist = np.bincount(sk[sk != _lib.SKIN_NOT_DRAWN], minlength=4)[:4]
        info[name] = dict(drawn=int(out["count"]), drawn_frac=round(out["count"] / n, 4), lod_hist=[int(h) for h in hist],
                          status=out["status"], bytes=cb.skin_drawn_algorithmic_bytes(sk))
    info["skin"] = dict(drawn=n, bytes=cb.skin_algorithmic_bytes())

    def use(name):
        if name in descs:
            cb._sel_desc, cb._sel_lists_host, cb._sel_row_host, _keep = descs[name]

    times = {k: [] for k in variants}
    for r in range(runs + 10):                                         # alternated; the first ten of each are warm-up
        for name, (_kw, fn) in variants.items():
            use(name)
            us = event_us(fn)
            if r >= 10:
                times[name].append(us)
    rows = {}
    for name in variants:
        t = tri(times[name])
        rows[name] = dict(us=t, **info[name], gbytes_per_s=round(info[name]["bytes"] / (t[1] * 1e-6) / 1e9, 1))
    return rows


def frames(n, runs):
    """the frame with and without skin_select: 1M entities (125 000 chains of 8), the characters on `n` of the roots"""
    raw = synth.entities_chains(125_000, 8, seed=2)
    scene, tl = tiler.tiled_scene(raw)
    scene["model_lod"] = np.asarray([[0, 3]], np.uint8)
    roots = tl["slot_of"][np.flatnonzero(raw["parent"] < 0)]
    ent = roots[:n].astype(np.uint32)
    loops = {}
    for key in ("plain", "skin_select"):
        batch = entities.EntityBatch(scene, DEV)
        cb, ch = character_batch(n, batch.mx, ent)
        cb.start_clock(ani_time=-ch["phase"].astype(np.float64), speed=np.ones(n, np.float32))
        loops[key] = frame.FrameLoop(batch, synth.camera(), characters=cb, pose_readers=(),
                                     skin_select=dict(lod_lists=thinning()) if key == "skin_select" else None)
    out = {k: [] for k in loops}
    dt = 1.0 / 120.0
    for f in range(runs + 10):
        for key, loop in loops.items():
            us = event_us(lambda: loop.clap_frame(1.0 + f * dt, dt))
            if f >= 10:
                out[key].append(us)
    d = loops["skin_select"].characters.download()
    sk = d["skinned"]
    res = {"frame_" + k + "_us": tri(v) for k, v in out.items()}
    res["frame_drawn"] = d["count"]
    res["frame_lod_hist"] = [int(h) for h in np.bincount(sk[sk != _lib.SKIN_NOT_DRAWN], minlength=4)[:4]]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chars", type=int, default=50_000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--frame", action="store_true")
    a = ap.parse_args()
    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    res = dict(chars=a.chars, verts_per_char=VPC, joints=J, runs=a.runs, abi=_lib.ABI_VERSION, unit="us [min, median, max]",
               lists="LOD 0 all, LOD 1 / 2 / 3 every 2nd / 4th / 8th vertex (synthetic)")
    res["rows"] = kernels(a.chars, a.runs)
    if a.frame:
        res.update(frames(a.chars, a.runs))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
