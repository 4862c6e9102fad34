"""What a frame with its views in device memory costs and buys (include/clapgpu.h, "Views in device memory").

(a) 1 M entities (BASELINE configs[1]: 125 000 chains of 8, tile layout, every entity dirty): the update with the fused cull
    + the visible list -- today's step -- against the update without cull + clapgpu_entities_cull_views + the visible
    list.  The difference is the price of the separate pass (the fused kernels take their frustum by value and stay as
    they are).
(b) clapgpu_views_calc alone, at n_views 1 and 5.
(c) the 10 k-entity testbed frame of tools/small_frame.py with the camera moving EVERY frame: issued eagerly with host
    views (set_camera rebuilds the descriptor); replayed as a graph with views_dev (set_camera writes the pinned source,
    the replay copies it); and re-captured every frame with host views, the only way a graph follows a camera without
    the view block (the capture alone: no warm-up frame, the state exists).  Wall clock around a synchronise.

Method: one process, warm-up, `--runs` timed calls per row with the rows ALTERNATED; (a) and (b)
between HIP events, (c) on the host clock.  Writes result.json and README.md into --out.
    python tools/frame_views_time.py [--runs 20] [--out profiles/frame_views]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clap_amd import _lib, animation, characters, entities, frame, lights, particles, physics, synth, tiler  # noqa: E402
from clap_amd.views import ViewBlock  # noqa: E402

DEV = "cuda:0"
WARM = 10


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


def wall_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def alternated(rows, runs, clock):
    times = {k: [] for k in rows}
    for r in range(runs + WARM):
        for name, fn in rows.items():
            us = clock(fn)
            if r >= WARM:
                times[name].append(us)
    return {k: tri(v) for k, v in times.items()}


def million(runs):
    scene, _tl = tiler.tiled_scene(synth.entities_chains(125_000, 8, seed=2))
    batch = entities.EntityBatch(scene, DEV)
    cam = synth.camera()
    fr = entities.view_calc_frustum(cam)[0]
    block = ViewBlock(DEV)
    block.set_camera(0, cam)
    block.upload()
    block.calc(1)

    def fused():
        batch.mq_update(fr, all_dirty=True)
        batch.compact_visible()

    def separate():
        batch.mq_update(None, all_dirty=True)
        batch.cull_views(block)
        batch.compact_visible()

    def update_only():
        batch.mq_update(None, all_dirty=True)

    def cull_only():
        batch.cull_views(block)
    fused()
    a = batch.download()
    separate()
    b = batch.download()
    assert np.array_equal(a["vis_mask"], b["vis_mask"]) and np.array_equal(a["visible"], b["visible"]), "the two steps disagree"
    t = alternated(dict(update_fused_cull_list=fused, update_cull_views_list=separate, update_no_cull=update_only,
                        cull_views_alone=cull_only), runs, event_us)
    t["visible"] = int(a["visible_count"])
    t["separate_pass_price_us"] = round(t["update_cull_views_list"][1] - t["update_fused_cull_list"][1], 1)
    return t


def views_calc(runs):
    block = ViewBlock(DEV)
    for s in range(_lib.VIEW_SLOTS):
        block.set_camera(s, synth.camera(pos=(s, 2 * s, 60)))
    block.upload()
    return alternated({"views_calc_1": lambda: block.calc(1), "views_calc_5": lambda: block.calc(5)}, runs, event_us)


def testbed(views_dev):
    """tools/small_frame.py's scene"""
    from oracle import binding as ob
    raw = synth.entities_flat(10_000, seed=1234)
    scene, tl = tiler.tiled_scene(raw)
    roots = tl["slot_of"][np.flatnonzero(raw["parent"] < 0)]
    batch = entities.EntityBatch(scene, DEV)
    n_bodies, n_chars, J, vpc = 128, 10, 64, 2000
    b = synth.sphere_bodies(n_bodies, box=16.0, seed=4)
    b["body_entity"] = roots[:n_bodies].astype(np.int32)
    world = physics.PhysWorld(b, synth.static_boxes(16, 16.0), pair_capacity=4096, device=DEV)
    feed = synth.character_feed(n_chars, seed=13, with_bodies=False)
    feed["entity"] = roots[n_bodies:n_bodies + n_chars].astype(np.uint32)
    cf = characters.CharacterFeed(feed, DEV)
    ls = lights.LightSet(DEV, 1920, 1080, lights.TILE_WIDTH)
    ls.load(synth.lights(16, seed=7))
    ls.set_carriers(roots[-8:].astype(np.uint32), np.arange(8, dtype=np.int32), np.zeros((8, 3), np.float32))
    sk, an = synth.skeleton(J, 8, seed=3), synth.animation(J, 30, 2.0, seed=3)
    ch = synth.characters(n_chars, J, seed=3)
    model = animation.SkinnedModel(sk, [an], mesh=synth.skinned_mesh(vpc, J, seed=3), device=DEV)
    cb = animation.CharacterBatch(model, n_chars, ch["trs0"], batch.mx, entity_index=feed["entity"],
                                  vert_first=np.zeros(n_chars, np.uint32), vert_count=np.full(n_chars, vpc, np.uint32))
    cb.start_clock(ani_time=-ch["phase"].astype(np.float64), speed=np.ones(n_chars, np.float32))
    ps = synth.particle_systems(n_sys=8, count=1024, radius=10.0, velocity=0.005)
    pos, vel, st = ob.particles_spawn(ps, synth.DRAND48_DEFAULT_STATE)
    pb = particles.ParticleBatch(ps, pos, vel, st, DEV)
    return frame.FrameLoop(batch, synth.camera(), world=world, feed=cf, lights=ls, characters=cb, particles=pb, contacts=True,
                           views_dev=views_dev)


def small_frame(runs):
    dt = 1.0 / 120.0
    eager, replayed, recaptured = testbed(False), testbed(True), testbed(False)
    now = {k: 0.0 for k in ("eager", "replayed", "recaptured")}
    step = [0]

    def cam():                                               # a slow orbit: another camera every call
        step[0] += 1
        a = 0.01 * step[0]
        return synth.camera(pos=(30.0 * np.sin(a), 5.0, 30.0 * np.cos(a)), quat=(0.0, float(np.sin(a / 2)), 0.0, float(np.cos(a / 2))))

    def eager_frame():
        now["eager"] += dt
        eager.set_camera(cam())
        eager.clap_frame(now["eager"], dt)

    replayed.capture(dt, warmup_now=dt)
    recaptured.capture(dt, warmup_now=dt)
    now["replayed"] = now["recaptured"] = dt

    def replay_frame():
        now["replayed"] += dt
        replayed.set_camera(cam())
        replayed.clap_frame_replay(now["replayed"])

    def recapture_frame():
        now["recaptured"] += dt
        recaptured.set_camera(cam())
        recaptured._build()                                  # the new descriptor, outside the capture
        recaptured._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(recaptured._graph):
            recaptured._issue(None, steps=1)
        recaptured.clap_frame_replay(now["recaptured"])
    return alternated(dict(eager_host_views=eager_frame, replay_views_dev=replay_frame, recapture_host_views=recapture_frame),
                      runs, wall_us)


README = """# Views in device memory: what they cost and buy

`python tools/frame_views_time.py` on one MI355X, ABI {abi}; us as [min, median, max] of {runs} runs after {warm} warm-up runs,
rows alternated in one process.  `isa_hashes.txt`: `tools/isa_hashes.sh` of entities.hip, visible.hip, lights.hip and
particles.hip at the parent commit and at this one, side by side -- every kernel the parent has keeps its hash.

## 1 M entities, every entity dirty (device events)

| step | us |
|---|---|
| update with the fused cull + visible list (the default) | {m[update_fused_cull_list]} |
| update without cull + `clapgpu_entities_cull_views` + visible list | {m[update_cull_views_list]} |
| update without cull, alone | {m[update_no_cull]} |
| `clapgpu_entities_cull_views`, alone | {m[cull_views_alone]} |

The separate pass costs {m[separate_pass_price_us]} us at the median ({m[visible]} entities visible).  The default stays the fused path.

## `clapgpu_views_calc` alone (device events)

| n_views | us |
|---|---|
| 1 | {v[views_calc_1]} |
| 5 | {v[views_calc_5]} |

## The 10 k-entity testbed frame, camera moving every frame (wall clock around a synchronise)

| how the frame follows the camera | us |
|---|---|
| issued eagerly, host views (`set_camera` rebuilds the descriptor) | {s[eager_host_views]} |
| graph replay, `views_dev=True` (`set_camera` + the source copy + one graph launch) | {s[replay_views_dev]} |
| graph re-captured every frame, host views (the only way without the view block) | {s[recapture_host_views]} |
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_views"))
    a = ap.parse_args()
    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    res = dict(abi=_lib.ABI_VERSION, runs=a.runs, warmup=WARM, unit="us [min, median, max]")
    res["million_entities"] = million(a.runs)
    res["views_calc"] = views_calc(a.runs)
    res["testbed_frame_moving_camera_wall"] = small_frame(a.runs)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "result.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(README.format(abi=res["abi"], runs=a.runs, warm=WARM, m=res["million_entities"], v=res["views_calc"],
                              s=res["testbed_frame_moving_camera_wall"]))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
