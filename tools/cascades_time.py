"""What the shadow cascades on the device cost and buy (include/clapgpu.h, "The shadow cascades on the device").

(a) clapgpu_cascades_calc alone, launch to launch between HIP events, next to clapgpu_views_calc over five slots.
(b) clapgpu_entities_bv_views at 1 M entities (tools/frame_views_time.py's scene) against the update with and without
    its fused pick: the update alone, the update with clapgpu_entities.bv, the separate pick alone, and the update
    followed by the separate pick.
(c) the 10 k-entity testbed frame of tools/small_frame.py with a camera that follows a falling body's entity
    (clapgpu_frame.camera) and one further view, the shadow light's: issued eagerly with the host fitting the light view
    behind the frame (synchronise, download the camera, clapgpu_cascades_calc_host, upload the light's slot: the next
    frame's light); issued eagerly with clapgpu_frame.cascades; and replayed as a graph with clapgpu_frame.cascades.
    Wall clock around a synchronise.

Method: one process, warm-up, `--runs` timed calls per row with the rows ALTERNATED.  Writes
result.json and README.md into --out.
    python tools/cascades_time.py [--runs 20] [--out profiles/cascades]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clap_amd import _lib, camera as cam_mod, cascades as cm, entities, frame, synth, tiler  # noqa: E402
from clap_amd.views import ViewBlock  # noqa: E402
import frame_views_time as fvt  # noqa: E402

DEV = "cuda:0"
LIGHT_DIR = (0.35, -1.0, 0.25)


def light_proj():
    m = np.zeros((4, 4), np.float32)
    m[0, 0], m[1, 1], m[2, 2], m[3, 2], m[3, 3] = 2 / 300.0, 2 / 300.0, -2 / 1999.9, -2000.1 / 1999.9, 1
    return m.ravel()


def block_for(cam, **kw):
    fov, aspect, near, far = (float(v) for v in cam["persp"])
    blk = cm.CascadesBlock(DEV)
    blk.set(LIGHT_DIR, cm.persp(fov, aspect, near, far, 0), light_slot=1, near_backup=5.0, **kw)
    blk.upload()
    return blk


def alone(runs):
    cam = synth.camera(pos=(3, 20, 60))
    views = ViewBlock(DEV)
    for s in range(_lib.VIEW_SLOTS):
        views.set_camera(s, cam)
    views.set_matrices(1, np.eye(4, dtype=np.float32), light_proj())
    views.upload()
    blk = block_for(cam)
    ent = type("E", (), {"_desc": _lib.Entities()})()
    return fvt.alternated({"cascades_calc": lambda: blk.calc(ent, views), "views_calc_5": lambda: views.calc(5)}, runs, fvt.event_us)


def million(runs):
    scene, _tl = tiler.tiled_scene(synth.entities_chains(125_000, 8, seed=2))
    batch = entities.EntityBatch(scene, DEV)
    cam = synth.camera()
    views = ViewBlock(DEV)
    views.set_camera(0, cam)
    views.upload()
    views.calc(1)
    res = torch.zeros(1, dtype=torch.int64, device=DEV)
    ctl = 12345
    batch.mq_update(None, all_dirty=True)
    torch.cuda.synchronize()
    ctl_pos = batch.pos_scale.view(-1, 4)[ctl, :3].cpu().numpy()
    batch.set_bv_query(cam["cam_pos"], ctl_pos, ctl)
    query = batch._desc.bv

    def update(fused):
        def fn():
            batch._desc.bv = query if fused else None
            batch.mq_update(None, all_dirty=True)
        return fn

    def pick():
        batch.bv_views(views, ctl_entity=ctl, result=res)

    def both():
        update(False)()
        pick()
    update(True)()
    pick()
    torch.cuda.synchronize()
    assert int(res.item()) == int(batch.bv_result.item()), "the separate pick and the fused pick disagree"
    t = fvt.alternated(dict(update_no_pick=update(False), update_fused_pick=update(True), bv_views_alone=pick,
                            update_then_bv_views=both), runs, fvt.event_us)
    t["fused_pick_price_us"] = round(t["update_fused_pick"][1] - t["update_no_pick"][1], 1)
    t["separate_pick_price_us"] = round(t["update_then_bv_views"][1] - t["update_no_pick"][1], 1)
    t["entities"] = batch.n
    return t


def testbed(cascades):
    """tools/camera_time.py's testbed frame (the camera follows body 0's entity) with the shadow light's view in slot 1"""
    base = fvt.testbed(True)
    w, batch = base.world, base.batch
    batch.set_views(None, matrices=[(np.eye(4, dtype=np.float32).ravel(), light_proj(), False)])
    ctl = int(w.body_entity[0].item())
    cam = base.cam
    _fov, aspect, near, far = (float(v) for v in cam["persp"])
    block = cam_mod.CameraBlock(DEV)
    block.set(cam["cam_quat"], near, far, aspect, ctl, ctl_skip=0)
    block.upload()
    blk = block_for(cam)
    loop = frame.FrameLoop(batch, cam, world=w, feed=base.feed, lights=base.lights, characters=base.characters,
                           particles=base.particles, contacts=True, views_dev=True, camera=block,
                           cascades=blk if cascades else None)
    return loop, blk


def small_frame(runs):
    dt = 1.0 / 120.0
    (host, hblk), (eager, _b1), (graph, _b2) = testbed(False), testbed(True), testbed(True)
    now = dict(host=0.0, eager=0.0, graph=dt)
    src_h = torch.zeros(_lib.VIEWS_SOURCE_BYTES // 4, dtype=torch.int32).pin_memory()
    mx_h = torch.zeros(16, dtype=torch.int32).pin_memory()
    at = _lib.VIEWS_SOURCE_BYTES // _lib.VIEW_SLOTS // 4

    def host_frame():
        now["host"] += dt
        host.clap_frame(now["host"], dt)
        src_h.copy_(host.views.source, non_blocking=True)
        torch.cuda.synchronize()
        _c, s = cm.calc_host(hblk.host[0], src_h.numpy().view(cm.VIEWS_SOURCE)[0])
        mx_h.numpy()[:] = s["slot"][1]["view_mx"].view(np.int32)
        host.views.source[at:at + 16].copy_(mx_h, non_blocking=True)      # the NEXT frame's light view

    def eager_frame():
        now["eager"] += dt
        eager.clap_frame(now["eager"], dt)

    graph.capture(dt, warmup_now=dt)

    def replay_frame():
        now["graph"] += dt
        graph.clap_frame_replay(now["graph"])
    return fvt.alternated(dict(eager_host_light_view=host_frame, eager_device_cascades=eager_frame, replay_device_cascades=replay_frame),
                          runs, fvt.wall_us)


README = """# The shadow cascades on the device: what they cost and buy

`python tools/cascades_time.py` on one MI355X, ABI {abi}; us as [min, median, max] of {runs} runs after {warm} warm-up
runs, rows alternated in one process.  `isa_hashes.txt`: `tools/isa_hashes.sh` of visible.hip, views.hip, camera.hip,
entities_edit.hip, entities.hip and entities_host.hip at the parent commit and at this one, side by side -- every kernel
the parent has keeps its hash; cascades.hip is new.

## `clapgpu_cascades_calc` alone (device events, launch to launch)

| call | us |
|---|---|
| `clapgpu_cascades_calc`, four cascades and the main view | {a[cascades_calc]} |
| `clapgpu_views_calc`, five slots | {a[views_calc_5]} |

## The bounding-volume pick at {m[entities]} entities (device events)

| what | us |
|---|---|
| the update, no pick | {m[update_no_pick]} |
| the update with its fused pick (`clapgpu_entities.bv`) | {m[update_fused_pick]} |
| `clapgpu_entities_bv_views` alone | {m[bv_views_alone]} |
| the update, then `clapgpu_entities_bv_views` | {m[update_then_bv_views]} |

Median against median, the update with its fused pick differs from the update without by {m[fused_pick_price_us]} us and
the update followed by the separate pass by {m[separate_pick_price_us]} us: the separate pass reads the boxes and flags
again (28 MB at 1 M entities).  Where the host has the two positions the fused pick is the cheaper one at this size; the
separate pass is what a frame pays for positions that exist only in device memory.  Smaller sizes were not measured.

## The 10 k-entity testbed frame, the camera following a falling body (wall clock around a synchronise)

| how the frame gets its light view | us |
|---|---|
| issued eagerly; the host fits it behind the frame (synchronise, download the camera, `clapgpu_cascades_calc_host`, upload: the next frame's light) | {s[eager_host_light_view]} |
| issued eagerly; `clapgpu_frame.cascades` (this frame's light, nothing read back) | {s[eager_device_cascades]} |
| graph replay; `clapgpu_frame.cascades` | {s[replay_device_cascades]} |
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cascades"))
    a = ap.parse_args()
    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    res = dict(abi=_lib.ABI_VERSION, runs=a.runs, warmup=fvt.WARM, unit="us [min, median, max]")
    res["cascades_calc_alone_events"] = alone(a.runs)
    res["bv_pick_1m_events"] = million(a.runs)
    res["testbed_frame_following_camera_wall"] = small_frame(a.runs)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "result.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(README.format(abi=res["abi"], runs=a.runs, warm=fvt.WARM, a=res["cascades_calc_alone_events"],
                              m=res["bv_pick_1m_events"], s=res["testbed_frame_following_camera_wall"]))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
