"""What the spotlights on the device cost and buy (include/clapgpu.h, "Spotlights on the device").

(a) clapgpu_lights_update alone at 1, 16 and 128 carriers, launch to launch between HIP events, next to
    clapgpu_lights_from_entities at 16 carriers.
(b) the 10 k-entity testbed frame of tools/small_frame.py with light 0 a spotlight on a falling body's entity, its view in
    slot 1: issued eagerly with the host's light_update behind the frame (synchronise, download the carrier,
    clapgpu_lights_update_host, upload the slots and the pose, then this frame's views, cull and shadow list); issued
    eagerly with clapgpu_frame.spots; and replayed as a graph with clapgpu_frame.spots.  Wall clock around a synchronise.
(c) the same testbed frame without any of the new fields, for the comparison with the parent commit: run this row from a
    checkout of the parent in the same visit (--default-only prints it alone; it needs nothing this commit adds).

Method: one process, warm-up, `--runs` timed calls per row with the rows ALTERNATED.  Writes
result.json and README.md into --out.
    python tools/spots_time.py [--runs 20] [--out profiles/spots] [--default-only] [--parent-json FILE ...]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clap_amd import _lib, entities, frame, lights as lm  # noqa: E402
import frame_views_time as fvt  # noqa: E402

DEV = "cuda:0"
CUTOFF = 0.6


def default_frame(runs):
    """the testbed frame as tools/frame_views_time.py builds it, host views: nothing of this commit is asked for"""
    dt = 1.0 / 120.0
    loop = fvt.testbed(False)
    now = [0.0]

    def fn():
        now[0] += dt
        loop.clap_frame(now[0], dt)
    return fvt.alternated(dict(default_frame_a=fn, default_frame_b=fn), runs, fvt.wall_us)


def alone(runs):
    from clap_amd import cascades as cm
    from clap_amd.views import ViewBlock
    n = 300
    rng = np.random.default_rng(5)
    q = rng.normal(size=(n, 4)).astype(np.float32)
    scene = dict(n=n, pos_scale=np.concatenate([rng.uniform(-40, 40, (n, 3)), np.ones((n, 1))], 1).astype(np.float32), rot=q,
                 parent=np.full(n, -1, np.int32), model=np.zeros(n, np.int32),
                 flags=np.full(n, _lib.E_ALIVE | _lib.E_VISIBLE | _lib.E_DIRTY, np.uint32), seqs=np.zeros(n, np.uint32),
                 level_start=np.asarray([0, n], np.uint32), model_aabb=np.float32([[-1, -1, -1, 1, 1, 1]]), model_skip=np.zeros(1, np.uint8))
    batch = entities.EntityBatch(scene, DEV)
    views = ViewBlock(DEV)
    for s in range(1, _lib.VIEW_SLOTS):
        views.set_pose(s, (0, 0, 0), (0, 0, 0, 1), lm.spot_persp(CUTOFF))
    views.upload()
    rows = {}
    for count in (1, 16, 128):
        ls = lm.LightSet(DEV)
        for _ in range(count):
            ls.light_set_cutoff(ls.light_get(), CUTOFF)
        ls.set_spots(np.arange(count) * 2, np.arange(count), np.zeros((count, 3), np.float32), 1 + np.arange(count) % 4)
        rows["lights_update_%d" % count] = (lambda l: lambda: l.update_from_entities(batch, views))(ls)
    ls = lm.LightSet(DEV)
    for _ in range(16):
        ls.light_get()
    ls.set_carriers(np.arange(16, dtype=np.uint32) * 2, np.arange(16, dtype=np.int32), np.zeros((16, 3), np.float32))
    rows["lights_from_entities_16"] = lambda: ls.from_entities(batch)
    assert cm.VIEWS_SOURCE.itemsize == _lib.VIEWS_SOURCE_BYTES
    return fvt.alternated(rows, runs, fvt.event_us)


def testbed(spots):
    """tools/small_frame.py's frame with a spotlight (slot 16 of the light set) riding body 0's entity, its view in slot 1"""
    base = fvt.testbed(True)
    w, batch, ls = base.world, base.batch, base.lights
    batch.set_views(None, matrices=[(np.eye(4, dtype=np.float32).ravel(), lm.spot_persp(CUTOFF), False)])
    idx = ls.light_get()
    ls.light_set_cutoff(idx, CUTOFF)
    carrier = int(w.body_entity[0].item())
    ls.set_spots([carrier], [idx], [[0.0, 0.5, 0.0]], [1])
    loop = frame.FrameLoop(batch, base.cam, world=w, feed=base.feed, lights=ls, characters=base.characters,
                           particles=base.particles, contacts=True, views_dev=True, view_lists=spots)
    if not spots:
        f = loop._build()
        f.spots = None
    return loop, carrier


def small_frame(runs):
    from clap_amd import cascades as cm
    dt = 1.0 / 120.0
    (host, carrier), (eager, _c1), (graph, _c2) = testbed(False), testbed(True), testbed(True)
    now = dict(host=0.0, eager=0.0, graph=dt)
    hb, hl = host.batch, host.lights
    row_h = torch.zeros(8, dtype=torch.float32).pin_memory()
    src_h = torch.zeros(_lib.VIEWS_SOURCE_BYTES // 4, dtype=torch.int32).pin_memory()
    out_h = torch.zeros(6, dtype=torch.float32).pin_memory()
    idx = int(hl._spots[2].cpu().numpy()[0])
    lights = dict(nr_lights=hl.nr_lights, pos=hl.pos, is_dir=hl.is_dir, active=hl.active)
    carriers = ([0], [idx], [[0.0, 0.5, 0.0]], [1])
    flags = np.asarray([_lib.E_DIRTY], np.uint32)
    words = _lib.VIEWS_SOURCE_BYTES // _lib.VIEW_SLOTS // 4

    def host_frame():
        now["host"] += dt
        host.clap_frame(now["host"], dt)
        row_h[:4].copy_(hb.pos_scale[carrier], non_blocking=True)
        row_h[4:].copy_(hb.rot[carrier], non_blocking=True)
        src_h.copy_(host.views.source, non_blocking=True)
        torch.cuda.synchronize()
        r = row_h.numpy()
        pos, d, _st, src = lm.update_host(r[None, :4], r[None, 4:], flags, carriers, lights, hl.dir, hl.cutoff,
                                          src_h.numpy().view(cm.VIEWS_SOURCE)[0])
        out_h.numpy()[:3], out_h.numpy()[3:] = pos[idx], d[idx]
        hl._d["pos"][idx].copy_(out_h[:3], non_blocking=True)
        hl._d["dir"][idx].copy_(out_h[3:], non_blocking=True)
        src_h.numpy()[:] = np.ascontiguousarray(src).reshape(1).view(np.int32)
        host.views.source[words:2 * words].copy_(src_h[words:2 * words], non_blocking=True)
        host.views.calc(2)
        hb.cull_views(host.views)
        hb.compact_view(0)

    def eager_frame():
        now["eager"] += dt
        eager.clap_frame(now["eager"], dt)

    graph.capture(dt, warmup_now=dt)

    def replay_frame():
        now["graph"] += dt
        graph.clap_frame_replay(now["graph"])
    return fvt.alternated(dict(eager_host_light_update=host_frame, eager_device_spots=eager_frame, replay_device_spots=replay_frame),
                          runs, fvt.wall_us)


README = """# Spotlights on the device: what they cost and buy

`python tools/spots_time.py` on one MI355X, ABI {abi}; us as [min, median, max] of {runs} runs after {warm} warm-up runs,
rows alternated in one process.  `isa_hashes.txt`: `tools/isa_hashes.sh` of every .hip file at the parent commit and at
this one, side by side -- every kernel the parent has keeps its hash; `k_lights_update` is new.  `kernel_resources.txt`:
`-Rpass-analysis=kernel-resource-usage` of lights.hip (`k_lights_update`: 21 VGPRs, 60 SGPRs, no private segment, 536
bytes of LDS).

`k_lights_update` is launch-bound by construction: one workgroup of 128 lanes that reads at most a few KB and writes at most
3 KB.  A roofline says nothing about it; what is reported is the launch-to-launch time next to the kernel it is modelled on.

## `clapgpu_lights_update` alone (device events, launch to launch)

| call | us |
|---|---|
| `clapgpu_lights_update`, 1 carrier (a spotlight with a view) | {a[lights_update_1]} |
| `clapgpu_lights_update`, 16 carriers | {a[lights_update_16]} |
| `clapgpu_lights_update`, 128 carriers | {a[lights_update_128]} |
| `clapgpu_lights_from_entities`, 16 carriers | {a[lights_from_entities_16]} |

## The 10 k-entity testbed frame, a spotlight on a falling body (wall clock around a synchronise)

| how the frame gets its spot | us |
|---|---|
| issued eagerly; the host runs light_update behind the frame (synchronise, download the carrier, `clapgpu_lights_update_host`, upload, then views, cull and the shadow list) | {s[eager_host_light_update]} |
| issued eagerly; `clapgpu_frame.spots` and `view_visible` (nothing read back) | {s[eager_device_spots]} |
| graph replay; `clapgpu_frame.spots` and `view_visible` | {s[replay_device_spots]} |

## The default frame against the parent commit (wall clock around a synchronise)

The testbed frame with none of the new fields, the row measured twice in one process (a, b), on this tree and on a
checkout of the parent commit in the same visit to the same machine.

| tree | a, us | b, us |
|---|---|---|
{default_rows}

{default_note}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spots"))
    ap.add_argument("--default-only", action="store_true", help="print the default frame's row alone (runs on the parent commit too)")
    ap.add_argument("--parent-json", nargs="*", default=[], help="outputs of --default-only from a checkout of the parent")
    ap.add_argument("--here-json", nargs="*", default=[], help="further outputs of --default-only from this tree")
    a = ap.parse_args()
    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    if a.default_only:
        print(json.dumps(dict(abi=_lib.ABI_VERSION, runs=a.runs, default_frame_wall=default_frame(a.runs))), flush=True)
        return
    res = dict(abi=_lib.ABI_VERSION, runs=a.runs, warmup=fvt.WARM, unit="us [min, median, max]")
    res["lights_update_alone_events"] = alone(a.runs)
    res["testbed_frame_spot_on_a_body_wall"] = small_frame(a.runs)
    here = [default_frame(a.runs)] + [json.load(open(p))["default_frame_wall"] for p in a.here_json]
    parent = [json.load(open(p))["default_frame_wall"] for p in a.parent_json]
    res["default_frame_wall"] = dict(this_tree=here, parent_commit=parent)
    rows = ["| this tree, process %d | %s | %s |" % (i + 1, r["default_frame_a"], r["default_frame_b"]) for i, r in enumerate(here)]
    rows += ["| parent commit, process %d | %s | %s |" % (i + 1, r["default_frame_a"], r["default_frame_b"]) for i, r in enumerate(parent)]
    if parent:
        pm = [r[k][1] for r in parent for k in ("default_frame_a", "default_frame_b")]
        hm = [r[k][1] for r in here for k in ("default_frame_a", "default_frame_b")]
        note = ("The parent's medians span %.1f to %.1f us in this visit (its own run-to-run spread: %.1f us); this tree's span %.1f to "
                "%.1f us." % (min(pm), max(pm), max(pm) - min(pm), min(hm), max(hm)))
    else:
        note = "The parent commit was not measured in this run."
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "result.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(README.format(abi=res["abi"], runs=a.runs, warm=fvt.WARM, a=res["lights_update_alone_events"],
                              s=res["testbed_frame_spot_on_a_body_wall"], default_rows="\n".join(rows), default_note=note))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
