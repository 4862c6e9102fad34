"""What the camera controller on the device costs and buys (include/clapgpu.h, "The camera controller on the device").

(a) clapgpu_camera_calc alone at the full physics scene of tools/ray_time.py (262 144 capsule-mix bodies, 5 000 statics):
    launch to launch between HIP events and on the host clock around a synchronise, through an index of the broadphase
    grid and by scan, for controls found by search whose loop runs 1, 2 and 4 iterations -- against the host loop it
    replaces on the same control: clapgpu_camera_target, then per iteration an upload of four rays, clapgpu_ray_cast, a
    synchronise, a download and clapgpu_camera_decide (clapgpu_camera_update_host), then the upload of the view source.
    The host loop runs here through ctypes with a Python callback per iteration, a few microseconds each; a C host
    would pay the launches, synchronisations and copies alone.
(b) the 10 k-entity testbed frame of tools/small_frame.py with a camera that follows a falling body's entity: issued
    eagerly with the host's camera behind the frame (synchronise, download the control, the host loop, upload the source
    for the next frame); issued eagerly with clapgpu_frame.camera; and replayed as a graph with clapgpu_frame.camera.
    Wall clock around a synchronise.

Method: one process, warm-up, `--runs` timed calls per row with the rows ALTERNATED.  Writes
result.json and README.md into --out.
    python tools/camera_time.py [--runs 20] [--out profiles/camera]"""
import argparse
import ctypes as C
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clap_amd import _lib, camera as cam_mod, frame  # noqa: E402
from clap_amd.views import ViewBlock  # noqa: E402
import frame_views_time as fvt  # noqa: E402
import ray_time  # noqa: E402

DEV = "cuda:0"


class OneEntity:
    """a clapgpu_entities of one control entity, as far as clapgpu_camera_calc reads it"""

    def __init__(self, pos, box=((-0.5, 0.0, -0.5), (0.5, 2.0, 0.5))):
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(DEV)
        self.pos_scale = np.asarray([[pos[0], pos[1], pos[2], 1.0]], np.float32)
        self.table = np.asarray([[*box[0], 0.0], [*box[1], 0.0]], np.float32)
        self.center = self.pos_scale[:, :3] + np.float32([0.0, 1.0, 0.0])
        self.keep = [dev(self.pos_scale, np.float32), dev([0], np.int32), dev(self.table, np.float32), dev(self.center, np.float32)]
        d = _lib.Entities()
        d.n, d.n_models = 1, 1
        d.pos_scale, d.model, d.model_table, d.center = [t.data_ptr() for t in self.keep]
        self._desc = d


class HostLoop:
    """the loop a host runs today, on buffers made once"""

    def __init__(self, w, grid, skip):
        self.w, self.grid = w, grid
        self.ray_h = torch.zeros((4, 8), dtype=torch.float64).pin_memory()
        self.ray_d = torch.zeros((4, 8), dtype=torch.float64, device=DEV)
        self.skip_d = torch.full((4,), int(skip), dtype=torch.int32, device=DEV)
        self.dist_d, self.hit_d = torch.zeros(4, dtype=torch.float64, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
        self.flags_d = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.out_h = torch.zeros(8, dtype=torch.float64).pin_memory()          # dist[4] | hit[4], flags[4] as int32 pairs
        self.out_d = torch.zeros(8, dtype=torch.float64, device=DEV)
        self.g, self.sg = w.body_geoms(), w.static_geoms()

    def cast(self, ray):
        self.ray_h.numpy()[:] = ray
        self.ray_d.copy_(self.ray_h, non_blocking=True)
        _lib.check(_lib.lib().clapgpu_ray_cast(cam_mod._stream(), self.w._bp if self.grid else None, C.byref(self.g), C.byref(self.sg),
                                               None, 4, self.ray_d.data_ptr(), self.skip_d.data_ptr(), self.dist_d.data_ptr(),
                                               self.hit_d.data_ptr(), None, self.flags_d.data_ptr()), "clapgpu_ray_cast")
        self.out_d[:4].copy_(self.dist_d)
        self.out_d[4:].view(torch.int32)[:4].copy_(self.hit_d)
        self.out_d[4:].view(torch.int32)[4:].copy_(self.flags_d)
        self.out_h.copy_(self.out_d, non_blocking=True)
        torch.cuda.synchronize()
        o = self.out_h.numpy()
        hit, flags = o[4:].view(np.int32)[:4], o[4:].view(np.int32)[4:]
        return hit != -1, np.where(hit != -1, o[:4], 0.0), flags.view(np.uint32)

    def run(self, rec, ent, views):
        r = rec.copy()
        r["target"], r["dist"] = cam_mod.target(int(r["flags"]), ent.pos_scale[0], ent.table[0, :3], ent.table[1, :3], ent.center[0],
                                                None, float(r["far_plane"]))
        out = cam_mod.update_host(r, self.cast)
        views._src.slot[0].pos[:] = [float(v) for v in out["pos"]]
        views.upload()
        return out


def alone(runs):
    w, b = ray_time.scene()
    w.bp_index()
    rng = np.random.Generator(np.random.PCG64(50))
    views = ViewBlock(DEV)
    views.set_pose(0, (0, 0, 0), (0, 0, 0, 1), np.eye(4, dtype=np.float32))
    views.upload()
    block = cam_mod.CameraBlock(DEV)
    found = {}
    for _ in range(400):                                     # controls whose loop runs 1, 2 and 4 iterations
        if len(found) == 3:
            break
        body = int(rng.integers(0, w.n))
        yaw, pitch, far = float(rng.uniform(-180, 180)), float(rng.uniform(-60, 10)), float(rng.choice([500.0, 12.0, 11.0]))
        y, p = np.radians(yaw) / 2, np.radians(pitch) / 2
        quat = np.float32([np.cos(y) * np.sin(p), np.sin(y) * np.cos(p), -np.sin(y) * np.sin(p), np.cos(y) * np.cos(p)])
        ent = OneEntity(b["pos"][body] - [0.0, b["yoffset"][body], 0.0])
        block.set(quat, 0.1, far, 16.0 / 9.0, 0, ctl_skip=body, character=True)
        block.upload()
        block.calc(ent, w, views, grid=True, meshes=False)
        it = int(block.download()["iterations"])
        if it in (1, 2, 4) and it not in found:
            found[it] = (ent, block.host[0].copy(), body)
    res = {}
    for it, (ent, rec, body) in sorted(found.items()):
        def dev(grid):
            def fn():
                block.calc(ent, w, views, grid=grid, meshes=False)
            return fn
        block.host[0] = rec
        block.upload()
        loops = {g: HostLoop(w, g, body) for g in (True, False)}
        want = loops[True].run(rec, ent, views)
        block.calc(ent, w, views, grid=True, meshes=False)
        got = block.download()
        assert all(np.array_equal(np.atleast_1d(got[k]).view(np.uint8), np.atleast_1d(want[k]).view(np.uint8))
                   for k in ("pos", "dist", "target", "iterations", "status")), "the device and the host loop disagree"
        ev = fvt.alternated({"camera_calc_index": dev(True), "camera_calc_scan": dev(False)}, runs, fvt.event_us)
        wall = fvt.alternated({"camera_calc_index": dev(True), "camera_calc_scan": dev(False),
                               "host_loop_index": lambda: loops[True].run(rec, ent, views),
                               "host_loop_scan": lambda: loops[False].run(rec, ent, views)}, runs, fvt.wall_us)
        res[f"iterations_{it}"] = dict(events=ev, wall=wall, dist=float(got["dist"]))
    res["searched_for"] = [1, 2, 4]
    return res


def testbed(camera, index=False):
    """tools/frame_views_time.py's testbed frame; the camera follows body 0's entity"""
    loop = fvt.testbed(True)
    w, batch = loop.world, loop.batch
    ctl = int(w.body_entity[0].item())
    block = None
    if camera:
        block = cam_mod.CameraBlock(DEV)
        loop = frame.FrameLoop(batch, loop.cam, world=w, feed=loop.feed, lights=loop.lights, characters=loop.characters,
                               particles=loop.particles, contacts=True, views_dev=True, camera=block, camera_index=index)
    cam = loop.cam
    _fov, aspect, near, far = (float(v) for v in cam["persp"])
    rec = np.zeros(1, cam_mod.CAMERA)[0]
    rec["quat"], rec["near_plane"], rec["far_plane"], rec["aspect"] = cam["cam_quat"], near, far, aspect
    rec["moved"], rec["ctl_entity"], rec["ctl_skip"], rec["flags"] = 1, ctl, 0, 0
    if camera:
        block.host[0] = rec
        block.upload()
    return loop, rec, ctl


def small_frame(runs):
    dt = 1.0 / 120.0
    (host, rec, ctl), (eager, _r1, _c1), (graph, _r2, _c2) = testbed(False), testbed(True), testbed(True)
    hl = HostLoop(host.world, False, 0)
    table = host.batch.model_table.cpu().numpy().reshape(-1, 2, 4)
    model = int(host.batch.model[ctl].item())
    now = dict(host=0.0, eager=0.0, graph=dt)
    ctl_h = torch.zeros(7, dtype=torch.float32).pin_memory()

    ent = types.SimpleNamespace(table=table[model])          # the control entity's values, downloaded every frame

    def host_frame():
        now["host"] += dt
        host.clap_frame(now["host"], dt)
        ctl_h[:4].copy_(host.batch.pos_scale.view(-1, 4)[ctl], non_blocking=True)
        ctl_h[4:].copy_(host.batch.center[ctl], non_blocking=True)
        torch.cuda.synchronize()
        c = ctl_h.numpy()
        ent.pos_scale, ent.center = c[None, :4].copy(), c[None, 4:].copy()
        hl.run(rec, ent, host.views)                          # uploads the source: the NEXT frame's camera

    def eager_frame():
        now["eager"] += dt
        eager.clap_frame(now["eager"], dt)

    graph.capture(dt, warmup_now=dt)

    def replay_frame():
        now["graph"] += dt
        graph.clap_frame_replay(now["graph"])
    return fvt.alternated(dict(eager_host_camera=host_frame, eager_device_camera=eager_frame, replay_device_camera=replay_frame),
                          runs, fvt.wall_us)


README = """# The camera controller on the device: what it costs and buys

`python tools/camera_time.py` on one MI355X, ABI {abi}; us as [min, median, max] of {runs} runs after {warm} warm-up runs,
rows alternated in one process.  `isa_hashes.txt`: `tools/isa_hashes.sh` of rays.hip, ray_trimesh.hip and visible.hip at
the parent commit and at this one, side by side -- every kernel the parent has keeps its hash; camera.hip is new.

## `clapgpu_camera_calc` alone: 262 144 bodies + 5 000 statics

The host loop is what the call replaces: `clapgpu_camera_target`, then per iteration an upload of four rays,
`clapgpu_ray_cast`, a synchronise, a download and the decision, then the upload of the view source -- here through
ctypes, with a Python callback per iteration.

| loop iterations | how | device events | wall clock around a synchronise |
|---|---|---|---|
{rows}

## The 10 k-entity testbed frame, the camera following a falling body (wall clock around a synchronise)

| how the frame gets its camera | us |
|---|---|
| issued eagerly; host camera behind the frame (synchronise, download, host loop, upload: the next frame's camera) | {s[eager_host_camera]} |
| issued eagerly; `clapgpu_frame.camera` (this frame's camera, nothing read back) | {s[eager_device_camera]} |
| graph replay; `clapgpu_frame.camera` | {s[replay_device_camera]} |
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera"))
    a = ap.parse_args()
    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    res = dict(abi=_lib.ABI_VERSION, runs=a.runs, warmup=fvt.WARM, unit="us [min, median, max]")
    res["camera_calc_alone"] = alone(a.runs)
    res["testbed_frame_following_camera_wall"] = small_frame(a.runs)
    rows = []
    for it in (1, 2, 4):
        r = res["camera_calc_alone"].get(f"iterations_{it}")
        if r is None:
            rows.append(f"| {it} | no such control found by the search | not measured | not measured |")
            continue
        for how, key in (("`clapgpu_camera_calc`, index", "camera_calc_index"), ("`clapgpu_camera_calc`, scan", "camera_calc_scan"),
                         ("host loop, index", "host_loop_index"), ("host loop, scan", "host_loop_scan")):
            rows.append(f"| {it} | {how} | {r['events'].get(key, 'n/a')} | {r['wall'][key]} |")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "result.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(README.format(abi=res["abi"], runs=a.runs, warm=fvt.WARM, rows="\n".join(rows), s=res["testbed_frame_following_camera_wall"]))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
