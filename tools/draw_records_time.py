"""What the draw records on the device cost and buy (include/clapgpu.h, "Draw records on the device").

(a) clapgpu_draw_records at bench.py's 1 M-entity population (125 000 chains of 8, tiled) under its camera, the living
    entities in 1 000 txmodels of a seeded render order, three ways: everything drawn (the plane all ones), the camera's
    cull, nothing drawn.  Launch to launch between HIP events, the drawn fraction with each row.  The yardstick is a
    device-to-device copy of the same byte count (read plus written) in the same process; the algorithmic bytes are
    128 + 192 + 40 per drawn entity plus 4 bytes and 1 bit per order entry.
(b) what it replaces at the same three rows: synchronise, download the plane, the LODs and the rows (mx, inv_mx), run
    clapgpu_draw_records_host, upload the records again.  Wall clock.
(c) the 10 k-entity testbed frame of tools/small_frame.py: eager with that host pass behind it, eager with
    clapgpu_frame.draw, replayed as a graph with clapgpu_frame.draw.  Wall clock around a synchronise.
(d) the same testbed frame without the new field (--default-only prints it alone: it runs on the parent commit too).

Per-kernel times are not split out here: the three launches are timed together.
Method: one process, warm-up, `--runs` timed calls per row with the rows ALTERNATED.  Writes
result.json into --out.
    python tools/draw_records_time.py [--runs 20] [--out profiles/draw_records] [--default-only] [--skip-million]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clap_amd import _lib, entities, frame, synth, tiler  # noqa: E402
import frame_views_time as fvt  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_US = 8e6                                          # 8 TB/s


def order_over(batch, n_groups, seed):
    from clap_amd import draw
    flags = batch.flags.cpu().numpy().view(np.uint32)
    alive = np.flatnonzero(flags & _lib.E_ALIVE).astype(np.uint32)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(alive)
    cuts = np.sort(rng.choice(len(perm), n_groups - 1, replace=False))
    return draw.DrawOrder.from_groups(np.split(perm, cuts), device=DEV)


def inputs_over(n, seed):
    from clap_amd import draw
    rng = np.random.default_rng(seed)
    return draw.DrawInputs(DEV, color=rng.random((n, 4), np.float32), color_pt=rng.integers(0, 2, n),
                           bloom_intensity=np.where(rng.random(n) < 0.5, 0.0, 0.7), bloom_threshold=np.zeros(n),
                           draw_flags=(rng.random(n) < 0.05).astype(np.uint32), character=np.full(n, -1))


def default_frame(runs):
    dt = 1.0 / 120.0
    loop = fvt.testbed(False)
    now = [0.0]

    def fn():
        now[0] += dt
        loop.clap_frame(now[0], dt)
    return fvt.alternated(dict(default_frame_a=fn, default_frame_b=fn), runs, fvt.wall_us)


def million(runs):
    from clap_amd import draw
    scene, _tl = tiler.tiled_scene(synth.entities_chains(125_000, 8, seed=2))
    batch = entities.EntityBatch(scene, DEV)
    fr = entities.view_calc_frustum(synth.camera())[0]
    batch.mq_update(fr, all_dirty=True)
    batch.alloc_lod()
    order = order_over(batch, 1000, 5)
    inputs = inputs_over(batch.n, 5)
    out = draw.DrawOutputs(order.n_order, order.n_groups, DEV)
    scratch = draw.scratch_for(order)
    p = draw.draw_pass(False, (0.5, 0.25), 3)
    planes = dict(all_drawn=torch.full_like(batch.vis_mask, -1), camera_cull=batch.vis_mask.clone(), none_drawn=torch.zeros_like(batch.vis_mask))
    res, rows_dev, rows_host = {}, {}, {}
    rec_h = torch.zeros((order.n_order, _lib.DRAW_RECORD_BYTES // 4), dtype=torch.int32).pin_memory()
    inp = {k: inputs[k].cpu().numpy() for k, _dt in draw.INPUT_KEYS}
    for name, plane in planes.items():
        draw.records(batch, order, out, p, inputs, plane=plane, lod=batch.cur_lod, scratch=scratch)
        _rec, count, _first, status = out.download()
        assert status == 0
        algo = count * (128 + 192 + 40) + order.n_order * 4 + order.n_order // 8
        res[name] = dict(drawn=count, drawn_fraction=round(count / order.n_order, 4), algorithmic_bytes=algo)
        rows_dev["records_" + name] = (lambda pl: lambda: draw.records(batch, order, out, p, inputs, plane=pl, lod=batch.cur_lod, scratch=scratch))(plane)
        a = torch.zeros(max(algo // 2, 16) // 4, dtype=torch.int32, device=DEV)
        b = torch.zeros_like(a)
        rows_dev["copy_" + name] = (lambda x, y: lambda: y.copy_(x))(a, b)

        def host_pass(pl=plane, k=min(count, order.n_order)):
            torch.cuda.synchronize()
            rec, _c, _f, _s = draw.records_host(batch.mx.cpu().numpy(), batch.inv_mx.cpu().numpy(), order, p, order.n_order,
                                                plane=pl.cpu().numpy().view(np.uint64), lod=batch.cur_lod.cpu().numpy(), inputs=inp)
            rec_h.numpy().reshape(-1).view(np.uint8)[:k * 192] = rec[:k].view(np.uint8).reshape(-1)
            out.records[:k].copy_(rec_h[:k], non_blocking=True)
        rows_host["host_pass_" + name] = host_pass
    dev_t = fvt.alternated(rows_dev, runs, fvt.event_us)
    host_t = fvt.alternated(rows_host, max(3, runs // 4), fvt.wall_us)
    for name in planes:
        r = res[name]
        r["records_us"], r["copy_same_bytes_us"], r["host_pass_wall_us"] = dev_t["records_" + name], dev_t["copy_" + name], host_t["host_pass_" + name]
        r["ratio_to_copy"] = round(r["records_us"][1] / r["copy_same_bytes_us"][1], 2)
        r["fraction_of_8TBs"] = round(r["algorithmic_bytes"] / r["records_us"][1] / HBM_BYTES_PER_US, 3)
    res["n_order"], res["n_groups"], res["n"] = order.n_order, order.n_groups, batch.n
    return res


def testbed(with_draw):
    from clap_amd import draw
    loop = fvt.testbed(True)
    batch = loop.batch
    order = order_over(batch, 50, 7)
    inputs = inputs_over(batch.n, 7)
    out = draw.DrawOutputs(order.n_order, order.n_groups, DEV)
    fd = draw.FrameDraw(order, inputs, main=(out, draw.draw_pass(False, (0.5, 0.25), 3)))
    if with_draw:
        loop.draw, loop._desc = fd, None
    return loop, fd


def small_frame(runs):
    from clap_amd import draw
    dt = 1.0 / 120.0
    (host, hfd), (eager, _e), (graph, _g) = testbed(False), testbed(True), testbed(True)
    now = dict(host=0.0, eager=0.0, graph=dt)
    hb = host.batch
    inp = {k: hfd.inputs[k].cpu().numpy() for k, _dt in draw.INPUT_KEYS}
    out, p = hfd.main
    rec_h = torch.zeros((out.capacity, _lib.DRAW_RECORD_BYTES // 4), dtype=torch.int32).pin_memory()

    def host_frame():
        now["host"] += dt
        host.clap_frame(now["host"], dt)
        torch.cuda.synchronize()
        rec, count, _f, _s = draw.records_host(hb.mx.cpu().numpy(), hb.inv_mx.cpu().numpy(), hfd.order, p, out.capacity,
                                               plane=hb.vis_mask.cpu().numpy().view(np.uint64), lod=hb.cur_lod.cpu().numpy(), inputs=inp)
        k = min(count, out.capacity)
        rec_h.numpy().reshape(-1).view(np.uint8)[:k * 192] = rec[:k].view(np.uint8).reshape(-1)
        out.records[:k].copy_(rec_h[:k], non_blocking=True)

    def eager_frame():
        now["eager"] += dt
        eager.clap_frame(now["eager"], dt)

    graph.capture(dt, warmup_now=dt)

    def replay_frame():
        now["graph"] += dt
        graph.clap_frame_replay(now["graph"])
    return fvt.alternated(dict(eager_host_pass=host_frame, eager_device_draw=eager_frame, replay_device_draw=replay_frame), runs, fvt.wall_us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draw_records"))
    ap.add_argument("--default-only", action="store_true", help="print the default frame's row alone (runs on the parent commit too)")
    ap.add_argument("--skip-million", action="store_true")
    a = ap.parse_args()
    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    if a.default_only:
        print(json.dumps(dict(abi=_lib.ABI_VERSION, runs=a.runs, default_frame_wall=default_frame(a.runs))), flush=True)
        return
    res = dict(abi=_lib.ABI_VERSION, runs=a.runs, warmup=fvt.WARM, unit="us [min, median, max]")
    if not a.skip_million:
        res["draw_records_1M_events"] = million(a.runs)
    res["testbed_frame_wall"] = small_frame(a.runs)
    res["default_frame_wall"] = default_frame(a.runs)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "result.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
