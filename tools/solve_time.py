"""Timing drivers for the contact solve (clapgpu_bodies_solve); profiles/solve/README.md holds what they measured.

    python tools/solve_time.py pass [--runs 5] [--k 10]
        the island page's workload -- 262 144 capsule-mix bodies (synth.capsule_bodies, box 60), the broadphase's real pair
        lists against each other and 64 static boxes, the narrowphase's records, the island pass -- and then the solve:
        launch to launch between HIP events, every call on the same restored state; the substep (collide, contacts,
        islands[, solve], step) with and without the solve: one JSON line.  Under rocprofv3 --kernel-trace --stats (a run
        of its own) the same run gives every kernel's time.
    python tools/solve_time.py pile [--bodies 4096 | --sizes 16,64,256,1024,4096]
        one island: a pile of spheres on a floor slab, each overlapping its neighbours -- the sequential tail of one lane,
        or the levels of a workgroup.  --sizes: one line per pile size.
Both modes: --wide-rows N sets clapgpu_solver.wide_rows (0: every island on one lane; 1: every island on a workgroup;
absent: clapgpu_solver_defaults'), --iterations N the sweeps (0: everything but the sweeps -- with --wide-rows 1 that is
the level pass and the buckets), --solve-only leaves the substep timings out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clap_amd import _lib, physics, synth  # noqa: E402
from islands_time import event_us  # noqa: E402

H = 1.0 / 120.0
STATE = ("pos", "quat", "lvel", "avel", "bflags", "adis_steps_left", "adis_time_left", "aabb", "axis", "geom_records")


def measure(w, res, runs, k, wide_rows=None, iterations=None, solve_only=False):
    def contacts():
        w.broadphase()
        w.contacts_geoms_both()
    contacts()
    w.islands(H)
    torch.cuda.synchronize()
    saved = {key: getattr(w, key).clone() for key in STATE}

    def restore():
        for key in STATE:
            getattr(w, key).copy_(saved[key])
    w.alloc_solve(res["rows_capacity"])
    if wide_rows is not None:
        w.solver.wide_rows = wide_rows
    if iterations is not None:
        w.solver.iterations = iterations
    total, status, _lam, key, level, wide = w.solve(H, want_lambda=True, want_levels=True)
    torch.cuda.synchronize()
    rows = int(total.item())
    res.update(wide_rows=int(w.solver.wide_rows), iterations=int(w.solver.iterations), wide_islands=int(wide.item()),
               levels_max=int(level[:max(rows, 1)].max().item()))
    isl = (key[:rows].cpu().numpy().view(np.uint64) >> np.uint64(32)).astype(np.int64)
    per = np.bincount(isl) if rows else np.zeros(1, np.int64)
    res.update(pairs=int(w.pair_total.item()), static_pairs=int(w.static_pair_total.item()),
               touching_pairs=int(w.contact2_total.item()), touching_static=int(w.static_contact2_total.item()),
               rows=rows, status=int(status.item()), islands_with_rows=int((per > 0).sum()), largest_island_rows=int(per.max()),
               scratch_MB=round(w.solve_scratch.numel() / 2 ** 20, 1))
    restore()
    res["restore_us"] = event_us(restore, k, runs)
    res["restore_solve_us"] = event_us(lambda: (restore(), w.solve(H)), k, runs)
    res["solve_alone_us"] = round(res["restore_solve_us"][1] - res["restore_us"][1], 2)
    if solve_only:
        print(json.dumps(res), flush=True)
        return

    def substep(solve):
        restore()
        w.bp_invalidate()
        contacts()
        w.islands(H)
        if solve:
            w.solve(H)
        w.world_step(H)
    res["restore_substep_us"] = event_us(lambda: substep(False), k, runs)
    res["restore_substep_solve_us"] = event_us(lambda: substep(True), k, runs)
    print(json.dumps(res), flush=True)


def run_pass(runs, k, **kw):
    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    n = 262_144
    b = synth.capsule_bodies(n, box=60.0, seed=4)
    w = physics.PhysWorld(b, synth.static_boxes(64, 60.0), device="cuda:0")
    measure(w, dict(bodies=n, rows_capacity=1 << 20, k=k, runs=runs, unit="us per call [min, median, max]"), runs, k, **kw)


def run_pile(n, runs, k, **kw):
    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    b = synth.sphere_bodies(n, box=64.0, seed=4)
    side = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    b["radius"][:] = 0.3
    b["pos"][:] = np.stack([2.0 + 0.5 * (i % side), np.full(n, 0.78), 2.0 + 0.5 * (i // side)], 1)   # 0.5 apart: neighbours overlap
    b["lvel"][:] *= 0.01
    b["cell"] = 1.0
    w = physics.PhysWorld(b, np.array([[-1e3, 1e3, -10.0, 0.5, -1e3, 1e3]]), device="cuda:0")
    measure(w, dict(bodies=n, pile=True, rows_capacity=8 * n, k=k, runs=runs, unit="us per call [min, median, max]"), runs, k,
            **kw)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("pass", "pile"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--bodies", type=int, default=4096)
    ap.add_argument("--sizes", type=lambda t: [int(x) for x in t.split(",")], default=None)
    ap.add_argument("--wide-rows", type=int, default=None)
    ap.add_argument("--iterations", type=int, default=None)
    ap.add_argument("--solve-only", action="store_true")
    a = ap.parse_args()
    kw = dict(wide_rows=a.wide_rows, iterations=a.iterations, solve_only=a.solve_only)
    if a.mode == "pass":
        run_pass(a.runs, a.k, **kw)
    else:
        for n in a.sizes or [a.bodies]:
            run_pile(n, a.runs, a.k, **kw)
