"""Times clapgpu_characters_move_ordered beside clapgpu_characters_move at workload B of profiles/slide/
(tools/mesh_contact_time.py's scene: 262 144 bodies on a terrain, 5 000 statics, the mesh set; tools/move_time.py's 65 536
movers), and says what the order is worth there: the levels, the conflict pairs, the movers the plain batch flags
MOVED_TARGET and the share of movers whose position the plain batch leaves elsewhere than the ordered call.

Method: warm; the two calls alternate, `--runs` times each, on one process and one box.  Every timed
pass starts from the restored bodies.  The ordered call synchronises the stream, so both are timed on the wall clock
between two device synchronisations, the restore outside the clock.  One JSON line.
    python tools/ordered_move_time.py [--movers 65536] [--runs 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from clap_amd import _lib, physics  # noqa: E402
from mesh_contact_time import scene  # noqa: E402
from move_time import KEYS, median, movers_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--movers", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    w, b, _terrain = scene("B")
    w.enable_forces()
    w.bodies_aabb()
    dt = 1.0 / 60.0
    mv = movers_of(w, b, a.movers, 10)
    IN = ("motion", "state", "jump", "jump_params", "velocity", "normal", "airborne")
    m = physics.CharacterMoves(w, mv["body"], mv["ray_off"], **{k: mv[k] for k in IN})
    snap = {k: getattr(w, k).clone() for k in KEYS}
    state0 = {k: getattr(m, k).clone() for k in ("velocity", "normal", "airborne")}
    body = torch.from_numpy(mv["body"].astype(np.int64)).to(w.device)

    def restore():
        for k in KEYS:
            getattr(w, k).copy_(snap[k])
        for k, t in state0.items():
            getattr(m, k).copy_(t)
        w.bp_invalidate()

    def wall_us(fn):
        restore()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, out

    plain = lambda: w.characters_move(m, dt)
    ordered = lambda: w.characters_move_ordered(m, dt)
    wall_us(plain)                                          # warm: both once (the ordered call finds its pair room here)
    wall_us(ordered)
    t_plain, t_ordered, t_order = [], [], []
    for _ in range(a.runs):                                 # alternated
        t, out = wall_us(plain)
        t_plain.append(t)
        flags = out["flags"].cpu().numpy().view(np.uint32)
        pos_plain = w.pos[body].clone()
        t, out = wall_us(ordered)
        t_ordered.append(t)
        pos_ordered = w.pos[body].clone()
        oflags = out["flags"].cpu().numpy().view(np.uint32)
        t, (_reach, _level, n_levels, pair_total) = wall_us(lambda: w.characters_order(m, dt))
        t_order.append(t)
    flagged = ((flags & 4) != 0) | (((flags >> 8) & 4) != 0)
    differ = (pos_plain != pos_ordered).any(1)
    tri = lambda v: [round(min(v), 1), round(median(v), 1), round(max(v), 1)]
    res = dict(bodies=w.n, statics=w.n_static, movers=a.movers, runs=a.runs, dt=dt, unit="us wall [min, median, max]",
               plain_move_us=tri(t_plain), ordered_move_us=tri(t_ordered), order_alone_us=tri(t_order),
               n_levels=int(out["n_levels"]), order_n_levels=int(n_levels), pair_total=int(pair_total),
               rounds=int(w.order_summary[3]), plain_flagged_moved_target=int(flagged.sum()),
               ordered_flagged_moved_target=int((((oflags & 4) != 0) | (((oflags >> 8) & 4) != 0)).sum()),
               movers_whose_pos_differs=int(differ.sum()), share_whose_pos_differs=round(float(differ.double().mean()), 5),
               scratch_bytes=_lib.characters_move_ordered_scratch_bytes(w.n, a.movers, w._order_capacity))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
