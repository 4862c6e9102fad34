"""Launch-to-launch times of the broadphase, the contacts and the step at 262 144 bodies.
    python tools/bp_time.py [spheres] [capsules] [--mixed] [--levels L] [--cell0 C]
--levels L: a multi-level grid (PhysWorld(bp_levels=L)); with --cell0 the level-0 cell replaces the scene's own cell (the
largest edge), e.g. the capsule mix binned from its smallest edge up.  --mixed: synth.mixed_bodies (cell0 0.25); without
--levels it runs on the one-level grid whose cell is the largest edge, the only exact one-level choice."""
import argparse, sys, os, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clap_amd import _lib, physics, synth
ap = argparse.ArgumentParser()
ap.add_argument("kinds", nargs="*")
ap.add_argument("--mixed", action="store_true")
ap.add_argument("--levels", type=int, default=1)
ap.add_argument("--cell0", type=float, default=None)
ap.add_argument("--n", type=int, default=262_144)
a = ap.parse_args()
_lib.check(_lib.lib().clapgpu_init(0),"init")
for kind in (tuple(a.kinds) or (() if a.mixed else ("spheres","capsules"))) + (("mixed",) if a.mixed else ()):
    if kind == "mixed":
        b = synth.mixed_bodies(a.n, box=64.0 * (a.n / 262_144) ** (1 / 3), cell0=0.25, seed=4)
        if a.levels == 1: b["cell"] = float(2.0 * b["radius"].max())
    else:
        b = synth.sphere_bodies(a.n, box=64.0, seed=4) if kind=="spheres" else synth.capsule_bodies(a.n, box=60.0, seed=4)
    if a.cell0 is not None: b["cell"] = a.cell0
    pw = physics.PhysWorld(b, synth.static_boxes(64, 64.0 if kind!="capsules" else 60.0), pair_capacity=4_000_000 if kind=="mixed" else 2_000_000,
                           device="cuda:0", bp_levels=a.levels)
    def t(fn, it=30):
        for _ in range(5): fn()
        ev=[(torch.cuda.Event(enable_timing=True),torch.cuda.Event(enable_timing=True)) for _ in range(it)]
        torch.cuda.synchronize()
        for a_,c in ev: a_.record(); fn(); c.record()
        torch.cuda.synchronize()
        return np.mean([a_.elapsed_time(c) for a_,c in ev])*1e3
    print(kind, "levels", a.levels, "cell", pw.cell, "broadphase us", t(pw.broadphase), "pairs", int(pw.pair_total.item()),
          "static pairs", int(pw.static_pair_total.item()), "status", pw.broadphase_status(),
          "contacts us", t(pw.contacts_geoms), "contacts (both lists, one launch) us", t(pw.contacts_geoms_both),
          "step us", t(lambda: pw.world_step(1/120)))
