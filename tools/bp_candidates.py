"""Candidates per body of the broadphase search, counted on the host in numpy (no GPU): the records in the cells a body
looks up -- own cell + the 13 after it on its own level, and on a multi-level grid the cells of its grown box on every
coarser level (clap_amd/csrc/bp_levels.h) -- against the overlapping pairs it has to find.  Cells, not slots: records of
far cells that share a slot are not counted.
    python tools/bp_candidates.py [--n 262144] [--levels 6]        (synth.mixed_bodies, cell0 0.25, box scaled with n)"""
import argparse, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clap_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=262_144)
ap.add_argument("--levels", type=int, default=6)
a = ap.parse_args()
b = synth.mixed_bodies(a.n, box=64.0 * (a.n / 262_144) ** (1 / 3), cell0=0.25, seed=4)
pos, r = b["pos"], b["radius"][:, None]
lo, hi = pos - r, pos + r
edge = (hi - lo).max(1)
key = lambda c: (c[:, 0] + (1 << 20)) * (1 << 42) + (c[:, 1] + (1 << 20)) * (1 << 21) + (c[:, 2] + (1 << 20))


def counts_at(cells_sorted, cnt, c):
    k = key(c)
    at = np.minimum(np.searchsorted(cells_sorted, k), len(cells_sorted) - 1)
    return np.where(cells_sorted[at] == k, cnt[at], 0)


for levels, cell0 in ((a.levels, 0.25), (1, float(edge.max()))):
    level = np.zeros(a.n, np.int64)
    for l in range(levels - 1):
        level += (edge > cell0 * 2.0 ** l) & (level == l)
    cand = np.zeros(a.n, np.int64)
    for L in range(levels):
        c = cell0 * 2.0 ** L
        on = level == L
        cells, cnt = np.unique(key(np.floor(pos[on] / c).astype(np.int64)), return_counts=True)
        if not len(cells):
            continue
        own = np.floor(pos[on] / c).astype(np.int64)
        for cq in range(13, 27):                             # same level
            cand[on] += counts_at(cells, cnt, own + [cq % 3 - 1, (cq // 3) % 3 - 1, cq // 9 - 1])
        cand[on] -= 1                                        # itself
        fine = level < L                                     # finer bodies looking up this level
        f0, f1 = np.floor((lo[fine] - c / 2) / c).astype(np.int64), np.floor((hi[fine] + c / 2) / c).astype(np.int64)
        for dz in range(3):
            for dy in range(3):
                for dx in range(3):
                    cc = f0 + [dx, dy, dz]
                    cand[fine] += np.where((cc <= f1).all(1), counts_at(cells, cnt, cc), 0)
    print(f"levels {levels} cell0 {cell0:g}: bodies per level {np.bincount(level, minlength=levels).tolist()}, "
          f"candidates per body mean {cand.mean():.1f} max {cand.max()}")
