"""Times clapgpu_bp_statics_update at the benchmark scene (262 144 bodies, the 5 000 statics of tools/ray_time.py), for the
one-level object and for the six-level mixed object of tools/bp_time.py --mixed --levels 6, against the only way to move a
static without it: clapgpu_bp_destroy + clapgpu_bp_create[_levels] with the same boxes (a host binning pass per level, an
allocation, an upload).  Both are wall clock around the call (the update synchronises the stream; the re-creation is
host work and blocking copies), alternated in one process, medians of --reps; every update moves ALL statics (each by up to
+-2 units).  One JSON line.  The per-kernel times of the update: run this under a kernel trace with --only-update.
    python tools/bp_statics_time.py [--reps 20] [--n 262144] [--statics 5000] [--only-update]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clap_amd import _lib, physics  # noqa: E402

LEVELS, CELL0, ONE_CELL = 6, 0.25, 1.0


def statics(ns):
    R = np.random.Generator(np.random.PCG64(5))
    lo = R.uniform(-5, 65, (ns, 3))
    bb = np.empty((ns, 6))
    bb[:, 0::2], bb[:, 1::2] = lo, lo + R.uniform(0.1, 3.0, (ns, 3))
    bb[0] = [-1e3, 1e3, -10.0, 0.0, -1e3, 1e3]
    return bb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=262_144)
    ap.add_argument("--statics", type=int, default=5000)
    ap.add_argument("--only-update", action="store_true")
    a = ap.parse_args()
    lib = _lib.lib()
    _lib.check(lib.clapgpu_init(0), "clapgpu_init")
    stream = physics._stream()
    st = statics(a.statics)
    R = np.random.Generator(np.random.PCG64(6))
    moved = []                                              # the box sets the repetitions alternate between
    for _ in range(2):
        d = np.repeat(R.uniform(-2.0, 2.0, (a.statics, 3)), 2, axis=1)
        moved.append(np.ascontiguousarray(st + d))
    moved_d = [torch.from_numpy(m).cuda() for m in moved]
    res = dict(bodies=a.n, statics=a.statics, reps=a.reps)
    for name, levels, cell in (("one_level", 1, ONE_CELL), (f"levels_{LEVELS}", LEVELS, CELL0)):
        def create(boxes):
            bp = C.c_void_p()
            if levels == 1:
                _lib.check(lib.clapgpu_bp_create(C.byref(bp), a.n, cell, a.statics, boxes.ctypes.data), "clapgpu_bp_create")
            else:
                _lib.check(lib.clapgpu_bp_create_levels(C.byref(bp), a.n, cell, levels, a.statics, boxes.ctypes.data),
                           "clapgpu_bp_create_levels")
            return bp

        bp, other = create(st), create(st)
        _lib.check(lib.clapgpu_bp_statics_update(stream, bp, a.statics, moved_d[1].data_ptr()), "clapgpu_bp_statics_update")   # warm: the allocation
        t_update, t_create = [], []
        for r in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _lib.check(lib.clapgpu_bp_statics_update(stream, bp, a.statics, moved_d[r % 2].data_ptr()), "clapgpu_bp_statics_update")
            t_update.append(time.perf_counter() - t0)
            if a.only_update:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lib.clapgpu_bp_destroy(other)
            other = create(moved[r % 2])
            torch.cuda.synchronize()
            t_create.append(time.perf_counter() - t0)
        ne, nl = C.c_uint32(0), C.c_uint32(0)
        _lib.check(lib.clapgpu_bp_statics_sizes(bp, None, C.byref(ne), C.byref(nl), None, None), "clapgpu_bp_statics_sizes")
        res[name] = dict(entries=ne.value, large=nl.value, update_us=float(np.median(t_update)) * 1e6,
                         update_us_min_max=[min(t_update) * 1e6, max(t_update) * 1e6])
        if t_create:
            ne2 = C.c_uint32(0)
            _lib.check(lib.clapgpu_bp_statics_sizes(other, None, C.byref(ne2), None, None, None), "clapgpu_bp_statics_sizes")
            res[name].update(recreate_us=float(np.median(t_create)) * 1e6,
                             recreate_us_min_max=[min(t_create) * 1e6, max(t_create) * 1e6], same_entries=ne2.value == ne.value)
        lib.clapgpu_bp_destroy(bp)
        lib.clapgpu_bp_destroy(other)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
