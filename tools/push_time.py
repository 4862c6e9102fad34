"""Timing drivers for the force accumulator and clapgpu_bodies_push (tools/profile_push.sh runs them).

    python tools/push_time.py step <libclapgpu.so | shipped> <null|zeros|tenth> [iters]
        iters steps of 262 144 capsule bodies (synth.capsule_bodies, bench_extras' physics size), for rocprofv3
        --kernel-trace.  The library is loaded with plain ctypes, so a build of the parent commit (no push entry point,
        another ABI version) runs too: it reads the descriptor up to geom_records and never sees facc.
        null: no accumulator.  zeros: an accumulator nobody adds to.  tenth: forces on a tenth of the bodies before
        every step (a device copy in front of each launch, not part of the kernel's time).
    python tools/push_time.py push [--movers 65536] [--runs 5] [--k 3]
        the slide of tools/slide_bench.py's workload B walk, and the push of its results, launch to launch between HIP
        events; one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clap_amd import _lib, synth  # noqa: E402


def step(lib, forces, iters):
    path = _lib.LIB_PATH if lib == "shipped" else os.path.join(ROOT, lib)
    L = C.CDLL(path)
    L.clapgpu_bodies_step.argtypes = [C.c_void_p, C.POINTER(_lib.Bodies), C.POINTER(_lib.World), C.c_double]
    assert L.clapgpu_init(0) == 0
    dev = torch.device("cuda:0")
    b = synth.capsule_bodies(262_144, box=60.0, seed=4)
    n = int(b["n"])
    t = {k: torch.from_numpy(np.ascontiguousarray(b[k], np.float64)).to(dev)
         for k in ("pos", "quat", "lvel", "avel", "mass", "radius", "yoffset", "adis_time_left", "length", "inertia")}
    t["bflags"] = torch.from_numpy(b["bflags"].view(np.int32)).to(dev)
    t["steps"] = torch.from_numpy(np.ascontiguousarray(b["adis_steps_left"], np.int32)).to(dev)
    t["entity"] = torch.from_numpy(np.ascontiguousarray(b["body_entity"], np.int32)).to(dev)
    t["aabb"], t["axis"] = torch.zeros((n, 6), dtype=torch.float64, device=dev), torch.zeros((n, 3), dtype=torch.float64, device=dev)
    t["records"] = torch.zeros((n, 8), dtype=torch.float64, device=dev)
    p = lambda k: t[k].data_ptr()
    d = _lib.Bodies(n, 1, p("pos"), p("quat"), p("lvel"), p("avel"), p("mass"), p("radius"), p("yoffset"), p("bflags"), p("steps"),
                    p("adis_time_left"), p("entity"))
    d.length, d.inertia, d.aabb, d.axis, d.geom_records = p("length"), p("inertia"), p("aabb"), p("axis"), p("records")
    L.clapgpu_geom_offset_rotation(d.geom_offset_R)
    w = _lib.World()
    L.clapgpu_world_defaults(C.byref(w))
    f0 = None
    if forces != "null":
        t["facc"] = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        d.facc = p("facc")
        if forces == "tenth":
            R = np.random.Generator(np.random.PCG64(17))
            f = np.zeros((n, 3))
            some = R.random(n) < 0.1
            f[some] = R.normal(0, 40.0, (int(some.sum()), 3))
            f0 = torch.from_numpy(f).to(dev)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(iters):
        if f0 is not None:
            t["facc"].copy_(f0)
        assert L.clapgpu_bodies_step(s, C.byref(d), C.byref(w), 1.0 / 120.0) == 0
    torch.cuda.synchronize()
    print(f"{lib} {forces}: {iters} steps of {n} bodies")


def push(movers, runs, k):
    from clap_amd import physics
    from mesh_contact_time import scene
    from slide_bench import Slide, event_us, mixes
    _lib.check(_lib.lib().clapgpu_init(0), "clapgpu_init")
    w, _b, _terrain = scene("B")
    w.enable_forces()
    w.bodies_aabb()
    mv, mix = mixes(w, movers, 10)
    vel, air = mix["walk"]
    s = Slide(w, mv, vel, air)

    def index_only():
        s.restore()
        w.bp_index()
    res = dict(bodies=w.n, statics=w.n_static, movers=movers, k=k, runs=runs, unit="us per call [min, median, max]")
    res["restore_index_us"] = event_us(index_only, k, runs)
    res["slide_walk_grid_us"] = event_us(lambda: s.call(True), k, runs)
    torch.cuda.synchronize()
    push_h, flags_h = s.push.cpu().numpy(), s.flags.cpu().numpy()
    res["pushing_slots"] = int(((push_h >= 0) & (flags_h == 0)[:, None]).sum())
    res["pushed_bodies"] = int(len(np.unique(push_h[(push_h >= 0) & (flags_h == 0)[:, None]])))
    res["scratch_bytes"] = _lib.bodies_push_scratch_bytes(movers)
    scratch = torch.zeros(res["scratch_bytes"], dtype=torch.uint8, device=w.device)
    pushed = torch.zeros(w.n, dtype=torch.int32, device=w.device)
    L = _lib.lib()

    def call():
        _lib.check(L.clapgpu_bodies_push(physics._stream(), C.byref(w._desc), C.byref(w.world), movers, s.body.data_ptr(),
                                         s.vel0.data_ptr(), s.push.data_ptr(), s.flags.data_ptr(), pushed.data_ptr(),
                                         scratch.data_ptr()), "clapgpu_bodies_push")
    res["push_us"] = event_us(call, k, runs)
    assert int(pushed.sum().item()) == res["pushing_slots"]
    slide = res["slide_walk_grid_us"][1] - res["restore_index_us"][1]
    res["slide_alone_us"] = round(slide, 1)
    res["push_over_slide"] = round(res["push_us"][1] / slide, 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "step":
        step(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 200)
    else:
        import argparse
        ap = argparse.ArgumentParser()
        ap.add_argument("mode")
        ap.add_argument("--movers", type=int, default=65536)
        ap.add_argument("--runs", type=int, default=5)
        ap.add_argument("--k", type=int, default=3)
        a = ap.parse_args()
        push(a.movers, a.runs, a.k)
