"""GPU: clapgpu_sweep_capsules_grid against the existing sweep fed host-built lists, and clapgpu_characters_slide against
the restatement of tests/slideref.py, bit for bit; the batch rules; the same bits twice and from a captured graph.

Scene B's slide is compared twice.  For bits, with the restatement run over the EXISTING device sweep
(PhysWorld.sweep_capsules with host-built canonical lists, the parent commit's way of doing the move, pinned by the
existing sweep tests).  Independently, with the restatement over tests/meshcontactref.sweep and the oracle's sweep
(slideref.SceneBSweep), within a tolerance: meshcontactref.sweep agrees with the device's mesh sweep to 1e-5 only
(test_sweep_onto_the_terrain), so it cannot pin bits.

CLAPGPU_SLIDE_MOVED_TARGET: the restatement's sweep does not say which bodies touched the probe, so the flag is pinned
three ways: it must be clear for a mover none of whose candidates is a mover of the batch; a set of movers that are not
each other's candidates has flags == 0 byte for byte; hand cases pin when it is set, and that it is a superset."""
import ctypes as C

import numpy as np
import pytest
import torch

from clap_amd import _lib, physics, synth
import slideref as sr
from meshscene import Scene, fetch, same_bits, rng

pytestmark = pytest.mark.gpu
DT = 1.0 / 30.0


def host_lists(bb, static_bb, movers, delta, margin=1e-3):
    cand, first = [], [0]
    for k, m in enumerate(movers):
        c = sr.canonical_candidates(bb[m, 0::2], bb[m, 1::2], delta[k], static_bb, bb, margin)
        cand += list(c)
        first.append(len(cand))
    return np.asarray(first, np.uint32), np.asarray(cand, np.uint32)


def sweep_deltas(n, seed):
    delta = rng(seed).normal(0, 1.0, (n, 3)).astype(np.float32)
    delta[:5] = 0                                           # no movement: frac 1
    delta[5:10] *= 1e-3                                     # shorter than a step
    delta[10:40, 0::2] = 0
    delta[10:40, 1] = -np.abs(delta[10:40, 1]) - 2.0        # straight down
    return delta


def three_ways(w, static_bb, movers, delta, sample=None):
    """grid, brute force and (on `sample`) the host-list call: equal bytes; returns the grid path's outputs"""
    w.bodies_aabb()
    w.bp_index()
    g = fetch(w.sweep_capsules_grid(movers, delta, grid=True))
    f = fetch(w.sweep_capsules_grid(movers, delta, grid=False))
    for name, a, c in zip(("frac", "normal", "hit", "flags"), g, f):
        assert same_bits(a, c), name
    idx = np.arange(len(movers)) if sample is None else sample
    bb = w.download()["aabb"]
    first, cand = host_lists(bb, static_bb, movers[idx], delta[idx])
    h = fetch(w.sweep_capsules(movers[idx], delta[idx], first, cand))
    for name, a, c in zip(("frac", "normal", "hit"), g, h):
        assert same_bits(a[idx], c), name
    return g


def world_a(dev):
    b, statics = sr.scene_a()
    return physics.PhysWorld(b, statics, device=dev), b, statics


def scene_b(dev, **kw):
    b, meshes = sr.scene_b()
    return Scene(dev, b, meshes, cap=(1 << 20, 1 << 20), **kw), b


# ------------------------------------------------------------------------------------------------- layer 1
def test_sweep_grid_scene_a(cuda_device):
    w, b, statics = world_a(cuda_device)
    movers = rng(2).choice(b["n"], 300, replace=False).astype(np.uint32)
    frac, _n, hit, flags = three_ways(w, statics, movers, sweep_deltas(300, 21))
    assert (frac[:5] == 1.0).all() and 30 < (frac < 1).sum() < 300 and (hit <= -2).any() and (hit >= 0).any()
    assert not flags.any()


def test_sweep_grid_scene_b_with_meshes(cuda_device):
    sc, b = scene_b(cuda_device)
    movers = rng(3).choice(b["n"], 300, replace=False).astype(np.uint32)
    frac, _n, hit, flags = three_ways(sc.w, sc.w._statics_host, movers, sweep_deltas(300, 22))
    assert (hit == -2 - sc.base).sum() > 30 and not flags.any()
    # without the mesh set the terrain is an OTHER static nobody resolves
    f0, _n0, h0, fl0 = fetch(sc.w.sweep_capsules_grid(movers, sweep_deltas(300, 22), grid=False, meshes=False))
    assert (fl0 & _lib.SLIDE_UNRESOLVED).sum() > 30 and not (h0 == -2 - sc.base).any()


def big_scene(dev, oversized=False):
    from test_rays_gpu import grid_scene
    return grid_scene(dev, oversized=oversized)


def test_sweep_grid_large_run(cuda_device):
    w, b, bb, _kind = big_scene(cuda_device)
    R = rng(31)
    n = 65536
    movers = R.integers(0, w.n, n).astype(np.uint32)
    delta = R.normal(0, 0.7, (n, 3)).astype(np.float32)
    delta[:64] = 0
    delta[64:128, 1] = -40.0                                # long: many cells, the scan
    delta[128:132, 0] = np.nan
    movers[132:136] = w.n + 5
    frac, _n, hit, flags = three_ways(w, bb, movers, delta, sample=R.choice(n, 2000, replace=False))
    assert (flags & _lib.SLIDE_INVALID).sum() == 8 and (frac[128:136] == 1).all() and (hit[128:136] == -1).all()
    assert (hit >= 0).sum() > 1000 and (hit <= -2).sum() > 100 and (flags & _lib.SLIDE_UNRESOLVED).sum() > 10


def test_sweep_grid_oversized_body_scans(cuda_device):
    w, b, bb, _kind = big_scene(cuda_device, oversized=True)
    w.bodies_aabb()
    w.bp_index()
    assert w.bp_index_status() == 1
    R = rng(32)
    movers = R.integers(0, w.n, 512).astype(np.uint32)
    delta = R.normal(0, 0.7, (512, 3)).astype(np.float32)
    c = w.cell                                              # down through the oversized sphere's rim (as the ray test)
    movers[:16] = np.arange(100, 116)
    pos = w.pos.cpu().numpy()
    pos[100:116] = b["pos"][7] + np.stack([np.full(16, 0.85 * c), np.full(16, 3.0), np.linspace(-0.2, 0.2, 16) * c], 1)
    w.pos.copy_(torch.from_numpy(pos))
    delta[:16] = [0, -4, 0]
    frac, _n, hit, _fl = three_ways(w, bb, movers, delta)
    assert w.bp_index_status() == 1 and (hit[:16] == 7).sum() >= 4      # (the sixteen also stand in each other's way)


def aliased_scene(dev):
    """4 096 bodies, half in a clump and half scattered over a box some 40 blocks wide, so that more blocks are occupied
    than the grid's 1 024 block buckets; 40 statics with boxes, two of them for the large list, one across a block
    boundary"""
    n = 4096
    b = synth.capsule_bodies(n, box=12.0, seed=61)
    R = rng(62)
    b["pos"][n // 2:] = R.uniform(-150.0, 150.0, (n - n // 2, 3))
    cell = b["cell"]
    ns = 40
    lo = R.uniform(-2.0, 14.0, (ns, 3))
    lo[32:] = R.uniform(-150.0, 150.0, (ns - 32, 3))
    bb = np.empty((ns, 6))
    bb[:, 0::2], bb[:, 1::2] = lo, lo + R.uniform(0.5, 3.0, (ns, 3))
    bb[0] = [-1e3, 1e3, -3.0, -1.0, -1e3, 1e3]              # a ground slab under the clump: the large list
    bb[1] = [-200, 200, 14, 15, -200, 200]                  # large as well
    bb[2] = [4 * cell - 0.5, 4 * cell + 0.5, 2, 3, 2, 3]    # across the block boundary at x = 4 cells
    kind = R.choice([_lib.GEOM_SPHERE, _lib.GEOM_CAPSULE, _lib.GEOM_BOX], ns).astype(np.uint8)
    kind[:3] = _lib.GEOM_BOX
    w = physics.PhysWorld(b, bb, device=dev)
    w.set_static_geoms(kind, *synth.geoms_of_aabbs(bb, kind))
    return w, b, bb


def test_rays_and_sweeps_share_one_lookup_of_an_aliased_index(cuda_device):
    """both consumers of grid_query_dev.h on one index whose buckets hold several blocks each: the grid path's bytes are
    the brute-force path's"""
    w, b, bb = aliased_scene(cuda_device)
    n = w.n
    assert n < 32768                                        # the grid's minimum: 1 024 block buckets
    blocks = np.floor(np.floor(b["pos"] / w.cell) / 4)
    assert len(np.unique(blocks, axis=0)) > 1024            # pigeonhole: blocks share buckets
    assert np.floor(bb[2, 0] / (4 * w.cell)) != np.floor(bb[2, 1] / (4 * w.cell))
    w.bp_index()
    assert w.bp_index_status() == 0
    # rays: out of the clump and across the scattered half, from 1 to some 70 cells long (a piece is at most one cell, so
    # the long ones skip what the piece before looked up), and straight down onto the slab
    R = rng(63)
    nr = 4096
    s = R.uniform(-2.0, 14.0, (nr, 3))
    s[nr // 2:] = R.uniform(-150.0, 150.0, (nr - nr // 2, 3))
    d = R.normal(size=(nr, 3))
    L = R.choice([2.0, 10.0, 40.0, 120.0], nr)
    s[:256, 1], d[:256], L[:256] = 13.0, [0, -1.0, 0], 40.0
    g = fetch(w.ray_cast(s, d, L, grid=True))
    f = fetch(w.ray_cast(s, d, L, grid=False))
    for name, x, y in zip(("dist", "hit", "contact", "flags"), g, f):
        assert same_bits(x, y), name
    sweeps = R.integers(0, n, nr).astype(np.uint32)
    delta = R.normal(0, 0.7, (nr, 3)).astype(np.float32)
    sweeps[:256] = np.argsort(b["pos"][:n // 2, 1])[:256]    # the lowest of the clump, down onto the slab
    delta[:256] = [0, -4, 0]
    sg = fetch(w.sweep_capsules_grid(sweeps, delta, grid=True))
    sf = fetch(w.sweep_capsules_grid(sweeps, delta, grid=False))
    for name, x, y in zip(("frac", "normal", "hit", "flags"), sg, sf):
        assert same_bits(x, y), name
    for hit in (g[1], f[1], sg[2], sf[2]):
        assert (hit >= 0).any() and (hit <= -2).any() and (hit == -1).any()


# ------------------------------------------------------------------------------------------------- layer 2
KEYS = ("pos", "quat", "lvel", "aabb", "axis", "geom_records")


def snapshot(w):
    return {k: getattr(w, k).clone() for k in KEYS}


def restore(w, snap):
    for k in KEYS:
        getattr(w, k).copy_(snap[k])
    w.bp_invalidate()


def check_geoms_current(w):
    got = {k: getattr(w, k).cpu().numpy().copy() for k in ("aabb", "axis", "geom_records")}
    w.bodies_aabb()
    for k, a in got.items():
        assert same_bits(a, getattr(w, k).cpu().numpy()), k


def slide_and_fetch(w, movers, v, air, dt=DT, grid=True):
    if grid:
        w.bp_index()
    vel, ff, push, flags = fetch(w.slide(movers, v, air, dt, grid=grid))
    return dict(pos=w.pos.cpu().numpy().copy(), lvel=w.lvel.cpu().numpy().copy(), velocity=vel, first_frac=ff, push_hit=push,
                flags=flags)


def compare_with(ref_world, out, before, movers, v, air, dt=DT, exact_flags=False):
    """pos, velocity, first_frac, push_hit byte for byte; flags: INVALID / UNRESOLVED clear, MOVED_TARGET clear for a
    mover none of whose candidates (ref_world.seen) is a mover of the batch -- exact_flags: clear for all"""
    moved = flagged = 0
    mset = set(int(m) for m in movers)
    for k, m in enumerate(movers):
        r = sr.run_mover(ref_world, m, v[k], air[k], dt)
        assert same_bits(out["pos"][m], r["pos"]), (k, m, out["pos"][m], r["pos"])
        assert same_bits(out["velocity"][k], r["velocity"]), k
        assert same_bits(out["first_frac"][k], r["first_frac"]), (k, out["first_frac"][k], r["first_frac"])
        assert same_bits(out["push_hit"][k], r["push_hit"]), (k, out["push_hit"][k], r["push_hit"])
        others = set(ref_world.seen) & (mset - {int(m)})
        assert (out["flags"][k] & ~_lib.SLIDE_MOVED_TARGET) == 0, (k, out["flags"][k])
        if exact_flags or not others:
            assert out["flags"][k] == 0, (k, out["flags"][k], others)
        for h in r["push_hit"]:                             # a pushed mover that moved: the flag must be there
            if h in mset and not same_bits(out["pos"][h], before["pos"][h].cpu().numpy()):
                assert out["flags"][k] == _lib.SLIDE_MOVED_TARGET, (k, h)
        flagged += out["flags"][k] != 0
        moved += not same_bits(r["pos"], before["pos"][m].cpu().numpy())
    rest = np.setdiff1d(np.arange(len(out["pos"])), movers)
    assert not out["lvel"][movers].any() and same_bits(out["lvel"][rest], before["lvel"].cpu().numpy()[rest])
    assert same_bits(out["pos"][rest], before["pos"].cpu().numpy()[rest])
    return moved, flagged


def apart(b, bb, movers, v, want):
    """movers (indices into `movers`) none of which can have another of them among its candidates: a mover stays within
    |v| * dt summed over its two calls of where it starts"""
    reach = (np.abs(v).sum(1) / 30.0 + 2e-3)[:, None]
    lo, hi = bb[movers][:, 0::2] - reach, bb[movers][:, 1::2] + reach
    keep = []
    for k in range(len(movers)):
        if all(not (np.all(bb[movers[j], 0::2] <= hi[k]) and np.all(bb[movers[j], 1::2] >= lo[k])) and
               not (np.all(bb[movers[k], 0::2] <= hi[j]) and np.all(bb[movers[k], 1::2] >= lo[j])) for j in keep):
            keep.append(k)
    assert len(keep) >= want, len(keep)
    return np.asarray(keep)


def test_slide_scene_a_against_the_restatement(cuda_device):
    w, b, statics = world_a(cuda_device)
    w.lvel.normal_()                                        # something for the call to zero, and to leave alone
    movers, v, air = sr.movers_a(b["n"])
    before = snapshot(w)
    out = slide_and_fetch(w, movers, v, air)
    moved, flagged = compare_with(sr.OracleSweep(b, statics), out, before, movers, v, air)
    assert moved > 150 and flagged > 0
    check_geoms_current(w)
    # movers that are not each other's candidates: the flags too, byte for byte (all zero)
    restore(w, before)
    sub = apart(b, w.download()["aabb"], movers, v, 20)
    alone = slide_and_fetch(w, movers[sub], v[sub], air[sub])
    compare_with(sr.OracleSweep(b, statics), alone, before, movers[sub], v[sub], air[sub], exact_flags=True)
    assert not alone["flags"].any()
    restore(w, before)
    brute = slide_and_fetch(w, movers, v, air, grid=False)
    for k in out:
        assert same_bits(out[k], brute[k]), k
    # dt below 1e-6: nothing at all; a long frame is the clamped one
    restore(w, before)
    w.bp_index()
    nothing = slide_and_fetch(w, movers, v, air, dt=0.9e-6, grid=False)
    assert same_bits(nothing["pos"], before["pos"].cpu().numpy()) and same_bits(nothing["lvel"], before["lvel"].cpu().numpy())
    assert same_bits(nothing["velocity"], v)
    w.sweep_capsules_grid(movers[:4], v[:4] * 0.01, grid=True)          # ... and the index is still there
    long = slide_and_fetch(w, movers, v, air, dt=1.0, grid=False)
    assert same_bits(long["pos"], out["pos"])


def test_slide_cluster_one_mover_at_a_time(cuda_device):
    w, b, statics = world_a(cuda_device)
    ref = sr.OracleSweep(b, statics)
    centre = b["pos"][np.argmin(np.abs(b["pos"] - 7.0).sum(1))]
    cluster = np.argsort(((b["pos"] - centre) ** 2).sum(1))[:8].astype(np.uint32)
    v = rng(41).normal(0, 20.0, (8, 3)).astype(np.float32)
    air = np.array([0, 1, 0, 1, 0, 1, 0, 1], np.uint8)
    before = snapshot(w)
    for k in range(8):
        restore(w, before)
        out = slide_and_fetch(w, cluster[k:k + 1], v[k:k + 1], air[k:k + 1])
        compare_with(ref, out, before, cluster[k:k + 1], v[k:k + 1], air[k:k + 1], exact_flags=True)
    restore(w, before)                                      # all eight at once: same moves, the flags may say MOVED_TARGET
    out = slide_and_fetch(w, cluster, v, air)
    compare_with(ref, out, before, cluster, v, air)


class DeviceListSweep:
    """slideref's sweep through the existing device call: PhysWorld.sweep_capsules with host-built canonical lists, the
    mover's position uploaded before every sweep (a second world, the poses from before the call)."""

    def __init__(self, w):
        self.w = w
        w.bodies_aabb()
        self.pos0, self.bb = w.pos.clone(), w.download()["aabb"]

    def mover(self, i):
        w = self.w
        pos = self.pos0[i].cpu().numpy().copy()
        self.seen = set()

        def sweep(delta):
            w.pos.copy_(self.pos0)
            w.pos[i] = torch.from_numpy(pos).to(w.device)
            w.bodies_aabb()
            bb = self.bb.copy()
            bb[i] = w.aabb[i].cpu().numpy()
            first, cand = host_lists(bb, w._statics_host, np.array([i]), np.asarray(delta, np.float32)[None])
            self.seen.update(int(c & 0x7fffffff) for c in cand if c >> 31 and int(c & 0x7fffffff) != i)
            f, n, h = fetch(w.sweep_capsules(np.array([i], np.uint32), np.asarray(delta, np.float32)[None], first, cand))
            return f[0], n[0], int(h[0])

        def move(step):
            for a in range(3):
                pos[a] = pos[a] + np.float64(step[a])

        return sweep, move, lambda: pos.copy()


def test_slide_scene_b_against_the_host_loop(cuda_device):
    sc, b = scene_b(cuda_device)
    ref_sc, _b = scene_b(cuda_device)
    w = sc.w
    movers, v, air = sr.movers_b(b)
    w.bodies_aabb()
    before = snapshot(w)
    out = slide_and_fetch(w, movers, v, air)
    moved, _flagged = compare_with(DeviceListSweep(ref_sc.w), out, before, movers, v, air)
    assert moved > 200 and (out["first_frac"][:, 0] < 1).sum() > 60
    # an independent reference: slideref over meshcontactref.sweep (the terrain) and the oracle's sweep (the bodies).
    # Tolerance: a sweep's frac and normal agree with meshcontactref.sweep to 1e-5 (test_sweep_onto_the_terrain); a
    # delta is at most 2 units long here and a mover makes at most six sweeps, each adding 2e-5 of position through its
    # frac and as much through the projection along its normal: 6 * 4e-5 < 3e-4.  Only movers whose sweeps never hit the
    # terrain and a body at once are compared: there SceneBSweep is the joint sweep exactly.
    import trimeshref as tr
    ind = sr.SceneBSweep(b, tr.bake(*sr.scene_b()[1][0]), sc.base)
    compared = 0
    for k, m in enumerate(movers):
        r = sr.run_mover(ind, m, v[k], air[k], DT)
        if ind.both:
            continue
        compared += 1
        assert np.abs(out["pos"][m] - r["pos"]).max() <= 3e-4, (k, m, out["pos"][m], r["pos"])
        assert np.abs(out["first_frac"][k] - r["first_frac"]).max() <= 1e-4, (k, out["first_frac"][k], r["first_frac"])
        assert np.array_equal(out["push_hit"][k], r["push_hit"]) and np.array_equal(out["velocity"][k], r["velocity"]), k
    assert compared >= 100, compared
    check_geoms_current(w)
    # the same state twice: the same bytes
    restore(w, before)
    again = slide_and_fetch(w, movers, v, air)
    for k in out:
        assert same_bits(out[k], again[k]), k


# ------------------------------------------------------------------------------------------------- batch rules
def pair_world(dev, statics, kinds=None, third=False):
    b = synth.capsule_bodies(8, box=1.0, seed=1)
    b["pos"][:] = [-500.0, -500.0, -500.0]
    b["pos"][:, 0] -= 10.0 * np.arange(8)
    sph = np.array([0, 1])
    b["length"][sph] = 0.0                                  # two spheres of radius 0.5, 0.5 apart
    b["radius"][:3] = 0.5
    b["pos"][sph[0]] = [0, 0, 0]
    b["pos"][sph[1]] = [float(b["radius"][sph].sum()) + 0.5, 0, 0]
    if third:                                               # a third sphere beside the gap, 0.17 from touching both
        b["length"][2] = 0.0
        b["pos"][2] = [0.75, 0, 0.8]
    w = physics.PhysWorld(b, np.asarray(statics, float).reshape(-1, 6), device=dev)
    if kinds is not None:
        ns = len(kinds)
        w.set_static_geoms(np.asarray(kinds, np.uint8), np.zeros((ns, 3)), np.tile([0, 0, 1.0], (ns, 1)), np.zeros(ns), np.zeros(ns))
    return w, b, sph.astype(np.uint32)


def test_batch_rules(cuda_device):
    far = [[-10, 10, -90, -89, -10, 10]]
    w, b, two = pair_world(cuda_device, far)
    p0 = w.pos.cpu().numpy().copy()
    # towards each other: both are blocked by the other where it was, both moved a little, both flagged
    v = np.array([[30, 0, 0], [-30, 0, 0]], np.float32)
    out = slide_and_fetch(w, two, v, [0, 0], grid=False)
    assert (out["flags"] == _lib.SLIDE_MOVED_TARGET).all() and (out["first_frac"][:, 0] < 1).all()
    assert out["push_hit"][0, 0] == two[1] and out["push_hit"][1, 0] == two[0]
    assert out["pos"][two[0], 0] > 0 and out["pos"][two[1], 0] < p0[two[1], 0]
    # the flag is exact for one touched mover: a mover of the batch that stays where it is does not raise it ...
    w, b, two = pair_world(cuda_device, far)
    out = slide_and_fetch(w, two, np.array([[30, 0, 0], [0, 0, 0]], np.float32), [0, 0], grid=False)
    assert list(out["flags"]) == [0, 0] and out["push_hit"][0, 0] == two[1] and same_bits(out["pos"][two[1]], p0[two[1]])
    # ... and a superset with several: between two movers of the batch that both stay, it is raised all the same
    w, b, two = pair_world(cuda_device, far, third=True)
    three = np.array([0, 1, 2], np.uint32)
    q0 = w.pos.cpu().numpy().copy()
    out = slide_and_fetch(w, three, np.array([[0, 0, 0], [0, 0, 0], [0, 0, -30]], np.float32), [0, 0, 0], grid=False)
    assert list(out["flags"]) == [0, 0, _lib.SLIDE_MOVED_TARGET] and same_bits(out["pos"][:2], q0[:2])
    assert out["first_frac"][2, 0] < 1 and out["push_hit"][2, 0] in (0, 1)
    alone = pair_world(cuda_device, far, third=True)[0]
    one = slide_and_fetch(alone, three[2:], np.array([[0, 0, -30]], np.float32), [0], grid=False)
    assert list(one["flags"]) == [0] and same_bits(one["pos"][2], out["pos"][2])       # the same move, without the flag
    # a body listed twice: every listing INVALID, and it stays; the other mover of the batch moves
    w, b, two = pair_world(cuda_device, far)
    out = slide_and_fetch(w, np.array([two[0], two[0], two[1]], np.uint32), np.array([[0, 30, 0]] * 3, np.float32), [0, 0, 0], grid=False)
    assert list(out["flags"]) == [_lib.SLIDE_INVALID, _lib.SLIDE_INVALID, 0]
    assert same_bits(out["pos"][two[0]], p0[two[0]]) and abs(out["pos"][two[1], 1] - 1.0) < 1e-6
    assert (out["first_frac"][:2] == 1).all() and (out["push_hit"][:2] == -1).all()
    # NaN velocity and a body past the set: INVALID
    w, b, two = pair_world(cuda_device, far)
    out = slide_and_fetch(w, np.array([two[0], 99], np.uint32), np.array([[np.nan, 1, 0], [1, 1, 1]], np.float32), [0, 1], grid=False)
    assert list(out["flags"]) == [_lib.SLIDE_INVALID] * 2 and same_bits(out["pos"], p0) and np.isnan(out["velocity"][0, 0])
    # an OTHER static without a mesh under the path: UNRESOLVED, nothing moves, the velocity stays
    w, b, two = pair_world(cuda_device, [[-0.2, 0.2, -3, -2, -1, 1]], kinds=[_lib.GEOM_OTHER])
    out = slide_and_fetch(w, two, np.array([[0, -90, 0], [0, -90, 0]], np.float32), [1, 1], grid=False)
    assert list(out["flags"]) == [_lib.SLIDE_UNRESOLVED, 0]
    assert same_bits(out["pos"][two[0]], p0[two[0]]) and out["velocity"][0, 1] == -90 and abs(out["pos"][two[1], 1] + 3.0) < 1e-6
    f, _n, h, fl = fetch(w.sweep_capsules_grid(two, np.array([[0, -3, 0], [0, -3, 0]], np.float32), grid=False))
    assert list(fl) == [_lib.SLIDE_UNRESOLVED, 0] and (f == 1).all() and (h == -1).all()


def test_index_and_mesh_set_refusals(cuda_device):
    w, b, statics = world_a(cuda_device)
    movers, v, air = sr.movers_a(b["n"])
    d = (v[:8] * 0.01).astype(np.float32)
    for call in (lambda: w.sweep_capsules_grid(movers[:8], d, grid=True), lambda: w.slide(movers[:8], v[:8], air[:8], DT, grid=True)):
        w.bp_invalidate()
        with pytest.raises(_lib.ClapGpuError):
            call()                                              # no index
        w.bp_index()
        w.broadphase()
        with pytest.raises(_lib.ClapGpuError):
            call()                                              # a collide since the index: as the ray cast refuses
    w.bp_index()
    w.sweep_capsules_grid(movers[:8], d, grid=True)             # the sweep leaves the index valid ...
    w.sweep_capsules_grid(movers[:8], d, grid=True)
    w.slide(movers[:8], v[:8], air[:8], DT, grid=True)          # ... the slide clears it
    with pytest.raises(_lib.ClapGpuError):
        w.sweep_capsules_grid(movers[:8], d, grid=True)
    # a bp created for another static count, a mesh set for another static count
    other = physics.PhysWorld(b, statics[:30], device=cuda_device)
    other.bp_index()
    w._bp, other._bp = other._bp, w._bp
    with pytest.raises(_lib.ClapGpuError):
        w.sweep_capsules_grid(movers[:8], d, grid=True)
    w._bp, other._bp = other._bp, w._bp
    sc, _b = scene_b(cuda_device)
    w._meshes = sc.w._meshes
    try:
        with pytest.raises(_lib.ClapGpuError):
            w.sweep_capsules_grid(movers[:8], d, grid=False)
        with pytest.raises(_lib.ClapGpuError):
            w.slide(movers[:8], v[:8], air[:8], DT, grid=False)
    finally:
        w._meshes = None


def test_slide_in_a_captured_graph(cuda_device):
    """captured with the default queue count; replayed twice on the restored and re-indexed state, and once over an index
    the boxes were binned again since: the eager call's bytes"""
    sc, b = scene_b(cuda_device)
    w = sc.w
    movers, v, air = sr.movers_b(b)
    w.bodies_aabb()
    before = snapshot(w)
    eager = slide_and_fetch(w, movers, v, air)
    restore(w, before)
    w.bp_index()
    dev = w.device
    vel0 = torch.from_numpy(v).to(dev)
    body_d = torch.from_numpy(movers.view(np.int32)).to(dev)
    air_d = torch.from_numpy(np.ascontiguousarray(air, np.uint8)).to(dev)
    vel = vel0.clone()
    n = len(movers)
    res = (vel, torch.ones((n, 2), dtype=torch.float32, device=dev), torch.full((n, 6), -1, dtype=torch.int32, device=dev),
           torch.zeros(n, dtype=torch.int32, device=dev))
    scratch = torch.zeros(w.n, dtype=torch.int32, device=dev)
    sl = _lib.Slide(n, body_d.data_ptr(), vel.data_ptr(), air_d.data_ptr(), res[1].data_ptr(), res[2].data_ptr(), res[3].data_ptr())
    sg = w.static_geoms()
    keep = (body_d, air_d, vel)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _lib.check(_lib.lib().clapgpu_characters_slide(physics._stream(), w._bp, C.byref(w._desc), C.byref(sg), w._meshes, DT,
                                                           C.byref(sl), scratch.data_ptr()), "clapgpu_characters_slide")
    torch.cuda.current_stream().wait_stream(side)
    def replay(prepare):
        restore(w, before)
        prepare()
        keep[2].copy_(vel0)
        g.replay()
        torch.cuda.synchronize()
        return dict(pos=w.pos.cpu().numpy().copy(), lvel=w.lvel.cpu().numpy().copy(), velocity=res[0].cpu().numpy(),
                    first_frac=res[1].cpu().numpy(), push_hit=res[2].cpu().numpy(), flags=res[3].cpu().numpy())

    for trial in range(2):                                  # index between replays as between eager calls: the slide clears it
        got = replay(w.bp_index)
        for k in eager:
            assert same_bits(eager[k], got[k]), (trial, k)
    # boxes binned again since the index -- a collide the captured call's grid view knows nothing of: the device's bin
    # count has moved on, so every sweep of the replay scans every geom instead.  The brute-force path's bytes
    restore(w, before)
    brute = slide_and_fetch(w, movers, v, air, grid=False)

    def stale():
        w.bp_index()
        w.broadphase()
    got = replay(stale)
    for k in brute:
        assert same_bits(brute[k], got[k]) and same_bits(eager[k], got[k]), ("stale index", k)


# ------------------------------------------------------------------------------------------------- characters
def test_characters_fall_walk_and_stay_on_the_terrain(cuda_device):
    """64 characters with bodies above scene B's terrain, 120 frames of character_move's order: ground collide -> gravity
    on the host's velocity array -> slide -> clapgpu_characters_update.  They end grounded, their feet (pos.y - yoffset)
    within a capsule radius of the terrain's closed-form height, every pos finite, the entities where the bodies are"""
    from clap_amd import characters, entities
    n, pool = 64, 256
    vx, idx = synth.heightfield(33, 32.0)
    bv, bi = synth.box_mesh()
    ident = [0.0, 0.0, 0.0, 1.0]
    meshes = [(vx, idx, 1.0, [0.0, 0.0, 0.0], ident), (bv, bi, 4.0, [40.0, 0.0, 16.0], ident)]
    R = rng(91)
    b = synth.capsule_bodies(pool, box=32.0, seed=91)
    b["quat"][:] = [1.0, 0.0, 0.0, 0.0]                     # characters do not tumble
    b["pos"][:, 0], b["pos"][:, 2] = R.uniform(8, 24, pool), R.uniform(8, 24, pool)
    b["pos"][:, 1] = sr.ground_b(b["pos"][:, 0], b["pos"][:, 2]) + b["yoffset"] + R.uniform(0.5, 2.5, pool)
    b["lvel"][:] = 0
    b["avel"][:] = 0
    sc = Scene(cuda_device, b, meshes, cap=(1 << 16, 1 << 16))
    w = sc.w
    # the characters: 64 bodies whose geom ends well above their feet (pos.y - yoffset), as an upright character's from
    # phys_geom_capsule_new does (a quarter of its height above them).  The ground ray reaches ray_len below the feet; a
    # geom that reaches down to the feet comes to rest on the sweep's back-up, up to half a radius above the ground, where
    # that ray never finds it -- in the reference as here.  The rest of the pool stands far away
    below = w.pos.cpu().numpy()[:, 1] - w.aabb.cpu().numpy()[:, 2]
    bodies = np.flatnonzero(below <= 0.6 * b["yoffset"])[:n].astype(np.uint32)
    assert len(bodies) == n
    away = np.setdiff1d(np.arange(pool), bodies)
    w.pos[torch.from_numpy(away).to(w.device)] = torch.tensor([-500.0, -500.0, -500.0], dtype=torch.float64, device=w.device)
    w.bodies_aabb()
    yoff, radius = b["yoffset"][bodies], b["radius"][bodies]
    feed = synth.character_feed(n, seed=92)
    feed["hist_pos"][:] = 0                                 # an empty history: nothing to teleport back to
    feed["hist_head"][:] = 0
    feed["hist_wrapped"][:] = 0
    feed["airborne"][:] = 1
    feed["body"] = bodies.astype(np.int32)
    feed["entity"] = np.arange(n, dtype=np.uint32)
    scene = synth.pad_levels(synth.entities_flat(n, seed=1))
    scene["pos_scale"] = scene["pos_scale"].copy()
    scene["pos_scale"][:n, :3] = (b["pos"][bodies] - np.stack([np.zeros(n), yoff, np.zeros(n)], 1)).astype(np.float32)
    batch = entities.EntityBatch(scene, cuda_device)
    cf = characters.CharacterFeed(feed, cuda_device)
    ray_off = np.asarray(yoff, float) * 0.8
    vel = np.zeros((n, 3), np.float32)
    vel[:, 0], vel[:, 2] = R.uniform(-1.5, 1.5, n), R.uniform(-1.5, 1.5, n)
    airborne = np.ones(n, np.uint8)
    dt = 1.0 / 60.0
    landed = np.zeros(n, bool)
    for frame in range(120):
        w.bp_index()
        grounded, _nrm, _dist, _hit, gflags = fetch(w.ground_collide(bodies, ray_off, airborne == 0, grid=True))
        assert not (gflags & (_lib.RAY_INVALID | _lib.RAY_UNRESOLVED)).any(), (frame, gflags)
        airborne = (grounded == 0).astype(np.uint8)
        landed |= grounded != 0
        vel[:, 1] = np.where(airborne != 0, vel[:, 1] - np.float32(9.8 * dt), 0).astype(np.float32)   # the host's gravity
        w.bp_index()
        v2, _ff, _push, flags = fetch(w.slide(bodies, vel, airborne, dt, grid=True))
        assert not (flags & (_lib.SLIDE_INVALID | _lib.SLIDE_UNRESOLVED)).any(), (frame, flags)
        vel = v2.copy()
        cf.set_airborne(airborne)
        cf.character_update(batch, w)
    w.bp_index()
    grounded = fetch(w.ground_collide(bodies, ray_off, airborne == 0, grid=True))[0]
    pos = w.pos.cpu().numpy()[bodies]
    assert np.isfinite(pos).all()
    assert grounded.all() and landed.all(), (grounded, landed)
    feet = pos[:, 1] - yoff
    off = np.abs(feet - sr.ground_b(pos[:, 0], pos[:, 2]))
    assert (off <= radius).all(), (off.max(), off.argmax(), radius[off.argmax()])
    cf.character_update(batch, w)
    ps = batch.pos_scale.cpu().numpy()[:n, :3]
    exp = np.stack([pos[:, 0], pos[:, 1] - yoff, pos[:, 2]], 1).astype(np.float32)
    assert same_bits(ps, exp)
