"""GPU: clapgpu_bodies_islands against tests/islandref.py.  Pairs and nc are synthetic arrays uploaded directly (the
entry point reads nothing else of the contact records); every comparison is == on bit patterns."""
import ctypes as C

import numpy as np
import pytest
import torch

from clap_amd import _lib, physics, synth
import islandref as ir
import pushref as pr
from meshscene import same_bits, rng

pytestmark = pytest.mark.gpu
H = 1.0 / 120.0
KEYS = ("bflags", "adis_steps_left", "adis_time_left", "lvel", "avel")


def put(w, name, a):
    a = np.ascontiguousarray(a)
    getattr(w, name).copy_(torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(w.device))


def put_state(w, st):
    for k in KEYS:
        put(w, k, st[k])


def put_pairs(w, pairs, nc, total=None):
    w.alloc_contacts()
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    m = len(pairs)
    assert m <= w.capacity
    rec = np.zeros((m, 160), np.uint8)
    rec[:, 100:104] = np.ascontiguousarray(nc, "<u4").view(np.uint8).reshape(m, 4)       # clapgpu_contact2.nc
    if m:
        w.pairs[:m] = torch.from_numpy(pairs.view(np.int32)).to(w.device)
        w.contact2_buf[:m] = torch.from_numpy(rec).to(w.device)
    w.pair_total[0] = m if total is None else total


def sleepers(b, awake):
    """every body asleep with spent counters and no velocity, but `awake`; HAS_JOINT on the awake ones"""
    n = int(b["n"])
    st = pr.step_state(b)
    asleep = ~np.isin(np.arange(n), awake)
    st["bflags"][asleep] |= pr.DISABLED
    st["bflags"][~asleep] |= pr.HAS_JOINT
    st["adis_steps_left"][asleep] = 0
    st["adis_time_left"][asleep] = -0.5
    st["lvel"][asleep] = 0
    st["avel"][asleep] = 0
    return st


def assert_islands(w, st, island, woken, want_island, want_woken, what=""):
    torch.cuda.synchronize()
    for k in KEYS:
        got = getattr(w, k).cpu().numpy()
        assert same_bits(got.view(np.uint32) if k == "bflags" else got, st[k]), (what, k)
    if island is not None:
        assert np.array_equal(island.cpu().numpy().view(np.uint32), want_island), (what, "island")
    if woken is not None:
        assert int(woken.item()) == want_woken, (what, "woken", int(woken.item()), want_woken)


def chain_pairs(order):
    p = np.stack([order[:-1], order[1:]], 1)
    p = np.stack([p.min(1), p.max(1)], 1)
    return p[np.lexsort((p[:, 1], p[:, 0]))].astype(np.uint32)             # ascending (i, j), as the broadphase emits


def run_against_ref(w, b, st, pairs, nc, what="", **kw):
    put_state(w, st)
    put_pairs(w, pairs, nc)
    island, woken = w.islands(H, **kw)
    want_island, want_woken = ir.islands(st, pairs, nc, h=H)
    assert_islands(w, st, island, woken, want_island, want_woken, what)
    return want_island, want_woken


# ------------------------------------------------------------------------------------------------- graphs
def test_long_chain_wakes_from_one_end(cuda_device):
    n = 20_000
    b = synth.capsule_bodies(n, box=64.0, seed=9)
    perm = rng(5).permutation(n)
    pairs = chain_pairs(perm)
    assert len(pairs) == n - 1 and len(pairs) > 8 * 256
    nc = np.where(np.arange(n - 1) % 3 == 0, 2, 1).astype(np.uint32)
    w = physics.PhysWorld(b, None, device=cuda_device)
    seen = []
    for trial in range(2):
        st = sleepers(b, [perm[0]])
        island, woken = run_against_ref(w, b, st, pairs, nc, trial)
        assert woken == n - 1 and not island.any() and not (st["bflags"] & pr.DISABLED).any()
        assert (st["adis_steps_left"][np.arange(n) != perm[0]] == 0).all()          # the flag alone: counters stay spent
        torch.cuda.synchronize()
        seen.append((w.island.cpu().numpy().copy(), w.bflags.cpu().numpy().copy()))
    assert same_bits(seen[0][0], seen[1][0]) and same_bits(seen[0][1], seen[1][1])


def test_star_with_the_hub_last(cuda_device):
    n = 5001
    b = synth.capsule_bodies(n, box=32.0, seed=10)
    pairs = np.stack([np.arange(n - 1), np.full(n - 1, n - 1)], 1).astype(np.uint32)    # every hook starts at parent[hub]
    w = physics.PhysWorld(b, None, device=cuda_device)
    island, woken = run_against_ref(w, b, sleepers(b, [n - 1]), pairs, np.ones(n - 1, np.uint32))
    assert woken == n - 1 and not island.any()


def test_components_without_an_awake_body_sleep_on(cuda_device):
    chains, length = 600, 7
    n = chains * length
    b = synth.capsule_bodies(n, box=32.0, seed=11)
    perm = rng(6).permutation(n).reshape(chains, length)
    pairs = np.concatenate([chain_pairs(c) for c in perm])
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    st = sleepers(b, perm[300:, 3])                                        # one awake member in the last 300 chains
    before = {k: st[k].copy() for k in KEYS}
    w = physics.PhysWorld(b, None, device=cuda_device)
    island, woken = run_against_ref(w, b, st, pairs, np.ones(len(pairs), np.uint32))
    assert woken == 300 * (length - 1)
    dead = perm[:300].ravel()
    torch.cuda.synchronize()
    for k in KEYS:                                                         # bit for bit what was uploaded
        got = getattr(w, k).cpu().numpy()
        assert same_bits((got.view(np.uint32) if k == "bflags" else got)[dead], before[k][dead]), k
    assert (before["bflags"][dead] & pr.DISABLED).all() and np.array_equal(island[perm[:300]].min(1), perm[:300].min(1))


def test_pairs_that_must_not_link(cuda_device):
    n = 1200
    b = synth.capsule_bodies(n, box=32.0, seed=12)
    pairs = np.stack([np.arange(n - 1), np.arange(1, n)], 1).astype(np.uint32)
    nc = np.ones(n - 1, np.uint32)
    nc[199] = 0                                                            # 0 .. 199 | 200 .. 399: cut by a pair that does not touch
    nc[399] = 0
    nc[599] = ir.CONTACT_DEEP                                              # 400 .. 599 | 600 .. 799: cut by a DEEP pair
    nc[799] = 0
    bad = np.array([[5, 5], [3, n + 7], [0xffffffff, 2], [250, 250], [n, n + 1]], np.uint32)   # self, out of range: nc 1
    pairs, nc = np.concatenate([pairs[:300], bad, pairs[300:]]), np.concatenate([nc[:300], np.ones(5, np.uint32), nc[300:]])
    awake = [0, 400, 800]
    w = physics.PhysWorld(b, None, device=cuda_device)
    st = sleepers(b, awake)
    island, woken = run_against_ref(w, b, st, pairs, nc, "cuts")
    asleep = (st["bflags"] & pr.DISABLED) != 0
    assert asleep[200:400].all() and asleep[600:800].all() and asleep.sum() == 400 and woken == 800 - 3
    # *pair_total above capacity: pairs from `capacity` on are not read (the buffers hold them; the call is told less)
    cut = len(pairs) - 150                                                 # inside 800 .. 1199
    st = sleepers(b, awake)
    put_state(w, st)
    put_pairs(w, pairs, nc, total=len(pairs) + 1000)
    _lib.check(_lib.lib().clapgpu_bodies_islands(physics._stream(), C.byref(w._desc), C.byref(w.world), H, w.pairs.data_ptr(),
                                                 w.pair_total.data_ptr(), cut, w.contact2_buf.data_ptr(),
                                                 w.island_scratch.data_ptr(), w.island.data_ptr(), w.island_woken.data_ptr()),
               "clapgpu_bodies_islands")
    want_island, want_woken = ir.islands(st, pairs, nc, h=H, total=len(pairs) + 1000, capacity=cut)
    assert_islands(w, st, w.island[:n], w.island_woken, want_island, want_woken, "capacity")
    assert ((st["bflags"][1050:] & pr.DISABLED) != 0).all() and ((st["bflags"] & pr.DISABLED) != 0).sum() >= 400 + 100


def test_edge_sizes_and_null_outputs(cuda_device):
    b1 = synth.capsule_bodies(1, box=4.0, seed=13)
    w1 = physics.PhysWorld(b1, None, device=cuda_device)
    for awake in ([0], []):
        run_against_ref(w1, b1, sleepers(b1, awake), np.array([[0, 0]], np.uint32), np.ones(1, np.uint32), ("n=1", awake))
    n = 65
    b = synth.capsule_bodies(n, box=8.0, seed=14)
    w = physics.PhysWorld(b, None, device=cuda_device)
    pairs, nc = chain_pairs(rng(7).permutation(n)), np.ones(n - 1, np.uint32)
    island, woken = run_against_ref(w, b, sleepers(b, [64]), pairs, nc, "n=65")
    assert woken == 64
    run_against_ref(w, b, sleepers(b, [64]), pairs[:0], nc[:0], "no pairs")             # *pair_total == 0
    st = sleepers(b, [64])
    put_state(w, st)
    put_pairs(w, pairs, nc)
    w.island.fill_(-1)
    w.island_woken.fill_(-1)
    assert w.islands(H, want_island=False, want_woken=False) == (None, None)
    ir.islands(st, pairs, nc, h=H)
    assert_islands(w, st, None, None, None, None, "NULL outputs")
    assert (w.island == -1).all().item() and int(w.island_woken.item()) == -1
    L = _lib.lib()                                                          # argument checks
    args = lambda **k: [physics._stream(), C.byref(w._desc), C.byref(w.world), H, k.get("pairs", w.pairs.data_ptr()),
                        k.get("total", w.pair_total.data_ptr()), w.capacity, w.contact2_buf.data_ptr(),
                        k.get("scratch", w.island_scratch.data_ptr()), None, None]
    assert L.clapgpu_bodies_islands(*args(scratch=None)) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_bodies_islands(*args(scratch=w.island_scratch.data_ptr() + 4)) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_bodies_islands(*args(total=None)) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_bodies_islands(*args(pairs=None)) == _lib.ERR_INVALID_ARGUMENTS
    assert _lib.bodies_islands_scratch_bytes(n) >= 4 * n


# ------------------------------------------------------------------------------------------------- with the step
@pytest.mark.parametrize("samples", [1, 4])
def test_a_body_put_to_sleep_beside_an_awake_one_is_stepped(samples, cuda_device):
    b = synth.capsule_bodies(2, box=4.0, seed=15)
    b["adis_average_samples"] = samples
    b["lvel"][:] = b["avel"][:] = 0
    b["lvel"][1] = [5.0, 0, 0]                                             # B moves
    b["adis_steps_left"][0] = 1                                            # A is idle and one step from sleep
    b["bflags"][:] = pr.AUTO_DISABLE | pr.HAS_JOINT                        # no gyroscopic term: A's velocity is gravity's alone
    g = np.array(pr.WORLD["gravity"])
    want_v = (H * (1.0 / b["mass"][0])) * (b["mass"][0] * g)               # one step of gravity from zero ...
    want_lvel = want_v * (1.0 - pr.WORLD["linear_damping"])                # ... which the world's damping then scales
    assert (want_v * want_v).sum() > pr.WORLD["linear_damping_threshold_sq"]
    for touching in (True, False):
        w = physics.PhysWorld(b, None, device=cuda_device)
        if samples > 1:
            w.adis_counter.fill_(samples - 1)                              # this sample fills the ring
        put_pairs(w, np.array([[0, 1]], np.uint32), np.ones(1, np.uint32), total=1 if touching else 0)
        island, woken = w.islands(H)
        w.world_step(H)
        d = w.download()
        assert int(d["adis_steps_left"][0]) <= 0 and d["adis_time_left"][0] <= 0, "A's counters are spent"
        assert not d["bflags"][1] & pr.DISABLED and int(d["adis_steps_left"][1]) == 30
        if touching:                                                       # asleep, woken in the same step, integrated from rest
            assert int(woken.item()) == 1 and island.cpu().tolist() == [0, 0]
            assert not d["bflags"][0] & pr.DISABLED
            assert same_bits(d["lvel"][0], want_lvel) and same_bits(d["pos"][0], b["pos"][0] + H * want_v)
        else:                                                              # its joint was with a static: no pair
            assert int(woken.item()) == 0 and island.cpu().tolist() == [0, 1]
            assert d["bflags"][0] & pr.DISABLED and not d["lvel"][0].any() and not d["avel"][0].any()
            assert same_bits(d["pos"][0], b["pos"][0])
        assert not (d["bflags"] & pr.HAS_JOINT).any()


def test_nobody_asleep_the_pass_changes_nothing(cuda_device):
    n = 4096
    b = synth.capsule_bodies(n, box=16.0, seed=16, resting_frac=0.2)
    b["adis_steps_left"][:] = rng(3).integers(2, 30, n)
    both = [physics.PhysWorld(b, None, device=cuda_device) for _ in range(2)]
    for k, w in enumerate(both):
        w.broadphase()
        w.contacts_geoms()
        if k == 0:
            _island, woken = w.islands(H)
        w.world_step(H)
    a, z = both[0].download(), both[1].download()
    assert int(woken.item()) == 0 and int(both[0].contact2_total.item()) >= 100 and a["pair_total"] <= both[0].capacity
    assert (a["adis_steps_left"] != b["adis_steps_left"]).any()
    for k in z:
        assert same_bits(np.asarray(a[k]), np.asarray(z[k])), k


# ------------------------------------------------------------------------------------------------- the frame
def row_scene():
    """64 sleeping capsules in a row, each overlapping the next, resting in a floor slab; body 64 is awake and overlaps
    the end of the row"""
    nb = 65
    b = synth.capsule_bodies(nb, box=4.0, seed=17)
    assert b["radius"].min() >= 0.1                                        # centres 0.15 apart: neighbours overlap, whatever their axes
    b["pos"][:] = np.stack([2.0 + 0.15 * np.arange(nb), np.full(nb, 1.08), np.full(nb, 2.0)], 1)   # 0.02 or more into the slab's top at y = 1
    b["lvel"][:64] = b["avel"][:64] = 0
    b["bflags"][:64] |= pr.DISABLED
    b["adis_steps_left"][:64] = 0
    b["lvel"][64] = [0.0, 0.0, 1.0]
    statics = np.array([[0.0, 14.0, 0.0, 1.0, 0.0, 4.0], [20.0, 21.0, 0.0, 1.0, 0.0, 1.0]])
    return b, statics


def frame_world(cuda_device, islands):
    from clap_amd import entities, frame, tiler
    raw = synth.entities_flat(600, seed=5)
    scene, tl = tiler.tiled_scene(raw)
    roots = tl["slot_of"][np.flatnonzero(raw["parent"] < 0)]
    scene["model_lod"] = np.asarray([[0, 3]], np.uint8)
    b, statics = row_scene()
    b["body_entity"] = roots[:b["n"]].astype(np.int32)
    batch = entities.EntityBatch(scene, cuda_device)
    world = physics.PhysWorld(b, statics, pair_capacity=8192, device=cuda_device)
    loop = frame.FrameLoop(batch, synth.camera(pos=(0, 10, 60)), world=world, contacts=True, islands=islands)
    return b, world, loop


def manual_substep(w):
    w.broadphase()
    w.contacts_geoms_both()
    out = w.islands(H)
    w.world_step(H)
    return out


STATE = ("pos", "quat", "lvel", "avel", "bflags", "adis_steps_left", "adis_time_left", "aabb", "axis", "geom_records")


def assert_same_world(a, z, what):
    da, dz = a.download(), z.download()
    for k in dz:
        assert same_bits(np.asarray(da[k]), np.asarray(dz[k])), (what, k)
    assert same_bits(a.island.cpu().numpy(), z.island.cpu().numpy()), (what, "island")
    assert int(a.island_woken.item()) == int(z.island_woken.item()), (what, "woken")


def test_frame_wakes_a_sleeping_row(cuda_device):
    b, manual, _ = frame_world(cuda_device, True)
    island, woken = manual_substep(manual)
    d = manual.download()
    assert int(woken.item()) == 64 and not (d["bflags"] & pr.DISABLED).any(), "the whole row wakes in the first substep"
    assert not island.cpu().numpy().any() and d["pair_total"] >= 64 and d["static_pair_total"] >= 64
    assert not same_bits(d["pos"][:64], b["pos"][:64])
    for _ in range(3):
        manual_substep(manual)
    _, framed, loop = frame_world(cuda_device, True)
    loop._issue(0.0, 4)
    assert_same_world(framed, manual, "frame of 4 substeps")
    # the same frame without the pass: the row sleeps on, where it was
    _, plain, loop0 = frame_world(cuda_device, False)
    loop0._issue(0.0, 4)
    d0 = plain.download()
    assert (d0["bflags"][:64] & pr.DISABLED).all() and not d0["bflags"][64] & pr.DISABLED
    assert same_bits(d0["pos"][:64], b["pos"][:64]) and getattr(plain, "island_scratch", None) is None


def test_frame_with_islands_in_a_captured_graph(cuda_device):
    _, eager, loop_e = frame_world(cuda_device, True)
    loop_e._issue(0.0, 1)
    _, w, loop = frame_world(cuda_device, True)
    saved = {k: getattr(w, k).clone() for k in STATE}
    loop.capture()
    for trial in range(2):
        for k in STATE:
            getattr(w, k).copy_(saved[k])
        w.bp_invalidate()
        w.island_woken.fill_(-1)
        loop.clap_frame_replay(0.0)
        assert_same_world(w, eager, ("replay", trial))
    assert int(w.island_woken.item()) == 64
