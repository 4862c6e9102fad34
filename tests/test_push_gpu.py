"""GPU: clapgpu_bodies_push and the force path of clapgpu_bodies_step against tests/pushref.py.  Every comparison is ==
on bit patterns: the same arithmetic in the same order, so no tolerance.  (The restatement itself: test_push.py, which
also walks it against the oracle's step where there are no forces.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from clap_amd import _lib, physics, synth
import pushref as pr
import slideref as sr
from meshscene import Scene, fetch, same_bits, rng

pytestmark = pytest.mark.gpu
DT = 1.0 / 30.0
H = 1.0 / 120.0
PUSH_KEYS = ("facc", "bflags", "adis_steps_left", "adis_time_left")


def dev_push_state(w):
    torch.cuda.synchronize()
    return dict(facc=w.facc.cpu().numpy()[:w.n], bflags=w.bflags.cpu().numpy().view(np.uint32),
                adis_steps_left=w.adis_steps_left.cpu().numpy(), adis_time_left=w.adis_time_left.cpu().numpy())


def assert_push_equal(w, want, pushed, want_pushed, what=""):
    got = dev_push_state(w)
    for k in PUSH_KEYS:
        assert same_bits(got[k], want[k]), (what, k)
    assert np.array_equal(pushed.cpu().numpy().view(np.uint32), want_pushed), (what, "pushed")


def put(w, name, a):
    t = getattr(w, name)
    a = np.ascontiguousarray(a)
    t.copy_(torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(w.device))


def sleepy_start(w, b, seed, awake=()):
    """the bodies asleep with spent counters (all but `awake`; without it, four in ten), all with something in their
    accumulators: what the push must wake, reset and add to.  Returns the host copy of that state."""
    R = rng(seed)
    n = int(b["n"])
    st = pr.push_state(b, R.normal(0, 3.0, (n, 3)))
    asleep = ~np.isin(np.arange(n), awake) if len(awake) else R.random(n) < 0.4
    st["bflags"][asleep] |= pr.DISABLED
    st["adis_steps_left"][asleep] = -1
    st["adis_time_left"][asleep] = -0.25
    for k in PUSH_KEYS:
        put(w, k, st[k])
    return st


# ------------------------------------------------------------------------------------------------- slide, then push
def slide_then_push(w, b, movers, v, air):
    w.enable_forces()
    w.world.adis_time = 0.125                                            # not the default: the reset must come from the world
    st = sleepy_start(w, b, 7, awake=movers)                          # everything the movers can walk into sleeps
    w.bodies_aabb()
    w.bp_index()
    vel, _ff, push, flags, pushed = w.slide_and_push(movers, v, air, DT)
    push_h, flags_h = push.cpu().numpy(), flags.cpu().numpy().view(np.uint32)
    assert not same_bits(vel.cpu().numpy(), v), "the slide zeroed some velocity[1]: the push must not use those"
    want_pushed = pr.push(st, b["mass"], movers, v, push_h, flags_h, world=dict(pr.WORLD, adis_time=0.125))
    assert want_pushed.sum() >= 5 and ((push_h >= 0).any(1) & (flags_h == 0)).sum() >= 5
    assert_push_equal(w, st, pushed, want_pushed)
    hit = want_pushed > 0
    woke = hit & ~np.isin(np.arange(w.n), movers)
    assert woke.sum() >= 5 and not (st["bflags"][hit] & 1).any() and (st["bflags"][~hit & ~np.isin(np.arange(w.n), movers)] & 1).all()
    assert (st["adis_steps_left"][woke] == 30).all() and (st["adis_time_left"][woke] == 0.125).all()
    return st, push_h, flags_h, want_pushed


def test_slide_and_push_scene_a(cuda_device):
    b, statics = sr.scene_a()
    w = physics.PhysWorld(b, statics, device=cuda_device)
    movers, v, air = sr.movers_a(b["n"])
    st, push_h, flags_h, want_pushed = slide_then_push(w, b, movers, v, air)
    # flagged movers push nothing: the same batch with every mover flagged leaves the state alone
    before = dev_push_state(w)
    pushed = w.bodies_push(movers, v, push_h, np.full(len(movers), _lib.SLIDE_MOVED_TARGET, np.uint32))
    assert_push_equal(w, before, pushed, np.zeros(w.n, np.uint32), "all flagged")
    # no flags array: every mover pushes, the flagged ones too
    want = pr.push(before, b["mass"], movers, v, push_h, None, world=dict(pr.WORLD, adis_time=0.125))
    assert_push_equal(w, before, w.bodies_push(movers, v, push_h, None), want, "flags NULL")


def test_slide_and_push_scene_b(cuda_device):
    b, meshes = sr.scene_b()
    sc = Scene(cuda_device, b, meshes, cap=(1 << 20, 1 << 20))
    movers, v, air = sr.movers_b(b)
    slide_then_push(sc.w, b, movers, v, air)


def test_push_ignores_bad_slots_and_movers(cuda_device):
    b = synth.capsule_bodies(64, box=8.0, seed=3)
    w = physics.PhysWorld(b, None, device=cuda_device, forces=True)
    st = sleepy_start(w, b, 9)
    pusher = np.array([0, 5, 64, 0xffffffff, 7], np.uint32)              # movers 2 and 3: no such body
    v = rng(4).normal(0, 5, (5, 3)).astype(np.float32)
    ph = np.array([[3, -1, 64, 3, -7, 2 ** 31 - 1], [3, 3, 3, 3, 3, 3], [1, 1, 1, 1, 1, 1], [2, 2, 2, 2, 2, 2],
                   [-1, -1, -1, -1, -1, 63]], np.int32)
    want = pr.push(st, b["mass"], pusher, v, ph)
    assert want[3] == 8 and want[63] == 1 and want.sum() == 9
    assert_push_equal(w, st, w.bodies_push(pusher, v, ph), want)
    # one mover alone (the single-block sort), and no pushed[] array
    want = pr.push(st, b["mass"], pusher[:1], v[:1], ph[:1])
    assert w.bodies_push(pusher[:1], v[:1], ph[:1], want_pushed=False) is None
    got = dev_push_state(w)
    for k in PUSH_KEYS:
        assert same_bits(got[k], st[k]), k


# ------------------------------------------------------------------------------------------------- the order
def test_crowd_sum_is_made_in_the_reference_order(cuda_device):
    """16 384 movers (98 304 slots, 384 workgroups of the key and apply launches) around 96 bodies.  On the CPU first:
    the scene has power -- at least 32 bodies take pushes from several movers and the reversed order gives other bits
    -- then the device equals the in-order sum for every body, twice (the second call adds to the first's sums)."""
    n_movers, n_targets = 16384, 96
    mass, pusher, v, ph = pr.crowd(n_movers, n_targets, seed=41)
    nb = len(mass)
    b = synth.sphere_bodies(nb, box=64.0, seed=6)
    b["mass"] = mass
    movers_of = [set() for _ in range(n_targets)]
    for k, h in zip(*np.nonzero(ph >= 0)):
        movers_of[ph[k, h]].add(k)
    assert sum(len(m) >= 2 for m in movers_of) >= 32
    st, rev = pr.push_state(b), pr.push_state(b)
    want = pr.push(st, mass, pusher, v, ph)
    pr.push(rev, mass, pusher, v, ph, reverse=True)
    differ = (st["facc"].view(np.uint64) != rev["facc"].view(np.uint64)).any(1)
    assert differ.sum() >= 1, "the order shows in the bits"
    print("crowd: bodies whose reversed sum differs:", int(differ.sum()), "of", n_targets, "longest run", int(want.max()))
    w = physics.PhysWorld(b, None, device=cuda_device, forces=True)
    pushed = w.bodies_push(pusher, v, ph)
    assert_push_equal(w, st, pushed, want, "first call")
    assert not same_bits(dev_push_state(w)["facc"], rev["facc"])
    want2 = pr.push(st, mass, pusher, v, ph)
    assert_push_equal(w, st, w.bodies_push(pusher, v, ph), want2, "second call")


# ------------------------------------------------------------------------------------------------- wake-up, kinematic
def download_state(w):
    d = w.download()
    d["facc"] = w.facc.cpu().numpy()[:w.n]
    d["adis_time_left"] = w.adis_time_left.cpu().numpy()
    return d


def assert_step_equal(w, st, what=""):
    d = download_state(w)
    for k in ("pos", "quat", "lvel", "avel", "facc", "adis_time_left"):
        assert same_bits(d[k], st[k]), (what, k)
    assert np.array_equal(d["bflags"], st["bflags"]) and np.array_equal(d["adis_steps_left"], st["adis_steps_left"]), what


def test_push_wakes_a_body_the_step_put_to_sleep(cuda_device):
    b = synth.capsule_bodies(32, box=8.0, seed=5, resting_frac=1.0)        # no gravity, at rest
    b["lvel"][:] = b["avel"][:] = 0
    b["bflags"][16:] &= ~np.uint32(pr.NO_GRAVITY)                         # the other half falls and stays awake
    w = physics.PhysWorld(b, None, device=cuda_device, forces=True)
    st = pr.step_state(b)
    steps = 0
    while not (w.download()["bflags"][:16] & 1).all():                    # the contact pass sets HAS_JOINT every substep
        w.bflags |= 16
        st["bflags"] |= 16
        w.world_step(H)
        pr.step_forces(b, st, H)
        steps += 1
        assert steps <= 40
    assert steps == 30
    assert_step_equal(w, st, "asleep")
    assert (st["bflags"][:16] & 1).all() and not (st["bflags"][16:] & 1).any() and (st["adis_steps_left"][:16] <= 0).all()
    # a sleeper with something in its accumulator keeps it through a step
    w.facc[2] = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    st["facc"][2] = [1.0, 2.0, 3.0]
    w.world_step(H)
    pr.step_forces(b, st, H)
    assert_step_equal(w, st, "sleeper keeps facc")
    assert st["facc"][2].tolist() == [1.0, 2.0, 3.0]
    # mover 20 walks into sleepers 2 and 5
    pusher, v = np.array([20], np.uint32), np.array([[3.5, 0.25, -1.75]], np.float32)
    ph = np.array([[2, 5, -1, -1, -1, -1]], np.int32)
    ps = {k: st[k] for k in PUSH_KEYS}
    want = pr.push(ps, b["mass"], pusher, v, ph)
    pushed = w.bodies_push(pusher, v, ph)
    assert_push_equal(w, ps, pushed, want)
    assert not (st["bflags"][[2, 5]] & 1).any() and (st["adis_steps_left"][[2, 5]] == 30).all()
    assert (st["bflags"][[0, 1, 3, 4]] & 1).all()
    f5, pos5, m5 = st["facc"][5].copy(), st["pos"][5].copy(), b["mass"][5]
    w.world_step(H)
    pr.step_forces(b, st, H)
    assert_step_equal(w, st, "awake")
    d = download_state(w)
    lvel5 = (H * (1.0 / m5)) * (f5 + 0.0)                                 # body 5: NO_GRAVITY, from rest
    damp = lvel5 * (1.0 - 0.001) if (lvel5 * lvel5).sum() > 1e-4 else lvel5
    assert same_bits(d["pos"][5], pos5 + H * lvel5) and same_bits(d["lvel"][5], damp) and not d["facc"][[2, 5]].any()
    assert f5.any() and not d["facc"].any()


def test_pushed_kinematic_body_wakes_and_keeps_its_velocities(cuda_device):
    """with the world's linear damping off: a moving kinematic body is damped like any other (ODE damps what it steps)"""
    b = synth.capsule_bodies(16, box=8.0, seed=15)
    b["bflags"][[3, 4]] |= pr.KINEMATIC
    b["bflags"][3] |= pr.DISABLED
    w = physics.PhysWorld(b, None, device=cuda_device, forces=True)
    w.world.linear_damping = 0.0
    world = dict(pr.WORLD, linear_damping=0.0)
    st = pr.step_state(b)
    pusher, v = np.array([9, 10], np.uint32), np.array([[2.0, -1.0, 0.5], [0.3, 0.2, 0.1]], np.float32)
    ph = np.array([[3, 4, -1, -1, -1, -1], [-1, -1, -1, 3, -1, 8]], np.int32)
    ps = {k: st[k] for k in PUSH_KEYS}
    want = pr.push(ps, b["mass"], pusher, v, ph)
    assert_push_equal(w, ps, w.bodies_push(pusher, v, ph), want)
    assert not st["bflags"][3] & pr.DISABLED and st["bflags"][3] & pr.KINEMATIC and st["facc"][[3, 4, 8]].all()
    w.world_step(H)
    pr.step_forces(b, st, H, world)
    assert_step_equal(w, st)
    d = download_state(w)
    assert same_bits(d["lvel"][[3, 4]], b["lvel"][[3, 4]]) and same_bits(d["avel"][[3, 4]] + 0.0, b["avel"][[3, 4]] + 0.0)
    assert not same_bits(d["pos"][[3, 4]], b["pos"][[3, 4]]) and not d["facc"].any()
    assert not same_bits(d["lvel"][8], b["lvel"][8])


# ------------------------------------------------------------------------------------------------- the step
def test_step_with_forces_at_full_size(cuda_device):
    """262 144 capsule bodies, random forces on a tenth of them before each of 5 substeps, some asleep, some kinematic,
    resting ones holding a joint: the restatement's bits, accumulators included"""
    n = 262_144
    b = synth.capsule_bodies(n, box=64.0, seed=4, resting_frac=0.2)
    R = rng(17)
    b["bflags"][R.random(n) < 0.05] |= pr.KINEMATIC
    b["bflags"][R.random(n) < 0.05] |= pr.DISABLED
    b["adis_steps_left"][R.random(n) < 0.3] = 3                            # some fall asleep inside the run
    w = physics.PhysWorld(b, None, device=cuda_device, forces=True)
    st = pr.step_state(b)
    joint = ((b["bflags"] & pr.NO_GRAVITY) != 0) & (np.arange(n) % 2 == 0)
    joint_d = torch.from_numpy(np.flatnonzero(joint)).to(w.device)
    for s in range(5):
        f = np.zeros((n, 3))
        some = R.random(n) < 0.1
        f[some] = R.normal(0, 40.0, (int(some.sum()), 3))
        st["facc"] += f
        w.facc += torch.from_numpy(f).to(w.device)
        st["bflags"][joint] |= 16
        w.bflags[joint_d] |= 16
        if s % 2:
            w.world_step(H, prebin=True)                                   # the instantiation that bins too
        else:
            w.world_step(H)
        stepped = pr.step_forces(b, st, H)
        assert_step_equal(w, st, s)
    asleep = (st["bflags"] & 1) != 0
    assert st["facc"][asleep].any() and not st["facc"][~asleep].any(), "only sleepers keep their accumulators"
    assert asleep.sum() > (b["bflags"] & 1).sum() and stepped.sum() > n // 2
    from oracle import binding as ob                                       # the geoms of the final state
    g = dict(st, aabb=np.zeros((n, 6)), axis=np.zeros((n, 3)))
    ob.bodies_aabb(b, g)
    d = w.download()
    assert same_bits(d["aabb"], g["aabb"]) and same_bits(d["axis"], g["axis"])


@pytest.mark.parametrize("kind", ["spheres", "capsules"])
def test_step_without_accumulator_is_the_step_with_zeros_and_the_oracles(kind, cuda_device):
    from oracle import binding as ob
    from test_physics_gpu import _run_steps, _assert_state_equal
    n = 20_000
    b = (synth.sphere_bodies(n, box=32.0, seed=8, resting_frac=0.2) if kind == "spheres"
         else synth.capsule_bodies(n, box=32.0, seed=8, resting_frac=0.2))
    plain = physics.PhysWorld(b, None, device=cuda_device)
    zeros = physics.PhysWorld(b, None, device=cuda_device, forces=True)
    assert plain._desc.facc is None and zeros._desc.facc
    st = ob.bodies_state(b)
    ob.bodies_aabb(b, st)
    dts = (1 / 60, 0.004, 0.005, 1 / 30, 0.3, 1 / 144)
    total = _run_steps(b, plain, st, dts)
    assert total == 12
    _assert_state_equal(plain.download(), st)
    resting = (b["bflags"] & 4) != 0
    with_joint = resting & (np.arange(n) % 2 == 0)
    _run_steps(b, plain, st, [1 / 120] * 31, joint_mask=with_joint)
    _assert_state_equal(plain.download(), st)
    jd = torch.from_numpy(np.flatnonzero(with_joint)).to(zeros.device)
    for k, dt in enumerate(list(dts) + [1 / 120] * 31):                   # _run_steps' loop on the other world
        for _ in range(zeros.phys_step_begin(dt)):
            if k >= len(dts):
                zeros.bflags[jd] |= 16
            zeros.world_step(1.0 / 120.0)
    assert zeros.time_acc.value == plain.time_acc.value
    a, z = plain.download(), zeros.download()
    for k in ("pos", "quat", "lvel", "avel", "aabb", "axis", "bflags", "adis_steps_left", "adis_time_left"):
        assert same_bits(a[k], z[k]), k
    assert (a["bflags"] & 1).any() and not zeros.facc.any().item()


# ------------------------------------------------------------------------------------------------- the frame
def test_frame_consumes_forces_in_its_first_substep(cuda_device):
    from clap_amd import entities, frame, tiler
    raw = synth.entities_flat(600, seed=5)
    scene, tl = tiler.tiled_scene(raw)
    roots = tl["slot_of"][np.flatnonzero(raw["parent"] < 0)]
    scene["model_lod"] = np.asarray([[0, 3]], np.uint8)
    nb = 300
    b = synth.capsule_bodies(nb, box=10.0, seed=5)
    b["body_entity"] = roots[:nb].astype(np.int32)
    f0 = rng(8).normal(0, 25.0, (nb, 3))
    for prebin in (False, True):
        batch = entities.EntityBatch(scene, cuda_device)
        world = physics.PhysWorld(b, synth.static_boxes(6, 10.0), pair_capacity=8192, device=cuda_device, forces=True)
        loop = frame.FrameLoop(batch, synth.camera(pos=(0, 10, 60)), world=world, prebin=prebin)
        st = pr.step_state(b, f0)
        put(world, "facc", f0)
        loop._issue(0.0, 0)                                               # a frame of 0 substeps: the forces survive
        assert_step_equal(world, st, "0 substeps")
        loop._issue(0.016, 2)
        pr.step_forces(b, st, H)
        after_one = st["lvel"].copy()
        assert not st["facc"].any()
        pr.step_forces(b, st, H)
        assert_step_equal(world, st, ("2 substeps", prebin))
        twice = pr.step_state(b, f0)                                       # what a second helping of the forces would give
        pr.step_forces(b, twice, H)
        twice["facc"][:] = f0
        pr.step_forces(b, twice, H)
        assert not same_bits(twice["lvel"], st["lvel"]) and not same_bits(after_one, b["lvel"])


# ------------------------------------------------------------------------------------------------- a captured graph
def test_slide_and_push_in_a_captured_graph(cuda_device):
    """slide + push captured once; replayed twice, each time on restored poses with FRESH velocities, accumulators and
    sleepers: both replays match the restatement fed with that replay's slide outputs, and the eager calls"""
    b, meshes = sr.scene_b()
    sc = Scene(cuda_device, b, meshes, cap=(1 << 20, 1 << 20))
    w = sc.w
    w.enable_forces()
    movers, v0, air = sr.movers_b(b)
    n, dev = len(movers), w.device
    w.bodies_aabb()
    keys = ("pos", "quat", "lvel", "aabb", "axis", "geom_records")
    before = {k: getattr(w, k).clone() for k in keys}
    body_d = torch.from_numpy(movers.view(np.int32)).to(dev)
    air_d = torch.from_numpy(np.ascontiguousarray(air, np.uint8)).to(dev)
    vel, given = torch.zeros((n, 3), dtype=torch.float32, device=dev), torch.zeros((n, 3), dtype=torch.float32, device=dev)
    first = torch.ones((n, 2), dtype=torch.float32, device=dev)
    push = torch.full((n, 6), -1, dtype=torch.int32, device=dev)
    flags = torch.zeros(n, dtype=torch.int32, device=dev)
    pushed = torch.zeros(w.n, dtype=torch.int32, device=dev)
    scratch = torch.zeros(w.n, dtype=torch.int32, device=dev)
    pscratch = torch.zeros(_lib.bodies_push_scratch_bytes(n), dtype=torch.uint8, device=dev)
    assert pscratch.numel() > 2 * 6 * n * 8 and pscratch.data_ptr() % 256 == 0
    sl = _lib.Slide(n, body_d.data_ptr(), vel.data_ptr(), air_d.data_ptr(), first.data_ptr(), push.data_ptr(), flags.data_ptr())
    sg = w.static_geoms()
    L = _lib.lib()

    def issue():
        _lib.check(L.clapgpu_characters_slide(physics._stream(), w._bp, C.byref(w._desc), C.byref(sg), w._meshes, DT, C.byref(sl),
                                              scratch.data_ptr()), "clapgpu_characters_slide")
        _lib.check(L.clapgpu_bodies_push(physics._stream(), C.byref(w._desc), C.byref(w.world), n, body_d.data_ptr(),
                                         given.data_ptr(), push.data_ptr(), flags.data_ptr(), pushed.data_ptr(),
                                         pscratch.data_ptr()), "clapgpu_bodies_push")

    def prepare(trial):
        for k in keys:
            getattr(w, k).copy_(before[k])
        w.bp_invalidate()
        w.bp_index()
        v = (v0 * np.float32(1.0 + 0.25 * trial)).astype(np.float32)
        vel.copy_(torch.from_numpy(v).to(dev))
        given.copy_(vel)
        return v, sleepy_start(w, b, 30 + trial)

    w.bp_index()                                                          # the captured slide asks for an index to look at
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            issue()
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for trial in range(2):
        v, st = prepare(trial)
        g.replay()
        torch.cuda.synchronize()
        push_h, flags_h = push.cpu().numpy().copy(), flags.cpu().numpy().view(np.uint32).copy()
        want = pr.push(st, b["mass"], movers, v, push_h, flags_h)
        assert want.sum() >= 5
        assert_push_equal(w, st, pushed, want, ("replay", trial))
        replayed = dev_push_state(w)
        prepare(trial)
        issue()                                                           # the eager calls on the same inputs
        assert same_bits(push.cpu().numpy(), push_h)
        assert_push_equal(w, replayed, pushed, want, ("eager", trial))
        seen.append(replayed["facc"].copy())
    assert not same_bits(seen[0], seen[1]), "fresh inputs: the replays are not each other's"
