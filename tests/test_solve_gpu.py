"""GPU: clapgpu_bodies_solve against tests/solveref.py.  The device makes its own contact lists (broadphase, both
narrowphase passes, mesh contacts, island pass); the downloaded lists go through the numpy restatement of the header's
rule and every comparison is == on bit patterns."""
import ctypes as C

import numpy as np
import pytest
import torch

from clap_amd import _lib, physics, synth
from clap_amd.synth import box_mesh
import meshscene
from meshscene import C2, IDENT, guarded_scratch, rng, same_bits
import pushref as pr
import solveref as sr

pytestmark = pytest.mark.gpu
H = 1.0 / 120.0
STATE = ("pos", "quat", "lvel", "avel", "bflags", "adis_steps_left", "adis_time_left", "aabb", "axis", "geom_records", "facc",
         "mass", "radius", "length", "inertia")
INF = float("inf")

# index plan of the scene
PAIRS0, N_PAIRS = 63, 100                 # (63, 64), (65, 66) ... (255, 256): one straddles a wavefront, one a workgroup
TRI0, N_TRI = 263, 50
CHAIN0, N_CHAIN = 413, 41                 # 413 rides on 414 and 415 and does not touch the ground: the root, no first contact
KIN0 = 454                                # 454 .. 463 kinematic sleepers touching the awake 464 .. 473; 474 .. 478 alone
SLEEP0 = 479                              # 479 (kinematic) and 480, both asleep, touching: an island that sleeps on
DEEP0 = 481                               # a capsule lying in the ground slab's top face
MESH0, N_MESH = 482, 20
N = 1000


def scene_bodies():
    b = synth.capsule_bodies(N, box=64.0, seed=23)
    R = rng(24)
    b["pos"][:] = np.stack([R.uniform(2, 62, N), R.uniform(20, 60, N), R.uniform(2, 62, N)], 1)    # isolated, mostly
    m = 40                                                                  # some of them among the small boxes
    b["pos"][N - m:] = np.stack([R.uniform(0, 30, m), R.uniform(4, 9, m), R.uniform(34, 64, m)], 1)
    off = lambda k: R.uniform(-1, 1, (k, 3)) * [0.06, 0.04, 0.06]     # under 0.2 apart: the thinnest two still overlap
    for k in range(N_PAIRS):
        c = np.array([2.0 + 3.0 * (k % 20), 10.0, 2.0 + 3.0 * (k // 20)])
        i = PAIRS0 + 2 * k
        b["pos"][i:i + 2] = c + off(2)
    par = [PAIRS0 + 2, PAIRS0 + 3]                                          # two parallel capsules side by side: a record of two contacts
    b["length"][par], b["radius"][par] = 1.0, 0.2
    b["quat"][par] = [1.0, 0.0, 0.0, 0.0]
    for k in range(N_TRI):
        c = np.array([2.0 + 3.0 * (k % 20), 14.0, 2.0 + 3.0 * (k // 20)])
        i = TRI0 + 3 * k
        b["pos"][i:i + 3] = c + off(3)
    ch = np.arange(CHAIN0, CHAIN0 + N_CHAIN)
    b["length"][ch] = 0.0
    b["radius"][ch] = 0.3
    b["inertia"][ch] = 0.4 * b["mass"][ch, None] * 0.09
    b["pos"][ch[1:]] = np.stack([5.0 + 0.4 * np.arange(N_CHAIN - 1), np.full(N_CHAIN - 1, 0.78), np.full(N_CHAIN - 1, 32.0)], 1)
    b["pos"][ch[0]] = [5.2, 0.78 + 0.45, 32.0]
    b["lvel"][ch] *= 0.1
    for k in range(10):
        c = np.array([2.0 + 3.0 * k, 17.0, 20.0])
        b["pos"][[KIN0 + k, KIN0 + 10 + k]] = c + off(2)
    b["pos"][KIN0 + 20:KIN0 + 25] = np.stack([2.0 + 3.0 * np.arange(5), np.full(5, 17.0), np.full(5, 24.0)], 1)
    kin = np.arange(KIN0, KIN0 + 25)
    kin = kin[(kin < KIN0 + 10) | (kin >= KIN0 + 20)]
    b["bflags"][kin] = pr.DISABLED | pr.KINEMATIC | pr.GYROSCOPIC
    b["pos"][[SLEEP0, SLEEP0 + 1]] = np.array([40.0, 17.0, 24.0]) + off(2)
    b["bflags"][SLEEP0] = pr.DISABLED | pr.KINEMATIC | pr.GYROSCOPIC
    b["bflags"][SLEEP0 + 1] |= pr.DISABLED
    b["lvel"][[SLEEP0, SLEEP0 + 1]] = b["avel"][[SLEEP0, SLEEP0 + 1]] = 0
    b["adis_steps_left"][SLEEP0 + 1] = 0
    b["length"][DEEP0], b["radius"][DEEP0] = 1.0, 0.2
    b["pos"][DEEP0] = [50.0, 0.5, 10.0]
    b["quat"][DEEP0] = [1.0, 0, 0, 0]
    ms = np.arange(MESH0, MESH0 + N_MESH)
    b["pos"][ms] = np.stack([50.0 + R.uniform(-0.8, 0.8, N_MESH), 13.0 + R.uniform(0.0, 0.15, N_MESH),
                             50.0 + R.uniform(-0.8, 0.8, N_MESH)], 1)
    b["facc"] = R.normal(0, 3.0, (N, 3)) * (R.uniform(0, 1, (N, 1)) < 0.5)
    b["cell"] = float((b["length"] + 2 * b["radius"]).max())
    return b


def materials(n, seed):
    R = rng(seed)
    pick = lambda vals: np.asarray(vals)[R.integers(0, len(vals), n)]
    return np.stack([pick([0.0, 0.0, 0.5]), pick([0.0, 0.1]), pick([0.0, 0.5, 0.5, INF]), pick([0.0, 0.2]), pick([0.0, 0.001])], 1)


def build_scene(dev):
    b = scene_bodies()
    R = rng(25)
    bb = np.zeros((64, 6))
    lo = np.stack([R.uniform(0, 28, 64), R.uniform(3, 8, 64), R.uniform(34, 62, 64)], 1)
    bb[:, 0::2], bb[:, 1::2] = lo, lo + R.uniform(1, 4, (64, 3))
    bb[0] = [-1e3, 1e3, -10.0, 0.5, -1e3, 1e3]                              # the ground slab
    bv, bi = box_mesh()
    mat, smat = materials(N, 26), materials(65, 27)
    mat[CHAIN0:CHAIN0 + N_CHAIN, 2] = 0.5                                   # the chain rubs: three rows a contact
    smat[0, 2] = 0.5
    sc = meshscene.Scene(dev, b, [(bv, bi, 2.0, [50.0, 12.0, 50.0], IDENT)], bb=bb, material=mat, static_material=smat,
                         cap=(1 << 14, 1 << 14), grow=1e-6)
    w = sc.w
    w.enable_forces(b["facc"])
    return b, w


def contact_pass(w):
    w.bodies_aabb()
    w.broadphase()
    w.contacts_geoms_both()
    w.contacts_meshes()
    w.islands(H)
    torch.cuda.synchronize()


def snapshot(w):
    return {k: getattr(w, k).clone() for k in STATE if getattr(w, k, None) is not None}


def restore(w, snap, keys=("lvel", "avel")):
    for k in keys:
        getattr(w, k).copy_(snap[k])


def host_state(w, snap):
    st = {k: v.cpu().numpy() for k, v in snap.items()}
    st["bflags"] = st["bflags"].view(np.uint32)
    for k in ("lvel", "avel", "pos", "quat", "facc"):
        st[k] = st[k][:w.n]
    return st


def lists(w):
    c = w.download_contacts2(C2)
    mrec, mref, mtotal, _capped = w.download_mesh_contacts(C2)
    d = w.download()
    assert d["pair_total"] <= w.capacity and d["static_pair_total"] <= w.static_capacity and mtotal <= w.mesh_contact_capacity
    return dict(static=(d["static_pairs"], c["static"][0]), mesh=(mrec, mref), body=(d["pairs"], c["body"][0]))


def reference(w, snap, **kw):
    return sr.solve(host_state(w, snap), w.island.cpu().numpy().view(np.uint32)[:w.n], H, **lists(w), **kw)


@pytest.fixture(scope="module")
def solved(cuda_device):
    """the scene after its contact pass, the state the solve saw, the reference's answer (made once) and the device's"""
    b, w = build_scene(cuda_device)
    contact_pass(w)
    snap = snapshot(w)
    want = reference(w, snap)
    w.alloc_solve(want["rows_total"] + 37)
    total, status, lam, key = w.solve(H, want_lambda=True)
    torch.cuda.synchronize()
    got = dict(lvel=w.lvel.cpu().numpy(), avel=w.avel.cpu().numpy(), row_lambda=lam.cpu().numpy(),
               row_key=key.cpu().numpy().view(np.uint64), rows_total=int(total.item()), status=int(status.item()))
    return b, w, snap, want, got


def test_the_scene_holds_what_it_should(solved):
    b, w, snap, want, _got = solved
    L = lists(w)
    st = host_state(w, snap)
    island = w.island.cpu().numpy().view(np.uint32)
    fl = st["bflags"]
    assert island[64] == 63 and island[256] == 255                          # the straddling pairs are islands
    touching = (L["body"][1]["nc"] & ~np.uint32(_lib.CONTACT_DEEP)) >= 1
    assert touching.sum() >= 150
    ch = np.arange(CHAIN0, CHAIN0 + N_CHAIN)
    assert (island[ch] == CHAIN0).all()
    chain_rows = (want["row_key"] >> np.uint64(32)) == CHAIN0
    assert chain_rows.sum() >= 117
    first = int(want["row_key"][chain_rows][0] & np.uint64(0xffffffff))     # the chain's first contact is a ground contact ...
    sp = L["static"][0]
    ground_bodies = sp[(sp[:, 1] == 0) & (L["static"][1]["nc"] == 1)][:, 0]
    assert CHAIN0 not in ground_bodies and first < len(sp)                  # ... of another body than its root
    assert not (fl[KIN0:KIN0 + 10] & pr.DISABLED).any(), "kinematic sleepers beside awake bodies woke"
    assert (fl[KIN0 + 20:KIN0 + 25] & pr.DISABLED).all() and (fl[[SLEEP0, SLEEP0 + 1]] & pr.DISABLED).all()
    assert (L["static"][1]["nc"] == _lib.CONTACT_DEEP).any() and L["static"][0][L["static"][1]["nc"] == _lib.CONTACT_DEEP][:, 0].tolist().count(DEEP0)
    assert len(L["mesh"][0]) >= 10
    mus = np.concatenate([L[k][1 if k != "mesh" else 0]["mu"] for k in L])
    assert (mus == 0).any() and (mus == 0.5).any() and np.isinf(mus).any() and np.isnan(mus).any()
    modes = np.concatenate([L[k][1 if k != "mesh" else 0]["mode"] for k in L])
    assert (modes & 4).any() and not (modes & 4).all()
    assert (L["body"][1]["nc"] == 2).any()
    lam = want["row_lambda"]
    assert (lam > 0).any() and (lam == 0).any() and (lam < 0).any()
    print(f"{want['rows_total']} rows, {len(np.unique(want['row_key'] >> np.uint64(32)))} islands with rows, "
          f"{int(chain_rows.sum())} rows in the chain")


def test_bits(solved):
    b, w, snap, want, got = solved
    k = want["rows_total"]
    assert got["status"] == 0 and got["rows_total"] == k and k > 500
    assert same_bits(got["row_key"][:k], want["row_key"])
    assert same_bits(got["row_lambda"][:k], want["row_lambda"])
    assert same_bits(got["lvel"][:w.n], want["lvel"]) and same_bits(got["avel"][:w.n], want["avel"])
    changed = (got["lvel"][:w.n] != snap["lvel"].cpu().numpy()[:w.n]).any(1)
    assert changed.sum() >= 300
    for name, t in snapshot(w).items():                                     # nothing else of the bodies changed
        if name not in ("lvel", "avel"):
            assert same_bits(t.cpu().numpy(), snap[name].cpu().numpy()), name


def test_same_bits_again_and_from_a_graph(solved):
    b, w, snap, want, got = solved

    def result():
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (w.lvel, w.avel, w.row_lambda, w.row_key, w.rows_total, w.solve_status)]
    runs = []
    for _ in range(2):                                                      # the scratch stays as the call before left it
        restore(w, snap)
        w.solve(H, want_lambda=True)
        runs.append(result())
    graph = torch.cuda.CUDAGraph()
    restore(w, snap)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        w.solve(H, want_lambda=True)
    for _ in range(2):
        restore(w, snap)
        w.row_lambda.fill_(-1.0)
        graph.replay()
        runs.append(result())
    k = want["rows_total"]
    for r in runs:
        assert same_bits(r[0][:w.n], want["lvel"]) and same_bits(r[1][:w.n], want["avel"])
        assert same_bits(r[2][:k], want["row_lambda"]) and same_bits(r[3].view(np.uint64)[:k], want["row_key"])
        assert int(r[4][0]) == k and int(r[5][0]) == 0


def test_capacity_and_absent_lists(solved):
    b, w, snap, want, got = solved
    k = want["rows_total"]
    keep = (w.solve_rows_capacity, w.solve_scratch, w.row_lambda, w.row_key)
    try:
        restore(w, snap)
        w.alloc_solve(k - 1)
        total, status = w.solve(H)
        torch.cuda.synchronize()
        assert int(status.item()) & 1 and int(total.item()) == k
        assert same_bits(w.lvel.cpu().numpy(), snap["lvel"].cpu().numpy())
        assert same_bits(w.avel.cpu().numpy(), snap["avel"].cpu().numpy())
        w.solve_status.zero_()
        w.alloc_solve(k)                                                    # exactly enough
        total, status = w.solve(H)
        torch.cuda.synchronize()
        assert int(status.item()) == 0 and same_bits(w.lvel.cpu().numpy()[:w.n], want["lvel"])
        # no list at all
        restore(w, snap)
        w.rows_total.fill_(-1)
        rc = _lib.lib().clapgpu_bodies_solve(physics._stream(), C.byref(w._desc), C.byref(w.world), C.byref(w.solver), H,
                                             w.island.data_ptr(), None, None, 0, None, None, None, None, 0, None, None, 0, None,
                                             w.solve_rows_capacity, w.solve_scratch.data_ptr(), None, None,
                                             w.rows_total.data_ptr(), w.solve_status.data_ptr(), None, None)
        torch.cuda.synchronize()
        assert rc == _lib.OK and int(w.rows_total.item()) == 0 and int(w.solve_status.item()) == 0
        assert same_bits(w.lvel.cpu().numpy(), snap["lvel"].cpu().numpy())
        assert same_bits(w.avel.cpu().numpy(), snap["avel"].cpu().numpy())
        L = _lib.lib()                                                      # argument checks
        args = [physics._stream(), C.byref(w._desc), C.byref(w.world), C.byref(w.solver), H, w.island.data_ptr(), None, None, 0,
                None, None, None, None, 0, w.pairs.data_ptr(), w.pair_total.data_ptr(), w.capacity, w.contact2_buf.data_ptr(),
                w.solve_rows_capacity, w.solve_scratch.data_ptr(), None, None, None, None, None, None]
        bad = lambda i, v: args[:i] + [v] + args[i + 1:]
        assert L.clapgpu_bodies_solve(*bad(5, None)) == _lib.ERR_INVALID_ARGUMENTS            # island
        assert L.clapgpu_bodies_solve(*bad(19, None)) == _lib.ERR_INVALID_ARGUMENTS           # scratch
        assert L.clapgpu_bodies_solve(*bad(19, w.solve_scratch.data_ptr() + 8)) == _lib.ERR_INVALID_ARGUMENTS
        assert L.clapgpu_bodies_solve(*bad(3, None)) == _lib.ERR_INVALID_ARGUMENTS            # solver
        assert _lib.bodies_solve_scratch_bytes(w.n, 1000) >= 1000 * 240 + w.n * 48
    finally:
        w.solve_rows_capacity, w.solve_scratch, w.row_lambda, w.row_key = keep
        restore(w, snap)


# ------------------------------------------------------------------------------------------------- at rest
def resting_sphere():
    b = synth.sphere_bodies(1, box=1.0, seed=1)
    b["pos"][:] = [0.0, 0.5, 0.0]
    b["radius"][:] = 0.5
    b["mass"][:] = 1.0
    b["lvel"][:] = b["avel"][:] = 0
    b["bflags"][:] = 0
    b["cell"] = 2.0
    return b, np.array([[-4.0, 4.0, -1.0, 0.0, -4.0, 4.0]])


def test_a_sphere_rests_on_the_floor(cuda_device):
    """tests/test_solve.py's resting sphere through phys_step(solve=True): the same fixed point and the same two bounds.
    Without contact response the sphere is some 480 m below the floor after these 10 s."""
    b, floor = resting_sphere()
    w = physics.PhysWorld(b, floor, device=cuda_device)
    steps = 0
    while steps < 1200:
        steps += w.phys_step(H, solve=True)
    d = w.download()
    want = 0.01 * 1.0 * 9.8 * H / 0.05
    depth = 0.5 - d["pos"][0, 1]
    print("substeps", steps, "depth", depth, "depth*", want, "lvel", d["lvel"][0], "status", int(w.solve_status.item()))
    assert int(w.solve_status.item()) == 0
    assert abs(depth - want) <= 1e-3 * want
    assert np.abs(d["lvel"][0]).max() <= 1e-6


# ------------------------------------------------------------------------------------------------- the scratch
def sunk_sphere():
    """the resting sphere 0.01 into its floor: one contact, rows that fit"""
    b, floor = resting_sphere()
    b["pos"][:, 1] = 0.49
    return b, floor, {}


def sleeping_row():
    """test_islands_gpu's row: 65 capsules in a floor slab and in each other, more rows than either capacity below holds"""
    from test_islands_gpu import row_scene
    b, statics = row_scene()
    return b, statics, dict(pair_capacity=8192)


@pytest.mark.parametrize("rows_capacity", [32, 33])
@pytest.mark.parametrize("scene", [sunk_sphere, sleeping_row], ids=["fits", "overflows"])
def test_solve_stays_inside_the_scratch_it_asks_for(cuda_device, scene, rows_capacity):
    """a scratch of exactly clapgpu_bodies_solve_scratch_bytes, 0xA5 behind it: the call leaves the tail alone and gives
    the bytes it gives on the wrapper's own scratch.  32 rows fill the 8-byte key arrays' 256-byte part, 33 start the
    next.  Rows that fit run every launch; rows that do not (status bit 0) run the clamps at the arrays' ends"""
    b, statics, kw = scene()
    w = physics.PhysWorld(b, statics, device=cuda_device, **kw)
    w.broadphase()
    w.contacts_geoms_both()
    w.islands(H)
    snap = snapshot(w)

    def result():
        total, status, lam, key = w.solve(H, want_lambda=True)
        torch.cuda.synchronize()
        k = int(total.item()) if int(total.item()) <= rows_capacity else 0   # rows that do not fit: none is written
        return dict(lvel=w.lvel.cpu().numpy().copy(), avel=w.avel.cpu().numpy().copy(), rows_total=int(total.item()),
                    status=int(status.item()), row_lambda=lam.cpu().numpy()[:k].copy(), row_key=key.cpu().numpy()[:k].copy())
    w.alloc_solve(rows_capacity)
    want = result()
    if scene is sunk_sphere:
        assert want["status"] == 0 and 1 <= want["rows_total"] <= 32 and not same_bits(want["lvel"], snap["lvel"].cpu().numpy())
    else:
        assert want["status"] & 1 and want["rows_total"] > 33 and same_bits(want["lvel"], snap["lvel"].cpu().numpy())
    restore(w, snap)
    w.solve_status.zero_()
    w.row_lambda.fill_(-1.0)
    w.row_key.fill_(-1)
    w.solve_scratch, tail = guarded_scratch(_lib.bodies_solve_scratch_bytes(w.n, rows_capacity), w.device)
    got = result()
    assert (tail == 0xA5).all().item(), ("written past the scratch", torch.nonzero(tail != 0xA5)[:8].flatten().tolist())
    for k in want:
        assert same_bits(got[k], want[k]) if isinstance(want[k], np.ndarray) else got[k] == want[k], k


# ------------------------------------------------------------------------------------------------- the frame
def frame_world(cuda_device, solve, islands=True):
    from clap_amd import entities, frame, tiler
    from test_islands_gpu import row_scene
    raw = synth.entities_flat(600, seed=5)
    scene, tl = tiler.tiled_scene(raw)
    roots = tl["slot_of"][np.flatnonzero(raw["parent"] < 0)]
    scene["model_lod"] = np.asarray([[0, 3]], np.uint8)
    b, statics = row_scene()
    b["body_entity"] = roots[:b["n"]].astype(np.int32)
    batch = entities.EntityBatch(scene, cuda_device)
    world = physics.PhysWorld(b, statics, pair_capacity=8192, device=cuda_device)
    loop = frame.FrameLoop(batch, synth.camera(pos=(0, 10, 60)), world=world, contacts=True, islands=islands, solve=solve)
    return b, world, loop


def assert_same_world(a, z, what):
    da, dz = a.download(), z.download()
    for k in dz:
        assert same_bits(np.asarray(da[k]), np.asarray(dz[k])), (what, k)
    assert same_bits(a.island.cpu().numpy(), z.island.cpu().numpy()), (what, "island")


def test_frame_solves_between_islands_and_step(cuda_device):
    b, manual, _ = frame_world(cuda_device, True)
    for _ in range(2):
        manual.broadphase()
        manual.contacts_geoms_both()
        manual.islands(H)
        manual.solve(H)
        manual.world_step(H)
    _, framed, loop = frame_world(cuda_device, True)
    loop._issue(0.0, 2)
    assert_same_world(framed, manual, "frame of 2 substeps with the solve")
    assert int(framed.solve_status.item()) == 0 and int(manual.rows_total.item()) >= 64
    # ... and it is the solve that acts: without it the row falls through its floor
    _, plain, loop0 = frame_world(cuda_device, False)
    loop0._issue(0.0, 2)
    assert not same_bits(plain.download()["lvel"], framed.download()["lvel"])
    assert getattr(plain, "solve_scratch", None) is None


def test_frame_without_solve_scratch_is_the_frame_before(cuda_device):
    _, plain, loop0 = frame_world(cuda_device, False)
    loop0._issue(0.0, 2)
    _, w, loop = frame_world(cuda_device, True)
    f = loop._build()
    f.solve_scratch = None                                                  # solver, capacity and status stay set
    loop._issue(0.0, 2)
    assert_same_world(w, plain, "solve_scratch NULL")
