"""GPU: moving statics (clapgpu_bp_statics_update, clap_amd/csrc/bp_restatic.hip).  After an update a broadphase object
must be the object a fresh create from the new boxes makes: its statics image array for array (against the fresh object
AND against tests/bpstaticsref.py, which tests/test_bp_statics_update.py holds to the host code), and every query through
it bit for bit.  No tolerance anywhere; the bounds alone compare by value (-0.0 == 0.0: fmin and an ordered-key reduction
may disagree on the sign of a zero).

The failure test injects a REPORTED launch failure on the host side (clapgpu_test_fail_after, as the drop-in's failure
test does): every kernel runs, nothing faults."""
import ctypes as C

import numpy as np
import pytest
import torch

import bpstaticsref as ref
import trimeshref as tr
from clap_amd import _lib, physics, synth
from meshscene import C2, IDENT, fetch, rng, same_bits

pytestmark = pytest.mark.gpu

LEVELS = (1, 4, 16)


# ------------------------------------------------------------------------------------------------- the object alone
class Bp:
    """a broadphase object over no bodies' boxes: create, update, read back"""

    def __init__(self, dev, boxes, levels, n_max=ref.N_MAX):
        self.L, self.dev, self.levels = _lib.lib(), dev, levels
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        st = np.ascontiguousarray(boxes, np.float64).reshape(-1, 6)
        self.n = len(st)
        self.bp = C.c_void_p()
        if levels == 1:
            _lib.check(self.L.clapgpu_bp_create(C.byref(self.bp), n_max, ref.CELL, self.n, st.ctypes.data if self.n else None),
                       "clapgpu_bp_create")
        else:
            _lib.check(self.L.clapgpu_bp_create_levels(C.byref(self.bp), n_max, ref.CELL, levels, self.n,
                                                       st.ctypes.data if self.n else None), "clapgpu_bp_create_levels")
        self.keep = None

    def close(self):
        bp, self.bp = self.bp, None
        if bp:
            self.L.clapgpu_bp_destroy(bp)

    __del__ = close

    def update_rc(self, boxes, n=None):
        t = torch.from_numpy(np.ascontiguousarray(boxes, np.float64).reshape(-1, 6)).to(self.dev)
        self.keep = t
        return self.L.clapgpu_bp_statics_update(self.stream, self.bp, len(t) if n is None else n, t.data_ptr() if len(t) else None)

    def update(self, boxes):
        _lib.check(self.update_rc(boxes), "clapgpu_bp_statics_update")

    def update_in_place(self, boxes):
        """the boxes written into the object's own copy, that pointer passed"""
        st = np.ascontiguousarray(boxes, np.float64).reshape(-1, 6)
        p = self.L.clapgpu_bp_static_aabb(self.bp)
        _lib.check(self.L.clapgpu_memcpy_h2d(p, st.ctypes.data, st.nbytes, self.stream), "clapgpu_memcpy_h2d")
        _lib.check(self.L.clapgpu_bp_statics_update(self.stream, self.bp, len(st), p), "clapgpu_bp_statics_update")

    def static_aabb(self):
        out = np.empty((self.n, 6))
        if self.n:
            _lib.check(self.L.clapgpu_memcpy_d2h(out.ctypes.data, self.L.clapgpu_bp_static_aabb(self.bp), out.nbytes, self.stream),
                       "clapgpu_memcpy_d2h")
            _lib.check(self.L.clapgpu_stream_sync(self.stream), "clapgpu_stream_sync")
        return out

    def image(self):
        return read_image(self.L, self.bp, self.stream, self.levels)


def read_image(L, bp, stream, levels):
    buckets, ne, nl = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    ls, bounds = (C.c_uint32 * 17)(), (C.c_double * 6)()
    _lib.check(L.clapgpu_bp_statics_sizes(bp, C.byref(buckets), C.byref(ne), C.byref(nl), ls, bounds), "clapgpu_bp_statics_sizes")
    assert buckets.value == ref.BUCKETS
    start = np.full(levels * (buckets.value + 1), 0xdeadbeef, np.uint32)
    entries, large = np.full(ne.value, 0xdeadbeef, np.uint32), np.full(nl.value, 0xdeadbeef, np.uint32)
    eb, lb = np.full((ne.value, 6), -7.0), np.full((nl.value, 6), -7.0)
    _lib.check(L.clapgpu_bp_statics_read(stream, bp, start.ctypes.data, entries.ctypes.data, large.ctypes.data, eb.ctypes.data,
                                         lb.ctypes.data), "clapgpu_bp_statics_read")
    return dict(start=start, entries=entries, large=large, entry_boxes=eb, large_boxes=lb, n_entries=ne.value, n_large=nl.value,
                large_start=np.array(ls[:], np.uint32), bounds=np.array(bounds[:]))


def assert_same_image(got, want, what):
    assert (got["n_entries"], got["n_large"]) == (want["n_entries"], want["n_large"]), what
    for name in ("start", "entries", "large", "entry_boxes", "large_boxes"):
        assert got[name].tobytes() == want[name].tobytes(), (what, name)
    k = min(len(got["large_start"]), len(want["large_start"]))
    assert np.array_equal(got["large_start"][:k], want["large_start"][:k]), (what, "large_start")
    assert np.all(got["bounds"] == want["bounds"]), (what, got["bounds"], want["bounds"])


def assert_is_the_object_of(dev, obj, boxes, what):
    """obj's image: a fresh create's from `boxes`, and the rule's"""
    fresh = Bp(dev, boxes, obj.levels)
    got = obj.image()
    assert_same_image(got, fresh.image(), what + ": against a fresh create")
    fresh.close()
    want = ref.image(boxes, obj.levels)
    if obj.levels == 1:
        want["large_start"] = np.zeros(2, np.uint32)         # a one-level object has no levels to tell apart
    assert_same_image(got, want, what + ": against the rule")
    assert obj.static_aabb().tobytes() == np.ascontiguousarray(boxes, np.float64).tobytes(), what


@pytest.mark.parametrize("levels", LEVELS)
def test_the_image(cuda_device, levels):
    a = ref.boxes(11)
    b = ref.boxes_moved(a, 12)
    many = ref.boxes_many(14, len(a))
    o = Bp(cuda_device, a, levels)
    address = o.L.clapgpu_bp_static_aabb(o.bp)
    assert_is_the_object_of(cuda_device, o, a, "as created")                 # the read-back of a fresh object
    o.update(b)
    assert_is_the_object_of(cuda_device, o, b, "A -> B")
    o.update(a)                                                              # fewer entries: the allocation again
    assert_is_the_object_of(cuda_device, o, a, "B -> A")
    o.update(many)                                                           # several times the entries: a larger one
    # 12 times A's registrations at one level, 6 at four, 2.2 at sixteen (there the one to eight registrations a static has
    # on each coarse level dominate both sets): always more than the allocation's room, 1.5 times what it has held
    assert ref.image(many, levels)["n_entries"] > 2 * max(ref.image(a, levels)["n_entries"], ref.image(b, levels)["n_entries"])
    assert_is_the_object_of(cuda_device, o, many, "A -> many")
    o.update_in_place(b)
    assert_is_the_object_of(cuda_device, o, b, "in place")
    assert o.L.clapgpu_bp_static_aabb(o.bp) == address
    o.close()


@pytest.mark.parametrize("levels", LEVELS)
def test_edge_objects(cuda_device, levels):
    a, b = ref.boxes(21), ref.boxes_moved(ref.boxes(21), 22)
    for n in (1, 63, 64, 65):
        o = Bp(cuda_device, a[:n], levels)
        o.update(b[:n])
        assert_is_the_object_of(cuda_device, o, b[:n], f"{n} statics")
        o.close()
    o = Bp(cuda_device, a[:0], levels)                                       # no statics: accepted, nothing done
    assert o.update_rc(a[:0]) == _lib.OK
    assert o.update_rc(a[:3]) == _lib.ERR_INVALID_ARGUMENTS
    o.close()
    big, small = ref.boxes_all_large(), ref.boxes_none_large(13)
    o = Bp(cuda_device, small, levels)
    o.update(big)
    assert o.image()["n_entries"] == 0
    assert_is_the_object_of(cuda_device, o, big, "all large")
    o.update(small)
    assert o.image()["n_large"] == 0
    assert_is_the_object_of(cuda_device, o, small, "none large")
    o.close()


# ------------------------------------------------------------------------------------------------- behaviour
N_BODIES, MESHES = 2048, 4
KINDS = np.array([_lib.GEOM_BOX, _lib.GEOM_SPHERE, _lib.GEOM_CAPSULE], np.uint8)
STANDERS = np.arange(256, 768)                                               # bodies placed on top of their static


def scene_boxes():
    """(A, B, mesh statics, their meshes, positions in A and in B): the box set, with MESHES small finite statics that own
    a cube mesh each and whose box is their posed mesh's, a little grown"""
    a = ref.boxes(11)
    b = ref.boxes_moved(a, 12)
    ok = np.flatnonzero(np.all(np.isfinite(a), 1) & np.all(np.isfinite(b), 1) & np.all(a[:, 1::2] - a[:, 0::2] < 3.5, 1) &
                        np.all(a[:, 1::2] > a[:, 0::2], 1) & np.all(b[:, 1::2] - b[:, 0::2] < 3.5, 1) & np.any(a != b, 1))
    ms = ok[:MESHES]
    vx, idx = synth.box_mesh(0.5)
    pa, pb = (a[ms, 0::2] + a[ms, 1::2]) / 2, (b[ms, 0::2] + b[ms, 1::2]) / 2
    for boxes, pos in ((a, pa), (b, pb)):
        for k, s in enumerate(ms):
            f = tr.bake(vx, idx, 1.5, pos[k], IDENT).reshape(-1, 3)
            boxes[s, 0::2], boxes[s, 1::2] = f.min(0) - 0.05, f.max(0) + 0.05
    return a, b, ms, (vx, idx), pa, pb


def scene_bodies(b_boxes, levels):
    """sphere bodies around the small finite statics of B (the first 256 around the mesh statics' neighbourhood too)"""
    R = rng(77)
    bodies = synth.sphere_bodies(N_BODIES, rmin=0.1, rmax=0.5, seed=9)
    if levels > 1:                                                           # mixed sizes: every level is lived on
        r = np.exp(R.uniform(np.log(0.1), np.log(3.5), N_BODIES))
        bodies.update(radius=r, yoffset=r.copy(), mass=4.0 / 3.0 * np.pi * r ** 3)
    bodies["cell"] = ref.CELL
    small = np.flatnonzero(np.all(np.isfinite(b_boxes), 1) & np.all(b_boxes[:, 1::2] - b_boxes[:, 0::2] < 20.0, 1) &
                           np.all(b_boxes[:, 1::2] >= b_boxes[:, 0::2], 1))
    s = R.choice(small, N_BODIES)
    c, h = (b_boxes[s, 0::2] + b_boxes[s, 1::2]) / 2, (b_boxes[s, 1::2] - b_boxes[s, 0::2]) / 2
    bodies["pos"] = c + R.uniform(-1.0, 1.0, (N_BODIES, 3)) * (h + 0.6)
    st = STANDERS                                                            # standing on their static's top face
    bodies["pos"][st, 1] = b_boxes[s[st], 3] + 0.8 * bodies["yoffset"][st]
    bodies["pos"][st, 0::2] = c[st, 0::2] + R.uniform(-0.5, 0.5, (len(st), 2)) * h[st, 0::2]
    bodies["lvel"] *= 0.2
    return bodies


def make_world(dev, bodies, boxes, ms, mesh, mesh_pos, levels):
    w = physics.PhysWorld(bodies, boxes, pair_capacity=1 << 16, static_pair_capacity=1 << 17, device=dev, bp_levels=levels,
                          leveled_index=levels > 1)
    set_geoms(w, boxes, ms)
    w.set_static_meshes(ms, [mesh[0]] * len(ms), [mesh[1]] * len(ms), [1.5] * len(ms), mesh_pos, [IDENT] * len(ms))
    return w


def set_geoms(w, boxes, ms):
    """the caller's static geom arrays: kinds by index, the mesh owners OTHER, the geoms filling the boxes"""
    kind = KINDS[np.arange(len(boxes)) % 3]
    kind[ms] = _lib.GEOM_OTHER
    with np.errstate(invalid="ignore"):
        w.set_static_geoms(kind, *synth.geoms_of_aabbs(boxes, kind))


def queries(w, boxes):
    """every query the issue names, in one fixed order; name -> arrays.  boxes: the statics' (to aim rays at)"""
    out = {}
    R = rng(5)
    w.bodies_aabb()
    w.broadphase()
    w.contacts_geoms_both()
    w.contacts_meshes()
    d = w.download()
    out["pairs"] = [d["pairs"], d["static_pairs"], np.array([d["pair_total"], d["static_pair_total"]])]
    c = w.download_contacts2(C2)
    out["contacts"] = [c["body"][0], np.array(c["body"][1]), c["static"][0], np.array(c["static"][1])]
    rec, mref, total, capped = w.download_mesh_contacts(C2)
    out["mesh_contacts"] = [rec, mref, np.array([total, capped])]
    w.bp_index()
    pos = d["pos"]
    ids = R.choice(N_BODIES, 512, replace=False)
    s, dr = pos[ids] + R.normal(0, 1.0, (512, 3)), R.normal(size=(512, 3))
    dr[:128] = [0.0, -1.0, 0.0]
    L = R.choice([1.0, 4.0, 30.0], 512)
    small = np.flatnonzero(np.all(np.isfinite(boxes), 1) & np.all(boxes[:, 1::2] - boxes[:, 0::2] < 20.0, 1) &
                           np.all(boxes[:, 1::2] >= boxes[:, 0::2], 1))
    t = R.choice(small, 256)                                                 # the second half: from outside a static towards its centre
    c, h = (boxes[t, 0::2] + boxes[t, 1::2]) / 2, np.linalg.norm((boxes[t, 1::2] - boxes[t, 0::2]) / 2, axis=1)
    u = R.normal(size=(256, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    s[256:], dr[256:], L[256:] = c + u * (h[:, None] + 1.0), -u, h + 2.0
    out["rays_grid"] = fetch(w.ray_cast(s, dr, L, grid=True))
    out["rays_brute"] = fetch(w.ray_cast(s, dr, L, grid=False))
    sw = R.choice(N_BODIES, 256, replace=False).astype(np.uint32)
    out["sweeps"] = fetch(w.sweep_capsules_grid(sw, R.normal(0, 0.6, (256, 3)).astype(np.float32)))
    sl = R.choice(N_BODIES, 256, replace=False).astype(np.uint32)
    out["slide"] = fetch(w.slide(sl, R.normal(0, 3.0, (256, 3)).astype(np.float32), R.integers(0, 2, 256), 1 / 30))
    w.bodies_aabb()
    w.bp_index()
    gr = R.choice(STANDERS, 256, replace=False).astype(np.uint32)
    out["ground"] = fetch(w.ground_collide(gr, np.full(256, 0.4), R.integers(0, 2, 256)))
    torch.cuda.synchronize()
    out["bodies"] = [w.pos.cpu().numpy(), w.lvel.cpu().numpy(), w.aabb.cpu().numpy()]
    return out


def assert_same_queries(got, want, what):
    for name in want:
        assert len(got[name]) == len(want[name])
        for k, (x, y) in enumerate(zip(got[name], want[name])):
            assert same_bits(x, y), (what, name, k)


@pytest.mark.parametrize("levels", (1, 4))
def test_behaviour(cuda_device, levels):
    a, b, ms, mesh, pa, pb = scene_boxes()
    bodies = scene_bodies(b, levels)
    moved = make_world(cuda_device, dict(bodies), a, ms, mesh, pa, levels)
    moved.update_statics(b)                                                  # boxes first,
    set_geoms(moved, b, ms)
    moved.pose_static_meshes(pb, [IDENT] * len(ms))                          # then the mesh pose; queries() indexes
    assert same_bits(moved._statics_host, np.ascontiguousarray(b))
    fresh = make_world(cuda_device, dict(bodies), b, ms, mesh, pb, levels)
    want = queries(fresh, b)
    # the scene reaches what it is about: statics are found by every query
    hit, sweep_hit, ground_hit = want["rays_brute"][1], want["sweeps"][2], want["ground"][3]
    print("pairs", want["pairs"][2], "touching", want["contacts"][1], want["contacts"][3], "mesh contacts", want["mesh_contacts"][2],
          "rays on statics / bodies", (hit <= -2).sum(), (hit >= 0).sum(), "sweeps", (sweep_hit <= -2).sum(), (sweep_hit >= 0).sum(),
          "ground", (ground_hit <= -2).sum(), (ground_hit >= 0).sum(), "slide flags", np.bincount(want["slide"][3], minlength=4))
    assert want["pairs"][2][1] > 2000 and want["contacts"][3] > 100 and want["mesh_contacts"][2][0] > 0
    assert (hit <= -2).sum() > 50 and (sweep_hit <= -2).sum() > 10 and (ground_hit <= -2).sum() > 10
    assert_same_queries(queries(moved, b), want, f"{levels} levels")
    for w in (moved, fresh):                                                 # the ground pass moved bodies: a new index
        w.bodies_aabb()
        w.bp_index()
    assert moved.bp_index_status() == fresh.bp_index_status()


# ------------------------------------------------------------------------------------------------- state
def static_pairs(w):
    w.broadphase()
    d = w.download()
    return d["static_pairs"], d["static_pair_total"], d["pairs"], d["pair_total"]


def test_state(cuda_device):
    a, b, ms, mesh, pa, pb = scene_boxes()
    bodies = scene_bodies(b, 1)
    w = make_world(cuda_device, dict(bodies), a, ms, mesh, pa, 1)
    fresh = make_world(cuda_device, dict(bodies), b, ms, mesh, pb, 1)
    ray = (bodies["pos"][:8], np.tile([0.0, -1.0, 0.0], (8, 1)), np.full(8, 2.0))
    w.bp_index()
    w.ray_cast(*ray, grid=True)
    w.update_statics(b)
    with pytest.raises(_lib.ClapGpuError) as e:
        w.ray_cast(*ray, grid=True)                                          # the index describes the old statics
    assert e.value.code == _lib.ERR_INVALID_ARGUMENTS
    w.ray_cast(*ray, grid=False)
    # a prebinned step, an update, a collide
    w.update_statics(a)
    for x in (w, fresh):
        x.world_step(1.0 / 120.0, prebin=True)
    w.update_statics(b)
    for x, y in zip(static_pairs(w), static_pairs(fresh)):
        assert np.array_equal(x, y)
    assert static_pairs(fresh)[1] > 2000
    # refusals
    L = _lib.lib()
    t = torch.from_numpy(np.ascontiguousarray(b)).to(cuda_device)
    assert L.clapgpu_bp_statics_update(physics._stream(), w._bp, len(b) - 1, t.data_ptr()) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_bp_statics_update(physics._stream(), w._bp, len(b), None) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_bp_statics_update(physics._stream(), None, len(b), t.data_ptr()) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_bp_statics_sizes(None, None, None, None, None, None) == _lib.ERR_INVALID_ARGUMENTS
    with pytest.raises(_lib.ClapGpuError):
        w.update_statics(b[:-1])


def test_status_bits_and_the_switch_survive(cuda_device):
    a, b, ms, mesh, pa, pb = scene_boxes()
    bodies = scene_bodies(b, 4)
    bodies["radius"][5] = 20.0                                               # an edge above the top cell (8): status bit 0
    w = make_world(cuda_device, bodies, a, ms, mesh, pa, 4)
    w.broadphase()
    assert w.broadphase_status() & 1
    w.bp_index()
    assert w.bp_index_status() & 4 == 0                                      # switched on: an index is built
    w.update_statics(b)
    assert w.broadphase_status() & 1                                         # sticky, kept
    with pytest.raises(_lib.ClapGpuError):
        w.bp_index_status()
    w.bp_index()
    assert w.bp_index_status() & 4 == 0                                      # the switch is still on


def test_a_frame_after_an_update(cuda_device):
    from clap_amd import entities, frame, tiler
    a, b, ms, mesh, pa, pb = scene_boxes()
    bodies = scene_bodies(b, 1)
    raw = synth.entities_flat(N_BODIES + 100, seed=5)
    scene, tl = tiler.tiled_scene(raw)
    roots = tl["slot_of"][np.flatnonzero(raw["parent"] < 0)]
    bodies["body_entity"][:] = roots[:N_BODIES]
    state = []
    for first, pos in ((a, pa), (b, pb)):
        batch = entities.EntityBatch(scene, cuda_device)
        w = make_world(cuda_device, dict(bodies), first, ms, mesh, pos, 1)
        if first is a:
            w.update_statics(b)
            set_geoms(w, b, ms)
            w.pose_static_meshes(pb, [IDENT] * len(ms))
        loop = frame.FrameLoop(batch, synth.camera(pos=(0, 10, 60)), world=w, contacts=True)
        now = 3.0
        for dt in (1 / 60, 1 / 120):
            now += dt
            loop.clap_frame(now, dt)
        torch.cuda.synchronize()
        d = w.download()
        s = {k: d[k] for k in ("pos", "quat", "lvel", "avel", "aabb", "pairs", "static_pairs")}
        s.update(totals=np.array([d["pair_total"], d["static_pair_total"]]))
        s.update({"c_" + k: np.concatenate([np.atleast_1d(x).view(np.uint8).reshape(-1) for x in v])
                  for k, v in w.download_contacts2(C2).items()})
        s.update({"e_" + k: v for k, v in batch.download().items() if isinstance(v, np.ndarray)})
        state.append(s)
    assert state[1]["totals"][1] > 2000
    for k in state[1]:
        assert same_bits(state[0][k], state[1][k]), k


# ------------------------------------------------------------------------------------------------- failure
def test_a_failed_update_leaves_the_old_statics(cuda_device, monkeypatch):
    monkeypatch.setenv("CLAPGPU_TEST_HOOKS", "1")                            # read by the library's first clapgpu_test_fail_after
    a = ref.boxes(11)
    b = ref.boxes_moved(a, 12)
    many = ref.boxes_many(14, len(a))
    L = _lib.lib()
    for levels, first, to in ((1, a, b), (4, a, many)):                      # the second: through the growth of the allocation
        bodies = scene_bodies(a, levels)
        w = physics.PhysWorld(bodies, first, pair_capacity=1 << 16, static_pair_capacity=1 << 17, device=cuda_device,
                              bp_levels=levels)
        w.update_statics(first)                                              # from the second allocation, as any later update
        before, pairs = read_image(L, w._bp, physics._stream(), levels), static_pairs(w)
        assert pairs[1] > 1000
        failed = 0
        to_d = torch.from_numpy(to).to(cuda_device)
        try:
            for k in range(64):
                L.clapgpu_test_fail_after(k)
                rc = L.clapgpu_bp_statics_update(physics._stream(), w._bp, len(to), to_d.data_ptr())
                L.clapgpu_test_fail_after(-1)
                if rc == _lib.OK:
                    break
                failed += 1
                assert rc == _lib.ERR_UNKNOWN
                assert_same_image(read_image(L, w._bp, physics._stream(), levels), before, f"failed at launch {k}")
                for x, y in zip(static_pairs(w), pairs):
                    assert np.array_equal(x, y)
        finally:
            L.clapgpu_test_fail_after(-1)
        assert 4 <= failed <= 8, f"{failed} launches failed: is the hook armed (CLAPGPU_TEST_HOOKS)?"
        fresh = Bp(cuda_device, to, levels)                                  # the update that went through
        assert_same_image(read_image(L, w._bp, physics._stream(), levels), fresh.image(), "after the clean update")
        fresh.close()
