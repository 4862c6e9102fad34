"""GPU: the mesh set in parts (clapgpu_trimesh_create_parts / _pose_meshes / _parts_status / _read).  The read-back image
is held to the checker of tests/trimeshpartsref.py; a partial pose must leave, byte for byte, the set a fresh creation
with the same poses makes; every query must answer with the plain set's bits; odd inputs, a captured graph and reported
launch failures (clapgpu_test_fail_after: every kernel runs, nothing faults)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from clap_amd import _lib, physics, synth
from clap_amd.synth import box_mesh, heightfield, icosphere
from meshscene import C2, IDENT, Scene, far_body, fetch, rng, same_bits, unit
import trimeshpartsref as pr

pytestmark = pytest.mark.gpu

RANGE, TWICE = 1, 2                                          # CLAPGPU_TRIMESH_POSE_RANGE, _TWICE


def rand_quat(R):
    return unit(R.normal(size=4)).astype(np.float32)        # x, y, z, w


def soup(R, k, at=(0.0, 0.0, 0.0)):
    """k random triangles around `at`: (vx, idx)"""
    vx = (R.uniform(-1, 1, (3 * k, 3)) + at).astype(np.float32)
    return vx, np.arange(3 * k, dtype=np.uint16).reshape(-1, 3)


class Bare:
    """A PhysWorld with one far body and len(meshes) box statics, for sets that are only built, posed and read"""

    def __init__(self, dev, meshes, parts=True):
        ns = max(len(meshes), 1)
        bb = np.tile([-1.0, 1.0, -1.0, 1.0, -1.0, 1.0], (ns, 1))
        self.w = physics.PhysWorld(far_body(), bb, device=dev)
        self.meshes = meshes
        self.static_index = np.arange(len(meshes), dtype=np.uint32)
        self.tri_first = np.concatenate([[0], np.cumsum([len(m[1]) for m in meshes])]).astype(np.uint32)
        self.set(parts=parts)

    def set(self, pos=None, quat=None, parts=True):
        m = self.meshes
        self.w.set_static_meshes(self.static_index, [x[0] for x in m], [x[1] for x in m], [x[2] for x in m],
                                 [x[3] for x in m] if pos is None else pos, [x[4] for x in m] if quat is None else quat, parts=parts)
        return self.w.read_static_meshes()

    def check(self):
        """the image through the checker, against both status calls; returns (image, (top, deepest, total))"""
        img = self.w.read_static_meshes()
        got = pr.check_image(img["nodes"], img["key"], img["tri"], img["part_root"], self.tri_first, self.static_index)
        on, top, deep, flags = self.w.static_meshes_parts_status()
        assert on and (top, deep) == got[:2], (top, deep, got)
        depth, ntri = self.w.static_meshes_status()
        assert ntri == int(self.tri_first[-1]) and depth == top + deep and got[2] in (depth, depth - 1), (depth, ntri, got)
        assert depth <= pr.HEIGHT_MAX
        return img, got


def same_image(a, b):
    return all(same_bits(a[k], b[k]) for k in ("nodes", "key", "tri", "part_root"))


# ------------------------------------------------------------------------------------------------- 1. structure
def test_structure_of_mixed_meshes_and_the_plain_sets_triangles(cuda_device):
    R = rng(1)
    meshes = [soup(R, k, (4.0 * j, 0.0, 0.0)) + (float(R.uniform(0.5, 2.0)), R.uniform(-3, 3, 3), rand_quat(R))
              for j, k in enumerate((0, 1, 2, 3, 65, 0, 1, 3))]
    b = Bare(cuda_device, meshes)
    img, (top, deep, _total) = b.check()
    assert top == 3 and deep >= 7                            # 6 parts; 65 triangles are at least 7 high
    assert list(img["part_root"][[0, 5]]) == [pr.NONE, pr.NONE]
    # the same triangles, bit for bit, as the plain set bakes: by (static, triangle)
    plain = b.set(parts=False)
    assert plain["part_root"] is None and not b.w.static_meshes_parts_status()[0]
    by_key = lambda im: im["tri"][np.lexsort((im["key"][:, 1], im["key"][:, 0]))]
    assert same_bits(by_key(img), by_key(plain))


@pytest.mark.parametrize("P", [0, 1, 2, 3, 64, 65])
def test_structure_by_part_count(cuda_device, P):
    R = rng(10 + P)
    sizes = [0, 0] if P == 0 else [0] + [int(R.integers(1, 4)) for _ in range(P)]
    meshes = [soup(R, k, R.uniform(-20, 20, 3)) + (1.0, R.uniform(-1, 1, 3), rand_quat(R)) for k in sizes]
    b = Bare(cuda_device, meshes)
    img, (top, _deep, total) = b.check()
    assert top == pr.top_height(P)
    if P == 0:
        assert total == 0 and b.w.static_meshes_status() == (0, 0)
    if P == 1:
        assert img["part_root"][1] in (0, pr.LEAF)          # node 0 is the one part's root


def test_structure_of_one_triangle_and_of_a_deep_part(cuda_device):
    R = rng(3)
    b = Bare(cuda_device, [soup(R, 0) + (1.0, [0.0, 0.0, 0.0], IDENT), soup(R, 1) + (2.0, [1.0, 2.0, 3.0], rand_quat(R))])
    img, got = b.check()
    assert got == (0, 1, 1) and list(img["nodes"][0]["child"]) == [pr.LEAF, pr.LEAF]
    # 4 096 copies of one triangle: identical centroids, one Morton code, so the triangle index alone splits the keys
    # and the part is the balanced tree over 12 index bits
    n = 4096
    one = np.array([[4.0, 1.0, 5.0], [5.0, 1.0, 6.5], [6.0, 1.0, 4.5]], np.float32)
    same = (np.tile(one, (n, 1)), np.arange(3 * n, dtype=np.uint16).reshape(-1, 3), 1.0, [0.0, 0.0, 0.0], IDENT)
    b = Bare(cuda_device, [same, soup(R, 3, (20.0, 0.0, 0.0)) + (1.0, [0.0, 0.0, 0.0], IDENT)])
    _img, (top, deepest, _total) = b.check()
    assert (top, deepest) == (1, 12), (top, deepest)
    # a part that does degenerate: point triangles at 2^-k along the diagonal (k = 0 .. 10; the codes of k = 2 .. 10 each
    # have a leading bit of their own, so the root parts k = 0, 1 from the rest and nine splits peel one leaf each) and 64
    # more at the origin below that chain (at least 6 levels of index bits): 1 + 9 + 6.  75 leaves, balanced, would be 7 high
    at = np.concatenate([[[2.0 ** -k] * 3 for k in range(11)], np.zeros((64, 3))]).astype(np.float32)
    chain = (np.repeat(at, 3, axis=0), np.arange(3 * len(at), dtype=np.uint16).reshape(-1, 3), 1.0, [3.0, 2.0, 1.0], IDENT)
    b = Bare(cuda_device, [chain, soup(R, 3, (20.0, 0.0, 0.0)) + (1.0, [0.0, 0.0, 0.0], IDENT)])
    _img, (top, deepest, _total) = b.check()
    assert top == 1 and 16 <= deepest <= pr.HEIGHT_MAX - 1, deepest


# ------------------------------------------------------------------------------------------------- 2. partial pose
def scene17():
    """the 17 meshes of test_trimesh_rays_gpu.test_pose_rebuild_matches_truth: a heightfield and 16 boxes and icospheres"""
    R = rng(21)
    bv, bi = box_mesh()
    iv, ii = icosphere()
    vx, idx = heightfield(64, 32.0)
    return [(vx, idx, 1.0, [0.0, 0.0, 0.0], IDENT)] + \
           [((bv, bi) if k % 2 else (iv, ii)) + (float(R.uniform(1, 3)), R.uniform(0, 30, 3), rand_quat(R)) for k in range(16)]


def part_rows(img, tf, m):
    """what belongs to mesh m alone: its slots' keys and triangles, its node rows"""
    k = int(tf[m + 1] - tf[m])
    r = int(img["part_root"][m])
    nodes = img["nodes"][r:r + k - 1] if k >= 2 else img["nodes"][:0]
    return img["key"][tf[m]:tf[m + 1]], img["tri"][tf[m]:tf[m + 1]], nodes


def test_partial_pose_equals_a_fresh_creation(cuda_device):
    meshes = scene17()
    b, fresh = Bare(cuda_device, meshes), Bare(cuda_device, meshes)
    tf = b.tri_first
    R = rng(22)
    pos = np.array([m[3] for m in meshes], np.float64)
    quat = np.array([m[4] for m in meshes], np.float32)
    b.check()
    for step, moved in enumerate(([3], [0], [1, 5, 16], list(range(17)))):
        before = b.w.read_static_meshes()
        pos[moved] += R.uniform(-2, 2, (len(moved), 3))
        quat[moved] = [rand_quat(R) for _ in moved]
        b.w.pose_static_meshes_some(moved, pos[moved], quat[moved])
        after, _got = b.check()
        assert b.w.static_meshes_parts_status()[3] == 0
        assert same_image(after, fresh.set(pos, quat)), step
        for m in range(17):
            rows_a, rows_b = part_rows(after, tf, m), part_rows(before, tf, m)
            if m in moved:
                assert same_bits(rows_a[2]["child"], rows_b[2]["child"]) and same_bits(rows_a[0], rows_b[0]), (step, m)
                assert not same_bits(rows_a[1], rows_b[1]), (step, m)
            else:
                assert all(same_bits(x, y) for x, y in zip(rows_a, rows_b)), (step, m)
    # the full pose of a set in parts: the same image again, by the refit alone
    pos += 0.25
    b.w.pose_static_meshes(pos, quat)
    assert same_image(b.check()[0], fresh.set(pos, quat))


# ------------------------------------------------------------------------------------------------- 3. same bits as the plain set
def bodies_over(n, seed):
    bd = synth.capsule_bodies(n, box=32.0, seed=seed)
    R = rng(seed)
    bd["pos"][:, 0], bd["pos"][:, 2] = R.uniform(1, 31, n), R.uniform(1, 31, n)
    bd["pos"][:, 1] = synth.terrain_y(bd["pos"][:, 0], bd["pos"][:, 2], 0.0, 1.0) + R.uniform(-0.4, 1.2, n)
    bd["lvel"][:] = 0
    return bd


def answers(sc, R):
    """every query that reads the mesh set, as host arrays in a fixed order"""
    w = sc.w
    out = list(sc.run())                                     # contacts_meshes: records, mesh_ref, total, capped pairs
    w.bp_index()
    n = 4096
    s = np.concatenate([R.uniform(-3, 35, (n // 2, 3)), np.stack([R.uniform(0, 32, n // 2), np.full(n // 2, 20.0),
                                                                   R.uniform(0, 32, n // 2)], 1)])
    d = np.concatenate([R.normal(size=(n // 2, 3)), np.tile([0, -1.0, 0], (n // 2, 1))])
    L = np.full(n, 50.0)
    rays = fetch(w.ray_cast(s, d, L, grid=False))
    out += rays + fetch(w.ray_cast(s, d, L, grid=True))
    nb = 512
    sb = np.arange(nb, dtype=np.uint32)
    delta = np.concatenate([R.uniform(-1, 1, (nb, 1)), R.uniform(-3, -0.5, (nb, 1)), R.uniform(-1, 1, (nb, 1))], 1).astype(np.float32)
    out += fetch(w.sweep_capsules_grid(sb, delta, grid=True))
    vel = np.concatenate([R.uniform(-3, 3, (nb, 1)), R.uniform(-6, 0, (nb, 1)), R.uniform(-3, 3, (nb, 1))], 1).astype(np.float32)
    out += fetch(w.slide(sb + nb, vel, np.zeros(nb, bool), 1.0 / 60.0, grid=True))
    w.bodies_aabb()                                          # the slide moved bodies: their boxes and the index again
    w.bp_index()
    ray_off = np.asarray(sc.bodies["yoffset"], float)[2 * nb:3 * nb] * 0.9
    out += fetch(w.ground_collide(sb + 2 * nb, ray_off, np.arange(nb) % 2 == 0, grid=True))
    out.append(w.pos.cpu().numpy())
    return out, rays


def test_every_query_answers_with_the_plain_sets_bits(cuda_device):
    meshes = scene17()
    bd = bodies_over(2048, 31)
    both = [Scene(cuda_device, copy.deepcopy(bd), meshes, cap=(1 << 20, 1 << 20), grow=3.0) for _ in range(2)]
    plain, parts = both
    parts.w.set_static_meshes(parts.mesh_static, *[[m[k] for m in meshes] for k in range(5)], parts=True)
    assert parts.w.static_meshes_parts_status()[0] and not plain.w.static_meshes_parts_status()[0]
    pos = np.array([m[3] for m in meshes], np.float64)
    quat = np.array([m[4] for m in meshes], np.float32)
    for round_ in range(2):
        if round_:                                           # one mesh moves: all poses here, that mesh alone there
            pos[4] += [0.5, -0.75, 0.25]
            quat[4] = rand_quat(rng(33))
            plain.w.pose_static_meshes(pos, quat)
            parts.w.pose_static_meshes_some([4], pos[[4]], quat[[4]])
        (a, rays), (b, _r) = answers(plain, rng(32 + round_)), answers(parts, rng(32 + round_))
        assert len(a) == len(b)
        for k, (x, y) in enumerate(zip(a, b)):
            assert same_bits(np.asarray(x), np.asarray(y)), (round_, k)
        assert a[2] > 200 and np.isin(rays[1], -2 - plain.mesh_static).sum() > 500, (a[2], "the queries found too little")


# ------------------------------------------------------------------------------------------------- 4. odd inputs
def test_odd_listings(cuda_device):
    meshes = scene17()
    b, fresh = Bare(cuda_device, meshes), Bare(cuda_device, meshes)
    R = rng(41)
    pos = np.array([m[3] for m in meshes], np.float64)
    quat = np.array([m[4] for m in meshes], np.float32)
    start = b.w.read_static_meshes()
    b.w.pose_static_meshes_some(np.zeros(0, np.uint32), np.zeros((0, 3)), np.zeros((0, 4), np.float32))    # n_moved == 0
    assert same_image(b.w.read_static_meshes(), start) and b.w.static_meshes_parts_status()[3] == 0
    b.w.pose_static_meshes_some([99], [[1.0, 2.0, 3.0]], [IDENT])                   # out of range: flagged, nothing else
    assert same_image(b.w.read_static_meshes(), start) and b.w.static_meshes_parts_status()[3] == RANGE
    b.w.pose_static_meshes(pos, quat)                                                # a full pose clears the flags
    assert same_image(b.w.read_static_meshes(), start) and b.w.static_meshes_parts_status()[3] == 0
    # listed more than once: the lowest list position wins, whatever the order of arrival
    first, second, other = R.uniform(0, 30, 3), R.uniform(0, 30, 3), R.uniform(0, 30, 3)
    q1, q2 = rand_quat(R), rand_quat(R)
    b.w.pose_static_meshes_some([5, 3, 5, 17, 5], [first, other, second, other, other], [q1, q2, q2, q1, q2])
    pos[5], quat[5], pos[3], quat[3] = first, q1, other, q2
    assert b.w.static_meshes_parts_status()[3] == RANGE | TWICE
    assert same_image(b.check()[0], fresh.set(pos, quat))
    b.w.pose_static_meshes(pos, quat)
    assert b.w.static_meshes_parts_status()[3] == 0 and same_image(b.w.read_static_meshes(), fresh.set(pos, quat))


def test_one_triangle_mesh_moves_and_an_empty_mesh_is_listed(cuda_device):
    tri = np.array([[-2, 0, -2], [-2, 0, 2], [2, 0, -2]], np.float32)
    one = np.array([[0, 1, 2]], np.uint16)
    bv, bi = box_mesh()
    none = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint16), 1.0, [0.0, 0.0, 0.0], IDENT)
    meshes = [(tri, one, 1.0, [0.0, 6.0, 0.0], IDENT), none, (bv, bi, 2.0, [10.0, 0.0, 0.0], IDENT),
              (tri, one, 1.0, [20.0, 6.0, 0.0], IDENT)]
    b, fresh = Bare(cuda_device, meshes), Bare(cuda_device, meshes)
    pos = np.array([m[3] for m in meshes], np.float64)
    quat = np.array([m[4] for m in meshes], np.float32)
    before = b.w.read_static_meshes()
    pos[3], quat[3] = [-7.0, 1.0, 2.0], rand_quat(rng(5))
    pos[1] = [1.0, 1.0, 1.0]                                 # the empty mesh: only its stored pose changes
    b.w.pose_static_meshes_some([3, 1], pos[[3, 1]], quat[[3, 1]])
    after, _got = b.check()
    assert same_image(after, fresh.set(pos, quat)) and not same_bits(after["tri"], before["tri"])
    assert b.w.static_meshes_parts_status()[3] == 0
    # all meshes empty: a listing is accepted and changes nothing
    e = Bare(cuda_device, [none, none])
    e.w.pose_static_meshes_some([1, 2], np.ones((2, 3)), [IDENT, IDENT])
    assert e.w.static_meshes_parts_status() == (True, 0, 0, RANGE) and e.check()[1] == (0, 0, 0)


def test_nan_position_hides_the_mesh_alone(cuda_device):
    meshes = scene17()
    both = [Scene(cuda_device, far_body(), meshes) for _ in range(2)]
    plain, parts = both
    parts.w.set_static_meshes(parts.mesh_static, *[[m[k] for m in meshes] for k in range(5)], parts=True)
    R = rng(51)
    n = 4096
    s = np.concatenate([R.uniform(-3, 35, (n // 2, 3)), np.stack([R.uniform(0, 32, n // 2), np.full(n // 2, 20.0),
                                                                   R.uniform(0, 32, n // 2)], 1)])
    d = np.concatenate([R.normal(size=(n // 2, 3)), np.tile([0, -1.0, 0], (n // 2, 1))])
    L = np.full(n, 50.0)
    was = fetch(parts.cast(s, d, L))
    victim = 1 + int(np.argmax([(was[1] == -2 - s_).sum() for s_ in parts.mesh_static[1:]]))   # the small mesh most rays hit
    on_it = was[1] == -2 - parts.mesh_static[victim]
    assert on_it.sum() > 3, on_it.sum()
    pos = np.array([m[3] for m in meshes], np.float64)
    quat = np.array([m[4] for m in meshes], np.float32)
    pos[victim, 1] = np.nan
    plain.w.pose_static_meshes(pos, quat)
    parts.w.pose_static_meshes_some([victim], pos[[victim]], quat[[victim]])
    a, b = fetch(plain.cast(s, d, L)), fetch(parts.cast(s, d, L))
    for x, y in zip(a, b):
        assert same_bits(x, y)
    assert not (b[1] == -2 - parts.mesh_static[victim]).any()
    for x, y in zip(was, b):                                 # the rays that hit another mesh, or nothing, answer as before
        assert same_bits(x[~on_it], y[~on_it])
    img = parts.w.read_static_meshes()
    tf = np.concatenate([[0], np.cumsum([len(m[1]) for m in meshes])])
    pr.check_image(img["nodes"], img["key"], img["tri"], img["part_root"], tf, parts.mesh_static)


# ------------------------------------------------------------------------------------------------- 5. capture
def captured(cuda_device, check_image):
    """a graph of pose_meshes and a ray cast, replayed twice (a second replay is where a stale stamp or bound would show)"""
    meshes = scene17()
    sc = Scene(cuda_device, far_body(), meshes)
    w = sc.w
    w.set_static_meshes(sc.mesh_static, *[[m[k] for m in meshes] for k in range(5)], parts=True)
    dev = w.device
    R = rng(61)
    n = 2048
    ray = np.zeros((n, 8))
    ray[:, 0:3], ray[:, 3:6], ray[:, 6] = R.uniform(-3, 35, (n, 3)), R.normal(size=(n, 3)), 50.0
    ray[: n // 2, 3:6] = [0.0, -1.0, 0.0]
    ray[: n // 2, 1] = 20.0
    rd = torch.from_numpy(ray).to(dev)
    moved = torch.tensor([2, 9], dtype=torch.int32, device=dev)
    pos0 = np.array([m[3] for m in meshes], np.float64)
    quat0 = np.array([m[4] for m in meshes], np.float32)
    p = torch.from_numpy(pos0[[2, 9]] + [[1.0, 0.5, -1.0], [-2.0, 0.0, 1.0]]).to(dev)
    q = torch.from_numpy(np.stack([rand_quat(R), rand_quat(R)])).to(dev)
    outs = lambda: [torch.full((n,), float("nan"), dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                    torch.full((n, 6), float("nan"), dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)]
    g, sg = w.body_geoms(), w.static_geoms()
    L = _lib.lib()

    def issue(o):
        _lib.check(L.clapgpu_trimesh_pose_meshes(physics._stream(), w._meshes, 2, moved.data_ptr(), p.data_ptr(), q.data_ptr()),
                   "clapgpu_trimesh_pose_meshes")
        _lib.check(L.clapgpu_ray_cast(physics._stream(), None, C.byref(g), C.byref(sg), w._meshes, n, rd.data_ptr(), None,
                                      *[t.data_ptr() for t in o]), "clapgpu_ray_cast")
    direct = outs()
    issue(direct)
    torch.cuda.synchronize()
    want = [t.cpu().numpy() for t in direct]
    image = w.read_static_meshes()
    w.pose_static_meshes(pos0, quat0)                        # back to the start: the replay has the same work to do
    unmoved = fetch(sc.cast(ray[:, 0:3], ray[:, 3:6], ray[:, 6]))
    assert not same_bits(unmoved[0], want[0])
    cap = outs()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            issue(cap)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        w.pose_static_meshes(pos0, quat0)
        for t, fresh_ in zip(cap, outs()):                  # as the direct call found them: a miss leaves dist and contact alone
            t.copy_(fresh_)
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(want, cap):
            assert same_bits(x, y.cpu().numpy())
        if check_image:
            assert same_image(w.read_static_meshes(), image) and w.static_meshes_parts_status()[3] == 0


def test_a_captured_partial_pose_and_ray_cast_replay_the_same_bits(cuda_device):
    captured(cuda_device, False)


def test_a_replayed_partial_pose_leaves_the_direct_calls_image(cuda_device):
    """The same graph, and the read-back image after each replay against the image the direct call left."""
    captured(cuda_device, True)


# ------------------------------------------------------------------------------------------------- 6. launch failures
def test_a_failed_partial_pose_is_mended_by_a_full_pose(cuda_device, monkeypatch):
    monkeypatch.setenv("CLAPGPU_TEST_HOOKS", "1")            # read by the library's first clapgpu_test_fail_after
    meshes = scene17()
    b, fresh = Bare(cuda_device, meshes), Bare(cuda_device, meshes)
    R = rng(71)
    pos = np.array([m[3] for m in meshes], np.float64)
    quat = np.array([m[4] for m in meshes], np.float32)
    moved = [0, 7, 12]
    pos[moved] += R.uniform(-2, 2, (3, 3))
    quat[moved] = [rand_quat(R) for _ in moved]
    want = fresh.set(pos, quat)
    dev = b.w.device
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    i_d, p_d, q_d = up(moved, np.int32), up(pos[moved], np.float64), up(quat[moved], np.float32)
    L = _lib.lib()
    failed = 0
    try:
        for k in range(16):
            L.clapgpu_test_fail_after(k)
            rc = L.clapgpu_trimesh_pose_meshes(physics._stream(), b.w._meshes, 3, i_d.data_ptr(), p_d.data_ptr(), q_d.data_ptr())
            L.clapgpu_test_fail_after(-1)
            torch.cuda.synchronize()
            if rc == _lib.OK:
                break
            failed += 1
            assert rc == _lib.ERR_UNKNOWN, rc
            b.w.pose_static_meshes(pos, quat)               # a full pose that succeeds makes the set whole
            assert same_image(b.check()[0], want), k
            b.w.pose_static_meshes([m[3] for m in meshes], [m[4] for m in meshes])
    finally:
        L.clapgpu_test_fail_after(-1)
    assert failed == 7, f"{failed} launches failed: is the hook armed (CLAPGPU_TEST_HOOKS)?"   # fill, mark, take, bake, centres, keys, top
    assert same_image(b.check()[0], want)
