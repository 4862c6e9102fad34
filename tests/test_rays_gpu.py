"""GPU: batched ray casts (clapgpu_bp_index / clapgpu_ray_cast / clapgpu_bodies_ground_collide) against the
long-double truth of tests/rayref.py, the grid path against the brute-force scan bit for bit, skip / ties / unresolved
rules, broadphase results unchanged by an index, and phys_body_ground_collide's arithmetic restated in numpy."""
import math

import numpy as np
import pytest

from clap_amd import _lib, synth
from meshscene import far_body, fetch, rng, same_bits, unit
import rayref

pytestmark = pytest.mark.gpu

SPHERE, CAPSULE, BOX, OTHER = _lib.GEOM_SPHERE, _lib.GEOM_CAPSULE, _lib.GEOM_BOX, _lib.GEOM_OTHER


def static_world(geoms, cuda_device, bodies=None):
    """A world whose statics are the given geoms (dicts as rayref takes them): AABBs for the broadphase."""
    from clap_amd import physics
    n = len(geoms)
    bb = np.zeros((n, 6))
    kind = np.zeros(n, np.uint8)
    pos, axis, rad, length = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    for i, g in enumerate(geoms):
        if g["kind"] == "box":
            bb[i], kind[i] = g["aabb"], BOX
        elif g["kind"] == "other":
            bb[i], kind[i] = g["aabb"], OTHER
        else:
            r, p = g["radius"], np.asarray(g["pos"], float)
            ax = np.asarray(g.get("axis", [0, 0, 1.0]), float)
            l = g.get("length", 0.0)
            ext = np.abs(ax) * l / 2 + r
            bb[i, 0::2], bb[i, 1::2] = p - ext, p + ext
            kind[i] = CAPSULE if g["kind"] == "capsule" else SPHERE
            pos[i], axis[i], rad[i], length[i] = p, ax, r, l
    w = physics.PhysWorld(bodies or far_body(), bb, device=cuda_device)
    w.set_static_geoms(kind, pos, axis, rad, length)
    return w


def fixture_rays(seed):
    """(geom, start, dir, length, class) per case."""
    R = rng(seed)
    cases = []
    for _ in range(60):                                                     # sphere, from outside
        c, r = R.uniform(-5, 5, 3), R.uniform(0.2, 2.0)
        s = c + unit(R.normal(size=3)) * R.uniform(r + 0.5, 10)
        tgt = c + unit(R.normal(size=3)) * r * R.uniform(0, 0.9)
        cases.append((dict(kind="sphere", pos=c, radius=r), s, tgt - s, 30.0, "sphere"))
    for _ in range(60):                                                     # capsule side and cap
        c, r, l = R.uniform(-5, 5, 3), R.uniform(0.2, 1.0), R.uniform(0.5, 3.0)
        ax = unit(R.normal(size=3))
        perp = unit(np.cross(ax, R.normal(size=3)))
        tgt = c + ax * R.uniform(-0.4, 0.4) * l + perp * r * R.uniform(0, 0.5)
        s = tgt + perp * R.uniform(2, 8) + ax * R.uniform(-0.2, 0.2)
        cases.append((dict(kind="capsule", pos=c, axis=ax, radius=r, length=l), s, tgt - s, 30.0, "capsule_side"))
        tgt = c + ax * l / 2 + perp * r * R.uniform(0, 0.5)
        s = c + ax * (l / 2 + R.uniform(2, 8)) + perp * R.uniform(-0.1, 0.1)
        cases.append((dict(kind="capsule", pos=c, axis=ax, radius=r, length=l), s, tgt - s, 30.0, "capsule_cap"))
    for _ in range(60):                                                     # box: face, edge, corner
        lo = R.uniform(-5, 5, 3)
        hi = lo + R.uniform(0.5, 3, 3)
        bb = np.empty(6)
        bb[0::2], bb[1::2] = lo, hi
        g = dict(kind="box", aabb=bb)
        tgt = R.uniform(lo, hi)
        a = R.integers(3)
        tgt[a] = lo[a]
        d = unit(R.normal(size=3))
        d[a] = abs(d[a]) + 0.3
        cases.append((g, tgt - d * R.uniform(2, 8), d, 30.0, "box_face"))
        e = tgt.copy()
        b2 = (a + 1) % 3
        e[b2] = lo[b2]
        dd = d.copy()
        dd[b2] = abs(dd[b2]) + 0.3
        cases.append((g, e - dd * 4, dd, 30.0, "box_edge"))
        corner = lo.copy()
        dc = np.abs(unit(R.normal(size=3))) + 0.2
        cases.append((g, corner - dc * 3, dc, 30.0, "box_corner"))
    for _ in range(40):                                                     # starts inside each kind
        c, r = R.uniform(-5, 5, 3), R.uniform(0.5, 2.0)
        cases.append((dict(kind="sphere", pos=c, radius=r), c + unit(R.normal(size=3)) * r * 0.5, R.normal(size=3), 30.0,
                      "inside_sphere"))
        ax, l = unit(R.normal(size=3)), R.uniform(0.5, 3.0)
        cases.append((dict(kind="capsule", pos=c, axis=ax, radius=r, length=l), c + ax * l * 0.3, R.normal(size=3), 30.0,
                      "inside_capsule"))
        bb = np.empty(6)
        bb[0::2], bb[1::2] = c - 1.0, c + R.uniform(0.5, 2, 3)
        cases.append((dict(kind="box", aabb=bb), c + R.uniform(-0.5, 0.4, 3), R.normal(size=3), 30.0, "inside_box"))
    for _ in range(40):                                                     # tangent: a hair inside the sphere's edge
        c, r = R.uniform(-5, 5, 3), R.uniform(0.5, 2.0)
        d = unit(R.normal(size=3))
        perp = unit(np.cross(d, R.normal(size=3)))
        s = c + perp * r * (1 - 1e-9) - d * 5
        cases.append((dict(kind="sphere", pos=c, radius=r), s, d, 30.0, "tangent"))
    for _ in range(40):                                                     # far from the origin, tiny radii
        c, r = 1e4 + R.uniform(-50, 50, 3), R.uniform(5e-4, 2e-3)
        tgt = c + unit(R.normal(size=3)) * r * 0.5
        s = tgt + unit(R.normal(size=3)) * 0.05
        cases.append((dict(kind="sphere", pos=c, radius=r), s, tgt - s, 1.0, "far_tiny"))
    return cases


def run_cases(cases, cuda_device, lengths=None):
    """One world per case group (each static well apart from the others), rays cast brute force."""
    out = []
    for k, (g, s, d, L, cls) in enumerate(cases):
        off = np.array([0.0, 0.0, 200.0 * k]) if cls != "far_tiny" else np.array([0.0, 0.0, 0.5 * k])
        g2 = dict(g)
        if "pos" in g2:
            g2["pos"] = np.asarray(g2["pos"]) + off
        if "aabb" in g2:
            g2["aabb"] = np.asarray(g2["aabb"]) + np.repeat(off, 2)
        out.append((g2, np.asarray(s) + off, np.asarray(d, float), L if lengths is None else lengths[k], cls))
    w = static_world([c[0] for c in out], cuda_device)
    dist, hit, contact, flags = fetch(w.ray_cast([c[1] for c in out], [c[2] for c in out], [c[3] for c in out], grid=False))
    return out, dist, hit, contact, flags


def test_colliders_against_long_double_truth(cuda_device):
    cases = fixture_rays(11)
    out, dist, hit, contact, flags = run_cases(cases, cuda_device)
    counts = {}
    for k, (g, s, d, L, cls) in enumerate(out):
        ref = rayref.cast(g, s, d, L)
        assert flags[k] == 0
        if ref is None:
            assert hit[k] == -1, (cls, k)
            continue
        tol, grazing = rayref.tolerance(g, s, d, L, ref)
        if grazing and hit[k] == -1:
            continue
        assert hit[k] == -2 - k, (cls, k, hit[k])
        assert abs(dist[k] - float(ref[0])) <= tol, (cls, k, dist[k], float(ref[0]), tol)
        assert np.allclose(contact[k, :3], np.asarray(ref[1], float), atol=tol * 2 + 1e-12), (cls, k)
        n = contact[k, 3:]
        assert abs(np.linalg.norm(n) - 1) < 1e-12
        if cls in ("box_edge", "box_corner"):                              # any face normal of the edge / corner
            assert np.count_nonzero(n) == 1 and float(np.dot(n, np.asarray(ref[2], float))) > 0.5, (cls, k, n)
        elif not grazing:
            assert np.allclose(n, np.asarray(ref[2], float), atol=1e-5), (cls, k, n, ref[2])
        counts[cls] = counts.get(cls, 0) + 1
    for cls, need in (("sphere", 50), ("capsule_side", 50), ("capsule_cap", 40), ("box_face", 50), ("box_edge", 40),
                      ("box_corner", 40), ("inside_sphere", 40), ("inside_capsule", 40), ("inside_box", 40),
                      ("tangent", 10), ("far_tiny", 35)):
        assert counts.get(cls, 0) >= need, (cls, counts)


def test_hit_at_length_and_one_ulp_short(cuda_device):
    cases = [c for c in fixture_rays(12) if c[4] in ("sphere", "capsule_side", "box_face")]
    out, dist, hit, _c, _f = run_cases(cases, cuda_device)
    ok = hit != -1
    assert ok.sum() >= 100
    sel = [c for c, h in zip(cases, ok) if h]
    d = dist[ok]
    _o, d2, h2, _c2, _f2 = run_cases(sel, cuda_device, lengths=d)                        # length == depth: a hit
    assert (h2 != -1).all() and np.array_equal(d2, d)
    _o, d3, h3, _c3, _f3 = run_cases(sel, cuda_device, lengths=np.nextafter(d, 0))      # the hit one ulp past length
    assert (h3 == -1).all()


def grid_scene(cuda_device, oversized=False):
    from clap_amd import physics
    b = synth.capsule_bodies(262_144, box=60.0, seed=4)
    b["lvel"][:] = 0
    if oversized:                                                          # a sphere with an AABB edge of 1.8 cells, above the rest,
        b["radius"][7] = b["cell"] * 0.9                                   # its centre at 0.95 of a cell in x
        b["length"][7] = 0.0
        b["pos"][7] = [10.95 * b["cell"], 100.0, 30.0]
    R = rng(5)
    ns = 5000
    lo = R.uniform(-5, 65, (ns, 3))
    ext = R.uniform(0.1, 3.0, (ns, 3))
    bb = np.empty((ns, 6))
    bb[:, 0::2], bb[:, 1::2] = lo, lo + ext
    bb[0] = [-1e3, 1e3, -10.0, 0.0, -1e3, 1e3]                             # a ground slab: the large list
    bb[1] = [-100, 100, 20, 21, -100, 100]                                 # large as well
    kind = R.choice([SPHERE, CAPSULE, BOX, OTHER], ns, p=[0.3, 0.3, 0.3, 0.1]).astype(np.uint8)
    kind[0] = BOX
    kind[1] = OTHER
    c, axis, r, length = synth.geoms_of_aabbs(bb, kind)
    w = physics.PhysWorld(b, bb, pair_capacity=4_000_000, static_pair_capacity=8_000_000, device=cuda_device)
    w.set_static_geoms(kind, c, axis, r, length)
    return w, b, bb, kind


def grid_rays(cell, n=65536, seed=9):
    R = rng(seed)
    s = R.uniform(-5, 65, (n, 3))
    d = R.normal(size=(n, 3))
    L = R.choice([2.0, 4.0, 20.0, 1e6], n)
    q = n // 8
    d[:q] = 0
    d[np.arange(q), R.integers(3, size=q)] = R.choice([-1.0, 1.0], q)        # axis-aligned
    s[q:2 * q] = np.round(s[q:2 * q] / cell) * cell                          # on cell boundaries
    s[2 * q:3 * q] = np.round(s[2 * q:3 * q] / (4 * cell)) * 4 * cell        # on block boundaries
    s[3 * q:4 * q, 1] = np.round(s[3 * q:4 * q, 1] / cell) * cell            # along a cell boundary plane
    d[3 * q:4 * q, 1] = 0
    corner = np.round(s[4 * q:5 * q] / cell) * cell                          # through cell corners
    d[4 * q:5 * q] = corner + cell * R.integers(1, 4, (q, 3)) - s[4 * q:5 * q]
    d[5 * q:5 * q + 64, 1] = -1
    d[5 * q:5 * q + 64, 0::2] = 0
    s[5 * q:5 * q + 64, 1] = 80                                              # straight down, 1e6 long, into the slab
    L[5 * q:5 * q + 64] = 1e6
    L[5 * q + 64:5 * q + 80] = 0.0                                           # zero length
    d[5 * q + 80:5 * q + 90] = 0.0                                           # zero direction
    d[5 * q + 90:5 * q + 100, 1] = np.nan                                    # NaN direction
    L[5 * q + 100:5 * q + 104] = -1.0
    return s, d, L


def test_grid_equals_brute_force(cuda_device):
    w, b, _bb, _kind = grid_scene(cuda_device)
    w.bp_index()
    assert w.bp_index_status() == 0
    s, d, L = grid_rays(w.cell)
    skip = np.where(np.arange(len(L)) % 5 == 0, np.arange(len(L)) % w.n, -1).astype(np.int32)
    g = fetch(w.ray_cast(s, d, L, skip=skip, grid=True))
    f = fetch(w.ray_cast(s, d, L, skip=skip, grid=False))
    for a, c in zip(g, f):
        assert same_bits(a, c)
    dist, hit, _contact, flags = g
    assert (hit >= 0).sum() > 1000 and (hit <= -2).sum() > 500
    assert (flags & _lib.RAY_INVALID).sum() == 24                          # zero / NaN directions, negative lengths
    assert (flags & _lib.RAY_UNRESOLVED).sum() > 10


def test_oversized_body_falls_back_and_flag_clears(cuda_device):
    w, b, _bb, _kind = grid_scene(cuda_device, oversized=True)
    w.bp_index()
    assert w.bp_index_status() == 1 and (w.broadphase_status() & 1)
    s, d, L = grid_rays(w.cell, n=2048, seed=10)
    # straight down through the oversized sphere's rim, 0.85 cell from its centre in x: the cells a piece looks up start
    # at x = (10.95 + 0.85 - 0.5) cells, past the centre's cell 10, so only the scan of every geom can find it
    c = w.cell
    s[:16] = b["pos"][7] + np.stack([np.full(16, 0.85 * c), np.full(16, 3.0), np.linspace(-0.2, 0.2, 16) * c], 1)
    d[:16] = [0, -1, 0]
    L[:16] = 5
    assert math.floor((s[0, 0] - 0.5 * c * (1 + 1e-9)) / c) > math.floor(b["pos"][7][0] / c)
    g = fetch(w.ray_cast(s, d, L, grid=True))
    f = fetch(w.ray_cast(s, d, L, grid=False))
    for a, c2 in zip(g, f):
        assert same_bits(a, c2)
    assert (g[1][:16] == 7).all()
    # the body shrinks back; a frame's collide + the next index: this index's flag clears, the sticky status keeps bit 0
    w.radius[7] = float(b["cell"]) * 0.1
    w.bodies_aabb()
    w.broadphase()
    w.bp_index()
    assert w.bp_index_status() == 0 and (w.broadphase_status() & 1)
    assert int(w.bp_index_status()) & 2 == 0
    g = fetch(w.ray_cast(s, d, L, grid=True))
    f = fetch(w.ray_cast(s, d, L, grid=False))
    for a, c in zip(g, f):
        assert same_bits(a, c)


def test_stale_or_missing_index_is_refused(cuda_device):
    from clap_amd import physics
    w = physics.PhysWorld(synth.capsule_bodies(2000, box=20.0, seed=3), synth.static_boxes(20, 20.0), device=cuda_device)
    s, d, L = np.zeros((4, 3)), np.tile([0, -1.0, 0], (4, 1)), np.ones(4)
    with pytest.raises(_lib.ClapGpuError):
        w.ray_cast(s, d, L, grid=True)                                      # never indexed
    w.bp_index()
    w.ray_cast(s, d, L, grid=True)
    w.broadphase()
    with pytest.raises(_lib.ClapGpuError):
        w.ray_cast(s, d, L, grid=True)                                      # a collide since
    w.bp_index()
    w.world_step(1 / 120, prebin=True)
    with pytest.raises(_lib.ClapGpuError):
        w.ray_cast(s, d, L, grid=True)                                      # a prebinning step since
    w.bp_index()
    n = w.n
    w.n = n - 1
    with pytest.raises(_lib.ClapGpuError):
        w.ray_cast(s, d, L, grid=True)                                      # another body count
    w.n = n
    w.bp_invalidate()
    with pytest.raises(_lib.ClapGpuError):
        w.ray_cast(s, d, L, grid=True)
    with pytest.raises(_lib.ClapGpuError):
        w.bp_index_status()


def test_skip_and_ties(cuda_device):
    # three spheres of the same radius at the same depth along x: a body and two statics; plus a box face at the same depth
    from clap_amd import physics
    b = synth.sphere_bodies(3, box=1.0, seed=2)
    b["lvel"][:] = 0
    b["radius"][:] = 0.5
    b["pos"][:] = [[10, 0, 0], [10, 0, 0], [-50, -50, -50]]                # bodies 0 and 1 coincide
    geoms = [dict(kind="sphere", pos=[10, 0, 0], radius=0.5), dict(kind="sphere", pos=[10, 0, 0], radius=0.5),
             dict(kind="box", aabb=[9.5, 12, -1, 1, -1, 1])]
    w = static_world(geoms, cuda_device, bodies=b)
    s, d = np.tile([0.0, 0, 0], (6, 1)), np.tile([1.0, 0, 0], (6, 1))
    skip = np.array([-1, 0, 1, -2, -3, -4], np.int32)
    for grid in (False, True):
        if grid:
            w.bp_index()
        dist, hit, _c, _f = fetch(w.ray_cast(s, d, 20.0, skip=skip, grid=grid))
        assert (dist == 9.5).all()
        assert list(hit) == [0, 1, 0, 0, 0, 0]
    # only statics: lower static index first; skipping a static moves on to the next one
    b["pos"][:2] = [[-50, 50, -50], [-50, 40, -50]]
    w = static_world(geoms, cuda_device, bodies=b)
    dist, hit, _c, _f = fetch(w.ray_cast(s[:4], d[:4], 20.0, skip=np.array([-1, -2, -3, -4], np.int32), grid=False))
    assert list(hit) == [-2, -3, -2, -2]
    assert (dist == 9.5).all()


def test_unresolved_matches_slab_test(cuda_device):
    R = rng(21)
    geoms, rays = [], []
    for k in range(200):
        z = 30.0 * k
        solid = dict(kind="box", aabb=[4, 6, -1, 1, z - 1, z + 1])
        tri = [1, 2, -1, 1, z - 1, z + 1] if k % 2 else [8, 9, -1, 1, z - 1, z + 1]   # before or after the box
        if k % 5 == 0:
            tri = [1, 2, 5, 6, z - 1, z + 1]                                            # off the ray
        geoms += [solid, dict(kind="other", aabb=tri)]
        L = 20.0 if k % 7 else 3.0                                                     # 3: ends before the box
        rays.append(([0.0, R.uniform(-0.5, 0.5), z + R.uniform(-0.5, 0.5)], [1.0, 0, 0], L))
    w = static_world(geoms, cuda_device)
    s, d, L = (np.array([r[i] for r in rays], float) for i in range(3))
    for grid in (False, True):
        if grid:
            w.bp_index()
        dist, hit, _c, flags = fetch(w.ray_cast(s, d, L, grid=grid))
        for k in range(200):
            bb = np.array(geoms[2 * k + 1]["aabb"], float)
            t = np.array([(bb[0] - s[k, 0]) / d[k, 0], (bb[1] - s[k, 0]) / d[k, 0]])
            inside = bb[2] <= s[k, 1] <= bb[3] and bb[4] <= s[k, 2] <= bb[5]
            enter = max(t.min(), 0.0) if inside and t.max() >= 0 and max(t.min(), 0.0) <= L[k] else math.inf
            best = dist[k] if hit[k] != -1 else math.inf
            assert bool(flags[k] & _lib.RAY_UNRESOLVED) == (enter <= best and enter < math.inf), (k, enter, best)


def _pairs(w):
    out = w.download()
    return out["pairs"].copy(), out["static_pairs"].copy()


def test_index_leaves_collide_results_alone(cuda_device):
    from clap_amd import physics
    b = synth.capsule_bodies(40_000, box=32.0, seed=8)
    st = synth.static_boxes(64, 32.0)
    ref = physics.PhysWorld(b, st, device=cuda_device)
    w = physics.PhysWorld(b, st, device=cuda_device)
    for x in (ref, w):
        x.broadphase()
        x.contacts_geoms_both()
    w.bp_index()                                                           # index -> collide
    w.broadphase()
    ref.broadphase()
    assert all(np.array_equal(a, c) for a, c in zip(_pairs(w), _pairs(ref)))
    for x in (ref, w):
        x.world_step(1 / 120, prebin=True)
    w.bp_index()                                                           # step_prebin -> index -> collide
    for x in (ref, w):
        x.broadphase()
        x.contacts_geoms_both()
    assert all(np.array_equal(a, c) for a, c in zip(_pairs(w), _pairs(ref)))
    dt = np.dtype([("b", np.uint8, 160)])
    cw, cr = w.download_contacts2(dt), ref.download_contacts2(dt)
    for k in cw:
        assert cw[k][1] == cr[k][1] and same_bits(cw[k][0], cr[k][0])


def test_frame_with_index_between_frames(cuda_device):
    from clap_amd import entities, frame, physics
    scene = synth.pad_levels(synth.entities_flat(2000, seed=3))
    b = synth.capsule_bodies(2000, box=20.0, seed=12)
    outs = []
    for with_index in (False, True):
        batch = entities.EntityBatch(scene, cuda_device)
        w = physics.PhysWorld(b, synth.static_boxes(16, 20.0), device=cuda_device)
        loop = frame.FrameLoop(batch, synth.camera(pos=(0, 10, 60)), world=w, contacts=True, prebin=True)
        for f in range(3):
            loop.clap_frame(f / 60, 1 / 60)
            if with_index:
                w.bp_index()
        loop.clap_frame(3 / 60, 1 / 60)
        outs.append((_pairs(w), w.download_contacts2(np.dtype([("b", np.uint8, 160)])), w.download()["pos"]))
    (p0, c0, x0), (p1, c1, x1) = outs
    assert all(np.array_equal(a, c) for a, c in zip(p0, p1))
    assert same_bits(x0, x1)
    for k in c0:
        assert c0[k][1] == c1[k][1] and same_bits(c0[k][0], c1[k][0])


def ground_reference(pos, yoffset, ray_off, grounded, dist, hit):
    """physics.c:695-744 in numpy float64 / float32 on the brute-force ray results."""
    roff = ray_off - 0.05
    ray_len = yoffset - roff + 1e-3
    n = len(pos)
    res = np.zeros(n, bool)
    dy = np.zeros(n, np.float32)
    branch = np.full(n, -1)
    for k in range(n):
        if hit[k] == -1:
            continue
        dk = dist[k]
        if grounded[k] and dk > ray_len[k]:
            dy[k], res[k], branch[k] = np.float32(-(dk - ray_len[k])), True, 0
        elif dk < ray_len[k]:
            dy[k], res[k], branch[k] = np.float32(ray_len[k] - dk), True, 1
        elif dk > ray_len[k]:
            branch[k] = 2
        else:
            res[k], branch[k] = True, 3
    return res, dy, branch


def test_ground_collide_against_reference_arithmetic(cuda_device):
    from clap_amd import physics
    R = rng(31)
    n = 4096
    b = synth.capsule_bodies(n, box=120.0, seed=14)
    b["lvel"][:] = 0
    ray_off = np.asarray(b["yoffset"], float) * R.uniform(0.7, 1.0, n)
    rl = b["yoffset"] - (ray_off - 0.05) + 1e-3
    b["pos"][:, 1] = b["yoffset"] + 1e-3 + rl * R.uniform(-0.9, 0.9, n)       # over a ground slab at y <= 0, within reach
    b["pos"][R.uniform(0, 1, n) < 0.15, 1] += 5.0                            # out of reach: misses
    statics = np.array([[-1e3, 1e3, -10.0, 0.0, -1e3, 1e3], [200, 201, 0, 1, 200, 201], [-200, -199, 0, 1, 5, 6]])
    w = physics.PhysWorld(b, statics, device=cuda_device)
    grounded = R.uniform(0, 1, n) < 0.5
    sel = np.arange(0, n, 2).astype(np.uint32)
    pos0 = w.pos.cpu().numpy().copy()
    # the same rays through clapgpu_ray_cast, brute force
    roff = ray_off[sel] - 0.05
    ray_len = b["yoffset"][sel] - roff + 1e-3
    start = np.stack([pos0[sel, 0].astype(np.float32), (pos0[sel, 1] - roff).astype(np.float32),
                      pos0[sel, 2].astype(np.float32)], 1).astype(np.float64)
    rd, rh, rc, rf = fetch(w.ray_cast(start, np.tile([0, -1.0, 0], (len(sel), 1)), ray_len * 2,
                                      skip=sel.astype(np.int32), grid=False))
    w.bp_index()
    out, normal, dist, hit, flags = fetch(w.ground_collide(sel, ray_off[sel], grounded[sel], grid=True))
    assert np.array_equal(hit, rh) and np.array_equal((flags & 3), rf)
    h = hit != -1
    assert same_bits(dist[h], rd[h])
    assert np.array_equal(normal[h], rc[h, 3:].astype(np.float32))
    res, dy, branch = ground_reference(pos0[sel], b["yoffset"][sel], ray_off[sel], grounded[sel], rd, rh)
    assert np.array_equal(out.astype(bool), res)
    for br in (-1, 0, 1, 2):                                                 # the miss and the three branches
        assert (branch == br).sum() >= 100, (br, np.bincount(branch + 1))
    pos1 = w.pos.cpu().numpy()
    exp = pos0.copy()
    moved = sel[(branch == 0) | (branch == 1)]
    exp[moved, 1] = pos0[moved, 1] + dy[(branch == 0) | (branch == 1)].astype(np.float64)
    assert same_bits(pos1, exp)
    aabb1, axis1, rec1 = w.aabb.cpu().numpy().copy(), w.axis.cpu().numpy().copy(), w.geom_records.cpu().numpy().copy()
    w.bodies_aabb()
    assert same_bits(aabb1, w.aabb.cpu().numpy()) and same_bits(axis1, w.axis.cpu().numpy())
    assert same_bits(rec1, w.geom_records.cpu().numpy())


def test_ground_collide_misses_and_moved_target(cuda_device):
    from clap_amd import physics
    b = synth.sphere_bodies(300, box=1.0, seed=3)
    b["lvel"][:] = 0
    b["radius"][:] = 0.5
    b["yoffset"][:] = 0.5
    b["pos"][:] = np.stack([np.arange(300) * 3.0, np.full(300, 50.0), np.zeros(300)], 1)   # nothing below: misses
    b["pos"][1] = [0.0, 51.03, 0.0]                                          # stacked on body 0
    w = physics.PhysWorld(b, np.array([[-1e3, 1e3, -10.0, 0.0, 200, 300]]), device=cuda_device)
    sel = np.arange(300, dtype=np.uint32)
    ray_off = np.full(300, 0.5)
    grounded = np.ones(300, bool)
    out, normal, dist, hit, flags = fetch(w.ground_collide(sel, ray_off, grounded, grid=False))
    assert (hit[2:] == -1).sum() >= 100 and not out[2:].any()
    assert hit[1] == 0 and not (flags[1] & _lib.RAY_MOVED_TARGET)          # body 0 hit nothing, so it did not move
    b["pos"][0, 1] = 0.53                                                    # its ray reaches the slab: grounded, moves down
    b["pos"][1, 1] = 1.56                                                    # ... and body 1's ray reaches body 0
    w2 = physics.PhysWorld(b, np.array([[-1e3, 1e3, -10.0, 0.0, -1e3, 1e3]]), device=cuda_device)
    out, normal, dist, hit, flags = fetch(w2.ground_collide(sel[:2], ray_off[:2], grounded[:2], grid=False))
    assert hit[0] == -2 and hit[1] == 0
    assert flags[1] & _lib.RAY_MOVED_TARGET and not flags[0] & _lib.RAY_MOVED_TARGET


def test_captured_prebin_frames_with_an_index_between_replays(cuda_device):
    """FrameLoop.capture(prebin=True): its collide has no bin launch and finds the counters the step left.  An index
    between replays keeps them: pairs, contacts and poses equal a run without the index.  After a replay the index is
    stale (the device's bin count moved on): rays through it scan every geom, and the status says so."""
    from clap_amd import entities, frame, physics
    scene = synth.pad_levels(synth.entities_flat(2000, seed=3))
    b = synth.capsule_bodies(4000, box=20.0, seed=12)
    dt = 1.0 / 120.0
    outs = []
    for with_index in (False, True):
        batch = entities.EntityBatch(scene, cuda_device)
        w = physics.PhysWorld(b, synth.static_boxes(16, 20.0), device=cuda_device)
        loop = frame.FrameLoop(batch, synth.camera(pos=(0, 10, 60)), world=w, contacts=True, prebin=True)
        loop.capture(dt, warmup_now=0.0)
        for f in range(1, 6):
            loop.clap_frame_replay(f * dt)
            if with_index:
                if f > 1:
                    assert w.bp_index_status() & 2                         # the replay binned again: stale
                    s, d, L = grid_rays(w.cell, n=512, seed=f)
                    s = s / 65 * 20
                    g = fetch(w.ray_cast(s, d, L, grid=True))
                    br = fetch(w.ray_cast(s, d, L, grid=False))
                    for a, c in zip(g, br):
                        assert same_bits(a, c)
                w.bp_index()
                assert w.bp_index_status() == 0
        torch_sync()
        outs.append((_pairs(w), w.download_contacts2(np.dtype([("b", np.uint8, 160)])), w.download()["pos"]))
    (p0, c0, x0), (p1, c1, x1) = outs
    assert len(p0[0]) > 1000
    assert all(np.array_equal(a, c) for a, c in zip(p0, p1))
    assert same_bits(x0, x1)
    for k in c0:
        assert c0[k][1] == c1[k][1] and same_bits(c0[k][0], c1[k][0])


def torch_sync():
    import torch
    torch.cuda.synchronize()


def test_start_on_a_sphere_surface_moving_outward(cuda_device):
    """The header's convention for a start exactly on the surface (C == 0): a hit at depth 0 with the OUTWARD normal,
    whether the ray leaves the sphere or enters it (the near root is 0 either way)."""
    w = static_world([dict(kind="sphere", pos=[0.0, 0.0, 0.0], radius=1.0)], cuda_device)
    dist, hit, contact, _f = fetch(w.ray_cast([[1.0, 0, 0], [1.0, 0, 0]], [[1.0, 0, 0], [-1.0, 0, 0]], 5.0, grid=False))
    assert list(hit) == [-2, -2]
    assert dist[0] == 0.0 and list(contact[0, 3:]) == [1.0, 0.0, 0.0]
    assert dist[1] == 0.0 and list(contact[1, 3:]) == [1.0, 0.0, 0.0]


def test_ground_collide_body_listed_twice(cuda_device):
    from clap_amd import physics
    b = synth.sphere_bodies(4, box=1.0, seed=3)
    b["lvel"][:] = 0
    b["radius"][:] = 0.5
    b["yoffset"][:] = 0.5
    b["pos"][:] = [[0.0, 0.52, 0.0], [3.0, 0.52, 0.0], [6.0, 0.52, 0.0], [9.0, 0.52, 0.0]]
    w = physics.PhysWorld(b, np.array([[-1e3, 1e3, -10.0, 0.0, -1e3, 1e3]]), device=cuda_device)
    pos0 = w.pos.cpu().numpy().copy()
    out, _n, _d, hit, flags = fetch(w.ground_collide(np.array([0, 1, 0, 2], np.uint32), np.full(4, 0.5), np.ones(4, bool),
                                                     grid=False))
    assert (flags[[0, 2]] & _lib.RAY_INVALID).all() and not out[[0, 2]].any()
    assert not (flags[[1, 3]] & _lib.RAY_INVALID).any() and out[[1, 3]].all()
    pos1 = w.pos.cpu().numpy()
    assert same_bits(pos1[0], pos0[0]) and same_bits(pos1[3], pos0[3])
    assert pos1[1, 1] != pos0[1, 1] and pos1[2, 1] != pos0[2, 1]
