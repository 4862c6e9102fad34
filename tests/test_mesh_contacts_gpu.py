"""GPU: contacts of sphere and capsule bodies against static triangle meshes (clapgpu_contacts_meshes), the capsule sweep
against meshes (clapgpu_sweep_capsules) and the frame's mesh contact pass, against the truth of
tests/meshcontactref.py.  Depth and normal must agree within TOL (relative to the scene's scale); pos must lie on the
closest set; a decision the truth flags as within the rounding margin may go either way."""
import os

import numpy as np
import pytest
import torch

from clap_amd import _lib, synth
from clap_amd.synth import box_mesh, heightfield
import meshcontactref as mc
import meshscene
from meshscene import C2, IDENT, rng
import trimeshref as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
RAW = np.dtype([("b", np.uint8, 160)])


def Scene(dev, bodies, meshes, cap=1 << 20, **kw):
    """meshscene.Scene as these tests build it: the meshes' boxes grown a little, both pair capacities `cap`"""
    return meshscene.Scene(dev, bodies, meshes, cap=(cap, cap), grow=1e-6, **kw)


def on_closest_set(pos, seg, depth, r, tri, tol):
    """pos lies on the triangle and at distance r - depth from the segment"""
    a, b = seg
    u = b - a
    L2 = u @ u
    s = 0.0 if L2 == 0 else min(max(((pos - a) @ u) / L2, 0.0), 1.0)
    dist = np.linalg.norm(a + s * u - pos)
    bary = mc._bary(*(x.astype(mc.LD) for x in (tri[0], tri[1] - tri[0], tri[2] - tri[0], pos)))
    return abs(dist - (r - depth)) <= tol and float(bary.min()) >= -1e-9


def check(sc, rec, ref, total, tol_scale=1.0):
    truth, capped, near, segs, pairs = sc.truth()
    tol = TOL * tol_scale
    got = {(int(p), int(t)): k for k, (p, t) in enumerate(ref)}
    keys = [(int(p), int(t)) for p, t in ref]
    assert keys == sorted(keys), "canonical order: ascending pair, then triangle"
    assert len(rec) == total
    compared = 0
    for p, t, cs, mg in truth:
        if (p, t) not in got:
            assert mg, ("missing", p, t)
            continue
        r = rec[got[(p, t)]]
        if mg:
            continue
        assert r["nc"] == len(cs), (p, t, r["nc"], len(cs))
        body, st = pairs[p]
        tri = sc.tris[int(st) - sc.base][t]
        rad = float(sc.bodies["radius"][body])
        for j, (cp, cn, cd) in enumerate(cs):
            gpos, gn, gd = (r["pos"], r["normal"], r["depth"]) if j == 0 else (r["pos2"], r["normal2"], r["depth2"])
            assert abs(gd - float(cd)) <= tol, (p, t, gd, cd)
            assert np.abs(gn - np.asarray(cn, float)).max() <= tol * 10, (p, t, gn, cn)
            # faces and the parallel pair: the one pos; the closest points: anywhere on a tied closest set
            assert (np.abs(gpos - np.asarray(cp, float)).max() <= tol * 10 or
                    on_closest_set(gpos, segs[body], gd, rad, tri, tol * 10)), (p, t, gpos, cp)
        compared += 1
    tk = {(p, t) for p, t, _c, _m in truth}
    for k in keys:
        assert k in tk or k in near, ("extra", k)
    return compared, capped


def bodies_over(n, seed, lo, hi, ground, kinds=("sphere", "capsule")):
    b = synth.capsule_bodies(n, box=hi - lo, seed=seed)
    R = rng(seed)
    b["pos"][:, 0] = R.uniform(lo, hi, n)
    b["pos"][:, 2] = R.uniform(lo, hi, n)
    b["pos"][:, 1] = ground(b["pos"][:, 0], b["pos"][:, 2]) + R.uniform(-0.6, 1.2, n)
    b["lvel"][:] = 0
    return b


def terrain_scene(dev, n=3000, seed=11, cap=1 << 20, **kw):
    vx, idx = heightfield(33, 32.0)
    bv, bi = box_mesh()
    meshes = [(vx, idx, 1.0, [0.0, 0.0, 0.0], IDENT), (bv, bi, 4.0, [40.0, 0.0, 16.0], IDENT)]
    b = bodies_over(n, seed, 0.0, 32.0, lambda x, z: np.sin(x * 0.37) * np.cos(z * 0.29))
    m = n // 6                                                          # some bodies around the box
    R = rng(seed + 1)
    b["pos"][:m] = np.stack([R.uniform(37, 43, m), R.uniform(-3, 3, m), R.uniform(13, 19, m)], 1)
    return Scene(dev, b, meshes, cap=cap, **kw)


# ------------------------------------------------------------------------------------------- against the truth
def test_scattered_bodies_on_terrain_and_box_against_truth(cuda_device):
    sc = terrain_scene(cuda_device)
    rec, ref, total, capped = sc.run()
    compared, tcapped = check(sc, rec, ref, total)
    assert compared > 1000, compared
    assert capped == tcapped
    assert set(np.unique(rec["nc"])) <= {1, 2}
    print(f"{compared} records compared, {total} found, {capped} capped")


def test_hand_cases(cuda_device):
    """one body each over the unit right triangle (y = 0, front face up): face, edge, vertex, behind, depth 0, a capsule
    through the face, the parallel pair, a sphere; plus a degenerate triangle that never touches"""
    vx = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0], [2, 0, 2], [3, 0, 2], [4, 0, 2]], np.float32)
    idx = np.array([[0, 1, 2], [3, 4, 5]], np.uint16)
    # (pos, radius, length, axis) of each body; capsules get their axis from the quaternion below
    cases = [([0.25, -0.1, 0.25], 0.5, 0.0, None, 3),                   # half-sunk sphere: face
             ([0.8, 0.2, 0.8], 0.5, 0.0, None, 5),                      # edge region
             ([-0.2, 0.1, -0.2], 0.5, 0.0, None, 5),                    # vertex region
             ([0.8, -0.2, 0.8], 0.5, 0.0, None, 0),                     # behind the face, outside: none
             ([0.25, 0.5, 0.25], 0.5, 0.0, None, 5),                    # depth exactly 0
             ([0.3, 0.1, 0.2], 0.1, 1.0, "up", 3),                      # a capsule through the face
             ([0.3, 0.2, 0.1], 0.25, 0.4, "x", 4),                      # lying just above: the parallel pair
             ([3.0, 0.1, 2.0], 0.5, 0.0, None, 0)]                      # over the degenerate triangle: none
    n = len(cases)
    b = synth.capsule_bodies(n, box=4.0, seed=3)
    b["pos"][:] = [c[0] for c in cases]
    b["radius"][:] = [c[1] for c in cases]
    b["length"][:] = [c[2] for c in cases]
    b["lvel"][:] = 0
    b["cell"] = 4.0                                                     # every body box within a broadphase cell
    # ODE's quat (w, x, y, z): the capsule geom's axis is z of the geom offset rotation; pick the body rotation
    # that gives the wanted axis from the world's own axis output
    sc = Scene(cuda_device, b, [(vx, idx, 1.0, [0.0, 0.0, 0.0], IDENT)])
    d = sc.w.download()
    want = {"up": [0, 1, 0], "x": [1, 0, 0]}
    for i, c in enumerate(cases):
        if c[3] is not None:
            ax = d["axis"][i]
            tgt = np.array(want[c[3]], float)
            if abs(abs(ax @ tgt) - 1) > 1e-12:                            # rotate the body so its axis becomes tgt
                v = np.cross(ax, tgt)
                ang = np.arctan2(np.linalg.norm(v), ax @ tgt)
                v = v / np.linalg.norm(v)
                q = np.concatenate([[np.cos(ang / 2)], v * np.sin(ang / 2)])
                q0 = b["quat"][i]
                w0, x0, y0, z0 = q0
                w1, x1, y1, z1 = q
                b["quat"][i] = [w1 * w0 - x1 * x0 - y1 * y0 - z1 * z0, w1 * x0 + x1 * w0 + y1 * z0 - z1 * y0,
                                w1 * y0 - x1 * z0 + y1 * w0 + z1 * x0, w1 * z0 + x1 * y0 - y1 * x0 + z1 * w0]
    sc = Scene(cuda_device, b, [(vx, idx, 1.0, [0.0, 0.0, 0.0], IDENT)])
    rec, ref, total, capped = sc.run()
    segs, d = sc.segments()
    for i, c in enumerate(cases):
        if c[3] == "up":
            assert abs(abs(d["axis"][i][1]) - 1) < 1e-9
        if c[3] == "x":
            assert abs(abs(d["axis"][i][0]) - 1) < 1e-9
    pairs = d["static_pairs"]
    by_body = {int(pairs[p][0]): k for k, (p, _t) in enumerate(ref)}
    for i, c in enumerate(cases):
        cs, _mg, rule = mc.collide(*segs[i], c[1], sc.tris[0][0 if c[0][0] < 1.5 else 1])
        assert rule == c[4], (i, rule)
        if rule == 0:
            assert i not in by_body, i
            continue
        r = rec[by_body[i]]
        assert r["nc"] == len(cs) and abs(r["depth"] - float(cs[0][2])) <= TOL, (i, r, cs)
        assert np.abs(r["normal"] - np.asarray(cs[0][1], float)).max() <= TOL, i
        if i == 4:
            assert r["depth"] == 0.0
        if rule == 4:
            assert abs(r["depth2"] - float(cs[1][2])) <= TOL and np.allclose(r["pos2"], np.asarray(cs[1][0], float))
    check(sc, rec, ref, total)
    assert capped == 0


def test_cap_keeps_the_deepest_records(cuda_device):
    vx, idx = heightfield(65, 4.0, amp=0.05)                             # fine: 8192 triangles of 1/16 edge
    b = synth.sphere_bodies(1, box=1.0, seed=2)
    b["pos"][:] = [[2.0, 0.3, 2.0]]
    b["radius"][:] = [0.6]
    b["lvel"][:] = 0
    b["cell"] = 4.0
    sc = Scene(cuda_device, b, [(vx, idx, 1.0, [0.0, 0.0, 0.0], IDENT)])
    rec, ref, total, capped = sc.run()
    assert capped == 1
    assert int(rec["nc"].sum()) <= 16 and total == len(rec)
    truth, tcapped, _near, _s, _p = sc.truth()
    assert tcapped == 1
    assert [(p, t) for p, t, _c, _m in truth] == [(int(p), int(t)) for p, t in ref]
    check(sc, rec, ref, total)


def test_capacity_overflow_writes_the_prefix(cuda_device):
    sc = terrain_scene(cuda_device, n=1500, seed=21)
    full = sc.run()
    cap = full[2] // 3
    part = sc.run(capacity=cap)
    assert part[2] == full[2] and len(part[0]) == cap
    assert np.array_equal(part[0].view(RAW), full[0][:cap].view(RAW)) and np.array_equal(part[1], full[1][:cap])


def test_surface_parameters_and_joint_flags(cuda_device):
    n = 600
    R = rng(31)
    mat = np.stack([R.uniform(0, 1, n), R.uniform(0, 2, n), R.uniform(0.1, 1, n), R.uniform(-0.1, 0.5, n),
                    R.uniform(-0.01, 0.05, n)], 1)
    smat = np.array([[0.2, 0.5, 0.8, 0.3, 0.02], [0.0, 0.0, 0.5, 0.0, 0.0]])
    sc = terrain_scene(cuda_device, n=n, seed=31, material=mat, static_material=smat)
    sc.w.bflags.zero_()
    rec, ref, total, _c = sc.run()
    d = sc.w.download()
    pairs = d["static_pairs"]
    touched = set()
    for k, (p, _t) in enumerate(ref):
        body, st = pairs[p]
        touched.add(int(body))
        m1, m2 = mat[body], smat[int(st) - sc.base]
        assert rec["bounce"][k] == max(m1[0], m2[0]) and rec["mu"][k] == np.sqrt(m1[2] * m2[2])
        assert rec["bounce_vel"][k] == (m1[1] + m2[1]) * 0.5
        erp = min(m1[3], m2[3]) if m1[3] > 0 and m2[3] > 0 else m1[3] if m1[3] > 0 else m2[3] if m2[3] > 0 else 0.05
        cfm = max(m1[4], m2[4]) if m1[4] > 0 and m2[4] > 0 else m1[4] if m1[4] > 0 else m2[4] if m2[4] > 0 else 0.01
        assert rec["soft_erp"][k] == erp and rec["soft_cfm"][k] == cfm
        assert rec["mode"][k] == 0x010 | 0x008 | (0x004 if max(m1[0], m2[0]) > 0 else 0)   # SOFT_CFM | SOFT_ERP | BOUNCE
    has = (d["bflags"] & _lib.BODY_HAS_JOINT) != 0
    assert set(np.nonzero(has)[0].tolist()) == touched and len(touched) > 50


def test_posed_rotated_scaled_mesh(cuda_device):
    sc = terrain_scene(cuda_device, n=1200, seed=41)
    q = np.array([0.0, np.sin(0.2), 0.0, np.cos(0.2)], np.float32)     # about y
    pos = np.array([[0.5, 0.0, -0.5], [40.0, -0.5, 16.0]])
    quat = np.stack([q, np.array([0.1, 0.2, 0.3, 0.9], np.float32) / np.float32(np.linalg.norm([0.1, 0.2, 0.3, 0.9]))])
    sc.w.pose_static_meshes(pos, quat)
    sc.meshes = [(m[0], m[1], m[2], pos[k], quat[k]) for k, m in enumerate(sc.meshes)]
    sc.tris = [tr.bake(*m) for m in sc.meshes]
    rec, ref, total, _c = sc.run()
    compared, _ = check(sc, rec, ref, total)
    assert compared > 150                                                # (parts of the turned meshes leave their boxes)


def test_two_runs_equal_bit_for_bit(cuda_device):
    sc = terrain_scene(cuda_device, n=3000, seed=51)
    a = sc.run()
    b = sc.run()
    assert a[2] == b[2] and a[3] == b[3]
    assert np.array_equal(a[0].view(RAW), b[0].view(RAW)) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------- regression guards
def test_existing_lists_and_sweep_unchanged(cuda_device):
    sc = terrain_scene(cuda_device, n=2000, seed=61)
    w = sc.w
    sc.run()
    w.contacts_geoms(set_joint_flags=False)
    st = w.download_contacts2(C2)["static"][0]
    pairs = w.download()["static_pairs"]
    meshed = pairs[:, 1] >= sc.base
    assert meshed.sum() > 100 and np.all(st["nc"][meshed] == 0)
    # the sweep with a NULL mesh set, through the raw call and through the wrapper
    R = rng(62)
    ns = 256
    sb = R.choice(w.n, ns, replace=False).astype(np.uint32)
    delta = R.normal(size=(ns, 3)).astype(np.float32)
    cf = np.arange(ns + 1, dtype=np.uint32) * 3
    cand = np.stack([np.full(ns, sc.base), np.full(ns, sc.base + 1), R.integers(0, w.n, ns) | (1 << 31)], 1).astype(np.uint32)
    import ctypes as C
    from clap_amd import physics
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).view(dt)).to(w.device)
    frac = torch.zeros(ns, dtype=torch.float32, device=w.device)
    nrm = torch.zeros((ns, 3), dtype=torch.float32, device=w.device)
    hit = torch.zeros(ns, dtype=torch.int32, device=w.device)
    g, sg = w.body_geoms(), w.static_geoms()
    args = [C.byref(g), C.byref(sg), None, ns, up(sb, np.int32).data_ptr(), up(delta, np.float32).data_ptr(),
            up(cf, np.int32).data_ptr(), up(cand.reshape(-1), np.int32).data_ptr(), frac.data_ptr(), nrm.data_ptr(), hit.data_ptr()]
    _lib.check(_lib.lib().clapgpu_sweep_capsules(physics._stream(), *args), "clapgpu_sweep_capsules")
    torch.cuda.synchronize()
    raw = [x.cpu().numpy() for x in (frac, nrm, hit)]
    f0, _n0, h0 = (x.cpu().numpy() for x in w.sweep_capsules(sb, delta, cf, cand.reshape(-1), meshes=False))
    assert np.array_equal(f0, raw[0]) and np.array_equal(h0, raw[2])


def test_sweep_onto_the_terrain(cuda_device):
    vx, idx = heightfield(33, 32.0)
    ground = lambda x, z: np.sin(x * 0.37) * np.cos(z * 0.29)
    n = 160
    b = bodies_over(n, 71, 4.0, 28.0, ground)
    b["pos"][:, 1] += 1.5
    sc = Scene(cuda_device, b, [(vx, idx, 1.0, [0.0, 0.0, 0.0], IDENT)])
    w = sc.w
    w.bodies_aabb()
    segs, d = sc.segments()
    R = rng(72)
    delta = np.concatenate([R.uniform(-1, 1, (n, 1)), R.uniform(-3.5, -1.0, (n, 1)), R.uniform(-1, 1, (n, 1))], 1).astype(np.float32)
    sb = np.arange(n, dtype=np.uint32)
    cf = np.arange(n + 1, dtype=np.uint32)
    cand = np.full(n, sc.base, np.uint32)
    frac, nrm, hit = (x.cpu().numpy() for x in w.sweep_capsules(sb, delta, cf, cand))
    f0, _n0, h0 = (x.cpu().numpy() for x in w.sweep_capsules(sb, delta, cf, cand, meshes=False))
    assert np.all(h0 == -1) and np.all(f0 == 1.0)                       # an OTHER static without its mesh: nothing
    L = b.get("length", np.zeros(n))
    hits = 0
    for i in range(n):
        ax = d["axis"][i]
        tf, tn, th = mc.sweep(b["pos"][i], float(b["radius"][i]), float(L[i]), ax, delta[i], sc.tris[0])
        assert (hit[i] == -2 - sc.base) == th, (i, hit[i], th)
        assert abs(float(frac[i]) - float(tf)) <= 1e-5, (i, frac[i], tf)
        assert np.abs(nrm[i] - tn).max() <= 1e-5, (i, nrm[i], tn)
        hits += th
    assert hits > n // 2, hits


def test_frame_loop_eager_and_captured(cuda_device):
    from clap_amd import entities, frame
    scene = synth.pad_levels(synth.entities_flat(2000, seed=3))
    dt = 1.0 / 120.0

    def world():
        return terrain_scene(cuda_device, n=2000, seed=81)

    def mesh_list(w):
        rec, ref, total, capped = w.download_mesh_contacts(RAW)
        return rec, ref, total, capped

    a = world()
    loop = frame.FrameLoop(entities.EntityBatch(scene, cuda_device), synth.camera(pos=(0, 10, 60)), world=a.w, contacts=True)
    loop.clap_frame(0.0, dt)
    first = mesh_list(a.w)
    s = world()
    s.w.broadphase()
    s.w.contacts_meshes()
    alone = mesh_list(s.w)
    assert first[2] == alone[2] > 500 and np.array_equal(first[0], alone[0]) and np.array_equal(first[1], alone[1])
    loop.clap_frame(dt, dt)
    second = mesh_list(a.w)
    c = world()
    cl = frame.FrameLoop(entities.EntityBatch(scene, cuda_device), synth.camera(pos=(0, 10, 60)), world=c.w, contacts=True)
    cl.capture(dt, warmup_now=0.0)
    cl.clap_frame_replay(dt)
    torch.cuda.synchronize()
    replayed = mesh_list(c.w)
    assert replayed[2] == second[2] and np.array_equal(replayed[0], second[0]) and np.array_equal(replayed[1], second[1])


def test_loaded_scene_through_set_static_meshes(cuda_device, tmp_path):
    from clap_amd import snapshot
    fix = os.path.join(ROOT, "tests", "golden", "scene_fixture")
    out = str(tmp_path / "scene.clps")
    snapshot.load_scene_json(os.path.join(fix, "scene.json"), out)
    comps = snapshot.load_scene(out)
    ent, col, bod = comps["entities"], comps["collision"], comps["bodies"]
    trim = np.nonzero(bod["geom_class"] == 2)[0]
    assert len(trim) >= 1
    meshes = []
    for bi in trim:
        e = bod["entity"][bi]
        m = ent["model"][e]
        vf, tf = col["vx_first"], col["tri_first"]
        meshes.append((col["vx"][vf[m]:vf[m + 1]], col["idx"][tf[m]:tf[m + 1]].astype(np.uint16), float(ent["pos_scale"][e, 3]),
                       ent["pos_scale"][e, :3].astype(np.float64), ent["rot"][e]))
    tris = np.concatenate([tr.bake(*m) for m in meshes]).reshape(-1, 3)
    lo, hi = tris.min(0), tris.max(0)
    n = 400
    R = rng(91)
    b = synth.capsule_bodies(n, box=4.0, seed=92)
    tri = tris.reshape(-1, 3, 3)                                        # near the surface, on both sides of it
    k = R.integers(0, len(tri), n)
    u, v = R.uniform(0, 1, n), R.uniform(0, 1, n)
    flip = u + v > 1
    u[flip], v[flip] = 1 - u[flip], 1 - v[flip]
    nrm = np.cross(tri[k, 1] - tri[k, 0], tri[k, 2] - tri[k, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    pt = tri[k, 0] + u[:, None] * (tri[k, 1] - tri[k, 0]) + v[:, None] * (tri[k, 2] - tri[k, 0])
    b["pos"][:] = pt + nrm * R.uniform(-0.2, 0.6, (n, 1))
    b["lvel"][:] = 0
    sc = Scene(cuda_device, b, meshes)
    rec, ref, total, _c = sc.run()
    compared, _ = check(sc, rec, ref, total, tol_scale=10.0)
    assert compared > 10, compared
