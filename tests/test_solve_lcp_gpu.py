"""GPU: clapgpu_bodies_solve[_wide] against tests/lcpref.py -- the dense boxed LCP of the header's rule -- and against
conservation of momentum, a closed-form resting stack and the geometry of tests/geomref.py.  tests/test_solve_gpu.py and
tests/test_solve_wide_gpu.py hold the kernels to tests/solveref.py bit for bit; this file never calls solveref: what it
asks is whether the rule the kernels compute is the physics, with the bounds of tests/test_solve_lcp.py (computed from
the same cond(A)).  The scenes' lists are written into the world's device tensors by hand; the island labels are the
device's own."""
import ctypes as C

import numpy as np
import pytest
import torch

from clap_amd import _lib, physics, synth
import geomref as gr
import lcpscenes as sc
import meshcontactref as mc
import meshscene
import test_solve_lcp as cpu

pytestmark = pytest.mark.gpu
H = sc.H
N = cpu.N
FAR = np.array([[900.0, 901.0, 900.0, 901.0, 900.0, 901.0]])               # a static nothing touches: the lists need one
PATHS = {"lane": 0, "workgroup": 1}                                         # clapgpu_solver.wide_rows


# ------------------------------------------------------------------------------------------------- helpers
def world_of(scene, dev):
    """a PhysWorld holding the scene's bodies (pos, quat, lvel, avel, mass, inertia, bflags, facc as the scene has them)"""
    st = scene["st"]
    n = len(st["mass"])
    b = synth.sphere_bodies(n, box=1.0, seed=1)
    for k in ("pos", "quat", "lvel", "avel", "mass", "bflags"):
        b[k] = np.array(st[k])
    b["radius"][:] = 0.1
    if st["inertia"] is not None:
        b["inertia"] = np.array(st["inertia"])
    b["facc"] = np.array(st["facc"])
    b["cell"] = 2.0
    return physics.PhysWorld(b, FAR, device=dev, forces=True)


def inject(w, static=None, body=None):
    """hand-made lists into the world's device tensors: (pairs [k, 2], records [k] of C2) each"""
    w.alloc_contacts()
    for lst, pairs, total, buf, cap in ((static, w.static_pairs, w.static_pair_total, w.static_contact2_buf, w.static_capacity),
                                        (body, w.pairs, w.pair_total, w.contact2_buf, w.capacity)):
        k = 0 if lst is None else len(lst[1])
        assert k <= cap
        if k:
            assert lst[1].dtype == meshscene.C2 == sc.C2 and lst[1].itemsize == 160
            pairs[:k] = torch.from_numpy(np.ascontiguousarray(lst[0]).astype(np.int32)).to(w.device)
            buf[:k] = torch.from_numpy(np.ascontiguousarray(lst[1]).view(np.uint8).reshape(k, 160)).to(w.device)
        total.fill_(k)


class Device:
    """a scene on the device: its world with the lists written and the islands made, and the state before any solve"""

    def __init__(self, scene, dev):
        self.scene = scene
        self.w = w = world_of(scene, dev)
        inject(w, static=scene.get("static"), body=scene.get("body"))
        w.islands(H)
        torch.cuda.synchronize()
        assert not (w.bflags.cpu().numpy().view(np.uint32) & _lib.BODY_DISABLED).any(), "a body fell asleep"
        self.before = (w.lvel.clone(), w.avel.clone())

    def solve(self, iterations, wide_rows, rows):
        """-> dict(lam [rows_total], key, lvel, avel, rows_total, status, wide_total); the world's velocities restored"""
        w = self.w
        w.lvel.copy_(self.before[0]), w.avel.copy_(self.before[1])
        w.alloc_solve(rows + 5)
        w.solver.iterations, w.solver.wide_rows, w.solver.cfm = iterations, wide_rows, self.scene["cfm"]
        assert w.solver.sor_w == cpu.SOR_W
        w.solve_status.zero_()
        w.row_lambda.fill_(float("nan"))
        w.row_key.fill_(-1)
        w.solve(H, want_lambda=True, want_levels=True)
        torch.cuda.synchronize()
        total = int(w.rows_total.item())
        n = w.n
        out = dict(lam=w.row_lambda.cpu().numpy()[:total].copy(), key=w.row_key.cpu().numpy().view(np.uint64)[:total].copy(),
                   lvel=w.lvel.cpu().numpy()[:n].copy(), avel=w.avel.cpu().numpy()[:n].copy(), rows_total=total,
                   status=int(w.solve_status.item()), wide_total=int(w.wide_total.item()))
        w.lvel.copy_(self.before[0]), w.avel.copy_(self.before[1])
        return out


def assert_canonical(got, S, wide_rows):
    assert got["status"] == 0 and got["rows_total"] == S.rows
    assert (got["key"] & np.uint64(0xffffffff)).tolist() == list(range(S.rows))
    assert (got["wide_total"] >= 1) if wide_rows else (got["wide_total"] == 0)


# ------------------------------------------------------------------------------------------------- scenes F, S, C
SCENES = {"F": lambda: sc.scene_free(), "S": lambda: sc.scene_free(inertia=False), "C": lambda: sc.scene_chain()}


@pytest.fixture(scope="module", params=list(SCENES))
def case(request, cuda_device):
    scene = SCENES[request.param]()
    return request.param, cpu.Truth(scene), Device(scene, cuda_device)


@pytest.mark.parametrize("path", ["lane", "workgroup", "default"])
def test_converged_solve_is_the_lcp_solution(case, path):
    """N sweeps on one lane (wide_rows 0), on a workgroup level by level (wide_rows 1) and at the default threshold (64:
    the workgroup for scene C, the lane for F and S): lambda is lambda*, the velocities are v + h invM J^T lambda*, and
    complementarity holds, all within tests/test_solve_lcp.py's bounds"""
    name, truth, dev = case
    S = truth.S
    wide_rows = PATHS.get(path, 64)
    got = dev.solve(N, wide_rows, S.rows)
    assert_canonical(got, S, wide_rows if path != "default" else S.rows >= 64)
    checks = truth.checks(got["lam"], got["lvel"], got["avel"])
    print(f"scene {name}, {path}: {S.rows} rows, cond(A) {S.cond:.3g}, {got['wide_total']} wide islands")
    cpu.report(f"scene {name}, {path}, {N} sweeps", checks)
    for k, (value, bound) in checks.items():
        assert value <= bound, (k, value, bound)


@pytest.mark.parametrize("path", list(PATHS))
def test_one_sweep_is_the_projected_gauss_seidel_row(case, path):
    name, truth, dev = case
    got = dev.solve(1, PATHS[path], truth.S.rows)
    assert_canonical(got, truth.S, PATHS[path])
    checks = truth.sweep_check(got["lam"])
    cpu.report(f"scene {name}, {path}, one sweep", checks)
    assert checks["sweep"][0] <= checks["sweep"][1]


# ------------------------------------------------------------------------------------------------- momentum
@pytest.fixture(scope="module")
def closed(cuda_device):
    scene = sc.scene_free(closed=True)
    return scene, Device(scene, cuda_device), cpu.system(scene).rows


@pytest.mark.parametrize("iterations", [1, 20])
@pytest.mark.parametrize("path", list(PATHS))
def test_the_solve_conserves_momentum(closed, path, iterations):
    """scene F without statics, kinematic body and NO_GRAVITY: P and L about the origin keep their values over a solve
    that has not converged -- every row's impulses are equal and opposite at every sweep"""
    scene, dev, rows = closed
    got = dev.solve(iterations, PATHS[path], rows)
    assert got["status"] == 0 and got["rows_total"] == rows and (got["wide_total"] >= 1) == bool(PATHS[path])
    drift, bound = cpu.momentum_check(scene["st"], got["lvel"], got["avel"])
    print(f"closed scene F, {path}, {iterations} sweeps: momentum drift {drift:.3g} (bound {bound:.3g})")
    assert np.abs(got["lvel"] - scene["st"]["lvel"]).max() > 0.1
    assert drift <= bound


# ------------------------------------------------------------------------------------------------- the stack
def test_a_stack_rests_at_its_closed_form(cuda_device):
    """tests/test_solve_lcp.py's stack of eight spheres through phys_step(solve=True): every contact ends at
    depth_i* = soft_cfm (g sum_{j >= i} m_j) h / soft_erp (derived there) within 1e-3, every speed under 1e-6.  The
    world's linear damping acts above a speed of 0.01 only, so not at rest, and no body carries AUTO_DISABLE: nothing
    here moves the fixed point."""
    n = sc.K_STACK
    b = synth.sphere_bodies(n, box=1.0, seed=1)
    b["pos"][:] = sc.stack_positions()
    b["radius"][:] = sc.R_STACK
    b["mass"][:] = sc.STACK_MASS
    b["lvel"][:] = b["avel"][:] = 0
    b["bflags"][:] = 0
    b["cell"] = 2.0
    w = physics.PhysWorld(b, sc.FLOOR, device=cuda_device)
    steps = 0
    while steps < 2400:
        steps += w.phys_step(H, solve=True)
    d = w.download()
    depth, want = sc.stack_depths(d["pos"][:n]), sc.stack_depths_at_rest()
    print("substeps", steps, "depth", depth, "depth*", want, "relative", np.abs(depth - want) / want, "max |v|",
          np.abs(d["lvel"][:n]).max(), "status", int(w.solve_status.item()), "rows", int(w.rows_total.item()))
    assert int(w.solve_status.item()) == 0 and int(w.rows_total.item()) == n
    assert (np.abs(depth - want) <= 1e-3 * want).all()
    assert np.abs(d["lvel"][:n]).max() <= 1e-6


# ------------------------------------------------------------------------------------------------- every producer
R_S, R_C, L_C, OVERLAP = 0.3, 0.2, 1.0, 0.02


def producers_scene(dev):
    """One overlapping pair (by about OVERLAP) for every pairing the narrowphase emits, the pairs 4 apart, at rest and
    without gravity.  -> (meshscene.Scene, cases [(name, body, other, kind of other, reference depth function)])"""
    R0 = (C.c_double * 12)()
    _lib.lib().clapgpu_geom_offset_rotation(R0)
    a0 = np.array([R0[2], R0[6], R0[10]])                                   # a capsule's axis at the identity quaternion
    k0 = int(np.argmax(np.abs(a0)))
    assert abs(abs(a0[k0]) - 1) < 1e-12                                     # a coordinate axis
    p, p2 = np.eye(3)[(k0 + 1) % 3], np.eye(3)[(k0 + 2) % 3]
    ident = np.array([1.0, 0, 0, 0])
    turn = np.concatenate([[np.sqrt(0.5)], np.sqrt(0.5) * p2])              # 90 degrees about p2: a0 -> +-p
    ext_y = L_C / 2 * abs(a0[1]) + R_C                                      # how far an unturned capsule reaches down
    bodies, statics, cases = [], [], []

    def body(pos, length=0.0, quat=ident):
        bodies.append((np.asarray(pos, float), length, quat))
        return len(bodies) - 1

    def static(kind, pos, box=None, axis=(0, 0, 1), radius=0.0, length=0.0):
        pos = np.asarray(pos, float)
        if box is None:
            half = radius + length / 2 * np.abs(axis)
            box = np.stack([pos - half, pos + half], 1).reshape(-1)
        statics.append((kind, pos, np.asarray(box, float), np.asarray(axis, float), radius, length))
        return len(statics) - 1
    at = lambda k: np.array([4.0 * k, 10.0, 0.0])
    # body pairs: the lower index is listed first
    c = at(0)
    cases.append(("sphere-sphere", body(c), body(c + sc.unit(np.array([1.0, 0.3, 0.2])) * (2 * R_S - OVERLAP)), "body"))
    c = at(1)
    cases.append(("capsule-sphere", body(c, L_C), body(c + p * (R_C + R_S - OVERLAP) + a0 * 0.2), "body"))
    c = at(2)
    cases.append(("sphere-capsule", body(c + p * (R_C + R_S - OVERLAP) + a0 * 0.2), body(c, L_C), "body"))
    c = at(3)
    cases.append(("capsules crossed", body(c, L_C), body(c + p2 * (2 * R_C - OVERLAP) + a0 * 0.15 + p * 0.1, L_C, turn), "body"))
    c = at(4)
    cases.append(("capsules parallel", body(c, L_C), body(c + p * (2 * R_C - OVERLAP) + a0 * 0.2, L_C), "body"))
    # statics
    top = 9.0
    for k, length in ((5, 0.0), (6, L_C)):
        c = at(k)
        s = static(_lib.GEOM_BOX, [c[0], top - 0.5, 0], box=[c[0] - 1, c[0] + 1, top - 1, top, -1, 1])
        reach = ext_y if length else R_S
        cases.append((f"{'capsule' if length else 'sphere'}-static box", body([c[0] + 0.2, top + reach - OVERLAP, 0.1], length), s, "static"))
    for k, (length, skind) in enumerate([(0.0, "sphere"), (L_C, "sphere"), (0.0, "capsule"), (L_C, "capsule")], 7):
        c = at(k)
        r = R_C if length else R_S
        if skind == "sphere":
            s = static(_lib.GEOM_SPHERE, c, radius=0.5)
            pos = c + p * (0.5 + r - OVERLAP) + a0 * (0.2 if length else 0.0)
        else:                                                               # a static capsule along p: crossed with a body's
            s = static(_lib.GEOM_CAPSULE, c, axis=p, radius=0.3, length=1.0)
            pos = c + p2 * (0.3 + r - OVERLAP) + p * 0.2 + a0 * (0.1 if length else 0.0)
        cases.append((f"{'capsule' if length else 'sphere'}-static {skind}", body(pos, length), s, "static"))
    # the mesh: a cube of side 2 whose top face is at y = top
    mc_ = at(11)
    mesh_pos = [mc_[0], top - 1.0, 0.0]
    cases.append(("sphere-mesh", body([mc_[0] + 0.3, top + R_S - OVERLAP, 0.1]), None, "mesh"))
    cases.append(("capsule-mesh", body([mc_[0] - 0.4, top + ext_y - OVERLAP, -0.3], L_C), None, "mesh"))
    n = len(bodies)
    b = synth.sphere_bodies(n, box=1.0, seed=1)
    b["pos"][:] = [x[0] for x in bodies]
    b["length"] = np.array([x[1] for x in bodies])
    b["quat"][:] = [x[2] for x in bodies]
    b["radius"][:] = np.where(b["length"] > 0, R_C, R_S)
    b["mass"][:] = np.linspace(1.0, 2.0, n)
    b["inertia"] = np.zeros((n, 3))
    I = (C.c_double * 3)()
    for i in range(n):
        if b["length"][i]:
            _lib.lib().clapgpu_mass_capsule_total(float(b["mass"][i]), 3, R_C, L_C, I)
        else:
            _lib.lib().clapgpu_mass_sphere_total(float(b["mass"][i]), R_S, I)
        b["inertia"][i] = I[0], I[1], I[2]
    b["lvel"][:] = b["avel"][:] = 0
    b["bflags"][:] = _lib.BODY_NO_GRAVITY
    b["cell"] = 2.0
    bv, bi = synth.box_mesh()
    geo = dict(pos=[s[1] for s in statics], axis=[s[3] for s in statics], radius=[s[4] for s in statics],
               length=[s[5] for s in statics])
    scene = meshscene.Scene(dev, b, [(bv, bi, 2.0, mesh_pos, meshscene.IDENT)], bb=[s[2] for s in statics],
                            kind=[s[0] for s in statics], geo=geo, cap=(1024, 1024), grow=1e-6)
    return scene, b, statics, cases


def reference_contact(case, b, statics, tris, pos, axis):
    """(depth, normal) of the pair from the float64 geometry: the deepest contact and its normal, which points from the
    other geom towards the case's first body"""
    _name, i, other, kind = case
    one = lambda x: np.asarray(x)[None]
    geom = lambda k: (one(pos[k]), one(axis[k]), one(b["radius"][k]), one(b["length"][k]))
    pi, ai, ri, li = geom(i)
    if kind == "mesh":
        seg = mc.segment_of(pos[i], axis[i], float(b["length"][i]))
        found = [cn for t in tris for cn in mc.collide(seg[0], seg[1], float(b["radius"][i]), t)[0]]
        if not found:
            return 0.0, None
        _p, nrm, depth = max(found, key=lambda cn: cn[2])
        return float(depth), np.asarray(nrm, float)
    if kind == "body":
        pj, aj, rj, lj = geom(other)
    else:
        skind, spos, sbox, saxis, sr_, sl = statics[other]
        pj, aj, rj, lj = one(spos), one(saxis), one(sr_), one(sl)
    if kind == "static" and statics[other][0] == _lib.GEOM_BOX:
        c = gr.capsule_box(pi, ai, ri, li, one(sbox)) if li[0] else gr.sphere_box(pi, ri, one(sbox))
    elif li[0] and lj[0]:
        c = gr.capsule_capsule(pi, ai, ri, li, pj, aj, rj, lj)
    elif li[0]:
        c = gr.capsule_sphere(pi, ai, ri, li, pj, rj)
    elif lj[0]:
        c = gr.sphere_capsule(pi, ri, pj, aj, rj, lj)
    else:
        c = gr.sphere_sphere(pi, ri, pj, rj)
    nc = int(c["nc"][0])
    if nc == 0:
        return 0.0, None
    assert nc in (1, 2)
    depth = float(c["depth"][0]) if nc == 1 else float(max(c["depth"][0], c["depth2"][0]))
    return depth, np.asarray(c["normal"][0], float)


def test_every_producers_records_push_its_bodies_apart(cuda_device):
    """The narrowphase, the static narrowphase and the mesh contacts each write a normal "from the static towards the
    body, from body 2 to body 1"; the solve assumes that sign.  End to end: the device makes its own lists, solves at
    the defaults and steps once; by the independent geometry every pair then overlaps less than before, body 1 has moved
    along the reference's normal and body 2 against it."""
    scene, b, statics, cases = producers_scene(cuda_device)
    w = scene.w
    w.bodies_aabb()
    before = w.download()
    pos0, axis0 = before["pos"][:w.n].copy(), before["axis"][:w.n].copy()
    w.broadphase()
    w.contacts_geoms_both()
    w.contacts_meshes()
    w.islands(H)
    total, status = w.solve(H)
    w.world_step(H)
    w.bodies_aabb()
    after = w.download()
    pos1, axis1 = after["pos"][:w.n], after["axis"][:w.n]
    assert int(status.item()) == 0 and int(total.item()) >= len(cases)
    nbody = sum(1 for c in cases if c[3] == "body")
    assert after["pair_total"] == nbody and after["static_pair_total"] == len(cases) - nbody
    two = w.download_contacts2(meshscene.C2)["body"][0]["nc"]
    assert sorted(two.tolist()) == [1] * (nbody - 1) + [2]                  # the parallel capsules: two contacts
    tris = scene.tris[0]
    for case in cases:
        name, i, other, kind = case
        d0, n0 = reference_contact(case, b, statics, tris, pos0, axis0)
        d1, _n1 = reference_contact(case, b, statics, tris, pos1, axis1)
        moved = (pos1[i] - pos0[i]) @ n0
        line = f"{name}: depth {d0:.6f} -> {d1:.6f}, body {i} moved {moved:.3g} along the normal"
        assert abs(d0 - OVERLAP) < 0.2 * OVERLAP, line
        assert moved > 1e-5 and d1 < d0 - 1e-5, line
        if kind == "body":
            back = (pos1[other] - pos0[other]) @ n0
            line += f", body {other} {back:.3g}"
            assert back < -1e-5, line
        print(line)
