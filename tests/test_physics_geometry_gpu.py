"""GPU: the parity-unpinned physics kernels (k_contacts_geoms, k_contacts_geoms_both, k_contacts_sphere_box,
k_sweep_capsules, k_bodies_step, k_skin) against tests/geomref.py, on the kernels' own outputs.

The fixtures and checks are those of tests/test_physics_geometry.py.  The reference is fed the geometry the kernel had
(pos, axis, radius, length downloaded from the PhysWorld); candidate pairs are written into the world directly, so
the narrowphase is measured on exactly the configurations chosen.  Also: the one-launch contact kernel with a grid
override beyond 2^16 workgroups (its ticket field is 16 bits wide)."""
import numpy as np
import pytest
import torch

import geomref as G
import test_physics_geometry as T
from oracle import binding as ob

pytestmark = pytest.mark.gpu


def body_dict(pos, radius, length):
    """A PhysWorld body set of resting capsules / spheres at pos (their axes are written afterwards)."""
    n = len(radius)
    return dict(n=n, pos=np.asarray(pos, np.float64), quat=np.tile([1.0, 0, 0, 0], (n, 1)), lvel=np.zeros((n, 3)),
                avel=np.zeros((n, 3)), mass=np.ones(n), radius=np.asarray(radius, np.float64),
                length=np.asarray(length, np.float64), inertia=np.ones((n, 3)), yoffset=np.zeros(n),
                bflags=np.full(n, 4, np.uint32), adis_steps_left=np.full(n, 30, np.int32), adis_time_left=np.zeros(n),
                body_entity=np.arange(n, dtype=np.int32), cell=float(np.max(np.asarray(length) + 2 * np.asarray(radius))))


def world_with(pos, axis, radius, length, statics=None, cap=None, device="cuda:0"):
    """A world whose narrowphase reads the body arrays (no one-sector records), with the axes written as given."""
    from clap_amd import physics
    w = physics.PhysWorld(body_dict(pos, radius, length), statics, pair_capacity=cap, device=device, geom_records=False)
    w.axis[:len(radius)] = torch.from_numpy(np.ascontiguousarray(axis, np.float64)).to(device)
    return w


def set_pairs(w, pairs, static=False):
    p = torch.from_numpy(np.ascontiguousarray(pairs, np.uint32).view(np.int32)).to(w.device)
    (w.static_pairs if static else w.pairs)[:len(pairs)] = p
    (w.static_pair_total if static else w.pair_total).fill_(len(pairs))


def geometry(w):
    torch.cuda.synchronize()
    n = w.n
    return (w.pos[:n].cpu().numpy(), w.axis[:n].cpu().numpy(), w.radius[:n].cpu().numpy(), w.length[:n].cpu().numpy())


SCALES = ((0.0, 1.0), (1e4, 4e-3), (np.array([-3e3, 1e4, 7e3]), 4e-3))


def test_capsule_capsule_kernel_against_reference(cuda_device):
    w_ = T.Worst()
    for offset, size in SCALES:
        f = T.capsule_pairs(1, offset, size)
        m = len(f["r1"])
        world = world_with(np.concatenate([f["pos1"], f["pos2"]]), np.concatenate([f["ax1"], f["ax2"]]),
                           np.concatenate([f["r1"], f["r2"]]), np.concatenate([f["l1"], f["l2"]]), cap=m, device=cuda_device)
        set_pairs(world, np.stack([np.arange(m), m + np.arange(m)], 1))
        world.contacts_geoms(set_joint_flags=False)
        rec, total = world.download_contacts2(ob.CONTACT2_DTYPE)["body"]
        pos, ax, r, l = geometry(world)
        g = dict(f, pos1=pos[:m], pos2=pos[m:], ax1=ax[:m], ax2=ax[m:], r1=r[:m], r2=r[m:], l1=l[:m], l2=l[m:])
        counts = T.check_capsule_capsule(rec, g, w_)
        assert total == int((rec["nc"] > 0).sum())
        assert counts["two-contact near_par_in"] >= 30 and counts["general near_par_out touching"] >= 30, counts
        assert counts["two-contact"] >= 100 and counts["well-conditioned"] >= 300 and counts["not touching"] >= 150, counts
        assert counts["d = 0"] >= 6 and counts["mid"] >= 10, counts
    print("worst error / bound:", w_.r)


def test_capsule_sphere_kernel_both_orders(cuda_device):
    w_ = T.Worst()
    for offset, size in SCALES[:2]:
        f = T.capsule_sphere_pairs(2, offset, size)
        m = len(f["r"])
        world = world_with(np.concatenate([f["cpos"], f["spos"]]), np.concatenate([f["ax"], np.tile([0, 1.0, 0], (m, 1))]),
                           np.concatenate([f["r"], f["rs"]]), np.concatenate([f["l"], np.zeros(m)]), cap=2 * m, device=cuda_device)
        set_pairs(world, np.concatenate([np.stack([np.arange(m), m + np.arange(m)], 1), np.stack([m + np.arange(m), np.arange(m)], 1)]))
        world.contacts_geoms(set_joint_flags=False)
        rec, _total = world.download_contacts2(ob.CONTACT2_DTYPE)["body"]
        pos, ax, r, l = geometry(world)
        g = dict(f, cpos=pos[:m], spos=pos[m:], ax=ax[:m], r=r[:m], rs=r[m:], l=l[:m])
        counts = T.check_capsule_sphere(rec[:m], rec[m:], g, w_)
        assert counts["cap_beyond"] >= 30 and counts["side"] >= 30 and counts["on_segment"] == 6, counts
    print("worst error / bound:", w_.r)


def test_capsule_box_kernel_against_reference(cuda_device):
    w_ = T.Worst()
    for offset, size in SCALES[:2]:
        f = T.capsule_box_pairs(3, offset, size)
        m = len(f["r"])
        world = world_with(f["pos"], f["ax"], f["r"], f["l"], statics=f["aabb"][None], cap=m, device=cuda_device)
        set_pairs(world, np.stack([np.arange(m), np.zeros(m, int)], 1), static=True)
        world.pair_total.fill_(0)
        world.contacts_geoms(set_joint_flags=False)
        rec, total = world.download_contacts2(ob.CONTACT2_DTYPE)["static"]
        pos, ax, r, l = geometry(world)
        counts = T.check_capsule_box(rec, dict(f, pos=pos, ax=ax, r=r, l=l), w_)
        assert total == int((rec["nc"] != 0).sum())
        assert counts["deep"] >= 60 and counts["face"] >= 30 and counts["edge"] >= 30 and counts["corner"] >= 20, counts
        assert counts["axis_parallel"] >= 30 and counts["not_unique"] >= 10 and counts["apart"] >= 50, counts
    print("worst error / bound:", w_.r)


def test_sphere_box_kernels_against_reference(cuda_device):
    """Sphere bodies against boxes through both kernels that collide them: the general narrowphase (k_contacts_geoms)
    and the sphere-only one (k_contacts_sphere_box), inside branch included."""
    w_ = T.Worst()
    for offset, size in SCALES[:2]:
        c, r, aabb = T.sphere_box_cases(4, offset, size)
        m = len(r)
        world = world_with(c, np.tile([0, 1.0, 0], (m, 1)), r, np.zeros(m), statics=aabb, cap=m, device=cuda_device)
        set_pairs(world, np.stack([np.arange(m), np.arange(m)], 1), static=True)
        world.pair_total.fill_(0)
        world.contacts_geoms(set_joint_flags=False)
        rec, _t = world.download_contacts2(ob.CONTACT2_DTYPE)["static"]
        pos, _ax, rr, _l = geometry(world)
        counts = T.check_sphere_box(rec, pos, rr, aabb, w_, "sphere-box (narrowphase)")
        assert counts["inside"] >= 50 and counts["outside"] >= 50 and counts["apart"] >= 50, counts
        world.contacts_static()
        rec1, _t1 = world.download_static_contacts(ob.CONTACT_DTYPE)
        counts = T.check_sphere_box(rec1, pos, rr, aabb, w_, "sphere-box (k_contacts_sphere_box)")
        assert counts["inside"] >= 50 and counts["outside"] >= 50 and counts["apart"] >= 50, counts
    print("worst error / bound:", w_.r)


def test_sweep_kernel_against_time_of_impact(cuda_device):
    sc = T.sweep_scene()
    n = len(sc["r"])
    world = world_with(sc["pos"], sc["ax"], sc["r"], sc["l"], statics=sc["saabb"], cap=1024, device=cuda_device)
    world.set_static_geoms(sc["skind"], pos=sc["spos"], axis=sc["sax"], radius=sc["srad"], length=sc["slen"])
    ns = len(sc["skind"])
    cand = np.tile(np.arange(ns, dtype=np.uint32), n)
    first = (np.arange(n + 1) * ns).astype(np.uint32)
    frac, normal, hit = world.sweep_capsules(np.arange(n, dtype=np.uint32), sc["delta"], first, cand)
    frac, normal, hit = frac.cpu().numpy(), normal.cpu().numpy(), hit.cpu().numpy()
    pos, ax, r, l = geometry(world)
    w_ = T.Worst()
    counts = T.check_sweeps(frac, normal, hit, sc, pos, ax, l, r, w_)
    assert counts["free"] >= 20 and counts["head_on"] >= 60 and counts["face"] >= 20 and counts["curved"] >= 10, counts
    assert counts["argmin"] >= 40, counts
    print("worst error / bound:", w_.r)


def _download_state(world):
    out = world.download()
    return dict(pos=out["pos"], quat=out["quat"], lvel=out["lvel"], avel=out["avel"], axis=out["axis"], aabb=out["aabb"],
                bflags=out["bflags"])


def test_body_step_kernel_against_equations(cuda_device):
    from clap_amd import physics
    b = T.step_bodies()
    w_ = T.Worst()
    for damping in (0.001, 0.0):
        world = physics.PhysWorld(b, None, device=cuda_device)
        world.world.linear_damping = damping
        world.world_step(T.H)
        T.check_step(_download_state(world), b, world.world, T.H, w_)
    print("worst error / bound:", w_.r)


def test_body_step_kernel_closed_forms(cuda_device):
    from clap_amd import physics
    b, kind = T.closed_form_bodies()
    w_ = T.Worst()
    for damping in (0.0, 0.01):
        bb = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}
        if damping:
            bb["bflags"] = bb["bflags"] | 4
        world = physics.PhysWorld(bb, None, device=cuda_device)
        world.world.linear_damping = damping
        s = _download_state(world)
        states = [(s["pos"], s["quat"], s["lvel"], s["avel"])]
        for _ in range(100):
            world.world_step(T.H)
            s = _download_state(world)
            states.append((s["pos"], s["quat"], s["lvel"], s["avel"]))
        T.check_closed_forms(states, bb, np.where(kind == 2, 2, -1) if damping else np.where(kind == 2, -1, kind), T.H,
                             world.world, w_)
    print("worst error / bound:", w_.r)


def test_skin_kernel_against_float64_sum(cuda_device):
    from clap_amd import animation, synth
    J, n = 32, 7
    sk = synth.skeleton(J, 8, seed=3)
    an = synth.animation(J, 30, 2.0, seed=3)
    ch = synth.characters(n, J, seed=3)
    sk["bind"] = ob.skeleton_bind(sk)
    vc = np.random.Generator(np.random.PCG64(12)).integers(1, 300, n).astype(np.uint32)
    mesh = synth.skinned_mesh(int(vc.sum()), J, seed=13)
    vf = np.concatenate([[0], np.cumsum(vc[:-1])]).astype(np.uint32)
    model = animation.SkinnedModel(sk, [an], mesh=mesh, bind=sk["bind"], device=cuda_device)
    batch = animation.CharacterBatch(model, n, ch["trs0"], ch["char_mx"], vert_first=vf, vert_count=vc)
    P = T.skin_palette(n, J)
    batch.joint_transforms.copy_(torch.from_numpy(P))
    batch.set_skin_w(True)
    batch.skin()
    out = batch.download()
    w_ = T.Worst()
    T.check_skin(out["out_position"], out["out_normal"], out["out_w"], mesh, vf, vc, P, w_)
    print("worst error / bound:", w_.r)


def test_contacts_both_with_a_grid_beyond_the_ticket_field(cuda_device, monkeypatch):
    """k_contacts_geoms_both counts finished workgroups in the top 16 bits of one word.  With capacities of 9 M and 8 M
    the list spans 66 407 workgroups; CLAPGPU_CONTACTS_GRID = 70 000 would launch all of them and no workgroup would
    see the last ticket (totals never stored, the word never reset for the next launch).  The launch is clamped to
    2^16 workgroups: two launches in a row and one at the default grid give the totals and records of the oracle, and
    of the reference.  About 2.7 GB of contact records."""
    from clap_amd import physics
    cap, scap = 9_000_000, 8_000_000
    assert (cap + scap + 255) // 256 > 70_000 - 4000 > 1 << 16
    f = T.capsule_pairs(1)
    m = len(f["r1"])
    boxes = T.capsule_box_pairs(3)
    mb = len(boxes["r"])
    pos = np.concatenate([f["pos1"], f["pos2"], boxes["pos"]])
    ax = np.concatenate([f["ax1"], f["ax2"], boxes["ax"]])
    r = np.concatenate([f["r1"], f["r2"], boxes["r"]])
    l = np.concatenate([f["l1"], f["l2"], boxes["l"]])
    world = world_with(pos, ax, r, l, statics=boxes["aabb"][None], cap=cap, device=cuda_device)
    world.static_capacity = scap
    world.static_pairs = torch.zeros((scap, 2), dtype=torch.int32, device=cuda_device)
    world.alloc_contacts()                                           # 9 M + 8 M records of 160 bytes
    bpairs = np.stack([np.arange(m), m + np.arange(m)], 1)
    spairs = np.stack([2 * m + np.arange(mb), np.zeros(mb, int)], 1)
    set_pairs(world, bpairs)
    set_pairs(world, spairs, static=True)
    gpos, gax, gr, gl = geometry(world)
    A = ob.geoms(len(gr), pos=gpos, axis=gax, radius=gr, length=gl)
    S = ob.geoms(1, kind=np.array([2], np.uint8), aabb=boxes["aabb"][None])
    exp, exp_total = ob.contacts_geoms(bpairs, A, A)
    exp_s, exp_s_total = ob.contacts_geoms(spairs, A, S)
    assert exp_total > 100 and exp_s_total > 100
    w_ = T.Worst()
    for grid in ("70000", "70000", None):
        if grid is None:
            monkeypatch.delenv("CLAPGPU_CONTACTS_GRID", raising=False)
        else:
            monkeypatch.setenv("CLAPGPU_CONTACTS_GRID", grid)
        world.contact2_total.fill_(0x7fffffff)
        world.static_contact2_total.fill_(0x7fffffff)
        world.contacts_geoms_both(set_joint_flags=False)
        got = world.download_contacts2(ob.CONTACT2_DTYPE)
        assert world.contact2_buf.shape[0] == cap and world.static_contact2_buf.shape[0] == scap
        assert got["body"][1] == exp_total and got["static"][1] == exp_s_total, (grid, got["body"][1], got["static"][1])
        assert got["body"][0].tobytes() == exp.tobytes() and got["static"][0].tobytes() == exp_s.tobytes(), grid
        g = dict(f, pos1=gpos[:m], pos2=gpos[m:2 * m], ax1=gax[:m], ax2=gax[m:2 * m], r1=gr[:m], r2=gr[m:2 * m],
                 l1=gl[:m], l2=gl[m:2 * m])
        T.check_capsule_capsule(got["body"][0], g, w_)
        T.check_capsule_box(got["static"][0], dict(boxes, pos=gpos[2 * m:], ax=gax[2 * m:], r=gr[2 * m:], l=gl[2 * m:]), w_)
