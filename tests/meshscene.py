"""What the GPU tests of rays, mesh rays and mesh contacts share: small helpers and the one Scene -- a PhysWorld whose
statics are some boxes or geoms, then one OTHER static per triangle mesh, with the meshes set.  The mesh generators
themselves are clap_amd.synth's."""
import numpy as np

from clap_amd import _lib, synth
from clap_amd._dev import upload
from guards import Guards
import meshcontactref as mc
import trimeshref as tr

BOX, OTHER = _lib.GEOM_BOX, _lib.GEOM_OTHER
IDENT = [0.0, 0.0, 0.0, 1.0]
C2 = np.dtype([("pos", np.float64, 3), ("normal", np.float64, 3), ("depth", np.float64), ("mu", np.float64),
               ("bounce", np.float64), ("bounce_vel", np.float64), ("soft_erp", np.float64), ("soft_cfm", np.float64),
               ("mode", np.uint32), ("nc", np.uint32), ("pos2", np.float64, 3), ("normal2", np.float64, 3),
               ("depth2", np.float64)])


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def fetch(res):
    return [t.cpu().numpy() for t in res]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def guarded_scratch(need, dev, guard=4096):
    """(scratch, tail): a zeroed scratch tensor of exactly `need` bytes, 256-byte aligned, followed in the same allocation
    by `guard` bytes of 0xA5 that a call given the scratch must leave alone (guards.Guards.scratch)"""
    assert need > 0
    g = Guards(dev, band=guard)
    scratch = g.scratch(need)
    assert scratch.data_ptr() % 256 == 0
    return scratch, g.bands()[1]


def unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def far_body(n=1):
    b = synth.sphere_bodies(n, box=1.0, seed=1)
    b["pos"][:] = [-500.0, -500.0, -500.0]
    b["lvel"][:] = 0
    return b


class Scene:
    """A PhysWorld over `bodies` (synth dict) whose statics are, in this order: `bb` (of `kind`, BOX by default, with the
    geoms `geo` where given, else none beyond their boxes), one OTHER static per mesh of `meshes` [(vx, idx, scale, pos,
    quat)] with its baked AABB grown by `grow`, the OTHER boxes `unmeshed` and the BOX `tail_boxes`; with the meshes
    set.  cap: (pair, static pair) capacity."""

    def __init__(self, dev, bodies, meshes, bb=None, kind=None, geo=None, unmeshed=(), tail_boxes=(), material=None,
                 static_material=None, cap=(4_000_000, 8_000_000), grow=0.0):
        from clap_amd import physics
        bb = np.zeros((0, 6)) if bb is None else np.asarray(bb, float).reshape(-1, 6)
        kind = np.full(len(bb), BOX, np.uint8) if kind is None else np.asarray(kind, np.uint8)
        self.base = len(bb)
        self.bodies = bodies
        self.meshes = meshes
        self.tris = [tr.bake(*m) for m in meshes]
        mbb = np.zeros((len(meshes), 6))
        for k, t in enumerate(self.tris):
            f = t.reshape(-1, 3)
            mbb[k, 0::2], mbb[k, 1::2] = f.min(0) - grow, f.max(0) + grow
        ub = np.asarray(list(unmeshed), float).reshape(-1, 6)
        tb = np.asarray(list(tail_boxes), float).reshape(-1, 6)            # boxes after the meshes (higher indices)
        allbb = np.concatenate([bb, mbb, ub, tb])
        allkind = np.concatenate([kind, np.full(len(meshes) + len(ub), OTHER, np.uint8), np.full(len(tb), BOX, np.uint8)])
        ns = len(allbb)
        g = geo or {}
        pad = lambda a, shape: np.concatenate([np.asarray(a, float).reshape((-1,) + shape), np.zeros((ns - self.base,) + shape)])
        c = (allbb[:, 0::2] + allbb[:, 1::2]) / 2
        self.w = w = physics.PhysWorld(bodies, allbb, pair_capacity=cap[0], static_pair_capacity=cap[1], device=dev)
        w.set_static_geoms(allkind, pad(g["pos"], (3,)) if "pos" in g else c,
                           pad(g["axis"], (3,)) if "axis" in g else np.tile([0, 0, 1.0], (ns, 1)),
                           pad(g["radius"], ()) if "radius" in g else np.zeros(ns),
                           pad(g["length"], ()) if "length" in g else np.zeros(ns))
        if material is not None:
            w.set_materials(material)
        if static_material is not None:
            w.static_material = upload(static_material, np.float64, w.device)
        self.mesh_static = self.base + np.arange(len(meshes))
        self.ref = tr.Meshes.from_list([(self.base + k, t) for k, t in enumerate(self.tris)])
        if meshes:
            w.set_static_meshes(self.mesh_static, [m[0] for m in meshes], [m[1] for m in meshes], [m[2] for m in meshes],
                                [m[3] for m in meshes], [m[4] for m in meshes])

    def cast(self, *a, **k):
        """brute force: these scenes have no broadphase index"""
        k.setdefault("grid", False)
        return self.w.ray_cast(*a, **k)

    def run(self, capacity=None, flags=True):
        w = self.w
        w.bodies_aabb()
        w.broadphase()
        w.contacts_meshes(set_joint_flags=flags, capacity=capacity)
        rec, ref, total, capped = w.download_mesh_contacts(C2)
        return rec, ref, total, capped

    def segments(self):
        d = self.w.download()
        L = self.bodies.get("length", np.zeros(self.w.n))
        return [mc.segment_of(self.bodies["pos"][i], d["axis"][i], float(L[i])) for i in range(self.w.n)], d

    def truth(self):
        """[(pair, tri, contacts, margin)] in canonical order, capped pairs, the (pair, tri) near a margin"""
        segs, d = self.segments()
        pairs = d["static_pairs"]
        out, capped, near = [], 0, set()
        for p, (body, st) in enumerate(pairs):
            k = int(st) - self.base
            if k < 0:
                continue
            a, b = segs[body]
            P = mc.Pair(a, b, float(self.bodies["radius"][body]), self.tris[k])
            capped += P.capped
            for t, cs, mg in P.kept:
                out.append((p, t, cs, mg))
            for t, _cs, mg in P.records:
                if mg:
                    near.add((p, t))
            near.update((p, t) for t in P.near)
        return out, capped, near, segs, pairs
