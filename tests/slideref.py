"""character_sweep_delta and character_apply_velocity (character.c:193-243, 245-310) restated in numpy float32 / float64
scalars, with the sweep a callable: what clapgpu_characters_slide is compared with.  Nothing here imports the device
code of the slide; the scenes of test_slide.py and test_slide_gpu.py are built here too.

The sweep callables:
  OracleSweep   oracle.binding.sweep_capsule over the oracle's geoms (the committed restatement of
                phys_body_sweep_capsule), candidates from the swept AABB as test_capsule_sweeps_match_restatement builds
                them: statics, then bodies with bit 31 set, with its 1e-3 margin
  MeshSweep     tests/meshcontactref.sweep against one mesh
The mover's position is patched between the iterations; everything else stays where it was before the call."""
import numpy as np

from clap_amd import synth

f32 = np.float32


def vec3_len(v):
    """linmath.h:40-51: p = 0; p += v[i] * v[i]; sqrtf(p)"""
    p = f32(0.0)
    for i in range(3):
        p = f32(p + f32(v[i] * v[i]))
    return np.sqrt(p, dtype=f32)


def vec3_scale(v, s):
    s = f32(s)
    return np.array([f32(f32(v[i]) * s) for i in range(3)], f32)


def vec3_mul_inner(a, b):
    p = f32(0.0)
    for i in range(3):
        p = f32(p + f32(b[i] * a[i]))
    return p


def character_sweep_delta(sweep, move, delta, min_normal_y, stop_on_block, log):
    """character.c:193-243.  sweep(delta) -> (frac, normal[3] float32, hit) from the mover's current position;
    move(step) is phys_body_move.  log gets one dict per sweep made.  Returns first_frac."""
    delta = np.asarray(delta, f32).copy()
    first_frac = f32(1.0)
    for it in range(3):
        if vec3_len(delta) < f32(1e-6):                                  # :200
            break
        frac, normal, hit = sweep(delta)
        frac, normal = f32(frac), np.asarray(normal, f32)
        filtered = bool(frac < f32(1.0) and normal[1] < f32(min_normal_y))
        if filtered:                                                      # :213
            frac = f32(1.0)
        if it == 0:
            first_frac = frac
        push = hit if (frac < f32(1.0) and hit >= 0) else -1              # :220 (statics have no body to push)
        moved = bool(frac > 0)
        if moved:                                                         # :223-227
            move(vec3_scale(delta, frac))
        log.append(dict(iter=it, frac=frac, filtered=filtered, push=push, moved=moved, hit=hit))
        if frac >= f32(1.0):
            break
        if frac <= f32(0.0) and stop_on_block:
            log[-1]["blocked"] = True
            break
        remaining = vec3_scale(delta, f32(f32(1.0) - frac))               # :235-239
        dot = vec3_mul_inner(remaining, normal)
        along = vec3_scale(normal, dot)
        delta = np.array([f32(remaining[i] - along[i]) for i in range(3)], f32)
    return first_frac


def character_apply_velocity(sweep, move, velocity, airborne, dt_sec):
    """The ENTITY3D_HAS_PHYSICS branch, character.c:254-310.  Returns dict(velocity, first_frac[2], push_hit[6], calls:
    the sweep logs of each character_sweep_delta call, changed: False when dt_sec < 1e-6 skipped everything)."""
    v = np.asarray(velocity, f32).copy()
    out = dict(velocity=v, first_frac=np.ones(2, f32), push_hit=np.full(6, -1, np.int32), calls=[], changed=False)
    dt = float(dt_sec)
    if dt < 1e-6:                                                         # :259
        return out
    if dt > 1.0 / 30.0:                                                   # :262
        dt = 1.0 / 30.0
    out["changed"] = True

    def call(k, delta, min_normal_y, stop):
        log = []
        ff = character_sweep_delta(sweep, move, delta, min_normal_y, stop, log)
        out["first_frac"][k] = ff
        for s in log:
            out["push_hit"][3 * k + s["iter"]] = s["push"]
        out["calls"].append(log)
        return ff

    if airborne and not (v[1] > 0):                                       # falling, :293-300
        v_delta = np.array([0, f32(np.float64(v[1]) * dt), 0], f32)
        h_delta = np.array([f32(np.float64(v[0]) * dt), 0, f32(np.float64(v[2]) * dt)], f32)
        v_moved = call(0, v_delta, 0.5, False)
        call(1, h_delta, -1.0, True)
        if v_moved < f32(1.0):
            v[1] = 0
    else:
        moved = call(0, vec3_scale(v, f32(dt)), -1.0, True)               # :280-284, :304-306
        if airborne and moved < f32(1.0):
            v[1] = 0
    return out


def groups(res):
    """which of the groups of test_slide.py's coverage check a mover's result belongs to"""
    sweeps = [s for c in res["calls"] for s in c]
    g = set()
    if res["calls"] and res["calls"][0] and res["calls"][0][0]["frac"] == 1.0 and not res["calls"][0][0]["filtered"]:
        g.add("free")
    if any(s.get("blocked") for s in sweeps):
        g.add("blocked")
    if any(sum(s["moved"] for s in c) >= 2 for c in res["calls"]):
        g.add("slid")
    if any(s["filtered"] for s in sweeps):
        g.add("filtered")
    if res["zeroed"]:
        g.add("zeroed")
    if (res["push_hit"] >= 0).any():
        g.add("pushed")
    return g


# ------------------------------------------------------------------------------------------------- sweeps
def capsule_box(pos, axis, radius, length):
    """dxCapsule::computeAABB / dxSphere::computeAABB as (lo[3], hi[3])"""
    h = np.abs(np.asarray(axis, float)) * (float(length) * 0.5) + float(radius)
    return np.asarray(pos, float) - h, np.asarray(pos, float) + h


def canonical_candidates(lo, hi, delta, static_bb, body_bb, margin=1e-3):
    """statics, then bodies (bit 31), ascending, whose AABB meets the swept box of (lo, hi) along delta"""
    d = np.asarray(delta, np.float64)
    slo, shi = np.minimum(lo, lo + d) - margin, np.maximum(hi, hi + d) + margin
    s_hit = np.flatnonzero(np.all((static_bb[:, 0::2] <= shi) & (static_bb[:, 1::2] >= slo), axis=1)) if len(static_bb) else \
        np.zeros(0, np.int64)
    b_hit = np.flatnonzero(np.all((body_bb[:, 0::2] <= shi) & (body_bb[:, 1::2] >= slo), axis=1))
    return np.concatenate([s_hit.astype(np.uint32), b_hit.astype(np.uint32) | np.uint32(1 << 31)])


class OracleSweep:
    """Scene A through the oracle.  One instance holds the poses from before the call; mover(i) gives the (sweep, move,
    position) of body i on a patched copy of the positions."""

    def __init__(self, b, statics):
        from oracle import binding as ob
        self.ob, self.b, self.statics = ob, b, np.ascontiguousarray(statics, np.float64)
        self.st = ob.bodies_state(b)
        ob.bodies_aabb(b, self.st)
        self.S = ob.geoms(len(statics), kind=np.full(len(statics), 2, np.uint8), aabb=self.statics)

    def mover(self, i):
        ob, b, st = self.ob, self.b, self.st
        pos = np.ascontiguousarray(st["pos"], np.float64).copy()
        self.seen = set()                                                 # the bodies among this mover's candidates
        A = ob.geoms(b["n"], pos=pos, axis=st["axis"], radius=b["radius"], length=b.get("length"))
        assert A[1][0] is pos                                             # the oracle reads the patched array
        L = float(b["length"][i]) if "length" in b else 0.0

        def sweep(delta):
            lo, hi = capsule_box(pos[i], st["axis"][i], b["radius"][i], L)
            cand = canonical_candidates(lo, hi, delta, self.statics, st["aabb"])
            self.seen.update(int(c & 0x7fffffff) for c in cand if c >> 31 and int(c & 0x7fffffff) != i)
            return ob.sweep_capsule(A, i, delta, self.S, cand)

        def move(step):
            for a in range(3):
                pos[i, a] = pos[i, a] + np.float64(step[a])

        return sweep, move, lambda: pos[i].copy()


class MeshSweep:
    """Scene B on the restatement alone: the mover against one mesh's triangles (meshcontactref.sweep)."""

    def __init__(self, b, axis, tris, static_index):
        self.b, self.axis, self.tris, self.hit = b, axis, tris, -2 - int(static_index)

    def mover(self, i):
        import meshcontactref as mc
        b = self.b
        pos = np.array(b["pos"][i], np.float64)
        L = float(b["length"][i]) if "length" in b else 0.0

        def sweep(delta):
            f, n, th = mc.sweep(pos, float(b["radius"][i]), L, self.axis[i], delta, self.tris)
            return f, n, (self.hit if th else -1)

        def move(step):
            for a in range(3):
                pos[a] = pos[a] + np.float64(step[a])

        return sweep, move, lambda: pos.copy()


class SceneBSweep:
    """Scene B on the restatement alone: the terrain (meshcontactref.sweep, static `static_index`) and the other bodies
    (the oracle's sweep over candidates from the swept AABB, no statics), each swept on its own.  The two are joined by
    the smaller frac, the mesh first on a tie (statics come before bodies).  That is the joint sweep exactly when only
    one of the two hits; when both hit it is the joint sweep unless the two first touched at different steps and the
    later one backs up further -- `both` counts the sweeps where both hit, for callers that need exactness.  The box
    mesh of scene B stands beside the terrain (x >= 38): movers_b keeps away from it."""

    def __init__(self, b, tris, static_index):
        self.bodies = OracleSweep(b, np.zeros((0, 6)))
        self.mesh = MeshSweep(b, self.bodies.st["axis"], tris, static_index)
        self.both = 0

    def mover(self, i):
        bs, bm, where = self.bodies.mover(i)
        ms, mm, _w = self.mesh.mover(i)
        self.both = 0
        self.seen = self.bodies.seen

        def sweep(delta):
            fm, nm, hm = ms(delta)
            fb, nb, hb = bs(delta)
            self.both += bool(f32(fm) < 1 and f32(fb) < 1)
            return (fm, nm, hm) if f32(fm) <= f32(fb) else (fb, nb, hb)

        def move(step):
            bm(step)
            mm(step)

        return sweep, move, where


def run_mover(world, i, velocity, airborne, dt_sec):
    """character_apply_velocity for body i of an OracleSweep / MeshSweep / any object with mover(i); adds pos, zeroed"""
    sweep, move, where = world.mover(int(i))
    res = character_apply_velocity(sweep, move, velocity, airborne, dt_sec)
    res["pos"] = where()
    res["zeroed"] = bool(res["changed"] and airborne and res["first_frac"][0] < f32(1.0))     # :283, :299
    return res


# ------------------------------------------------------------------------------------------------- scenes
N_MOVERS = 300


def scene_a():
    """6 000 capsules in a 14-unit box plus 40 static boxes (test_capsule_sweeps_match_restatement's)"""
    b = synth.capsule_bodies(6000, box=14.0, seed=19)
    return b, synth.static_boxes(40, 14.0)


def movers_a(n_bodies, seed=3):
    """(movers, velocity [n, 3] float32, airborne [n]): walkers, jumpers and fallers with speeds of a few units a frame"""
    rng = np.random.Generator(np.random.PCG64(seed))
    movers = rng.choice(n_bodies, N_MOVERS, replace=False).astype(np.uint32)
    v = rng.normal(0, 14.0, (N_MOVERS, 3)).astype(np.float32)
    airborne = np.zeros(N_MOVERS, np.uint8)
    airborne[100:] = 1
    v[100:170, 1] = np.abs(v[100:170, 1]) + 1.0                           # rising
    v[170:, 1] = -np.abs(v[170:, 1]) - 1.0                                # falling
    v[:4] = 0                                                             # no movement
    v[4:8] *= 1e-5                                                        # below the 1e-6 exit
    v[8:20, 0] = v[8:20, 2] = 0                                           # straight up or down
    return movers, v, airborne


def ground_b(x, z):
    return np.sin(x * 0.37) * np.cos(z * 0.29)


def scene_b(n=3000, seed=11):
    """tests/meshscene.py's terrain plus box: (bodies, meshes) for meshscene.Scene -- capsules scattered over a 33 x 33
    height field of side 32, some of them around a box mesh beside it"""
    vx, idx = synth.heightfield(33, 32.0)
    bv, bi = synth.box_mesh()
    ident = [0.0, 0.0, 0.0, 1.0]
    meshes = [(vx, idx, 1.0, [0.0, 0.0, 0.0], ident), (bv, bi, 4.0, [40.0, 0.0, 16.0], ident)]
    b = synth.capsule_bodies(n, box=32.0, seed=seed)
    R = np.random.Generator(np.random.PCG64(seed))
    b["pos"][:, 0] = R.uniform(0.0, 32.0, n)
    b["pos"][:, 2] = R.uniform(0.0, 32.0, n)
    b["pos"][:, 1] = ground_b(b["pos"][:, 0], b["pos"][:, 2]) + R.uniform(0.2, 2.5, n)
    b["lvel"][:] = 0
    m = n // 6                                                            # some bodies around the box
    R = np.random.Generator(np.random.PCG64(seed + 1))
    b["pos"][:m] = np.stack([R.uniform(37, 43, m), R.uniform(-3, 3, m), R.uniform(13, 19, m)], 1)
    return b, meshes


def movers_b(b, seed=5):
    """(movers, velocity, airborne) over the terrain, away from its rim and from the box mesh: walkers pressed onto the
    slope, jumpers, and fallers with a sideways push -- among the bodies scattered there, so that every branch is taken"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n_bodies = int(b["n"])
    inner = np.flatnonzero((np.arange(n_bodies) >= n_bodies // 6) & (np.abs(b["pos"][:, 0] - 16) < 11) &
                           (np.abs(b["pos"][:, 2] - 16) < 11))
    movers = rng.choice(inner, N_MOVERS, replace=False).astype(np.uint32)
    v = rng.normal(0, 12.0, (N_MOVERS, 3)).astype(np.float32)
    airborne = np.zeros(N_MOVERS, np.uint8)
    airborne[100:] = 1
    v[:100, 1] = -np.abs(v[:100, 1])                                      # walkers pressed onto the slope
    v[100:150, 1] = np.abs(v[100:150, 1]) + 1.0
    v[150:, 1] = -np.abs(v[150:, 1]) * 3 - 5.0                            # fallers that reach the ground
    return movers, v, airborne
