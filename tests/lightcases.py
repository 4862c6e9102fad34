"""Chosen inputs for the light grid (clap_amd/csrc/lights.hip): lights next to every decision the kernel makes.

The kernel is a chain of decisions -- fabsf(w) < 1e-3, (double)ndc.z > 1.0, distsq < rsq at four corners -- and is held
to the oracle bit for bit only because its fp32 operation order is the reference's and nothing is contracted.  A
random light almost never lies next to one of them.  The builders here put lights there: a coordinate is moved until
the oracle's answer changes and then bisected in float32 until the two positions are adjacent floats, so that one
rounding made differently on either side decides the bit.

Everything is built with the oracle on the CPU, is deterministic, and uses no GPU.  A case is a dict
(name, lights, cam, view, proj, width, height, cell); `lights` is a dict as made by clap_amd.synth.lights().
tests/test_light_edges.py checks that the cases are what they claim.
"""
import functools

import numpy as np

from clap_amd import synth
from oracle import binding as ob

F32 = np.float32
M = synth.LIGHTS_MAX

CAMERAS = {
    "identity": synth.camera(),
    "tilted_z01": synth.camera(pos=(1.0, 2.0, 3.0), quat=synth.quat_from_euler_xyz(0.1, 0.2, -0.05), ndc_z_zero_one=1),
    "wide_off": synth.camera(pos=(-30.0, 12.0, 25.0), quat=synth.quat_from_euler_xyz(-0.15, 0.4, 0.05), fov_deg=110.0),
}
GRIDS = [(1000, 600, 64), (640, 384, 32)]          # 1000 is no multiple of 64: the last tile column hangs over the screen


def matrices(cam):
    _fr, view, proj = ob.frustum_from_camera(cam)
    return np.asarray(view, F32).copy(), np.asarray(proj, F32).copy()


def light_set(n, active=1):
    """n slots of point lights at the origin with the default attenuation and no colour: a blank to fill in."""
    return dict(nr_lights=n, pos=np.zeros((n, 3), F32), color=np.zeros((n, 3), F32),
                attenuation=np.tile(np.asarray([1, 0, 0], F32), (n, 1)), is_dir=np.zeros(n, np.int32),
                active=np.full(n, active, np.uint32))


def copy_set(L):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in L.items()}


def case(name, lights, cam, grid, mats=None):
    view, proj = mats if mats is not None else matrices(cam)
    w, h, cell = grid
    return dict(name=name, lights=lights, cam=cam, view=view, proj=proj, width=w, height=h, cell=cell)


def oracle_tiles(c, compute=None):
    """The case's tile masks u32[th][tw][4] by the oracle (or by another build's light_grid_compute)."""
    return (compute or ob.light_grid_compute)(c["lights"], c["view"], c["proj"], c["width"], c["height"], c["cell"])


def columns(tiles):
    """bool[th][tw][128]: bit i of every tile"""
    th, tw, _ = tiles.shape
    return np.unpackbits(np.ascontiguousarray(tiles).view(np.uint8), bitorder="little").reshape(th, tw, 128).astype(bool)


def world_from_view(cam, pv):
    """View-space points (camera looks down -Z) to world space, in float64; the result is rounded to float32."""
    x, y, z, w = (float(v) for v in cam["cam_quat"])
    R = np.asarray([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)
    return (np.asarray(pv, np.float64) @ R.T + cam["cam_pos"].astype(np.float64)).astype(F32)


# ------------------------------------------------------------------------------------------------- 1. disc edges
def disc_lights(cam, grid, seed=1):
    """128 point lights in front of the camera, one in every slot, each with a disc of one to three cells on the screen
    and its centre on it: every one lights some tiles and not all of them."""
    w, h, cell = grid
    rng = np.random.Generator(np.random.PCG64(seed))
    fov, aspect = float(cam["persp"][0]), float(cam["persp"][1])
    ty = np.tan(fov / 2.0)
    depth = rng.uniform(5.0, 80.0, M)
    pv = np.stack([rng.uniform(-0.8, 0.8, M) * ty * aspect * depth, rng.uniform(-0.8, 0.8, M) * ty * depth, -depth], 1)
    L = light_set(M)
    L["pos"] = world_from_view(cam, pv)
    # colours and linear terms in steps of 1/16 and 1/64: short mantissas, which keep the fixture of these sets small
    L["color"] = (np.ceil(rng.uniform(0.2, 1.0, (M, 3)) * rng.uniform(0.5, 4.0, (M, 1)) * 16.0) / 16.0).astype(F32)
    # radius ~ sqrt(256 max(colour) / quadratic) in the world, times fx / depth * width / 2 on the screen
    r_px = rng.uniform(1.0, 3.0, M) * cell
    r_world = r_px * depth / (1.0 / (ty * aspect) * w / 2.0)
    L["attenuation"] = np.stack([np.ones(M), np.ceil(rng.uniform(0.02, 0.8, M) * 64.0) / 64.0, 256.0 * L["color"].max(1) / r_world ** 2], 1).astype(F32)
    return L


def bisect_columns(base_set, cam, grid, compute=None):
    """For every slot at once (bit i of a tile depends on light i alone): move coordinate i % 3 of light i until its bit
    column changes, then bisect in float32 to two adjacent floats.  Returns (near, far, bracketed): two whole light sets
    -- `near` keeps every slot's column as in base_set, `far` has the first position on the other side -- and the
    bool[128] of the slots for which a change was found."""
    view, proj = matrices(cam)
    w, h, cell = grid
    fn = compute or ob.light_grid_compute

    def cols(pos):
        L = copy_set(base_set)
        L["pos"] = pos
        return columns(fn(L, view, proj, w, h, cell))

    base = cols(base_set["pos"])
    n = base_set["nr_lights"]
    axis = np.arange(n) % 3
    at = np.arange(n)
    lo = base_set["pos"][at, axis].copy()
    hi = lo.copy()
    found = np.zeros(n, bool)
    step = np.full(n, 0.25, F32)
    for _ in range(12):                                    # up to +512 world units: far beyond every disc
        pos = base_set["pos"].copy()
        trial = (lo + step).astype(F32)                    # lo stays the base position: its column is base's
        pos[at, axis] = np.where(found, lo, trial)
        changed = (cols(pos)[..., :n] != base[..., :n]).any(axis=(0, 1)) & ~found
        hi = np.where(changed, trial, hi)
        found |= changed
        step = np.where(found, step, step * 2).astype(F32)
        if found.all():
            break
    for _ in range(64):
        mid = ((lo.astype(np.float64) + hi.astype(np.float64)) / 2.0).astype(F32)
        open_ = found & (mid != lo) & (mid != hi)
        if not open_.any():
            break
        pos = base_set["pos"].copy()
        pos[at, axis] = np.where(open_, mid, lo)
        same = ~(cols(pos)[..., :n] != base[..., :n]).any(axis=(0, 1))
        lo = np.where(open_ & same, mid, lo)
        hi = np.where(open_ & ~same, mid, hi)
    near, far = copy_set(base_set), copy_set(base_set)
    near["pos"][at, axis] = lo
    far["pos"][at, axis] = np.where(found, hi, lo)
    return near, far, found


@functools.lru_cache(maxsize=None)
def disc_edge_pairs():
    """[(near case, far case, bracketed)] for every camera and grid: 2 x 128 lights, each slot on either side of its edge."""
    out = []
    for cname, cam in CAMERAS.items():
        for grid in GRIDS:
            near, far, found = bisect_columns(disc_lights(cam, grid), cam, grid)
            tag = f"disc_{cname}_{grid[0]}x{grid[1]}c{grid[2]}"
            out.append((case(tag + "_near", near, cam, grid), case(tag + "_far", far, cam, grid), found))
    return out


# ------------------------------------------------------------------------------------------------- 2. gate edges
GATE_CAMERAS = {
    "identity": synth.camera(),
    "identity_z01": synth.camera(ndc_z_zero_one=1),
    "tilted": synth.camera(pos=(1.0, 2.0, 3.0), quat=synth.quat_from_euler_xyz(0.1, 0.2, -0.05)),
    "tilted_z01": CAMERAS["tilted_z01"],
}
GATE_GRID = (640, 384, 64)
# a light this strong reaches tiles from the far plane (radius ~ 500 world units) and from next to the eye
GATE_COLOR, GATE_ATT = (1.0, 1.0, 1.0), (1.0, 0.1, 0.001)
# slot of (far lit, far gated, eye lit, eye gated, behind x 4): both ballots, and the ends of each
GATE_SLOTS = dict(far_lit=5, far_gated=69, eye_lit=101, eye_gated=37, behind=(63, 64, 0, 127))
BEHIND_DEPTHS = (-0.0005, -0.002, -5.0, -600.0)            # negative w, on both sides of |w| = 1e-3


def _lit(pos, cam, mats, compute=None):
    L = light_set(1)
    L["pos"][0], L["color"][0], L["attenuation"][0] = pos, GATE_COLOR, GATE_ATT
    return bool((compute or ob.light_grid_compute)(L, mats[0], mats[1], *GATE_GRID).any())


def bisect_along(cam, mats, t_lit, t_gated):
    """A light straight ahead at depth t: from a lit depth and a gated one to two positions that differ in one coordinate
    by one float32 step, the first lit and the second not."""
    def at(t):
        return world_from_view(cam, [0.0, 0.0, -t])
    a, b = float(t_lit), float(t_gated)
    assert _lit(at(a), cam, mats) and not _lit(at(b), cam, mats)
    for _ in range(30):                                    # close in along the ray first
        m = (a + b) / 2.0
        if _lit(at(m), cam, mats):
            a = m
        else:
            b = m
    p, q = at(a), at(b)
    # then walk from p to q one coordinate at a time; the coordinate at which the answer changes is bisected in float32
    for ax in range(3):
        nxt = p.copy()
        nxt[ax] = q[ax]
        if _lit(nxt, cam, mats):
            p = nxt
            continue
        lo, hi = p[ax], q[ax]
        while True:
            mid = F32((np.float64(lo) + np.float64(hi)) / 2.0)
            if mid == lo or mid == hi:
                break
            trial = p.copy()
            trial[ax] = mid
            if _lit(trial, cam, mats):
                lo = mid
            else:
                hi = mid
        p, nxt = p.copy(), p.copy()
        p[ax], nxt[ax] = lo, hi
        return p, nxt, ax
    raise AssertionError("the answer did not change between the two depths")


@functools.lru_cache(maxsize=None)
def gate_cases():
    """One light set per camera: the two sides of ndc.z > 1 and of |w| < 1e-3 as adjacent floats, and lights behind the eye.
    Returns [(case, dict(far=(p, q, axis), eye=(p, q, axis)))]."""
    out = []
    for cname, cam in GATE_CAMERAS.items():
        mats = matrices(cam)
        far = bisect_along(cam, mats, 400.0, 600.0)
        eye = bisect_along(cam, mats, 0.01, 0.0005)
        L = light_set(M, active=0)
        slots = [GATE_SLOTS["far_lit"], GATE_SLOTS["far_gated"], GATE_SLOTS["eye_lit"], GATE_SLOTS["eye_gated"]]
        slots += list(GATE_SLOTS["behind"])
        pts = [far[0], far[1], eye[0], eye[1]] + [world_from_view(cam, [0.0, 0.0, -t]) for t in BEHIND_DEPTHS]
        for s, p in zip(slots, pts):
            L["active"][s] = 1
            L["pos"][s], L["color"][s], L["attenuation"][s] = p, GATE_COLOR, GATE_ATT
        out.append((case("gate_" + cname, L, cam, GATE_GRID, mats), dict(far=far, eye=eye)))
    return out


# ------------------------------------------------------------------------------------------------- 3. radius edges
RADIUS_LIGHTS = [
    # name, slot, pos, colour, attenuation (constant, linear, quadratic)
    ("linear_only", 2, (0.5, 0.2, -10.0), (1, 1, 1), (1.0, 0.5, 0.0)),             # 0 / 0
    ("constant_only", 34, (-0.5, 0.2, -10.0), (1, 1, 1), (1.0, 0.0, 0.0)),          # 0 / 0, and not directional
    ("linear_only_neg", 66, (0.5, -0.2, -10.0), (1, 1, 1), (1.0, -0.5, 0.0)),       # x / 0
    ("neg_discriminant", 98, (0.0, 0.0, -10.0), (1, 1, 1), (1000.0, 1.0, 1.0)),     # sqrt of a negative number
    ("colour_zero_nan", 31, (1.0, 1.0, -10.0), (0, 0, 0), (1.0, 2.0, 200.0)),
    ("colour_zero_negative_radius", 32, (-1.0, 1.0, -10.0), (0, 0, 0), (99.0, 2.0, 0.01)),   # radius -90: its square counts
    ("radius_sq_overflows", 64, (3.0, -2.0, -40.0), (1e30, 1.0, 1.0), (1.0, 0.1, 1e-8)),
    ("colour_inf", 95, (3.0, 2.0, -40.0), (np.inf, 1.0, 1.0), (1.0, 0.1, 1.0)),
    ("on_the_camera_plane", 96, (0.3, 0.2, 0.0), (1, 1, 1), (1.0, 2.0, 200.0)),     # -vp.z == 0
    ("pos_x_inf", 63, (np.inf, 0.0, -10.0), (1, 1, 1), (1.0, 2.0, 2.0)),
    ("pos_z_minus_inf", 127, (0.0, 0.0, -np.inf), (1, 1, 1), (1.0, 2.0, 2.0)),
    ("pos_z_plus_inf", 0, (0.0, 0.0, np.inf), (1, 1, 1), (1.0, 2.0, 2.0)),
    ("ordinary", 1, (0.0, 0.0, -10.0), (1, 1, 1), (1.0, 2.0, 200.0)),               # so that the case has both answers
]


@functools.lru_cache(maxsize=None)
def radius_cases():
    """Degenerate attenuations, colours and positions, under the identity camera and the tilted one."""
    out = []
    for cname in ("identity", "tilted_z01"):
        cam = CAMERAS[cname]
        L = light_set(M, active=0)
        for _name, s, pos, col, att in RADIUS_LIGHTS:
            L["active"][s] = 1
            with np.errstate(invalid="ignore"):
                L["pos"][s] = world_from_view(cam, pos) if np.all(np.isfinite(pos)) else np.asarray(pos, F32)
            L["color"][s], L["attenuation"][s] = col, att
        out.append(case("radius_" + cname, L, cam, (640, 384, 64)))
    return out


# ------------------------------------------------------------------------------------------------- 4. slots and words
LONE_SLOTS = (0, 31, 32, 63, 64, 95, 96, 127)
NR_LIGHTS = (1, 63, 64, 65, 127, 128)
DIR_SLOTS = (1, 31, 32, 62, 64, 90, 97, 126)
SLOT_GRID = (640, 384, 64)


def lone_bit(s):
    """The tile u32[4] that holds bit s alone"""
    t = np.zeros(4, np.uint32)
    t[s // 32] = np.uint32(1) << np.uint32(s % 32)
    return t


@functools.lru_cache(maxsize=None)
def slot_cases():
    cam = CAMERAS["identity"]
    out = []
    for s in LONE_SLOTS:
        for kind in ("dir", "point"):
            L = light_set(s + 1, active=0)
            L["active"][s] = 1
            if kind == "dir":
                L["is_dir"][s] = 1
            else:                                          # a disc of some 10^4 pixels: it covers the screen
                L["pos"][s], L["color"][s], L["attenuation"][s] = (0.0, 0.0, -10.0), (4, 4, 4), (1.0, 0.1, 0.001)
            # the other slots would light tiles if they were looked at: released, they must not be
            for o in range(s):
                L["pos"][o], L["color"][o], L["attenuation"][o] = (0.0, 0.0, -10.0), (4, 4, 4), (1.0, 0.1, 0.001)
            out.append(case(f"lone_{kind}_{s}", L, cam, SLOT_GRID))
    base = disc_lights(cam, SLOT_GRID, seed=4)
    for n in NR_LIGHTS:
        L = {k: (v[:n].copy() if isinstance(v, np.ndarray) else n) for k, v in base.items()}
        out.append(case(f"nr_lights_{n}", L, cam, SLOT_GRID))
    L = copy_set(base)
    L["is_dir"][list(DIR_SLOTS)] = 1
    out.append(case("dir_in_every_word", L, cam, SLOT_GRID))
    L = light_set(12, active=0)
    for s in (9, 10, 11):
        L["pos"][s], L["color"][s], L["attenuation"][s] = (0.0, 0.0, -10.0), (4, 4, 4), (1.0, 0.1, 0.001)
    L["active"][[9, 11]] = 1
    out.append(case("released_between_two_lit", L, cam, SLOT_GRID))
    return out


# ------------------------------------------------------------------------------------------------- 5. grid shapes
# (width, height, cell) -> tiles: a wave takes 16 tiles and a block 64
SHAPES = {
    1: (10, 7, 64),            # cell > width and height
    15: (113, 5, 8),           # 15 x 1, theight = 1, width % cell != 0
    16: (3, 61, 4),            # 1 x 16, twidth = 1
    17: (260, 16, 16),         # 17 x 1
    63: (283, 223, 32),        # 9 x 7
    64: (512, 512, 64),        # 8 x 8, nothing hangs over
    65: (127, 50, 10),         # 13 x 5
    129: (853, 59, 20),        # 43 x 3
}


@functools.lru_cache(maxsize=None)
def shape_cases():
    cam = CAMERAS["identity"]
    return [case(f"tiles_{n}", disc_lights(cam, grid, seed=5), cam, grid) for n, grid in SHAPES.items()]


# ------------------------------------------------------------------------------------------------- 7. carriers
CARRIER_COUNTS = (1, 127, 128, 129, 257)


def carrier_case(nc, seed=7):
    """A carrier list of nc entries over a small entity scene.  One slot is named by carrier k and by k + 128 (and by
    k + 256 where that exists): the kernel walks the list in strides of 128, so the same lane meets them in different
    turns.  The last one wins.  The list also holds an entity >= n, a slot < 0, a slot >= nr_lights, a released slot, a
    child entity and a clean entity, where it is long enough.  Returns dict(scene, lights, carriers, dirty, oracle_carriers):
    oracle_carriers is the list without the entity >= n, which the oracle (like the reference, which holds pointers) cannot
    be asked about."""
    from clap_amd import _lib
    scene = synth.pad_levels(synth.entities_chains(300, 2, seed=5))
    n = int(scene["n"])
    L = synth.lights(120, seed=3, inactive_frac=0.0)
    L["is_dir"][:] = 0
    released = 5
    L["active"][released] = 0
    R = np.random.Generator(np.random.PCG64(seed + nc))
    roots, kids = np.flatnonzero(scene["parent"] < 0), np.flatnonzero(scene["parent"] >= 0)
    ent = R.choice(roots, nc, replace=False).astype(np.uint32)
    # every carrier its own slot at first (slots 8..119 in turn, so no slot is named twice by chance below 112 carriers)
    light = (8 + np.arange(nc) % 112).astype(np.int32)
    k = 0
    twice = 3                                               # the slot named at k, k + 128 and k + 256
    for j in range(k, nc, 128):
        light[j] = twice
    if nc > 60:
        light[1] = light[60] = 4                            # a second doubled slot, inside one stride: two lanes of one turn
    special = {}
    if nc >= 127:
        special = dict(entity_past_n=20, slot_negative=21, slot_past_nr=22, released=23, child=24, clean=25)
        ent[20] = n + 3
        light[20], light[24], light[25] = 6, 7, 2           # slots that no other carrier names
        light[21] = -1
        light[22] = 120                                     # == nr_lights
        light[23] = released
        ent[24] = kids[0]
        clean_entity = int(ent[25])
    scene["flags"] = scene["flags"].copy()
    if special:
        scene["flags"][clean_entity] &= ~np.uint32(_lib.E_DIRTY)
    dirty = ((scene["flags"] & _lib.E_DIRTY) != 0).astype(np.uint8)
    carriers = dict(entity=ent, light=light, off=R.normal(size=(nc, 3)).astype(F32))
    keep = ent < n
    oracle_carriers = {key: v[keep] for key, v in carriers.items()}
    return dict(scene=scene, lights=L, carriers=carriers, oracle_carriers=oracle_carriers, dirty=dirty, twice=twice, k=k,
                special=special)


def carrier_expected(c, all_dirty):
    d = np.ones_like(c["dirty"]) if all_dirty else c["dirty"]
    return ob.lights_from_entities(c["oracle_carriers"], c["scene"]["pos_scale"], c["scene"]["parent"], d, c["lights"])


# ------------------------------------------------------------------------------------------------- the fixture's cases
def fixture_cases():
    """What tests/golden/lightgrid_edges.npz holds (tools/make_golden.py): the gate cases, the radius cases and one
    disc-edge pair of sets."""
    near, far, _found = disc_edge_pairs()[0]
    return [c for c, _ in gate_cases()] + list(radius_cases()) + [near, far]
