"""The fixtures of tests/test_skin_drawn*.py: numpy only, so that the CPU tests can hold the GPU tests' own inputs to the
properties that make them tests (something selected, something not, every LOD, an extra-plane-only character).

A case is a dict: n, J, vert_first, vert_count, n_verts (of the pool), planes [uint64 words], n_entities, entity, cur_lod,
n_lods, row, lod_first, lod_count, list -- the arguments of skinselref.select and of CharacterBatch.set_skin_select."""
import numpy as np

from skinselref import LOD_ALL, pack_plane


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def sorted_pick(R, hi, k):
    """k ascending distinct indices below hi"""
    return np.sort(R.choice(hi, k, replace=False)).astype(np.uint32)


def tables(lists):
    """rows of per-LOD entries (an array, or None for LOD_ALL) -> (lod_first, lod_count, list)"""
    first, count, out = [], [], []
    for row in lists:
        for entries in row:
            if entries is None:
                first.append(LOD_ALL); count.append(0)
            else:
                first.append(sum(len(o) for o in out)); count.append(len(entries)); out.append(np.asarray(entries, np.uint32))
    n_lods = len(lists[0])
    lst = np.concatenate(out) if out else np.zeros(0, np.uint32)
    return (np.asarray(first, np.uint32).reshape(-1, n_lods), np.asarray(count, np.uint32).reshape(-1, n_lods), lst)


def shared_mesh(n, vpc):
    return np.zeros(n, np.uint32), np.full(n, vpc, np.uint32), vpc


def case(n, J, vf, vc, n_verts, planes, n_entities, entity=None, cur_lod=None, n_lods=0, row=None, lists=None):
    c = dict(n=n, J=J, vert_first=vf, vert_count=vc, n_verts=n_verts, planes=planes, n_entities=n_entities, entity=entity,
             cur_lod=cur_lod, n_lods=n_lods, row=row, lod_first=None, lod_count=None, list=None)
    if lists is not None:
        c["lod_first"], c["lod_count"], c["list"] = tables(lists)
        c["n_lods"] = c["lod_first"].shape[1]
    return c


def ref_args(c):
    """the arguments of skinselref.select"""
    return dict(n_chars=c["n"], vert_count=c["vert_count"], planes=c["planes"], n_entities=c["n_entities"], entity=c["entity"],
                cur_lod=c["cur_lod"], n_lods=c["n_lods"], row=c["row"], lod_first=c["lod_first"], lod_count=c["lod_count"],
                lst=c["list"])


# (a) character counts: 64 joints, one plane, entity slots permuted so that slots 63, 64 and 127 are used
COUNTS = (1, 63, 64, 65, 200)


def counts(n):
    R = rng(100 + n)
    n_ent, vpc = 256, 70                                        # 70 vertices: a second trip of the wavefront, 6 lanes wide
    rest = [s for s in R.permutation(n_ent) if s not in (63, 64, 127)]
    entity = np.asarray(([63, 64, 127] + rest)[:n], np.uint32)
    bits = R.random(n_ent) < 0.5
    bits[[63, 127]] = True
    bits[64] = False                                            # a used slot that is not drawn (n > 1)
    cur_lod = R.integers(0, 4, n_ent).astype(np.int32)
    if n >= 7:                                                  # every LOD once, whatever the draw
        cur_lod[entity[3:7]] = np.arange(4)
        bits[entity[3:7]] = True
    lists = [[None, sorted_pick(R, vpc, 35), sorted_pick(R, vpc, 10), sorted_pick(R, vpc, 3)]]
    vf, vc, nv = shared_mesh(n, vpc)
    return case(n, 64, vf, vc, nv, [pack_plane(bits)], n_ent, entity=entity, cur_lod=cur_lod, lists=lists)


# (b) five planes: a character visible in the last plane only, one visible in none; with and without an entity list
def planes(with_entity):
    R = rng(7 if with_entity else 8)
    n, n_ent, vpc = 90, 192 if with_entity else 90, 40
    entity = R.permutation(n_ent)[:n].astype(np.uint32) if with_entity else None
    slot = (lambda c: int(entity[c])) if with_entity else (lambda c: c)
    bits = [R.random(n_ent) < 0.12 for _ in range(5)]
    for p in range(5):
        bits[p][slot(5)] = p == 4                              # character 5: the last plane only
        bits[p][slot(6)] = False                               # character 6: none
        bits[p][slot(7)] = p == 2                              # character 7: an extra plane only
    cur_lod = R.integers(0, 4, n_ent).astype(np.int32)
    cur_lod[[slot(5), slot(7), slot(8), slot(9)]] = [0, 1, 2, 3]
    bits[0][[slot(8), slot(9)]] = True
    lists = [[None, sorted_pick(R, vpc, 20), sorted_pick(R, vpc, 9), sorted_pick(R, vpc, 2)]]
    vf, vc, nv = shared_mesh(n, vpc)
    return case(n, 64, vf, vc, nv, [pack_plane(b) for b in bits], n_ent, entity=entity, cur_lod=cur_lod, lists=lists)


# (c) ragged meshes of 1 .. 700 vertices in 3 rows; lists of 0, 1, 63, 64, 65, 255, 256 and 257 entries; one row LOD_ALL
def lod_lists(with_tables=True):
    R = rng(21)
    n = 42
    row = (np.arange(n) % 3).astype(np.uint32)
    vc = R.integers(1, 701, n).astype(np.uint32)
    vc[row == 0] = 700                                          # row 0's lists reach beyond vertex 256 of a long mesh
    vc[row == 1] = R.integers(300, 701, int((row == 1).sum()))
    vc[2] = 1; vc[5] = 700                                      # row 2 (whole meshes): the shortest and the longest
    vf = np.concatenate([[0], np.cumsum(vc[:-1])]).astype(np.uint32)
    lists = [[sorted_pick(R, 700, 257), sorted_pick(R, 700, 256), sorted_pick(R, 700, 255), sorted_pick(R, 700, 65)],
             [sorted_pick(R, 300, 64), sorted_pick(R, 300, 63), sorted_pick(R, 300, 1), np.zeros(0, np.uint32)],
             [None, None, None, None]]
    assert lists[0][0].max() > 256
    bits = R.random(n) < 0.6
    cur_lod = R.integers(0, 4, n).astype(np.int32)
    cur_lod[:12] = np.repeat(np.arange(4), 3)                   # every (row, LOD) pair: characters 0 .. 11
    bits[:12] = True
    bits[12:16] = False
    return case(n, 64, vf, vc, int(vc.sum()), [pack_plane(bits)], n, cur_lod=cur_lod, row=row if with_tables else None,
                lists=lists if with_tables else None)


# (d) joint counts 1 and 200
def joints(J):
    R = rng(300 + J)
    n, vpc = 9, 100
    bits = np.asarray([1, 0, 1, 1, 0, 1, 0, 1, 1], bool)
    cur_lod = np.asarray([0, 1, 1, 2, 2, 3, 3, 0, 2], np.int32)
    lists = [[None, sorted_pick(R, vpc, 30), sorted_pick(R, vpc, 5), sorted_pick(R, vpc, 1)]]
    vf, vc, nv = shared_mesh(n, vpc)
    return case(n, J, vf, vc, nv, [pack_plane(bits)], n, cur_lod=cur_lod, lists=lists)


# (e) the three range bits, one case each
def range_bit(which):
    R = rng(40)
    n, n_ent, vpc = 20, 24, 50
    entity = np.arange(n, dtype=np.uint32)
    bits = np.ones(n_ent, bool)
    bits[[3, 9, 10, 15]] = False
    cur_lod = (np.arange(n_ent) % 4).astype(np.int32)
    l1 = sorted_pick(R, vpc, 12)
    if which == "entity":
        entity[4], entity[11] = n_ent, 0xFFFFFFF0              # the first slot past the planes, and one far past them
    elif which == "lod":
        cur_lod[2], cur_lod[7] = -1, 4
    else:
        l1[-1] = vpc                                           # a listed index equal to vert_count
    lists = [[None, l1, sorted_pick(R, vpc, 6), sorted_pick(R, vpc, 2)]]
    vf, vc, nv = shared_mesh(n, vpc)
    return case(n, 64, vf, vc, nv, [pack_plane(bits)], n_ent, entity=entity, cur_lod=cur_lod, lists=lists)


# (f) the plain call: everything drawn, no tables
def plain():
    R = rng(50)
    n = 23
    vc = R.integers(1, 700, n).astype(np.uint32)
    vf = np.concatenate([[0], np.cumsum(vc[:-1])]).astype(np.uint32)
    return case(n, 64, vf, vc, int(vc.sum()), [pack_plane(np.ones(n, bool))], n)


# (g) the captured graph: the planes of two replays
def graph_planes():
    R = rng(60)
    c = counts(65)
    second = R.random(c["n_entities"]) < 0.4
    second[[63, 64]] = [False, True]                            # what the first plane drew / left out, the other way round
    return c, pack_plane(second)


# (h) the frame: a flat scene whose characters stand in a disc around the camera, so that the LOD rule
#     (|d^2 - edge^2| / 3600: LOD 1 from ~60 units, LOD 3 from ~104) gives every LOD, and a second view (a light's)
FRAME_CHARS, FRAME_J, FRAME_VPC = 200, 24, 90


def frame_scene():
    """-> scene (level-major, padded), camera, the light's camera, the characters' entity slots, the LOD tables"""
    from clap_amd import synth
    R = rng(12)
    raw = synth.entities_flat(3000, seed=12)
    scene = synth.pad_levels(raw)
    scene["model_lod"] = np.asarray([[0, 3]], np.uint8)
    cam = synth.camera(pos=(0, 20, 120))
    light = synth.camera(pos=(150, 60, 120), quat=(0.0, 0.70710678, 0.0, 0.70710678), fov_deg=50.0)    # looks down -X
    ent = np.sort(scene["slot_of"][R.choice(3000, FRAME_CHARS, replace=False)]).astype(np.uint32)
    r, phi = 160.0 * np.sqrt(R.random(FRAME_CHARS)), R.uniform(0, 2 * np.pi, FRAME_CHARS)
    scene["pos_scale"][ent, 0] = (r * np.cos(phi)).astype(np.float32)
    scene["pos_scale"][ent, 1] = R.uniform(10, 30, FRAME_CHARS).astype(np.float32)
    scene["pos_scale"][ent, 2] = (120.0 + r * np.sin(phi)).astype(np.float32)
    lists = tables([[None, sorted_pick(R, FRAME_VPC, 40), sorted_pick(R, FRAME_VPC, 12), sorted_pick(R, FRAME_VPC, 4)]])
    return scene, cam, light, ent, lists


SELECTIVE = {                                                  # the cases whose point is that SOME characters are drawn
    **{f"counts_{n}": (lambda n=n: counts(n)) for n in COUNTS if n >= 63},
    "planes_entity": lambda: planes(True), "planes_plain": lambda: planes(False),
    "lists": lambda: lod_lists(True), "no_rows": lambda: lod_lists(False),
    "joints_1": lambda: joints(1), "joints_200": lambda: joints(200),
    "range_entity": lambda: range_bit("entity"), "range_lod": lambda: range_bit("lod"), "range_list": lambda: range_bit("list"),
    "graph_first": lambda: graph_planes()[0],
}
