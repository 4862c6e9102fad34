"""The statics image of a broadphase object, in plain numpy / Python loops: the yardstick of the device re-registration
(clapgpu_bp_statics_update).  Written from the image rule, not from the host code that bins at create time:

* per level l the cell is c = cell * 2^l and a box is grown by c * 0.5 * (1 + 1e-9);
* a cell coordinate is floor(x / c) held to +-5e8 (NaN: -5e8), a block coordinate the cell coordinate >> 2;
* a static is LARGE when an edge is inverted or NaN, or when it covers more than 64 blocks; otherwise it is entered once
  per distinct hash bucket among its blocks;
* the CSR runs over the buckets, ascending static index inside a bucket; a leveled object lays its levels end to end,
  starts offset, with large_start[l] .. large_start[l + 1] level l's part of the large list;
* the bounds are the union of the boxes that are registered (not large) on some level.
"""
import math

import numpy as np

CELL = 1.0
N_MAX = 2048                    # bodies of the objects the tests make: 1024 block buckets
BUCKETS = 1024


def cell_coord(x, c):
    if math.isnan(x):
        return -500000000
    q = x / c
    if math.isnan(q) or q < -5.0e8:
        return -500000000
    if q > 5.0e8:
        return 500000000
    return int(math.floor(q))


def block_hash(bx, by, bz, mask):
    m = 0xffffffff
    h = ((bx & m) * 73856093 & m) ^ ((by & m) * 19349663 & m) ^ ((bz & m) * 83492791 & m)
    return (h ^ (h >> 15)) & mask


def static_buckets(box, c, buckets):
    """None for a large static, else (the distinct buckets of its blocks in first-met order, its number of blocks)"""
    grow = c * 0.5 * (1.0 + 1e-9)
    rng = []
    for a in range(3):
        lo, hi = float(box[2 * a]), float(box[2 * a + 1])
        if not lo <= hi:
            return None
        rng.append((cell_coord(lo - grow, c) >> 2, cell_coord(hi + grow, c) >> 2))
    n = 1
    for lo, hi in rng:
        n *= hi - lo + 1
    if n > 64:
        return None
    seen = []
    for z in range(rng[2][0], rng[2][1] + 1):
        for y in range(rng[1][0], rng[1][1] + 1):
            for x in range(rng[0][0], rng[0][1] + 1):
                h = block_hash(x, y, z, buckets - 1)
                if h not in seen:
                    seen.append(h)
    return seen, n


def image(boxes, levels, buckets=BUCKETS, cell=CELL):
    """dict: start uint32 [levels * (buckets + 1)], entries / large uint32, entry_boxes / large_boxes float64 [.., 6],
    n_entries, n_large, large_start [levels + 1], bounds [6]; plus what the tests assert about the box set per level:
    self_collisions (registered statics with two blocks in one bucket), shared (buckets holding several statics),
    level_large (large statics per level)."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 6)
    start, entries, large, large_start = [], [], [], [0]
    lo, hi = [math.inf] * 3, [-math.inf] * 3
    self_collisions, shared, level_large = [], [], []
    for l in range(levels):
        c = cell * 2.0 ** l
        per = [[] for _ in range(buckets)]
        n_self = n_large = 0
        for s, box in enumerate(boxes):
            got = static_buckets(box, c, buckets)
            if got is None:
                large.append(s)
                n_large += 1
                continue
            n_self += len(got[0]) < got[1]
            for h in got[0]:
                per[h].append(s)
            for a in range(3):
                lo[a], hi[a] = min(lo[a], float(box[2 * a])), max(hi[a], float(box[2 * a + 1]))
        for b in range(buckets):
            start.append(len(entries))
            entries += per[b]
        start.append(len(entries))
        large_start.append(len(large))
        self_collisions.append(n_self)
        shared.append(sum(len(p) > 1 for p in per))
        level_large.append(n_large)
    entries, large = np.array(entries, np.uint32), np.array(large, np.uint32)
    return dict(start=np.array(start, np.uint32), entries=entries, large=large,
                entry_boxes=boxes[entries.astype(np.int64)].reshape(-1, 6), large_boxes=boxes[large.astype(np.int64)].reshape(-1, 6),
                n_entries=len(entries), n_large=len(large), large_start=np.array(large_start, np.uint32),
                bounds=np.array(lo + hi, np.float64), self_collisions=self_collisions, shared=shared, level_large=level_large)


def _box(lo, size):
    lo, size = np.asarray(lo, np.float64), np.broadcast_to(np.asarray(size, np.float64), (3,))
    return [lo[0], lo[0] + size[0], lo[1], lo[1] + size[1], lo[2], lo[2] + size[2]]


def boxes(seed):
    """About 300 statics for cell 1.0 and 1024 buckets (see the module's tests for what they must exercise)."""
    r = np.random.default_rng(seed)
    out = []
    for _ in range(200):                                         # small, anywhere in +-2000: their block hashes collide
        out.append(_box(r.uniform(-2000.0, 2000.0, 3), r.uniform(0.2, 3.0, 3)))
    for k in range(20):                                          # exactly on cell and block boundaries
        o = r.integers(-300, 300, 3) * (4 if k % 2 else 1)
        out.append(_box(o, [1.0, 4.0, 8.0][k % 3]))
    for k in range(12):                                          # 4 x 4 x 4 = 64 blocks: registered
        o = 4.0 * r.integers(-200, 200, 3)
        out.append(_box(o + 0.6, 11.8))
    for k in range(6):                                           # 5 x 13 x 1 = 65 blocks: large
        o = 4.0 * r.integers(-200, 200, 3)
        out.append(_box(o + 0.6, [15.8, 47.8, 2.8]))
    for k in range(10):                                          # registered on the coarse levels only
        out.append(_box(r.uniform(-1500.0, 1500.0, 3), r.uniform(20.0, 400.0, 3)))
    out.append([-5.0e8, 5.0e8, -1.0, 1.0, -3.0, -2.0])          # an edge of 1e9: the block product overflows
    out.append([-5.0e8, 5.0e8, -5.0e8, 5.0e8, -5.0e8, 5.0e8])
    out.append([3.0, 2.0, -7.0, -6.0, 10.0, 11.0])              # inverted
    out.append([-12.0, -11.0, math.nan, 4.0, 0.0, 1.0])         # NaN
    out.append([-math.inf, math.inf, 5.0, 6.0, -9.0, -8.0])     # +-inf
    out.append([100.0, math.inf, -50.0, -49.0, 7.0, 8.0])
    dup = [out[3], out[3], out[3], out[205], out[205], out[225], out[225]]            # coincident duplicates
    out += dup
    out += [_box(r.uniform(-2000.0, 0.0, 3), r.uniform(0.2, 3.0, 3)) for _ in range(300 - len(out))]
    a = np.array(out, np.float64)
    return a[r.permutation(len(a))]


def boxes_moved(a, seed):
    """B: A with a third translated by up to +-40 cells, a few resized across the 64-block line, one turned NaN."""
    r = np.random.default_rng(seed)
    b = np.array(a, np.float64)
    n = len(b)
    for s in r.choice(n, n // 3, replace=False):
        d = r.uniform(-40.0, 40.0, 3)
        b[s, 0:2] += d[0]
        b[s, 2:4] += d[1]
        b[s, 4:6] += d[2]
    finite = [s for s in range(n) if np.all(np.isfinite(b[s])) and np.all(b[s, 1::2] - b[s, 0::2] < 5.0) and
              np.all(b[s, 1::2] >= b[s, 0::2])]
    for k, s in enumerate(r.choice(finite, 8, replace=False)):
        o = 4.0 * np.floor(b[s, 0::2] / 4.0)
        b[s] = _box(o + 0.6, 11.8 if k % 2 else [15.8, 47.8, 2.8])               # to 64 blocks (registered) / 65 (large)
    s = int(r.choice(finite))
    b[s, 4] = math.nan
    return b


def boxes_many(seed, n=300):
    """n statics of 64 blocks each on level 0: several times the registrations of boxes()"""
    r = np.random.default_rng(seed)
    return np.array([_box(4.0 * r.integers(-400, 400, 3) + 0.6, 11.8) for _ in range(n)], np.float64)


def boxes_all_large(n=70):
    """large on every level of a 16-level object of cell 1.0: inverted, NaN, or wider than 64 blocks of the top level"""
    out = []
    for k in range(n):
        out.append([[1.0 + k, 0.0 + k, 0.0, 1.0, 0.0, 1.0], [0.0, 1.0, math.nan, 1.0, -float(k), 1.0],
                    [-5.0e8, 5.0e8, -5.0e8, 5.0e8, float(k), k + 1.0]][k % 3])
    return np.array(out, np.float64)


def boxes_none_large(seed, n=70):
    r = np.random.default_rng(seed)
    return np.array([_box(r.uniform(-500.0, 500.0, 3), r.uniform(0.1, 2.0, 3)) for _ in range(n)], np.float64)
