"""The multi-level broadphase grid's rule in numpy (clap_amd/csrc/bp_levels.h), and the brute-force ground truth its
tests compare against.  Imports neither the library nor the oracle.

Boxes are float64 [n, 6] rows (minx, maxx, miny, maxy, minz, maxz); overlap is inclusive, as the device's boxes_overlap.
"""
import numpy as np


# ---------------------------------------------------------------------------------------------- ground truth
def overlap_matrix(a, b):
    """[len(a), len(b)] bool: box a[i] meets box b[j] (touching counts; the negated form lets NaN overlap, as on the device)."""
    m = np.ones((len(a), len(b)), bool)
    for x in range(3):
        m &= ~((a[:, None, 2 * x] > b[None, :, 2 * x + 1]) | (a[:, None, 2 * x + 1] < b[None, :, 2 * x]))
    return m


def brute_pairs(aabb):
    """Every overlapping (i, j), i < j, ascending: int64 [m, 2]."""
    m = np.triu(overlap_matrix(aabb, aabb), 1)
    return np.argwhere(m).astype(np.int64).reshape(-1, 2)


def brute_static_pairs(aabb, statics):
    """Every overlapping (body, static), ascending: int64 [m, 2]."""
    if statics is None or len(statics) == 0:
        return np.zeros((0, 2), np.int64)
    return np.argwhere(overlap_matrix(aabb, statics)).astype(np.int64).reshape(-1, 2)


def sphere_aabb(bodies):
    pos, r = np.asarray(bodies["pos"], np.float64), np.asarray(bodies["radius"], np.float64)[:, None]
    out = np.empty((len(pos), 6))
    out[:, 0::2], out[:, 1::2] = pos - r, pos + r
    return out


# ---------------------------------------------------------------------------------------------- the rule
def box_level(aabb, cell0, levels):
    """(level [n], over [n]): the lowest level whose cell cell0 * 2^l is not smaller than the largest edge, compared
    level by level; an edge equal to the cell fits, a NaN edge fits level 0; over: above the top level's cell."""
    edge = np.stack([aabb[:, 1] - aabb[:, 0], aabb[:, 3] - aabb[:, 2], aabb[:, 5] - aabb[:, 4]], 1)
    level = np.zeros(len(aabb), np.int64)
    c = float(cell0)
    for l in range(levels - 1):
        level += ((edge > c).any(1) & (level == l))
        c *= 2.0
    return level, (edge > c).any(1) & (level == levels - 1)


def cell_coord(x, cell):
    with np.errstate(invalid="ignore"):
        c = np.floor(np.asarray(x, np.float64) / cell)
    c = np.where(c > -5.0e8, c, -5.0e8)                     # also NaN
    return np.minimum(c, 5.0e8).astype(np.int64)


def centre_cell(aabb, cell):
    """[n, 3]: the cell of each box centre for per-box cell sizes `cell` [n]."""
    return np.stack([cell_coord((aabb[:, 2 * a] + aabb[:, 2 * a + 1]) * 0.5, cell) for a in range(3)], 1)


def owner(i, j, level):
    """The member of pair (i, j) whose search finds it, as far as the levels decide: the finer one; -1 for a same-level
    pair, which today's cell rule assigns (own cell: the smaller index; else the body whose cell comes first)."""
    return np.where(level[i] < level[j], i, np.where(level[j] < level[i], j, -1))


def coarse_lookup(lo, hi, cell_l, grow=0.5, inclusive=True):
    """Per axis, the cells [first, last] a finer body with extent [lo, hi] looks up on a level of cell size cell_l: the
    cells met by the extent grown by `grow` cells, both ends inclusive.  (The two mutants of the tests: grow = 0, and
    inclusive = False for an upper bound that leaves its cell out.)"""
    first, last = cell_coord(lo - grow * cell_l, cell_l), cell_coord(hi + grow * cell_l, cell_l)
    return first, last if inclusive else last - 1


def rule_reaches(aabb, pairs, cell0, levels, grow=0.5, inclusive=True):
    """bool [m]: does the rule look at the partner of each (overlapping) pair?  Same level: the partner's cell is among
    the 27 around the owner's (the own cell and the 13 after it, seen from the member whose cell comes first).  Different
    levels: the coarser member's centre cell is among the cells the finer one looks up on that level."""
    level, _ = box_level(aabb, cell0, levels)
    cell = cell0 * 2.0 ** level
    i, j = pairs[:, 0], pairs[:, 1]
    fine = np.where(level[i] <= level[j], i, j)
    coarse = np.where(level[i] <= level[j], j, i)
    same = level[i] == level[j]
    cc = centre_cell(aabb[coarse], cell[coarse])
    fc = centre_cell(aabb[fine], cell[fine])
    ok = np.ones(len(pairs), bool)
    for a in range(3):
        first, last = coarse_lookup(aabb[fine, 2 * a], aabb[fine, 2 * a + 1], cell[coarse], grow, inclusive)
        ok &= np.where(same, np.abs(cc[:, a] - fc[:, a]) <= 1, (first <= cc[:, a]) & (cc[:, a] <= last))
    return ok
