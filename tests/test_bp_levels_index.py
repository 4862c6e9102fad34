"""CPU: the leveled index of a multi-level broadphase object (clapgpu_bp_leveled_index): its entry point is bound, and the
lookup rule of clap_amd/csrc/grid_query_dev.h restated in numpy over tests/bplevelref.py -- every box that meets a query
box has its (level, centre cell) inside the cells the query looks up on that level."""
import numpy as np

import bplevelref as ref
from clap_amd import _lib

CELL0, LEVELS = 0.25, 6                                     # a power of two: every level's cell is exact


def test_entry_point_is_bound():
    assert _lib.ABI_VERSION >= 44
    assert "clapgpu_bp_leveled_index" in _lib.SYMBOLS


def query_cells(lo, hi, c, grow=0.5 * (1.0 + 1e-9)):
    """grid_range: per axis the cells [first, last] of size c that a query extent [lo, hi] looks up (c a power of two
    times CELL0, so c * 0.5 * (1 + 1e-9) on the device and grow * c here are the same double)"""
    return ref.cell_coord(lo - grow * c, c), ref.cell_coord(hi + grow * c, c)


def reached(boxes, queries, grow=0.5 * (1.0 + 1e-9)):
    """(meets [nb, nq], reached [nb, nq]): box b meets query q; b's centre cell on its level is among q's cells there"""
    level, over = ref.box_level(boxes, CELL0, LEVELS)
    assert not over.any()
    c = CELL0 * 2.0 ** level
    cc = ref.centre_cell(boxes, c)
    ok = np.ones((len(boxes), len(queries)), bool)
    for a in range(3):
        first, last = query_cells(queries[None, :, 2 * a], queries[None, :, 2 * a + 1], c[:, None], grow)
        ok &= (first <= cc[:, a, None]) & (cc[:, a, None] <= last)
    return ref.overlap_matrix(boxes, queries), ok


def inputs():
    R = np.random.Generator(np.random.PCG64(21))
    nb = nq = 2000
    edge = np.exp(R.uniform(np.log(0.05), np.log(8.0), (nb, 3)))
    lo = R.uniform(0.0, 12.0, (nb, 3))
    k = np.arange(nb) % LEVELS
    exact = np.arange(nb) < 300                             # edges of exactly cell * 2^l, corners on multiples of 2^-10
    edge[exact] = (CELL0 * 2.0 ** k[exact])[:, None]
    lo[exact] = np.round(lo[exact] * 1024.0) / 1024.0
    on_edge = (np.arange(nb) >= 300) & (np.arange(nb) < 600)                # centres exactly on cell boundaries of their level
    edge[on_edge] = (CELL0 * 2.0 ** k[on_edge] * 0.75)[:, None]
    centre = np.round(lo[on_edge] / (CELL0 * 2.0 ** k[on_edge])[:, None]) * (CELL0 * 2.0 ** k[on_edge])[:, None]
    lo[on_edge] = centre - edge[on_edge] * 0.5              # 0.375 of a power of two: exact
    boxes = np.stack([lo, lo + edge], 2).reshape(nb, 6)
    qlo = R.uniform(0.0, 12.0, (nq, 3))
    qext = np.exp(R.uniform(np.log(0.01), np.log(6.0), (nq, 3)))
    queries = np.stack([qlo, qlo + qext], 2).reshape(nq, 6)
    corner = np.arange(nq) < 400                            # queries that touch a box in one point: its maximum corner
    queries[corner, 0::2] = boxes[:400, 1::2]
    queries[corner, 1::2] = boxes[:400, 1::2] + qext[corner]
    point = (np.arange(nq) >= 400) & (np.arange(nq) < 800)  # zero extent: a box's minimum corner, a point inside, a centre
    p = np.where((np.arange(400) % 3 == 0)[:, None], boxes[400:800, 0::2],
                 np.where((np.arange(400) % 3 == 1)[:, None], boxes[400:800, 0::2] + 0.3 * edge[400:800],
                          (boxes[400:800, 0::2] + boxes[400:800, 1::2]) * 0.5))
    queries[point, 0::2] = p
    queries[point, 1::2] = p
    return boxes, queries


def test_the_cells_of_a_query_hold_every_box_that_meets_it():
    boxes, queries = inputs()
    level, _ = ref.box_level(boxes, CELL0, LEVELS)
    c = CELL0 * 2.0 ** level
    edge = boxes[:, 1::2] - boxes[:, 0::2]
    # the inputs hold what they are meant to hold
    assert len(set(level[(edge == c[:, None]).all(1)])) == LEVELS, "edges of exactly the cell, on every level"
    centre = (boxes[:, 0::2] + boxes[:, 1::2]) * 0.5
    assert ((centre / c[:, None] == np.round(centre / c[:, None])).all(1)).sum() >= 250, "centres on cell boundaries"
    assert (queries[:, 0::2] == queries[:, 1::2]).all(1).sum() == 400, "degenerate queries"
    meets, ok = reached(boxes, queries)
    one_point = (queries[:400, 0::2] == boxes[:400, 1::2]).all(1)
    assert one_point.all() and meets[np.arange(400), np.arange(400)].all(), "queries that touch a box in one point"
    assert meets[np.arange(400, 800), np.arange(400, 800)].all(), "degenerate queries on and in boxes"
    assert meets.sum() > 20_000 and np.all(np.bincount(level[np.nonzero(meets)[0]], minlength=LEVELS) > 200)
    assert ok[meets].all(), np.argwhere(meets & ~ok)[:8]
    # ... and the test can tell: without the half cell the rule misses boxes
    _, bare = reached(boxes, queries, grow=0.0)
    assert not bare[meets].all()
