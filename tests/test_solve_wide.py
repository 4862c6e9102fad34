"""CPU: the level schedule of clapgpu_bodies_solve's wide path (include/clapgpu.h, tests/solvelevelref.py) is exact --
executing solveref's rows level after level, the rows inside a level in reversed order, gives the bits of the sequential
sweep -- and the interface is there.  Nothing here touches the device (tests/test_solve_wide_gpu.py does)."""
import ctypes as C
import os

import numpy as np
import pytest

import geomref as gr
import solvelevelref as lr
import solveref as sr
from clap_amd import _lib
from test_solve import H, state


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_abi_and_symbol():
    assert _lib.ABI_VERSION >= 40
    assert "clapgpu_bodies_solve" in _lib.SYMBOLS and "wide_rows" in [f[0] for f in _lib.Solver._fields_]


def test_symbol_is_bound(built_lib):
    assert built_lib.clapgpu_bodies_solve.argtypes == _lib.SYMBOLS["clapgpu_bodies_solve"][1]


def test_solver_layout():
    assert _lib.Solver.wide_rows.offset == 4 and _lib.Solver.wide_rows.size == 4
    assert _lib.Solver.iterations.offset == 0 and _lib.Solver.sor_w.offset == 8 and _lib.Solver.cfm.offset == 16
    assert C.sizeof(_lib.Solver) == 24
    assert not hasattr(_lib.Solver, "pad")


def test_scratch_bytes_do_not_shrink_with_the_rows(built_lib):
    """Row counts small enough that the sort sizes its work space without asking a device (tests/test_solve_wide_gpu.py
    asks for the large ones).  The wide path's part: 28 bytes a row and 4 a body"""
    n = 1000
    sizes = [built_lib.clapgpu_bodies_solve_scratch_bytes(n, r) for r in (0, 1, 31, 32, 33, 1000, 1001)]
    print(sizes)
    assert all(sizes) and sizes == sorted(sizes)
    assert sizes[5] >= 1000 * (240 + 8 + 8 + 8 + 28) + n * (48 + 4 + 4)


def spheres_scene(pos, lvel, pairs, order):
    """overlapping spheres with friction, their contacts (from geomref) listed in `order`: solveref.solve's arguments"""
    st = state(pos, lvel=lvel, inertia=np.full((len(pos), 3), 0.1))
    pairs = np.asarray(pairs, np.uint32)
    recs = []
    for i, j in pairs:
        c = gr.sphere_sphere(st["pos"][i:i + 1], st["radius"][i:i + 1], st["pos"][j:j + 1], st["radius"][j:j + 1])
        assert c["nc"][0] == 1
        recs.append(sr.record(np.asarray(c["pos"][0], float), np.asarray(c["normal"][0], float), float(c["depth"][0]), mu=0.5))
    return st, np.zeros(len(pos), np.uint32), dict(body=(pairs[order], sr.records([recs[k] for k in order])))


def chain_scene(order):
    """tests/test_solve.py's chain(): three overlapping spheres in a row, their two contacts listed in `order`"""
    return spheres_scene([[0.0, 0, 0], [0.83, 0.1, 0], [1.61, 0.35, 0.2]], [[0.3, 0, 0], [0, 0.1, 0], [-0.7, 0.2, 0.1]],
                         [[0, 1], [1, 2]], order)


def ladder_scene():
    """six spheres in a row, the odd contacts listed before the even ones: levels three rows wide"""
    pos = [[0.8 * k, 0.05 * (k % 3), 0.03 * k] for k in range(6)]
    lvel = [[0.3 - 0.1 * k, 0.02 * k, 0.1 * (k % 2)] for k in range(6)]
    return spheres_scene(pos, lvel, [[0, 1], [2, 3], [4, 5], [1, 2], [3, 4]], [0, 1, 2, 3, 4])


def check_schedule(st, island, lists, widths):
    want = sr.solve(st, island, H, **lists)
    got = lr.solve_by_levels(st, island, H, **lists)                        # reversed inside every level
    assert got["lvel"].tobytes() == want["lvel"].tobytes() and got["avel"].tobytes() == want["avel"].tobytes()
    assert got["row_lambda"].tobytes() == want["row_lambda"].tobytes()
    assert got["row_key"].tobytes() == want["row_key"].tobytes()
    assert (want["lvel"] != st["lvel"]).any() and (want["row_lambda"] != 0).any()
    bodies, _key = lr.row_bodies(st, island, **lists)
    for levels in got["schedule"].values():
        assert [len(level) for level in levels] == widths
        for level in levels:
            named = [b for k in level for b in bodies[k] if b is not None]
            assert len(named) == len(set(named)), "two rows of a level share a body"
    return got


def test_the_chain_level_by_level_is_the_sequential_sweep():
    """every row of the chain names body 1: six levels of one row, in either list order"""
    for order in ([0, 1], [1, 0]):
        got = check_schedule(*chain_scene(order), widths=[1] * 6)
        assert got["row_level"].tolist() == [1, 2, 3, 4, 5, 6]


def test_levels_wider_than_a_row_reversed_inside_are_the_sequential_sweep():
    got = check_schedule(*ladder_scene(), widths=[3, 3, 3, 2, 2, 2])
    assert got["row_level"].tolist() == [1, 2, 3] * 3 + [4, 5, 6] * 2
    # and the order inside a level is free where the order of the lists is not: another list order, other bits
    st, island, lists = ladder_scene()
    pairs, recs = lists["body"]
    swapped = dict(body=(pairs[[3, 4, 0, 1, 2]], recs[[3, 4, 0, 1, 2]]))
    other = sr.solve(st, island, H, **swapped)
    assert other["lvel"].tobytes() != got["lvel"].tobytes()


def test_the_rule_on_lists_alone():
    """an absent body 2 is no dependency, islands do not see each other, a row that names a body of an earlier row waits"""
    key = np.array([(0 << 32) | 0, (5 << 32) | 1, (0 << 32) | 2, (0 << 32) | 3, (5 << 32) | 4, (0 << 32) | 5], np.uint64)
    bodies = [(0, None), (5, None), (1, None), (0, 1), (5, 6), (1, 2)]
    assert lr.levels(key, bodies).tolist() == [1, 1, 1, 2, 2, 3]
    lv, wide = lr.expected_levels(key, bodies, 0)
    assert not lv.any() and wide == 0
    lv, wide = lr.expected_levels(key, bodies, 3)
    assert lv.tolist() == [1, 0, 1, 2, 0, 3] and wide == 1
    lv, wide = lr.expected_levels(key, bodies, 1)
    assert lv.tolist() == [1, 1, 1, 2, 2, 3] and wide == 2
