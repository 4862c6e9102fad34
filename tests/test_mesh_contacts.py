"""CPU: the truth of tests/meshcontactref.py on hand-computed cases of the sphere / capsule against triangle rule
(include/clapgpu.h), the MAX_CONTACTS selection and the sweep restatement."""
import numpy as np
import pytest

import meshcontactref as mc

# the unit right triangle in the y = 0 plane, front face up: (v1 - v0) x (v2 - v0) = (0, 1, 0) * 1
TRI = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])


def one(a, b, r, tri=TRI):
    cs, margin, rule = mc.collide(a, b, r, tri)
    return [(np.asarray(p, float), np.asarray(n, float), float(d)) for p, n, d in cs], margin, rule


def test_face_sphere_above_the_interior():
    cs, margin, rule = one([0.25, 0.3, 0.25], [0.25, 0.3, 0.25], 0.5)
    assert rule == 5 and not margin and len(cs) == 1                     # a sphere above the face: the closest point
    p, n, d = cs[0]
    assert np.allclose(n, [0, 1, 0]) and d == pytest.approx(0.2) and np.allclose(p, [0.25, 0, 0.25])


def test_half_sunk_sphere_is_a_face_contact():
    cs, _m, rule = one([0.25, -0.1, 0.25], [0.25, -0.1, 0.25], 0.5)
    assert rule == 3 and len(cs) == 1
    p, n, d = cs[0]
    assert np.allclose(n, [0, 1, 0]) and d == pytest.approx(0.6) and np.allclose(p, [0.25, 0, 0.25])


def test_edge_and_vertex_regions():
    # beyond the hypotenuse x + z = 1, above the plane: the normal points from the edge's closest point
    c = np.array([0.8, 0.2, 0.8])
    cs, _m, rule = one(c, c, 0.5)
    assert rule == 5 and len(cs) == 1
    q = np.array([0.5, 0.0, 0.5])
    p, n, d = cs[0]
    assert np.allclose(p, q) and np.allclose(n, (c - q) / np.linalg.norm(c - q))
    assert d == pytest.approx(0.5 - np.linalg.norm(c - q))
    # beyond vertex v0 = origin
    c = np.array([-0.2, 0.1, -0.2])
    cs, _m, _r = one(c, c, 0.5)
    p, n, d = cs[0]
    assert np.allclose(p, 0) and d == pytest.approx(0.5 - 0.3)


def test_behind_the_face_and_degenerate_are_none():
    assert one([0.25, -0.7, 0.25], [0.25, -0.7, 0.25], 0.5)[0] == []      # m <= -r, not crossing
    assert one([0.8, -0.2, 0.8], [0.8, -0.2, 0.8], 0.5)[0] == []          # behind, outside: a neighbour's contact
    flat = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])
    assert one([0.5, 0.1, 0], [0.5, 0.1, 0], 1.0, flat)[0] == []


def test_depth_zero_is_a_contact():
    cs, _m, _r = one([0.25, 0.5, 0.25], [0.25, 0.5, 0.25], 0.5)
    assert len(cs) == 1 and cs[0][2] == 0.0


def test_capsule_through_the_face():
    cs, _m, rule = one([0.25, 0.6, 0.25], [0.3, -0.4, 0.2], 0.1)
    assert rule == 3 and len(cs) == 1
    p, n, d = cs[0]
    assert np.allclose(n, [0, 1, 0]) and d == pytest.approx(0.5) and np.allclose(p, [0.3, 0, 0.2])


def test_parallel_pair_takes_the_second_slot():
    cs, _m, rule = one([0.1, 0.2, 0.1], [0.5, 0.2, 0.1], 0.25)
    assert rule == 4 and len(cs) == 2
    assert np.allclose(cs[0][0], [0.1, 0, 0.1]) and np.allclose(cs[1][0], [0.5, 0, 0.1])
    assert cs[0][2] == pytest.approx(0.05) and cs[1][2] == pytest.approx(0.05)


def test_sphere_is_a_length_zero_capsule():
    a = np.array([0.3, 0.2, 0.3])
    assert mc.segment_of(a, [0, 0, 1], 0.0)[0].tolist() == a.tolist()
    cs, _m, rule = one(a, a, 0.25)
    assert rule == 5 and len(cs) == 1                                      # never the parallel case


def test_cap_keeps_the_deepest_while_they_fit():
    # 40 small triangles under a big sphere: 16 records kept, deepest first, written in triangle order
    tris = []
    for i in range(40):
        x = 0.05 * i
        tris.append([[x, -0.01 * i, 0.0], [x, -0.01 * i, 0.04], [x + 0.04, -0.01 * i, 0.0]])
    tris = np.array(tris)
    p = mc.Pair([1.0, 0.3, 0.0], [1.0, 0.3, 0.0], 2.0, tris)
    assert len(p.records) == 40 and p.capped and len(p.kept) == 16
    depths = {t: max(c[2] for c in cs) for t, cs, _m in p.records}
    best = sorted(depths, key=lambda t: (-depths[t], t))[:16]
    assert [t for t, _c, _m in p.kept] == sorted(best)


def test_sweep_restatement_stops_on_the_floor():
    big = np.array([[[-10.0, 0, -10], [-10.0, 0, 10], [10.0, 0, -10]], [[10.0, 0, -10], [-10.0, 0, 10], [10.0, 0, 10]]])
    frac, n, hit = mc.sweep([0.0, 1.0, 0.0], 0.25, 0.0, [0, 0, 1], [0.0, -2.0, 0.0], big)
    assert hit and np.allclose(n, [0, 1, 0]) and 0.3 < frac < 0.4           # 0.75 of 2.0 down to touch, minus the backup
