"""CPU: the order of a crowd restated (tests/orderref.py) on hand cases -- a line, the line reversed, two clusters, the
special cases, a mutant of the level rule; the binding's symbols; clapgpu_characters_order and
clapgpu_characters_move_ordered refuse bad arguments before any HIP call.  (The device side: test_order_gpu.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

from clap_amd import _lib
import orderref as orf

DT = 1.0 / 60.0
G = np.float32(-9.8)


def spheres(x, r=0.5):
    """bodies of radius r at (x, 0, 0): (aabb, pos, yoffset)"""
    pos = np.stack([np.asarray(x, float), np.zeros(len(x)), np.zeros(len(x))], 1)
    aabb = np.stack([pos[:, 0] - r, pos[:, 0] + r, pos[:, 1] - r, pos[:, 1] + r, pos[:, 2] - r, pos[:, 2] + r], 1)
    return aabb, pos, np.full(len(x), r)


def still(body, world, dt=DT, **over):
    """movers that stand still on `world` (their reach is their box grown by the pad and the ray), but for `over`"""
    aabb, pos, yo = world
    n = len(body)
    a = dict(body=np.asarray(body), ray_off=np.full(n, 0.4), motion=np.zeros((n, 2), np.float32),
             velocity=np.zeros((n, 3), np.float32))
    a.update(over)
    return a, orf.reach_boxes(a["body"], a["ray_off"], a["motion"], a["velocity"], aabb, pos, yo, G, dt)


LINE = spheres(np.arange(5) * 0.9)          # each box meets the next one only (0.9 < 1 < 1.8)


def test_a_line_is_one_level_per_mover_and_so_is_the_line_reversed():
    a, reach = still(np.arange(5), LINE)
    level, n_levels, pairs = orf.levels(a["body"], reach, 5)
    assert level.tolist() == [0, 1, 2, 3, 4] and n_levels == 5 and pairs == 4
    a, reach = still(np.arange(5)[::-1], LINE)
    level, n_levels, pairs = orf.levels(a["body"], reach, 5)
    assert level.tolist() == [0, 1, 2, 3, 4] and n_levels == 5 and pairs == 4      # by position in the list: body 4 goes first


def test_the_list_decides_not_the_place():
    a, reach = still([0, 2, 4, 1, 3], LINE)
    level, n_levels, _ = orf.levels(a["body"], reach, 5)
    assert level.tolist() == [0, 0, 0, 1, 1] and n_levels == 2


def test_two_clusters_far_apart_level_on_their_own():
    world = spheres(np.concatenate([np.arange(3) * 0.9, 1000 + np.arange(4) * 0.9]))
    a, reach = still([0, 3, 1, 4, 2, 5, 6], world)
    level, n_levels, pairs = orf.levels(a["body"], reach, 7)
    assert level.tolist() == [0, 0, 1, 1, 2, 2, 3] and n_levels == 4 and pairs == 5


def test_the_mutant_rule_gives_other_levels_on_the_line():
    a, reach = still(np.arange(5), LINE)
    assert orf.levels(a["body"], reach, 5, earlier=False)[0].tolist() == [4, 3, 2, 1, 0]
    assert orf.levels(a["body"], reach, 5)[0].tolist() != orf.levels(a["body"], reach, 5, earlier=False)[0].tolist()


def test_reach_grows_with_the_velocity_the_motion_and_the_ray():
    world = spheres([0.0])
    a, base = still([0], world)
    ray_len = 0.5 - (0.4 - 0.05) + 1e-3
    start = float(np.float32(0.0 - 0.35))
    pad = 1e-6 + 2.0 ** -20 * (2 * ray_len - start)                              # the ray's end is the largest magnitude
    T0 = float(np.float64(np.float32(9.8))) * DT * DT                            # standing still, A is a frame of gravity
    assert abs(base[0, 1] - (0.5 + T0 + pad)) < 1e-12 and abs(base[0, 3] - (0.5 + ray_len + T0 + pad)) < 1e-12
    assert abs(base[0, 2] - (-0.5 - ray_len - T0 - pad)) < 1e-12                 # the grown box ends below the ray
    _, deep = still([0], world, ray_off=np.array([0.0]), dt=0.9e-6)              # a ray from above the centre, T = 0
    rl, st = 0.5 + 0.05 + 1e-3, float(np.float32(0.05))
    assert -0.5 - rl > st - 2 * rl and abs(deep[0, 2] - (st - 2 * rl - (1e-6 + 2.0 ** -20 * (2 * rl - st)))) < 1e-12
    _, fast = still([0], world, velocity=np.float32([[3.0, -4.0, 0.0]]))
    T = 7.0 * DT                                                                 # on top of the frame of gravity
    assert abs(fast[0, 1] - base[0, 1] - T) < 1e-6 and abs(fast[0, 5] - base[0, 5] - T) < 1e-6
    assert abs(fast[0, 3] - base[0, 3] - T) < 1e-6
    _, walk = still([0], world, motion=np.float32([[2.0, -1.0]]))
    assert abs(walk[0, 1] - (base[0, 1] - T0) - 9.0 * DT) < 1e-6                 # B = 3 * (|dx| + |dz|) above A = |g| dt
    # dt: nothing slides below 1e-6, and 1 / 30 at the most
    assert np.array_equal(still([0], world, velocity=np.float32([[3.0, 0.0, 0.0]]), dt=0.9e-6)[1], still([0], world, dt=0.9e-6)[1])
    _, long = still([0], world, velocity=np.float32([[3.0, 0.0, 0.0]]), dt=1.0)
    assert abs(long[0, 1] - 0.5 - (3.0 + 9.8) / 30.0) < 1e-5
    # a branch that is not finite counts as 0: the velocity is NaN, the walking bound stays
    _, nanv = still([0], world, velocity=np.float32([[np.nan, 0.0, 0.0]]), motion=np.float32([[2.0, -1.0]]))
    assert np.array_equal(nanv, walk)
    _, nanv = still([0], world, velocity=np.float32([[np.nan, np.inf, 0.0]]))
    assert np.isfinite(nanv).all() and abs(nanv[0, 1] - 0.5) < 1e-5              # A is not finite either way: T = 0
    # a ray that is not cast has no length
    _, noray = still([0], world, ray_off=np.array([np.nan]))
    assert np.isfinite(noray).all() and abs(noray[0, 3] - 0.5 - T0) < 1e-5 and abs(noray[0, 2] + 0.5 + T0) < 1e-5
    _, noray = still([0], world, ray_off=np.array([5.0]))                          # a negative ray_len
    assert abs(noray[0, 3] - 0.5 - T0) < 1e-5


def test_a_body_listed_twice_is_level_0_and_conflicts_with_nobody():
    a, reach = still([0, 1, 2, 1, 3, 4], LINE)
    level, n_levels, pairs = orf.levels(a["body"], reach, 5)
    assert orf.classes(a["body"], reach, 5).tolist() == [0, 1, 0, 1, 0, 0]
    assert level.tolist() == [0, 0, 0, 0, 1, 2] and n_levels == 3                 # the line is cut at body 1
    assert pairs == 4 + 1 + 2                                                     # the pair search still sees both listings
    a, reach = still([0, 7, 1], LINE)                                             # no body of the set
    assert np.isnan(reach[1]).all() and orf.levels(a["body"], reach, 5)[0].tolist() == [0, 0, 1]


def test_a_box_that_is_not_finite_stands_alone():
    world = spheres(np.concatenate([np.arange(3) * 0.9, [1000.0, 2000.0]]))
    a, reach = still([0, 3, 1, 4, 2], world, ray_off=np.array([0.4, -np.inf, 0.4, 0.4, 0.4]))
    assert not np.isfinite(reach[1]).all() and np.isfinite(reach[[0, 2, 3, 4]]).all()
    assert orf.classes(a["body"], reach, 5).tolist() == [0, 2, 0, 0, 0]
    level, n_levels, pairs = orf.levels(a["body"], reach, 5)
    assert level.tolist() == [0, 1, 2, 2, 3] and n_levels == 4 and pairs == 2      # far body 4 waits for it too
    world[0][3, 0] = np.nan                                                        # a NaN box row
    a, reach = still([3, 0], world)
    assert orf.levels(a["body"], reach, 5)[0].tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------- the binding
NAMES = ("clapgpu_characters_order", "clapgpu_characters_order_scratch_bytes", "clapgpu_characters_move_ordered",
         "clapgpu_characters_move_ordered_scratch_bytes")


def test_abi_and_symbols():
    for name in NAMES:
        assert name in _lib.SYMBOLS, name
    assert _lib.ABI_VERSION >= 43


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def fake(p):
    def bodies(**gone):
        b = _lib.Bodies(4, 1, p, p, p, p, p, p, p, p, p, p, p)
        b.facc, b.aabb = p, p
        for k in gone:
            setattr(b, k, None)
        return b

    def moves(n=2, **gone):
        m = _lib.CharactersMove(n, *([p] * 15))
        for k, v in gone.items():
            setattr(m, k, v)
        return m
    return bodies, moves


@pytest.fixture(scope="module")
def aligned():
    buf = (C.c_double * 256)()
    base = C.addressof(buf)
    p = (base + 255) & ~255                                                # 256-byte aligned, inside buf
    assert p + 512 <= base + C.sizeof(buf)
    return buf, p


def test_order_refuses_bad_arguments_before_any_hip_call(L, aligned):
    _keep, p = aligned
    bodies, moves = fake(p)
    w = _lib.World()
    bad = _lib.ERR_INVALID_ARGUMENTS
    summary = (C.c_uint32 * 4)(9, 9, 9, 9)

    def call(b=bodies(), w=w, m=moves(), obp=C.c_void_p(p), reach=p, level=p, summary=summary, scratch=p, cap=16):
        ref = lambda x: None if x is None else C.byref(x)
        return L.clapgpu_characters_order(None, obp, ref(b), ref(w), 1.0 / 60.0, ref(m), cap, reach, level, summary, scratch)
    assert call(m=None) == bad and call(b=None) == bad and call(w=None) == bad
    assert call(obp=None) == bad and call(summary=None) == bad
    for field in ("aabb", "pos", "yoffset"):
        assert call(b=bodies(**{field: 1})) == bad, field
        assert call(b=bodies(**{field: 1}), m=moves(0)) == bad, field        # also for an empty batch
    for field in ("body", "ray_off", "motion", "velocity"):
        assert call(m=moves(**{field: None})) == bad, field
    assert call(reach=None) == bad and call(level=None) == bad
    assert call(scratch=None) == bad and call(scratch=p + 64) == bad
    assert call(m=moves(0)) == _lib.OK and list(summary) == [0, 0, 0, 0]
    summary[0] = 9
    assert call(m=_lib.CharactersMove(0), scratch=None, reach=None, level=None) == _lib.OK and summary[0] == 0
    assert L.clapgpu_characters_order_scratch_bytes(0, 100) == 0
    assert L.clapgpu_characters_order_scratch_bytes(10, 100) % 256 == 0 < L.clapgpu_characters_order_scratch_bytes(10, 0)


def test_move_ordered_refuses_bad_arguments_before_any_hip_call(L, aligned):
    _keep, p = aligned
    bodies, moves = fake(p)
    w, sg, e = _lib.World(), _lib.Geoms(), _lib.Entities()
    e.rot = e.flags = p
    bad = _lib.ERR_INVALID_ARGUMENTS
    n_levels = C.c_uint32(7)

    def call(b=bodies(), w=w, sg=sg, e=None, m=moves(), scratch=p, bp=None, obp=C.c_void_p(p), nl=n_levels, level=None):
        ref = lambda x: None if x is None else C.byref(x)
        return L.clapgpu_characters_move_ordered(None, bp, obp, ref(b), ref(w), ref(sg), None, ref(e), 1.0 / 60.0, ref(m), 16,
                                                 level, ref(nl), scratch)
    assert call(m=None) == bad and call(b=None) == bad and call(w=None) == bad and call(sg=None) == bad
    for field in ("pos", "quat", "lvel", "radius", "yoffset", "facc", "mass", "bflags", "adis_steps_left", "adis_time_left", "aabb"):
        assert call(b=bodies(**{field: 1})) == bad, field
        assert call(b=bodies(**{field: 1}), m=moves(0)) == bad, field        # also for an empty batch
    for field in [f[0] for f in _lib.CharactersMove._fields_[1:16]]:
        assert call(m=moves(**{field: None})) == bad, field
    assert call(m=moves(entity=p)) == bad and call(m=moves(yaw_quat=p)) == bad                # one of the pair
    assert call(m=moves(entity=p, yaw_quat=p)) == bad                                         # the pair without entities
    assert call(m=moves(entity=p, yaw_quat=p), e=_lib.Entities()) == bad                      # ... without rot / flags
    assert call(m=moves(entity=p, yaw_quat=p + 4), e=e) == bad                                # a quat array off 16 bytes
    assert call(scratch=None) == bad and call(scratch=p + 64) == bad
    assert call(obp=None) == bad and call(obp=None, m=moves(0)) == bad and call(nl=None) == bad
    assert n_levels.value == 7                                                                # a refusal writes nothing
    assert call(m=moves(0)) == _lib.OK and n_levels.value == 0
    n_levels.value = 7
    assert call(m=_lib.CharactersMove(0), scratch=None) == _lib.OK and n_levels.value == 0    # n == 0: nothing else is asked
    assert L.clapgpu_characters_move_ordered_scratch_bytes(100, 0, 64) == 0
    assert L.clapgpu_characters_move_ordered_scratch_bytes(100, (1 << 28) + 1, 64) == 0
