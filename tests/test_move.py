"""CPU: the restatement of character_move's decision (tests/moveref.py) on a table of hand cases, one per branch; its
character states against the binding's; clapgpu_characters_move refuses bad arguments before any HIP call.  (The device
side: test_move_gpu.py; the binding's descriptors against the header: test_cabi.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from clap_amd import _lib
import moveref as mr

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = f32(-9.8)
DT = 1.0 / 60.0
UP = [0.0, 1.0, 0.0]


def one(ray_flags=0, grounded_out=True, state=mr.CS_IDLE, jump=False, motion=(0.0, 0.0), jump_params=(2.0, 5.0),
        velocity=(0.0, 0.0, 0.0), normal=UP, airborne=0, dt=DT):
    v, a, r, ap = mr.character_move_decide_one(ray_flags, grounded_out, state, jump, motion, jump_params, velocity, normal,
                                               airborne, G, dt)
    return np.asarray(v, f32), a, r, ap


def bits(a):
    return np.asarray(a, f32).tobytes()


def fall(v1, dt):
    return f32(f64(f32(v1)) + f64(G) * f64(dt))


def test_abi_and_symbols():
    assert "clapgpu_characters_move" in _lib.SYMBOLS and "clapgpu_characters_move_scratch_bytes" in _lib.SYMBOLS
    assert _lib.ABI_VERSION >= 39


def test_airborne_gets_gravity_and_asks_for_falling():
    v, a, r, ap = one(grounded_out=False, state=mr.CS_FALLING, velocity=(1.5, -2.0, 0.25))
    assert bits(v) == bits([1.5, fall(-2.0, DT), 0.25]) and (a, r, ap) == (1, mr.CS_FALLING, 1)
    # the sum is made in double and rounded once: float arithmetic gives another last bit somewhere
    assert any(fall(x, DT) != f32(f32(x) + f32(G * f32(DT))) for x in np.linspace(-3, 3, 64))


def test_jump_protection_overrides_a_ray_that_found_ground():
    v, a, r, ap = one(grounded_out=True, state=mr.CS_JUMPING, velocity=(0.0, 2.0, 0.0), motion=(1.0, 0.0))
    assert (a, r, ap) == (1, mr.CS_FALLING, 1) and bits(v) == bits([0.0, fall(2.0, DT), 0.0])
    # not while coming down, and not in another state
    assert one(grounded_out=True, state=mr.CS_JUMPING, velocity=(0.0, 0.0, 0.0))[1:] == (0, mr.CS_IDLE, 0)
    assert one(grounded_out=True, state=mr.CS_JUMPING, velocity=(0.0, -1.0, 0.0))[1:] == (0, mr.CS_IDLE, 0)
    assert one(grounded_out=True, state=mr.CS_JUMP_START, velocity=(0.0, 2.0, 0.0))[1:] == (0, mr.CS_IDLE, 0)


def test_dt_at_the_threshold_applies_nothing_and_just_above_does():
    v, a, r, ap = one(grounded_out=False, velocity=(0.0, -1.0, 0.0), dt=1e-6)
    assert bits(v) == bits([0.0, -1.0, 0.0]) and (a, r, ap) == (1, mr.CS_FALLING, 0)
    above = np.nextafter(1e-6, 1.0)
    v, a, r, ap = one(grounded_out=False, velocity=(0.0, -1.0, 0.0), dt=above)
    assert bits(v) == bits([0.0, fall(-1.0, above), 0.0]) and (a, r, ap) == (1, mr.CS_FALLING, 1)
    # the grounded walker does not look at dt: the reference still rotates it
    assert one(motion=(1.0, 0.0), dt=0.0)[1:] == (0, mr.CS_MOVING, 1)


def test_walking_on_flat_ground():
    dx, dz = f32(0.7), f32(-1.3)
    for state, coef in ((mr.CS_IDLE, f32(0.3)), (mr.CS_MOVING, f32(1.0)), (mr.CS_FALLING, f32(0.3))):
        v, a, r, ap = one(state=state, motion=(dx, dz), velocity=(9.0, 9.0, 9.0))
        # (1, 0, 0) x (0, 1, 0) = (0, 0, 1) and (0, 1, 0) x (0, 0, 1) = (1, 0, 0)
        assert bits(v) == bits([f32(dx * coef), 0.0, f32(dz * coef)]), state
        assert (a, r, ap) == (0, mr.CS_MOVING, 1)


def test_start_and_waking_get_the_velocity_but_do_not_apply_it():
    for state in (mr.CS_START, mr.CS_WAKING):
        v, a, r, ap = one(state=state, motion=(1.0, 0.0), velocity=(9.0, 9.0, 9.0))
        assert bits(v) == bits([f32(0.3), 0.0, 0.0]) and (a, r, ap) == (0, mr.CS_MOVING, 0), state


def test_walking_on_a_slope_stays_in_its_plane():
    n = np.array([0.3, 0.9, -0.2], f32)
    v, a, r, ap = one(state=mr.CS_MOVING, motion=(1.0, 0.5), normal=n)
    assert (a, r, ap) == (0, mr.CS_MOVING, 1)
    nd = n.astype(f64) / np.linalg.norm(n.astype(f64))
    newz = np.cross([1.0, 0.0, 0.0], nd)
    newx = np.cross(nd, newz)
    want = newx / np.linalg.norm(newx) * 1.0 + newz / np.linalg.norm(newz) * 0.5
    assert np.abs(v - want).max() <= 4 * 2.0 ** -23 * np.abs(want).max()    # a handful of float roundings
    assert abs(np.dot(v.astype(f64), nd)) <= 1e-6


def test_zero_normal_keeps_the_velocity_and_still_moves():
    v, a, r, ap = one(motion=(1.0, 1.0), normal=(0.0, 0.0, 0.0), velocity=(3.0, 4.0, 5.0))
    assert bits(v) == bits([3.0, 4.0, 5.0]) and (a, r, ap) == (0, mr.CS_MOVING, 1)


def test_no_motion_asks_for_idle():
    v, a, r, ap = one(state=mr.CS_MOVING, motion=(0.0, -0.0), velocity=(3.0, 4.0, 5.0))
    assert bits(v) == bits([3.0, 4.0, 5.0]) and (a, r, ap) == (0, mr.CS_IDLE, 0)


def test_jump_from_idle_and_from_moving():
    dx, dz, fwd, up = f32(0.6), f32(-0.8), f32(2.5), f32(6.0)
    want = bits([f32(dx * fwd), up, f32(dz * fwd)])
    v, a, r, ap = one(state=mr.CS_IDLE, jump=True, motion=(dx, dz), jump_params=(fwd, up), velocity=(1.0, 1.0, 1.0))
    assert bits(v) == want and (a, r, ap) == (0, mr.CS_JUMP_START, 0)
    v, a, r, ap = one(state=mr.CS_MOVING, jump=True, motion=(dx, dz), jump_params=(fwd, up))
    assert bits(v) == want and (a, r, ap) == (1, mr.CS_JUMP_START, 0)
    # airborne: character_jump returns false before it is asked (the branch above it has left already)
    assert one(grounded_out=False, jump=True, motion=(dx, dz))[2] == mr.CS_FALLING


def test_nan_velocity():
    nan = f32(np.nan)
    v, a, r, ap = one(grounded_out=False, velocity=(1.0, nan, 2.0))
    assert np.isnan(v[1]) and bits(v[[0, 2]]) == bits([1.0, 2.0]) and (a, r, ap) == (1, mr.CS_FALLING, 1)
    # NaN > 0 is false: no jump protection, and the walking velocity replaces it
    v, a, r, ap = one(grounded_out=True, state=mr.CS_JUMPING, velocity=(nan, nan, nan), motion=(1.0, 0.0))
    assert bits(v) == bits([f32(0.3), 0.0, 0.0]) and (a, r, ap) == (0, mr.CS_MOVING, 1)
    # a NaN motion has a length that is not 0
    assert one(motion=(nan, 0.0))[2] == mr.CS_MOVING


def test_flagged_ray_ends_the_mover():
    for f in (mr.RAY_INVALID, mr.RAY_UNRESOLVED, mr.RAY_UNRESOLVED | mr.RAY_MOVED_TARGET):
        for air in (0, 1):
            v, a, r, ap = one(ray_flags=f, grounded_out=False, airborne=air, velocity=(1.0, 2.0, 3.0), motion=(1.0, 1.0), jump=True)
            assert bits(v) == bits([1.0, 2.0, 3.0]) and (a, r, ap) == (air, mr.CS_NONE, 0)
    assert one(ray_flags=mr.RAY_MOVED_TARGET, motion=(1.0, 0.0))[2] == mr.CS_MOVING          # reported, and goes on


def test_batch_is_the_single_rule_per_mover():
    R = np.random.Generator(np.random.PCG64(5))
    n = 64
    a = dict(ray_flags=R.choice([0, 0, 0, 1, 2, 4], n), grounded_out=R.integers(0, 2, n), state=R.integers(0, 7, n),
             jump=R.integers(0, 4, n) == 0, motion=R.normal(0, 1, (n, 2)).astype(f32) * (R.integers(0, 3, (n, 1)) > 0),
             jump_params=R.uniform(1, 5, (n, 2)).astype(f32), velocity=R.normal(0, 3, (n, 3)).astype(f32),
             normal=R.normal(0, 1, (n, 3)).astype(f32), airborne=R.integers(0, 2, n))
    out = mr.character_move_decide(gravity_y=G, dt_sec=DT, **a)
    assert set(out["request"].tolist()) == {mr.CS_NONE, mr.CS_IDLE, mr.CS_MOVING, mr.CS_JUMP_START, mr.CS_FALLING}
    for k in range(n):
        v, air, r, ap = mr.character_move_decide_one(*[a[key][k] for key in a], G, DT)
        assert bits(out["velocity"][k]) == bits(v) and (out["airborne"][k], out["request"][k], out["applied"][k]) == (air, r, ap)


# ------------------------------------------------------------------------------------------------- the binding
def test_restatement_and_binding_name_the_same_character_states():
    """tests/test_cabi.py holds _lib's CS_* to the header's CLAPGPU_CS_*; this holds the restatement's to _lib's"""
    names = ("CS_START", "CS_WAKING", "CS_IDLE", "CS_MOVING", "CS_JUMP_START", "CS_JUMPING", "CS_FALLING", "CS_NONE")
    assert [getattr(mr, k) for k in names] == [getattr(_lib, k) for k in names]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_move_refuses_bad_arguments_before_any_hip_call(L):
    buf = (C.c_double * 256)()
    base = C.addressof(buf)
    p = (base + 255) & ~255                                                # 256-byte aligned, inside buf
    assert p + 512 <= base + C.sizeof(buf)

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
    w, sg, e = _lib.World(), _lib.Geoms(), _lib.Entities()
    e.rot = e.flags = p
    bad = _lib.ERR_INVALID_ARGUMENTS

    def call(b=bodies(), w=w, sg=sg, e=None, m=moves(), scratch=p, bp=None):
        ref = lambda x: None if x is None else C.byref(x)
        return L.clapgpu_characters_move(None, bp, ref(b), ref(w), ref(sg), None, ref(e), 1.0 / 60.0, ref(m), scratch)
    assert call(m=None) == bad and call(b=None) == bad and call(w=None) == bad and call(sg=None) == bad
    for field in ("pos", "quat", "lvel", "radius", "yoffset", "facc", "mass", "bflags", "adis_steps_left", "adis_time_left"):
        assert call(b=bodies(**{field: 1})) == bad, field
        assert call(b=bodies(**{field: 1}), m=moves(0)) == bad, field        # also for an empty batch
    for field in [f[0] for f in _lib.CharactersMove._fields_[1:16]]:
        assert call(m=moves(**{field: None})) == bad, field
    assert call(m=moves(entity=p)) == bad and call(m=moves(yaw_quat=p)) == bad                # one of the pair
    assert call(m=moves(entity=p, yaw_quat=p)) == bad                                         # the pair without entities
    assert call(m=moves(entity=p, yaw_quat=p), e=_lib.Entities()) == bad                      # ... without rot / flags
    assert call(m=moves(entity=p, yaw_quat=p + 4), e=e) == bad                                # a quat array off 16 bytes
    assert call(scratch=None) == bad and call(scratch=p + 64) == bad
    assert call(b=bodies(aabb=1), bp=C.c_void_p(p)) == bad                                    # an index needs the boxes
    assert call(m=moves(0)) == _lib.OK
    assert call(m=_lib.CharactersMove(0), scratch=None) == _lib.OK                            # n == 0: nothing else is asked
    assert L.clapgpu_characters_move_scratch_bytes(100, 0) == 0
    assert L.clapgpu_characters_move_scratch_bytes(100, (1 << 28) + 1) == 0


def test_frame_refuses_a_move_without_its_world(L):
    f = _lib.FrameDesc()
    ent = _lib.Entities()
    f.entities = C.pointer(ent)
    m = _lib.CharactersMove(0)
    f.move = C.pointer(m)
    assert L.clapgpu_frame_issue(None, C.byref(f), 0.0, 0) == _lib.ERR_INVALID_ARGUMENTS


def test_header_integration_and_restatement_name_the_same_rule():
    header = open(os.path.join(ROOT, "include", "clapgpu.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    doc = mr.__doc__
    for text in (header, integ, doc):
        flat = re.sub(r"[\s*]+", " ", text)
        for phrase in ("velocity[1] > 0", "1e-6", "JUMP_START", "FALLING", "0.3f", "jump_forward", "state < IDLE"):
            assert phrase in flat or phrase.replace("state < IDLE", "state >= IDLE") in flat, phrase
