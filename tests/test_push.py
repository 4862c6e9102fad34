"""CPU: the restatement of phys_body_push over a batch and of the step with a force accumulator (tests/pushref.py) on hand
cases; the restated step against the oracle's where they overlap (no forces); clapgpu_bodies_push refuses bad arguments
before any HIP call; the flag and the descriptor match the header.  (The device side: test_push_gpu.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from clap_amd import _lib, synth
import pushref as pr
import slideref as sr

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def little(n=6):
    b = synth.capsule_bodies(n, box=4.0, seed=2)
    return b, pr.push_state(b)


def hits(n, **slots):
    ph = np.full((n, 6), -1, np.int32)
    for key, h in slots.items():                                          # k0q2=5: mover 0, slot 2 pushes body 5
        k, q = key[1:].split("q")
        ph[int(k), int(q)] = h
    return ph


def test_one_push_is_the_float_product_widened():
    b, st = little()
    b["mass"][1] = 72.3
    v = np.array([[1.37, -9.81, 0.003]], f32)
    pushed = pr.push(st, b["mass"], np.array([1], np.uint32), v, hits(1, k0q0=4))
    want = np.array([f64(f32(f32(72.3) * v[0, j])) for j in range(3)])
    assert st["facc"][4].tobytes() == want.tobytes()
    assert f64(f32(72.3)) * f64(v[0, 0]) != want[0], "the product is rounded to float before it is widened"
    assert pushed.tolist() == [0, 0, 0, 0, 1, 0] and not st["facc"][[0, 1, 2, 3, 5]].any()


def test_push_enables_and_resets_the_counters():
    b, st = little()
    st["bflags"][3] |= pr.DISABLED | pr.KINEMATIC
    st["adis_steps_left"][3], st["adis_time_left"][3] = -2, -0.5
    before = st["bflags"].copy()
    pr.push(st, b["mass"], np.array([0], np.uint32), np.ones((1, 3), f32), hits(1, k0q5=3),
            world=dict(pr.WORLD, adis_steps=7, adis_time=0.25))
    assert st["bflags"][3] == before[3] & ~np.uint32(pr.DISABLED) and st["bflags"][3] & pr.KINEMATIC
    assert st["adis_steps_left"][3] == 7 and st["adis_time_left"][3] == 0.25
    keep = np.arange(6) != 3
    assert np.array_equal(st["bflags"][keep], before[keep]) and (st["adis_steps_left"][keep] == 30).all()


def test_order_of_two_pushers_changes_the_bits():
    """fp64 addition is not associative: onto an accumulator that holds 1.0, forces of 2^-53 and 1.5 * 2^-53 give
    1 + 2^-52 in one order (the first is a tie that rounds to even, the second rounds up) and 1 + 2^-51 in the other
    (the first rounds up, the second is a tie from an odd mantissa)"""
    b, st = little()
    b["mass"][:2] = [1.0, 1.0]
    v = np.array([[2.0 ** -53, 0, 0], [1.5 * 2.0 ** -53, 0, 0]], f32)
    pusher = np.array([0, 1], np.uint32)
    ph = hits(2, k0q0=5, k1q0=5)
    st["facc"][5, 0] = 1.0
    a, c = pr.push_state(b, st["facc"]), pr.push_state(b, st["facc"])
    pr.push(a, b["mass"], pusher, v, ph)
    pr.push(c, b["mass"], pusher[::-1].copy(), v[::-1].copy(), ph)
    assert a["facc"][5, 0] == 1.0 + 2.0 ** -52 and c["facc"][5, 0] == 1.0 + 2.0 ** -51
    r = pr.push_state(b, st["facc"])
    pr.push(r, b["mass"], pusher, v, ph, reverse=True)
    assert r["facc"].tobytes() == c["facc"].tobytes(), "reverse= is the other list order"


def test_slots_of_one_mover_go_in_call_order_and_repeat():
    b, st = little()
    v = np.array([[0.1, 0.2, 0.3]], f32)
    pushed = pr.push(st, b["mass"], np.array([2], np.uint32), v, hits(1, k0q0=4, k0q1=4, k0q3=4, k0q4=1))
    one = pr.force_of(b["mass"], [2], v, 0).astype(f64)
    assert st["facc"][4].tobytes() == ((one + one) + one).tobytes() and st["facc"][1].tobytes() == one.tobytes()
    assert pushed[4] == 3 and pushed[1] == 1


def test_flagged_movers_and_bad_slots_push_nothing():
    b, st = little()
    v = np.ones((4, 3), f32)
    ph = hits(4, k0q0=1, k1q0=1, k2q0=6, k2q1=-7, k2q2=2 ** 31 - 1, k3q0=1)
    pusher = np.array([0, 2, 3, 6], np.uint32)                             # mover 3's body is out of range
    flags = np.array([0, 4, 0, 0], np.uint32)                              # mover 1: MOVED_TARGET, the host redoes it
    pushed = pr.push(st, b["mass"], pusher, v, ph, flags)
    assert pushed.tolist() == [0, 1, 0, 0, 0, 0]
    assert st["facc"][1].tobytes() == pr.force_of(b["mass"], pusher, v, 0).astype(f64).tobytes()
    st2 = pr.push_state(b)
    assert pr.push(st2, b["mass"], pusher, v, ph, np.array([1, 2, 4, 0], np.uint32)).sum() == 0 and not st2["facc"].any()


def test_crowd_scene_has_power():
    """what test_push_gpu.py's crowd test relies on: many bodies pushed by several movers, an order that shows"""
    mass, pusher, v, ph = pr.crowd(4096, 64, seed=41)
    nb = len(mass)
    movers_of = [set() for _ in range(nb)]
    for k in range(len(pusher)):
        for h in ph[k][ph[k] >= 0]:
            movers_of[h].add(k)
    assert sum(len(m) >= 2 for m in movers_of) >= 32
    b = dict(n=nb, bflags=np.zeros(nb, np.uint32), adis_steps_left=np.zeros(nb, np.int32), adis_time_left=np.zeros(nb))
    a, r = pr.push_state(b), pr.push_state(b)
    pa, pb = pr.push(a, mass, pusher, v, ph), pr.push(r, mass, pusher, v, ph, reverse=True)
    assert np.array_equal(pa, pb) and (a["facc"].view(np.uint64) != r["facc"].view(np.uint64)).any()


# ------------------------------------------------------------------------------------------------- the step
def test_step_with_one_force_by_hand():
    b = synth.sphere_bodies(3, box=4.0, seed=3)
    b["bflags"][:] = [0, pr.NO_GRAVITY, pr.KINEMATIC]
    b["lvel"][:] = [[0.5, 0.25, -1.0]] * 3
    st = pr.step_state(b, [[3.0, -1.5, 0.7]] * 3)
    h = 1.0 / 120.0
    stepped = pr.step_forces(b, st, h, dict(pr.WORLD, linear_damping=0.0))
    assert stepped.all() and not st["facc"].any()
    m = b["mass"]
    f0 = np.array([3.0, -1.5 + m[0] * -9.8, 0.7])
    assert st["lvel"][0].tobytes() == (b["lvel"][0] + (h * (1.0 / m[0])) * f0).tobytes()
    assert st["lvel"][1].tobytes() == (b["lvel"][1] + (h * (1.0 / m[1])) * np.array([3.0, -1.5, 0.7])).tobytes()
    assert st["lvel"][2].tobytes() == b["lvel"][2].tobytes(), "kinematic: invMass 0"
    assert st["pos"][2].tobytes() == (b["pos"][2] + h * b["lvel"][2]).tobytes(), "... and it still moves at its velocity"


def test_disabled_bodies_keep_their_accumulator():
    b = synth.capsule_bodies(4, box=4.0, seed=3)
    b["bflags"][1] |= pr.DISABLED
    b["bflags"][2] |= pr.HAS_JOINT | pr.NO_GRAVITY                          # at rest with a joint, one step from sleep
    b["lvel"][2] = b["avel"][2] = 0
    b["adis_steps_left"][2] = 1
    st = pr.step_state(b, np.full((4, 3), 2.0))
    stepped = pr.step_forces(b, st, 1.0 / 120.0)
    assert stepped.tolist() == [True, False, False, True]
    assert st["facc"].tolist() == [[0] * 3, [2.0] * 3, [2.0] * 3, [0] * 3]
    assert st["bflags"][2] & pr.DISABLED and not st["bflags"][2] & pr.HAS_JOINT


@pytest.mark.parametrize("kind", ["spheres", "capsules"])
def test_restated_step_without_forces_is_the_oracles(kind):
    """zeros in the accumulator: the restatement walks the oracle's step (gyroscopic torque, damping, auto-disable
    of the resting bodies that hold a joint) bit for bit, which pins every part of it the forces do not touch"""
    from oracle import binding as ob
    n = 3000
    b = (synth.sphere_bodies(n, box=32.0, seed=8, resting_frac=0.2) if kind == "spheres"
         else synth.capsule_bodies(n, box=32.0, seed=8, resting_frac=0.2))
    joint = ((b["bflags"] & 4) != 0) & (np.arange(n) % 2 == 0)
    st_o, st = ob.bodies_state(b), pr.step_state(b)
    for _ in range(33):
        st_o["bflags"][joint] |= 16
        st["bflags"][joint] |= 16
        ob.bodies_step(b, st_o, 1.0 / 120.0)
        pr.step_forces(b, st, 1.0 / 120.0)
    for k in ("pos", "quat", "lvel", "avel", "adis_time_left"):
        assert np.array_equal(st[k].view(np.uint64), st_o[k].view(np.uint64)), k
    assert np.array_equal(st["bflags"], st_o["bflags"]) and np.array_equal(st["adis_steps_left"], st_o["adis_steps_left"])
    assert (st["bflags"] & 1).any() and not st["facc"].any()


# ------------------------------------------------------------------------------------------------- the scenes
def pushing_movers(world, movers, v, air):
    out = []
    for k, m in enumerate(movers):
        out.append(sr.run_mover(world, m, v[k], air[k], 1.0 / 30.0)["push_hit"])
    return np.array(out)


def test_slide_scenes_push_bodies():
    """scene A and scene B of the slide tests, reused: in each at least 5 movers push a body, and the restated push of
    those batches lands on bodies"""
    import trimeshref as tr
    b, statics = sr.scene_a()
    movers, v, air = sr.movers_a(b["n"])
    pa = pushing_movers(sr.OracleSweep(b, statics), movers, v, air)
    bb, meshes = sr.scene_b()
    mv, vb, ab = sr.movers_b(bb)
    pb = pushing_movers(sr.SceneBSweep(bb, tr.bake(*meshes[0]), 0), mv, vb, ab)
    for name, bodies, mvs, vel, ph in (("A", b, movers, v, pa), ("B", bb, mv, vb, pb)):
        assert ((ph >= 0).any(axis=1)).sum() >= 5, name
        st = pr.push_state(bodies)
        pushed = pr.push(st, bodies["mass"], mvs, vel, ph)
        assert pushed.sum() == (ph >= 0).sum() and (st["facc"][pushed > 0] != 0).any(axis=1).all(), name


# ------------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_push_refuses_null_descriptors_and_arrays(L):
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    p = ptr.value

    def bodies(**gone):
        b = _lib.Bodies(4, 1, p, p, p, p, p, p, p, p, p, p, p)
        b.facc = p
        for k in gone:
            setattr(b, k, None)
        return b
    w = _lib.World()
    a = [ptr, ptr, ptr, ptr, ptr, ptr]                                    # pusher, velocity, push_hit, flags, pushed, scratch
    call = lambda b, w, n, *x: L.clapgpu_bodies_push(None, b, w, n, *x)
    assert call(None, C.byref(w), 2, *a) == _lib.ERR_INVALID_ARGUMENTS
    assert call(C.byref(bodies()), None, 2, *a) == _lib.ERR_INVALID_ARGUMENTS
    for field in ("facc", "mass", "bflags", "adis_steps_left", "adis_time_left"):
        assert call(C.byref(bodies(**{field: 1})), C.byref(w), 2, *a) == _lib.ERR_INVALID_ARGUMENTS, field
    for k in (0, 1, 2, 5):                                                 # flags and pushed may be NULL
        x = list(a)
        x[k] = None
        assert call(C.byref(bodies()), C.byref(w), 2, *x) == _lib.ERR_INVALID_ARGUMENTS, k
    assert call(C.byref(bodies()), C.byref(w), 0, None, None, None, None, None, None) == _lib.OK
    assert call(C.byref(bodies(facc=1)), C.byref(w), 0, None, None, None, None, None, None) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_bodies_push_scratch_bytes(0) == 0 and L.clapgpu_bodies_push_scratch_bytes((1 << 28) + 1) == 0


def test_kinematic_flag_and_bodies_fields_match_header():
    src = open(os.path.join(ROOT, "include", "clapgpu.h")).read()
    line = [l for l in src.splitlines() if l.startswith("#define CLAPGPU_BODY_KINEMATIC ")][0]
    assert re.search(r"\(1u << (\d+)\)", line).group(1) == "5" and _lib.BODY_KINEMATIC == 1 << 5 == pr.KINEMATIC
    body = re.search(r"typedef struct clapgpu_bodies \{(.*?)\} clapgpu_bodies;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)(\[\d+\])?\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.Bodies._fields_]
    assert names[-1] == "facc" and names[-2] == "geom_records", "appended: positional initialisers keep their meaning"
    assert _lib.Bodies(4, 1).facc is None
    assert _lib.ABI_VERSION >= 36
