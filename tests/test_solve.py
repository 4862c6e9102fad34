"""CPU: the contact-solve rule of include/clapgpu.h (tests/solveref.py) is physics, before the device is held to it bit
for bit (tests/test_solve_gpu.py).  Contacts come from the float64 geometry of tests/geomref.py, the step from
tests/pushref.py; nothing here touches the device.  These are the easy corner (identity quaternions, contact points on
the line of centres, one to three rows); the independent truth for the whole rule -- rotated anisotropic bodies, the
angular half of a row, coupled rows -- is tests/lcpref.py, which tests/test_solve_lcp.py holds solveref to."""
import numpy as np

import geomref as gr
import pushref as pr
import solveref as sr
from clap_amd import _lib

H = 1.0 / 120.0
EPS = float(np.finfo(np.float64).eps)
BOX = np.array([[-4.0, 4.0, -1.0, 0.0, -4.0, 4.0]])                      # the floor: top face at y = 0


def state(pos, radius=0.5, mass=1.0, lvel=None, flags=0, inertia=None):
    pos = np.asarray(pos, float).reshape(-1, 3)
    n = len(pos)
    st = dict(pos=pos.copy(), quat=np.tile([1.0, 0, 0, 0], (n, 1)), lvel=np.zeros((n, 3)), avel=np.zeros((n, 3)),
              bflags=np.full(n, flags, np.uint32), adis_steps_left=np.full(n, 30, np.int32), adis_time_left=np.zeros(n),
              facc=np.zeros((n, 3)), mass=np.full(n, mass), radius=np.full(n, radius), inertia=inertia)
    if lvel is not None:
        st["lvel"][:] = lvel
    return st


def floor_contact(st, i=0, **surface):
    c = gr.sphere_box(st["pos"][i:i + 1], st["radius"][i:i + 1], BOX)
    if not c["nc"][0]:
        return None
    return sr.record(np.asarray(c["pos"][0], float), np.asarray(c["normal"][0], float), float(c["depth"][0]), **surface)


def substep(st, **surface):
    """contact with the floor -> solve -> step, for body 0; returns the depth the solve saw"""
    rec = floor_contact(st, **surface)
    depth = None
    if rec is not None:
        depth = float(rec["depth"])
        out = sr.solve(st, np.arange(len(st["mass"])), H, static=(np.array([[0, 0]], np.uint32), sr.records([rec])))
        st["lvel"], st["avel"] = out["lvel"], out["avel"]
    pr.step_forces(dict(mass=st["mass"]), st, H)
    return depth


def test_abi():
    assert _lib.ABI_VERSION >= 38 and "clapgpu_bodies_solve" in _lib.SYMBOLS


def test_a_sphere_comes_to_rest_on_the_floor():
    """The fixed point of the rule: at rest the normal row holds lambda (1 + cfm m / h) = erp depth / h^2 + m |g| and the
    step needs lambda = m |g|, so depth* = soft_cfm m |g| h / soft_erp.  One row under SOR contracts by |1 - w| = 0.3 a
    sweep (0.3^20 = 3.5e-11 of lambda); the soft contact is an over-damped spring with time constant
    (1 - erp) / erp h = 0.16 s, so 1 200 substeps (10 s) leave e^-60 of the start.  The world's linear damping (0.001
    above a speed of 0.01) acts on the way down only."""
    st = state([[0.0, 0.5, 0.0]])
    want = 0.01 * 1.0 * 9.8 * H / 0.05
    depth = None
    for _ in range(1200):
        depth = substep(st)
    print("depth", depth, "depth*", want, "lvel", st["lvel"][0])
    assert abs(want - 0.0163) < 1e-4
    assert abs(depth - want) <= 1e-3 * want
    assert np.abs(st["lvel"][0]).max() <= 1e-6


def test_head_on_spheres_exchange_momentum():
    st = state([[-0.45, 0, 0], [0.45, 0, 0]], lvel=[[1.0, 0, 0], [-1.0, 0, 0]], flags=pr.NO_GRAVITY)
    c = gr.sphere_sphere(st["pos"][0:1], st["radius"][0:1], st["pos"][1:2], st["radius"][1:2])
    rec = sr.record(np.asarray(c["pos"][0], float), np.asarray(c["normal"][0], float), float(c["depth"][0]), bounce=1.0,
                    bounce_vel=0.0)
    assert rec["mode"] & sr.CONTACT_BOUNCE
    n = np.asarray(c["normal"][0], float)
    before = (st["lvel"][0] - st["lvel"][1]) @ n
    out = sr.solve(st, np.zeros(2, np.uint32), H, body=(np.array([[0, 1]], np.uint32), sr.records([rec])))
    after = (out["lvel"][0] - out["lvel"][1]) @ n
    p0, p1 = (st["mass"][:, None] * st["lvel"]).sum(0), (st["mass"][:, None] * out["lvel"]).sum(0)
    bound = 8 * EPS * (st["mass"][:, None] * out["impulse_abs"]).sum(0)
    print("relative normal velocity", before, "->", after, "momentum", p0, "->", p1, "bound", bound)
    assert before < 0 < after
    assert (np.abs(p1 - p0) <= bound).all() and bound.max() < 1e-13
    assert out["rows_total"] == 1 and out["row_lambda"][0] > 0


def test_friction_is_a_force_limit():
    """mu bounds the friction row's lambda, a force: a substep takes at most h mu / m off the sliding speed, whatever the
    load; inertia NULL, so the sphere slides without rolling.  n = (0, 1, 0) gives t1 = (-1, 0, 0), t2 = (0, 0, 1): sliding
    along x engages one friction row."""
    mu, m = 0.5, 1.0
    st = state([[0.0, 0.49, 0.0]], lvel=[[1.0, 0, 0]])
    stopped = False
    for k in range(400):
        rec = floor_contact(st, mu=mu)
        assert rec is not None
        v0 = st["lvel"][0, 0]
        out = sr.solve(st, np.arange(1), H, static=(np.array([[0, 0]], np.uint32), sr.records([rec])))
        assert out["rows_total"] == 3
        v1 = out["lvel"][0, 0]
        assert v0 - v1 <= H * mu / m * (1 + 1e-12), (k, v0, v1)
        assert v1 >= 0 and v1 <= v0, (k, v0, v1)                           # slower, never backwards
        assert out["lvel"][0, 2] == 0
        st["lvel"], st["avel"] = out["lvel"], out["avel"]
        pr.step_forces(dict(mass=st["mass"]), st, H)
        stopped = stopped or v1 < 1e-9
    assert stopped, st["lvel"]


def test_a_kinematic_wall_is_not_moved():
    """A stiff contact (soft_cfm 1e-10: with the default 0.01 the row is a damper that takes 1 / 2.2 of the approach a
    substep) against a KINEMATIC capsule: invM = 0 and invI = 0 on the capsule's side, so it keeps its bits and the
    sphere alone answers -- its approach velocity becomes the ERP term c = (erp / h) depth >= 0."""
    st = state([[0.0, 0.0, 0.0], [0.9, 0.0, 0.0]], lvel=[[2.0, 0.3, 0], [-0.5, 0, 0.25]], flags=pr.NO_GRAVITY)
    st["bflags"][1] |= pr.KINEMATIC
    st["avel"][1] = [0.1, -0.2, 0.3]
    st["inertia"] = np.full((2, 3), 0.1)
    c = gr.sphere_capsule(st["pos"][0:1], st["radius"][0:1], st["pos"][1:2], np.array([[0.0, 1.0, 0.0]]), np.array([0.5]),
                          np.array([1.0]))
    assert c["nc"][0] == 1
    n = np.asarray(c["normal"][0], float)
    rec = sr.record(np.asarray(c["pos"][0], float), n, float(c["depth"][0]), soft_cfm=1e-10, mu=0.5)
    out = sr.solve(st, np.zeros(2, np.uint32), H, body=(np.array([[0, 1]], np.uint32), sr.records([rec])))
    assert out["lvel"][1].tobytes() == st["lvel"][1].tobytes() and out["avel"][1].tobytes() == st["avel"][1].tobytes()
    r2 = np.asarray(c["pos"][0], float) - st["pos"][1]
    rel = lambda lv, av: (lv[0] - (lv[1] + np.cross(av[1], r2))) @ n        # the sphere's contact point is on its n axis
    before, after = rel(st["lvel"], st["avel"]), rel(out["lvel"], out["avel"])
    cterm = 0.05 / H * float(c["depth"][0])
    print("approach", before, "->", after, "ERP term", cterm)
    assert before < 0 <= after and abs(after - cterm) <= 1e-6


def test_a_sleeping_island_is_left_alone():
    st = state([[-0.45, 0, 0], [0.45, 0, 0]], lvel=[[1.0, 0, 0], [-1.0, 0, 0]], flags=pr.DISABLED)
    c = gr.sphere_sphere(st["pos"][0:1], st["radius"][0:1], st["pos"][1:2], st["radius"][1:2])
    rec = sr.record(np.asarray(c["pos"][0], float), np.asarray(c["normal"][0], float), float(c["depth"][0]), mu=0.5)
    floor = floor_contact(state([[0.0, 0.4, 0.0]]))
    out = sr.solve(st, np.zeros(2, np.uint32), H, static=(np.array([[0, 0]], np.uint32), sr.records([floor])),
                   body=(np.array([[0, 1]], np.uint32), sr.records([rec])))
    assert out["rows_total"] == 0 and out["status"] == 0
    assert out["lvel"].tobytes() == st["lvel"].tobytes() and out["avel"].tobytes() == st["avel"].tobytes()


def chain(order):
    """three overlapping spheres in a row, their two contacts listed in `order`"""
    st = state([[0.0, 0, 0], [0.83, 0.1, 0], [1.61, 0.35, 0.2]], lvel=[[0.3, 0, 0], [0, 0.1, 0], [-0.7, 0.2, 0.1]],
               inertia=np.full((3, 3), 0.1))
    pairs = np.array([[0, 1], [1, 2]], np.uint32)
    recs = []
    for i, j in pairs:
        c = gr.sphere_sphere(st["pos"][i:i + 1], st["radius"][i:i + 1], st["pos"][j:j + 1], st["radius"][j:j + 1])
        assert c["nc"][0] == 1
        recs.append(sr.record(np.asarray(c["pos"][0], float), np.asarray(c["normal"][0], float), float(c["depth"][0]), mu=0.5))
    return sr.solve(st, np.zeros(3, np.uint32), H, body=(pairs[order], sr.records([recs[k] for k in order])))


def test_the_row_order_matters_and_is_fixed():
    a, again, b = chain([0, 1]), chain([0, 1]), chain([1, 0])
    assert a["lvel"].tobytes() == again["lvel"].tobytes() and a["avel"].tobytes() == again["avel"].tobytes()
    assert a["row_lambda"].tobytes() == again["row_lambda"].tobytes()
    assert a["lvel"].tobytes() != b["lvel"].tobytes() or a["avel"].tobytes() != b["avel"].tobytes()
    assert np.abs(a["lvel"] - b["lvel"]).max() < 1e-3                     # the same physics, other roundings and sweeps
    assert [int(k) & 0xffffffff for k in a["row_key"]] == list(range(6)) and not (a["row_key"] >> np.uint64(32)).any()
