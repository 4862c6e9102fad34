"""GPU: the order of a crowd (clapgpu_characters_order, clapgpu_characters_move_ordered; clap_amd/csrc/order.hip).
Reach boxes and levels against tests/orderref.py, bit for bit; the reach box against what a mover moved alone really
touches; the ordered move of a crowd against clapgpu_characters_move called once per mover in list order, byte for byte;
movers that cannot reach each other; too small a pair capacity; brute force and no meshes; both calls on arrays under
guard bands with a scratch and a pair room of exactly the size asked for.  Every comparison is == on bit patterns.  (The restatement on hand cases and the refusals: test_order.py.)"""
import numpy as np
import pytest
import torch

from clap_amd import _lib, physics, synth
import orderref as orf
import slideref as sr
from meshscene import Scene, same_bits, rng
from test_move_gpu import KEYS, OUT, DT, snapshot, restore, body_state, sleepy, movers, make, run_call, apart_movers, coverage

pytestmark = pytest.mark.gpu
CENTRE = np.array([16.0, 16.0])
CROWD = 120                                                 # test 3's movers
CHUNK = 8                                                   # order.hip's ORDER_CHUNK: rounds between two read-backs
SEED, SPEED = 21, 4.0


@pytest.fixture(scope="module")
def terrain(cuda_device):
    """test_move_gpu's scene B (3 000 capsules over the terrain mesh), the 200 bodies nearest to its middle drawn together
    to 0.45 of their distance from it and down to just above the ground: a crowd whose members touch"""
    b, meshes = sr.scene_b(n=3000)
    near = nearest(b, 200)
    b["pos"][near, 0] = CENTRE[0] + 0.45 * (b["pos"][near, 0] - CENTRE[0])
    b["pos"][near, 2] = CENTRE[1] + 0.45 * (b["pos"][near, 2] - CENTRE[1])
    b["pos"][near, 1] = sr.ground_b(b["pos"][near, 0], b["pos"][near, 2]) + b["yoffset"][near] + rng(2).uniform(-0.03, 0.6, 200)
    sc = Scene(cuda_device, b, meshes, cap=(1 << 20, 1 << 20))
    sleepy(sc.w, 8)
    sc.w.bodies_aabb()
    return sc.w, b, snapshot(sc.w)


def nearest(b, n):
    n_bodies = int(b["n"])
    d = np.hypot(b["pos"][:, 0] - CENTRE[0], b["pos"][:, 2] - CENTRE[1])
    d[:n_bodies // 6] = np.inf                                               # those stand around the box mesh
    return np.argsort(d, kind="stable")[:n].astype(np.uint32)


def crowd(b, n, seed=SEED, speed=SPEED):
    """n movers out of the 200 in the middle, in a shuffled order, test_move_gpu's mix of states"""
    bodies = nearest(b, 200)[rng(seed).permutation(200)[:n]]
    return movers(b, bodies, seed + 1, speed=speed)


def reference(w, b, mv, dt=DT):
    d = w.download()
    reach = orf.reach_boxes(mv["body"], mv["ray_off"], mv["motion"], mv["velocity"], d["aabb"], d["pos"], b["yoffset"],
                            np.float32(w.world.gravity[1]), dt)
    return (reach,) + orf.levels(mv["body"], reach, w.n)


def order(w, mv, dt=DT, **kw):
    reach, level, n_levels, pair_total = w.characters_order(make(w, mv), dt, **kw)
    return reach.cpu().numpy(), level.cpu().numpy().view(np.uint32), n_levels, pair_total


# ------------------------------------------------------------------------------------------------- 1. levels and boxes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_levels_and_boxes_are_the_restatement(terrain, n):
    w, b, before = terrain
    restore(w, before)
    mv = crowd(b, n)
    if n >= 63:
        mv["body"][7] = mv["body"][3]                                        # a body listed twice
        mv["velocity"][5] = np.nan                                           # that branch's bound counts as 0
        mv["ray_off"][11] = -np.inf                                          # an infinite ray: a box that is not finite
        mv["body"][13] = w.n + 5                                             # no body of the set
        mv["ray_off"][17] = np.nan                                           # no ray: a finite box
    want_reach, want_level, want_n, want_pairs = reference(w, b, mv)
    reach, level, n_levels, pair_total = order(w, mv)
    print("movers", n, "n_levels", n_levels, "pair_total", pair_total, "rounds", w.order_summary[3])
    assert same_bits(reach, want_reach), np.flatnonzero((reach != want_reach).any(1))[:8]
    assert same_bits(level, want_level), np.flatnonzero(level != want_level)[:8]
    assert (n_levels, pair_total) == (want_n, want_pairs)
    if n >= 63:
        cls = orf.classes(mv["body"], want_reach, w.n)
        assert cls[[3, 7, 13]].tolist() == [orf.OUT] * 3 and cls[11] == orf.ALONE and cls[[5, 17]].tolist() == [0, 0]
        assert not level[[3, 7, 13]].any() and level[11] == level[:11].max() + 1 and (level[12:][cls[12:] == 0] > level[11]).all()
        assert n_levels >= 3
    for k in KEYS:                                                           # nothing moved
        assert same_bits(getattr(w, k).cpu().numpy(), before[k].cpu().numpy()), k


def test_a_line_longer_than_the_round_chunk_converges(cuda_device):
    """12 spheres of radius 0.5 at 0.9 from each other: each meets the next alone, one level each, and a hop of the
    relaxation per round (the pairs share a wavefront), so the convergence loop reads its word back more than once"""
    n = CHUNK + 4
    b = synth.sphere_bodies(n, box=1.0, seed=5)
    b["radius"][:] = 0.5
    b["yoffset"][:] = 0.5
    b["pos"][:] = np.stack([0.9 * np.arange(n), np.zeros(n), np.zeros(n)], 1)
    w = physics.PhysWorld(b, None, device=cuda_device, forces=True)
    mv = movers(b, np.arange(n, dtype=np.uint32), 3, speed=0.0)
    mv["motion"][:] = 0
    for bodies in (np.arange(n), np.arange(n)[::-1].copy()):
        mv["body"] = bodies.astype(np.uint32)
        want = reference(w, b, mv)
        assert want[1].tolist() == list(range(n))
        reach, level, n_levels, pair_total = order(w, mv)
        assert same_bits(reach, want[0]) and same_bits(level, want[1]) and (n_levels, pair_total) == (n, n - 1)
        assert w.order_summary[3] > CHUNK, w.order_summary


# ------------------------------------------------------------------------------------------------- 2. the reach box
def inside(box, reach):
    return (box[0::2] >= reach[0::2]).all() and (box[1::2] <= reach[1::2]).all()


def meets(box, reach):
    return (box[0::2] <= reach[1::2]).all() and (box[1::2] >= reach[0::2]).all()


def test_reach_holds_what_a_mover_alone_touches(terrain):
    w, b, before = terrain
    restore(w, before)
    mv = crowd(b, 200)
    reach = order(w, mv)[0]
    aabb0 = before["aabb"].cpu().numpy()
    statics = w._statics_host
    moved = touched = 0
    for k in range(200):
        restore(w, before)
        out, bodies = run_call(w, {key: v[k:k + 1] for key, v in mv.items()})
        i = mv["body"][k]
        assert inside(aabb0[i], reach[k]), (k, "before")
        assert inside(bodies["aabb"][i], reach[k]), (k, "after", bodies["aabb"][i], reach[k])
        moved += not same_bits(bodies["aabb"][i], aabb0[i])
        for h in [out["collision"][0]] + out["push_hit"][0].tolist():
            if h >= 0:
                assert meets(aabb0[h], reach[k]), (k, "body", h)
                touched += 1
            elif h <= -2:
                assert meets(statics[-2 - h], reach[k]), (k, "static", -2 - h)
        others = np.delete(np.arange(w.n), i)                                # and nobody else moved
        assert same_bits(bodies["pos"][others], before["pos"].cpu().numpy()[others]), k
    print("reach: movers that moved", moved, "bodies they reported", touched)
    assert moved > 100 and touched > 10


# ------------------------------------------------------------------------------------------------- 3. the crowd
def run_ordered(w, mv, dt=DT, **kw):
    m = make(w, mv)
    res = w.characters_move_ordered(m, dt, **kw)
    out = {k: res[k].cpu().numpy().copy() for k in OUT}
    out["flags"] = out["flags"].view(np.uint32)
    return out, body_state(w), res["level"].cpu().numpy().view(np.uint32), res["n_levels"]


def one_at_a_time(w, mv, dt=DT, **kw):
    single = {k: [] for k in OUT}
    for k in range(len(mv["body"])):                                         # in list order, on the world the others left
        o, _ = run_call(w, {key: v[k:k + 1] for key, v in mv.items()}, dt=dt, **kw)
        for key in OUT:
            single[key].append(o[key][0])
    return {k: np.asarray(v) for k, v in single.items()}, body_state(w)


def moved_target(flags):
    return ((flags & 4) != 0) | (((flags >> 8) & 4) != 0)


def two_level_pushes(out, level, n_bodies):
    """bodies pushed by movers of two different levels: the deferred push's case"""
    lo, hi = np.full(n_bodies, 1 << 30), np.full(n_bodies, -1)
    for k in np.flatnonzero((out["flags"] >> 8) == 0):
        for h in out["push_hit"][k]:
            if h >= 0:
                lo[h], hi[h] = min(lo[h], level[k]), max(hi[h], level[k])
    return int((hi > lo).sum())


@pytest.fixture(scope="module")
def crowd_case(terrain):
    """the crowd of test 3: (movers, the one-at-a-time loop's result, the plain batch's, the ordered call's)"""
    w, b, before = terrain
    mv = crowd(b, CROWD)
    restore(w, before)
    seq = one_at_a_time(w, mv)
    restore(w, before)
    batch = run_call(w, mv)
    restore(w, before)
    ordered = run_ordered(w, mv)
    return mv, seq, batch, ordered


def same_results(got, want, what):
    for k in OUT:
        assert same_bits(got[0][k], want[0][k]), (what, k, np.flatnonzero((np.atleast_2d(got[0][k].T) != np.atleast_2d(want[0][k].T)).any(0))[:8])
    for k in KEYS:
        assert same_bits(got[1][k], want[1][k]), (what, "bodies", k)


def test_ordered_crowd_is_the_one_at_a_time_loop(terrain, crowd_case):
    w, b, before = terrain
    mv, seq, batch, (out, bodies, level, n_levels) = crowd_case
    wrong = int((batch[1]["pos"][mv["body"]] != seq[1]["pos"][mv["body"]]).any(1).sum())
    flagged = int(moved_target(batch[0]["flags"]).sum())
    two = two_level_pushes(out, level, w.n)
    print("crowd", CROWD, "n_levels", n_levels, "plain batch: movers with another pos", wrong, "flagged MOVED_TARGET", flagged,
          "bodies pushed from two levels", two, coverage(out, "ordered"))
    # the scene: the test cannot pass without the order mattering
    assert n_levels >= 3 and wrong >= 1 and flagged >= 1 and two >= 1
    assert (mv["jump"] != 0).any() and (out["request"] == _lib.CS_JUMP_START).any()
    same_results((out, bodies), seq, "ordered against the loop")
    assert not moved_target(out["flags"]).any()
    assert not same_bits(bodies["facc"], before["facc"].cpu().numpy())
    restore(w, before)                                                       # the levels are those of the inputs
    assert same_bits(level, reference(w, b, mv)[1]) and n_levels == int(level.max()) + 1


# ------------------------------------------------------------------------------------------------- 4. nothing conflicts
def test_movers_apart_are_one_level_and_the_plain_call(terrain):
    w, b, before = terrain
    restore(w, before)
    cand = rng(6).choice(b["n"], 1500, replace=False)
    mv = movers(b, cand, 14, speed=2.0)
    mv["jump"][:] = 0
    keep = apart_movers(b, w.download()["aabb"], cand, mv, 70, DT)
    mv = {k: v[keep] for k, v in mv.items()}
    plain = run_call(w, mv)
    restore(w, before)
    out, bodies, level, n_levels = run_ordered(w, mv)
    assert n_levels == 1 and not level.any()
    same_results((out, bodies), plain, "apart")
    assert int(out["applied"].sum()) > 10


# ------------------------------------------------------------------------------------------------- 5. the pair capacity
def test_too_small_a_pair_capacity_moves_nothing(terrain, crowd_case):
    w, b, before = terrain
    mv, seq, _batch, ordered = crowd_case
    restore(w, before)
    with pytest.raises(_lib.ClapGpuError) as err:
        run_ordered(w, mv, pair_capacity=1)
    assert err.value.code == _lib.ERR_TOO_LARGE
    torch.cuda.synchronize()
    for k in KEYS:
        assert same_bits(getattr(w, k).cpu().numpy(), before[k].cpu().numpy()), k
    with pytest.raises(_lib.ClapGpuError) as err:
        order(w, mv, pair_capacity=1)
    assert err.value.code == _lib.ERR_TOO_LARGE and w.order_summary[1] > 1      # how many there are
    out, bodies, level, n_levels = run_ordered(w, mv, pair_capacity=w.order_summary[1])   # exactly enough
    same_results((out, bodies), ordered[:2], "after the refusal")
    assert same_bits(level, ordered[2]) and n_levels == ordered[3]


# ------------------------------------------------------------------------------------------------- 6. other paths
def test_brute_force_gives_the_same_and_no_meshes_its_own_loop(terrain, crowd_case):
    """grid=False is the ordered result of test 3 byte for byte.  meshes=False is another physical case (the terrain is
    then an OTHER static nobody resolves, and the movers over it end at the ray), so it is held to its own one-at-a-time
    loop, and to the same levels: the order does not look at the statics"""
    w, b, before = terrain
    mv, _seq, _batch, ordered = crowd_case
    restore(w, before)
    out, bodies, level, n_levels = run_ordered(w, mv, grid=False)
    same_results((out, bodies), ordered[:2], "bp=None")
    assert same_bits(level, ordered[2]) and n_levels == ordered[3]
    restore(w, before)
    seq = one_at_a_time(w, mv, meshes=False)
    restore(w, before)
    out, bodies, level, n_levels = run_ordered(w, mv, meshes=False)
    same_results((out, bodies), seq, "meshes=False")
    assert same_bits(level, ordered[2]) and ((out["flags"] & _lib.RAY_UNRESOLVED) != 0).any()


def test_order_of_no_movers(terrain):
    w, b, before = terrain
    restore(w, before)
    empty = {k: v[:0] for k, v in crowd(b, 2).items()}
    reach, level, n_levels, pair_total = order(w, empty)
    assert len(reach) == 0 and len(level) == 0 and (n_levels, pair_total) == (0, 0)
    out, bodies, level, n_levels = run_ordered(w, empty)
    assert n_levels == 0 and all(len(out[k]) == 0 for k in OUT)
    for k in KEYS:
        assert same_bits(bodies[k], before[k].cpu().numpy()), k


# ------------------------------------------------------------------------------------------------- 7. where it writes
@pytest.fixture
def g(cuda_device, monkeypatch):
    """tests/guards.py's registry with its hook under the mirrors: every device array between two bands of 0xA5"""
    import guards
    reg = guards.Guards(cuda_device)
    guards.install(monkeypatch, reg)
    return reg


@pytest.mark.parametrize("n,q", [(65, 1), (65, 63), (65, 65), (300, 257)], ids=["q1", "q63", "q65", "q257_of_300"])
@pytest.mark.parametrize("grid", [True, False], ids=["grid", "bp_null"])
def test_ordered_move_writes_inside_its_arrays(n, q, grid, g, cuda_device):
    """test_extents_gpu's crowded world and counts: the order and the ordered move on arrays under guard, a scratch of
    exactly *_scratch_bytes and a pair room of exactly pair_total; no band is touched, and the result is the loop's"""
    box = 4.0 if n <= 65 else 7.0
    b = synth.capsule_bodies(n, box=box, seed=19)
    stand = np.arange(0, n, 2)
    b["pos"][stand, 1] = 0.5 + b["yoffset"][stand] + rng(30).uniform(-0.04, 0.04, len(stand))
    w = physics.PhysWorld(b, synth.static_boxes(12, box), device=cuda_device)
    sleepy(w, 7)
    w.bodies_aabb()
    before = snapshot(w)
    mv = movers(b, rng(200 + q).choice(n, q, replace=False), 11)
    want_reach, want_level, want_n, want_pairs = reference(w, b, mv)
    cap = max(want_pairs, 1)
    w._order_scratch = g.scratch(_lib.characters_order_scratch_bytes(q, cap))
    reach, level, n_levels, pair_total = order(w, mv, pair_capacity=cap)
    g.check(f"characters_order of {q}")
    assert same_bits(reach, want_reach) and same_bits(level, want_level) and (n_levels, pair_total) == (want_n, want_pairs)
    w._order_scratch = g.scratch(_lib.characters_move_ordered_scratch_bytes(w.n, q, cap))
    got = run_ordered(w, mv, grid=grid, pair_capacity=cap)
    g.check(f"characters_move_ordered of {q}, grid={grid}")
    assert same_bits(got[2], want_level) and got[3] == want_n
    restore(w, before)
    same_results(got[:2], one_at_a_time(w, mv, grid=grid), (q, grid))
    if q > 1:
        assert n_levels >= 3 and got[0]["applied"].any() and (got[0]["collision"] != -1).any()
