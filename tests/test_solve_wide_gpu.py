"""GPU: clapgpu_bodies_solve's wide path -- a large island walked level by level on a workgroup -- against tests/solveref.py
(the sequential sweep) and tests/solvelevelref.py (the levels).  The device makes its own contact lists; every
comparison is == on bit patterns, and the wide path must give the bits of the lane path."""
import ctypes as C

import numpy as np
import pytest
import torch

from clap_amd import _lib, physics, synth
from clap_amd._dev import upload
from meshscene import C2, guarded_scratch, same_bits
import solvelevelref as lr
import solveref as sr
import test_solve_gpu as base

pytestmark = pytest.mark.gpu
H = base.H
FLOOR = np.array([[-1e3, 1e3, -10.0, 0.5, -1e3, 1e3]])
WIDE_WORKGROUPS = 1024                                                      # CLAPGPU_SOLVE_WIDE_WORKGROUPS (include/clapgpu.h)


# ------------------------------------------------------------------------------------------------- helpers
def host_state(w, snap):
    st = {k: v.cpu().numpy() for k, v in snap.items()}
    st["bflags"] = st["bflags"].view(np.uint32)
    for k in ("lvel", "avel", "pos", "quat", "facc"):
        if k in st:
            st[k] = st[k][:w.n]
    return st


def plain_lists(w):
    """the static and the body list of a world without meshes"""
    c = w.download_contacts2(C2)
    d = w.download()
    assert d["pair_total"] <= w.capacity and d["static_pair_total"] <= w.static_capacity
    return dict(static=(d["static_pairs"], c["static"][0]), body=(d["pairs"], c["body"][0]))


class Case:
    """a world after its contact pass, the state the solve saw, the sequential answer and the levels: made once"""

    def __init__(self, w, lists=plain_lists, contact_pass=None):
        self.w = w
        if contact_pass is None:
            w.bodies_aabb()
            w.broadphase()
            w.contacts_geoms_both()
            w.islands(H)
            torch.cuda.synchronize()
        else:
            contact_pass(w)
        self.snap = base.snapshot(w)
        st, island, L = host_state(w, self.snap), w.island.cpu().numpy().view(np.uint32)[:w.n], lists(w)
        self.want = sr.solve(st, island, H, **L)
        self.bodies, key = lr.row_bodies(st, island, **L)
        assert same_bits(key, self.want["row_key"])                         # two enumerations, one order
        self.rows = self.want["rows_total"]
        self.per_island = lr.island_rows(key)

    def run(self, wide_rows, capacity=None, scratch=None):
        w = self.w
        base.restore(w, self.snap)
        w.alloc_solve(self.rows + 37 if capacity is None else capacity)
        if scratch is not None:
            w.solve_scratch = scratch
        w.solver.wide_rows = wide_rows
        w.solve_status.zero_()
        w.row_lambda.fill_(-1.0)
        w.row_key.fill_(-1)
        w.row_level.fill_(-1)
        w.wide_total.fill_(-1)
        w.solve(H, want_lambda=True, want_levels=True)
        return self.result()

    def result(self):
        w = self.w
        torch.cuda.synchronize()
        return dict(lvel=w.lvel.cpu().numpy()[:w.n].copy(), avel=w.avel.cpu().numpy()[:w.n].copy(),
                    row_lambda=w.row_lambda.cpu().numpy().copy(), row_key=w.row_key.cpu().numpy().view(np.uint64).copy(),
                    row_level=w.row_level.cpu().numpy().view(np.uint32).copy(), rows_total=int(w.rows_total.item()),
                    status=int(w.solve_status.item()), wide_total=int(w.wide_total.item()))

    def check(self, got, wide_rows):
        """the sequential sweep's bits, the reference's levels in the wide islands and 0 in the others"""
        k, want = self.rows, self.want
        assert got["status"] == 0 and got["rows_total"] == k
        assert same_bits(got["row_key"][:k], want["row_key"])
        level, wide = lr.expected_levels(want["row_key"], self.bodies, wide_rows)
        assert got["wide_total"] == wide == sum(1 for c in self.per_island.values() if wide_rows and c >= wide_rows)
        assert same_bits(got["row_level"][:k], level)
        assert not got["row_level"][k:].any()
        assert same_bits(got["row_lambda"][:k], want["row_lambda"])
        assert same_bits(got["lvel"], want["lvel"]) and same_bits(got["avel"], want["avel"])
        return level

    def both(self):
        """wide_rows 1 and 0: each the reference's bits, hence each other's; returns the levels"""
        wide, lane = self.run(1), self.run(0)
        level = self.check(wide, 1)
        self.check(lane, 0)
        assert not lane["row_level"].any() and lane["wide_total"] == 0
        for name in ("lvel", "avel", "row_lambda", "row_key"):
            assert same_bits(wide[name], lane[name]), name
        assert not same_bits(wide["lvel"], self.snap["lvel"].cpu().numpy()[:self.w.n])             # and something happened
        return level


def spheres(pos, dev, mu=0.5):
    """spheres of radius 0.3 at `pos` over the floor slab (top face y = 0.5), as tools/solve_time.py's pile makes them;
    every contact with friction mu"""
    n = len(pos)
    b = synth.sphere_bodies(n, box=64.0, seed=4)
    b["radius"][:] = 0.3
    b["pos"][:] = pos
    b["lvel"][:] *= 0.01
    b["cell"] = 1.0
    w = physics.PhysWorld(b, FLOOR, device=dev)
    mat = lambda k: np.tile([0.0, 0.0, mu, 0.0, 0.0], (k, 1))
    w.set_materials(mat(n))
    w.static_material = upload(mat(1), np.float64, w.device)
    return w


def grid_positions(n, side, pitch=0.5):
    i = np.arange(n)
    return np.stack([2.0 + pitch * (i % side), np.full(n, 0.78), 2.0 + pitch * (i // side)], 1)


# ------------------------------------------------------------------------------------------------- 1: the mixed scene
@pytest.fixture(scope="module")
def mixed(cuda_device):
    _b, w = base.build_scene(cuda_device)
    return Case(w, lists=base.lists, contact_pass=base.contact_pass)


@pytest.mark.parametrize("wide_rows", [1, 4, 64, 1 << 30])
def test_the_mixed_scene_at_every_threshold(mixed, wide_rows):
    """pairs, triples, the 41-sphere friction chain, kinematic bodies, sleepers, the deep record, the mesh bodies: 1 sends
    every island to a workgroup, 4 the triples and up, 64 the chain and the heaps, 2^30 none"""
    per = mixed.per_island
    assert mixed.rows > 500 and per[base.CHAIN0] >= 117
    assert min(per.values()) < 4 <= max(c for c in per.values() if c < 64) and max(per.values()) < 1 << 30
    got = mixed.run(wide_rows)
    level = mixed.check(got, wide_rows)
    wide = sum(1 for c in per.values() if c >= wide_rows)
    assert got["wide_total"] == wide and (wide == 0) == (wide_rows == 1 << 30)
    assert (level[:mixed.rows] == 0).sum() == sum(c for c in per.values() if c < wide_rows)     # lane islands carry level 0
    print(f"wide_rows {wide_rows}: {wide} of {len(per)} islands wide, {int(level.max())} levels at most")


# ------------------------------------------------------------------------------------------------- 2, 3: one island
@pytest.fixture(scope="module")
def pile(cuda_device):
    return Case(spheres(grid_positions(289, 17), cuda_device))


def test_a_pile_has_levels_wider_than_the_workgroup(pile):
    assert len(pile.per_island) == 1 and 2400 <= pile.rows <= 2600
    level = pile.both()
    width = np.bincount(level)
    assert width[1] == width[2] == width[3] == 289                          # the floor contacts' normal and friction rows: > 256
    print(f"{pile.rows} rows, {len(width) - 1} levels, widest {int(width.max())}")


@pytest.fixture(scope="module")
def stack(cuda_device):
    pos = np.stack([np.full(32, 2.0), 0.78 + 0.5 * np.arange(32), np.full(32, 2.0)], 1)
    return Case(spheres(pos, cuda_device))


def test_a_stack_has_narrow_levels(stack):
    """every sphere touches the one below and the one above: neighbouring contacts share a body, so a level holds at
    most every other contact (16 rows) and a contact's three rows follow each other; listed bottom-up it is one or two
    rows a level"""
    assert len(stack.per_island) == 1 and stack.rows == 3 * 32
    level = stack.both()
    width = np.bincount(level)[1:]
    print(f"{stack.rows} rows, {len(width)} levels, widths {width.tolist()}")
    assert width.max() <= 16 and len(width) >= 6


# ------------------------------------------------------------------------------------------------- 4: more islands than workgroups
def test_more_wide_islands_than_workgroups(cuda_device):
    n = WIDE_WORKGROUPS + 300
    case = Case(spheres(grid_positions(n, 37, pitch=1.0), cuda_device))
    assert len(case.per_island) == n and set(case.per_island.values()) == {3}
    level = case.both()
    assert case.run(1)["wide_total"] == n
    assert np.bincount(level).tolist() == [0, n, n, n]


# ------------------------------------------------------------------------------------------------- 5: rows that do not fit
def test_rows_that_do_not_fit_and_absent_lists(stack):
    w, k = stack.w, stack.rows
    before = stack.snap
    got = stack.run(1, capacity=k - 1)
    assert got["status"] & 1 and got["rows_total"] == k and got["wide_total"] == 0 and not got["row_level"].any()
    assert same_bits(got["lvel"], before["lvel"].cpu().numpy()[:w.n]) and same_bits(got["avel"], before["avel"].cpu().numpy()[:w.n])
    # rows_capacity 0 (the wrapper reads 0 as "the default": the library itself is asked): any row is one too many
    for t in (w.solve_status, w.rows_total, w.wide_total):
        t.fill_(0 if t is w.solve_status else -1)
    lists = [w.static_pairs.data_ptr(), w.static_pair_total.data_ptr(), w.static_capacity, w.static_contact2_buf.data_ptr(),
             None, None, None, 0, w.pairs.data_ptr(), w.pair_total.data_ptr(), w.capacity, w.contact2_buf.data_ptr()]
    head = [physics._stream(), C.byref(w._desc), C.byref(w.world), C.byref(w.solver), H, w.island.data_ptr()]
    rc = _lib.lib().clapgpu_bodies_solve(*head, *lists, 0, w.solve_scratch.data_ptr(), None, None, w.rows_total.data_ptr(),
                                         w.solve_status.data_ptr(), w.row_level.data_ptr(), w.wide_total.data_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.OK and int(w.solve_status.item()) & 1 and int(w.rows_total.item()) == k and int(w.wide_total.item()) == 0
    assert same_bits(w.lvel.cpu().numpy(), before["lvel"].cpu().numpy()) and same_bits(w.avel.cpu().numpy(), before["avel"].cpu().numpy())
    got = stack.run(1, capacity=k)                                          # exactly enough
    stack.check(got, 1)
    # no list at all
    base.restore(w, before)
    w.rows_total.fill_(-1)
    w.wide_total.fill_(-1)
    w.row_level.fill_(-1)
    args = [physics._stream(), C.byref(w._desc), C.byref(w.world), C.byref(w.solver), H, w.island.data_ptr(), None, None, 0,
            None, None, None, None, 0, None, None, 0, None, w.solve_rows_capacity, w.solve_scratch.data_ptr(), None, None,
            w.rows_total.data_ptr(), w.solve_status.data_ptr(), w.row_level.data_ptr(), w.wide_total.data_ptr()]
    L = _lib.lib()
    assert L.clapgpu_bodies_solve(*args) == _lib.OK
    torch.cuda.synchronize()
    assert int(w.rows_total.item()) == 0 and int(w.wide_total.item()) == 0 and int(w.solve_status.item()) == 0
    assert not w.row_level[:w.solve_rows_capacity].any().item()
    assert same_bits(w.lvel.cpu().numpy(), before["lvel"].cpu().numpy()) and same_bits(w.avel.cpu().numpy(), before["avel"].cpu().numpy())
    bad = lambda i, v: args[:i] + [v] + args[i + 1:]
    assert L.clapgpu_bodies_solve(*bad(24, w.row_level.data_ptr() + 2)) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_bodies_solve(*bad(25, w.wide_total.data_ptr() + 1)) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_bodies_solve(*bad(19, None)) == _lib.ERR_INVALID_ARGUMENTS              # scratch
    # the scratch grows with the rows, the wide path's 28 bytes a row and 4 a body in it, whatever wide_rows is
    sizes = [_lib.bodies_solve_scratch_bytes(1000, r) for r in (0, 1, 33, 1000, 4096, 100_000, 1 << 20)]
    assert all(sizes) and sizes == sorted(sizes)
    assert sizes[3] >= 1000 * (240 + 8 + 8 + 8 + 28) + 1000 * (48 + 4 + 4)


# ------------------------------------------------------------------------------------------------- 6: the scratch, the graph
def test_wide_solve_stays_inside_its_scratch_and_replays_from_a_graph(pile):
    """a scratch of exactly clapgpu_bodies_solve_scratch_bytes and exactly the rows, 0xA5 behind it"""
    w, k = pile.w, pile.rows
    try:
        scratch, tail = guarded_scratch(_lib.bodies_solve_scratch_bytes(w.n, k), w.device)
        got = pile.run(1, capacity=k, scratch=scratch)
        assert (tail == 0xA5).all().item(), ("written past the scratch", torch.nonzero(tail != 0xA5)[:8].flatten().tolist())
        pile.check(got, 1)
        graph = torch.cuda.CUDAGraph()
        base.restore(w, pile.snap)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph):
            w.solve(H, want_lambda=True, want_levels=True)
        for _ in range(2):
            base.restore(w, pile.snap)
            w.row_lambda.fill_(-1.0)
            w.row_level.fill_(-1)
            w.wide_total.fill_(-1)
            graph.replay()
            pile.check(pile.result(), 1)
        assert (tail == 0xA5).all().item()
    finally:
        w.solve_scratch = None                                              # the next alloc_solve makes all of it anew


# ------------------------------------------------------------------------------------------------- 7: the frame
def test_frame_follows_wide_rows(cuda_device):
    worlds = []
    for wide_rows in (1, 0):
        _b, w, loop = base.frame_world(cuda_device, True)
        w.alloc_solve()
        w.solver.wide_rows = wide_rows
        loop._issue(0.0, 2)
        torch.cuda.synchronize()
        assert int(w.solve_status.item()) == 0
        worlds.append(w)
    base.assert_same_world(worlds[0], worlds[1], "two substeps with wide_rows 1 and 0")
    _b, plain, loop0 = base.frame_world(cuda_device, False)
    loop0._issue(0.0, 2)
    assert not same_bits(plain.download()["lvel"], worlds[0].download()["lvel"])                 # and it is the solve that acts
