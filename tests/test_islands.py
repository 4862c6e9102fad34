"""CPU: the restatement of the island pass (tests/islandref.py) against a breadth-first search and against pushref's
step, and the ABI the pass added."""
from collections import deque

import numpy as np

from clap_amd import _lib, synth
import islandref as ir
import pushref as pr

H = 1.0 / 120.0


def bfs_components(n, pairs, nc):
    adj = [[] for _ in range(n)]
    for (a, b), c in zip(pairs, nc):
        a, b = int(a), int(b)
        if (int(c) & 0x7fffffff) >= 1 and a < n and b < n and a != b:
            adj[a].append(b)
            adj[b].append(a)
    out = np.full(n, -1, np.int64)
    for s in range(n):                                                     # ascending: s is the smallest of what it reaches
        if out[s] >= 0:
            continue
        out[s] = s
        q = deque([s])
        while q:
            x = q.popleft()
            for y in adj[x]:
                if out[y] < 0:
                    out[y] = s
                    q.append(y)
    return out.astype(np.uint32)


def test_components_against_bfs_on_random_graphs():
    R = np.random.Generator(np.random.PCG64(12))
    seen_multi = 0
    for g in range(200):
        n = int(R.integers(1, 301))
        m = int(R.integers(0, 2 * n + 1))
        pairs = R.integers(0, n, (m, 2)).astype(np.uint32)                 # self pairs come by themselves
        if m:
            dup = R.integers(0, m, m // 4)
            pairs = np.concatenate([pairs, pairs[dup], pairs[dup][:, ::-1]])   # duplicates, some reversed
            bad = R.random(len(pairs)) < 0.05
            pairs[bad, int(R.integers(0, 2))] = n + R.integers(0, 5, int(bad.sum()))   # out of range
            pairs[R.random(len(pairs)) < 0.02] = 0xffffffff
        nc = R.choice(np.array([0, 1, 2, ir.CONTACT_DEEP, ir.CONTACT_DEEP | 1], np.uint32), len(pairs),
                      p=[0.25, 0.4, 0.2, 0.1, 0.05])
        got = ir.components(n, pairs, nc)
        want = bfs_components(n, pairs, nc)
        assert np.array_equal(got, want), g
        assert (got <= np.arange(n)).all() and (got[got] == got).all()
        seen_multi += int((np.bincount(got, minlength=n) > 2).any())
    assert seen_multi >= 100


def test_components_total_and_capacity_cut_the_list():
    pairs = np.array([[0, 1], [1, 2], [2, 3]], np.uint32)
    nc = np.ones(3, np.uint32)
    assert ir.components(4, pairs, nc).tolist() == [0, 0, 0, 0]
    assert ir.components(4, pairs, nc, total=2).tolist() == [0, 0, 0, 3]
    assert ir.components(4, pairs, nc, total=9, capacity=1).tolist() == [0, 0, 2, 3]


def test_seed_then_step_without_joints_is_the_step():
    """nobody asleep, nobody falling asleep: the seed's bookkeeping followed by a step that finds no HAS_JOINT gives what
    the step alone gives, counters included"""
    n = 500
    b = synth.capsule_bodies(n, box=12.0, seed=21, resting_frac=0.3)
    b["adis_steps_left"][:] = np.random.Generator(np.random.PCG64(2)).integers(2, 30, n)
    b["bflags"][::2] |= pr.HAS_JOINT
    assert not (b["bflags"] & pr.DISABLED).any()
    alone, split = pr.step_state(b), pr.step_state(b)
    pr.step_forces(b, alone, H)
    ir.seed(split, pr.WORLD, H)
    assert not (split["bflags"] & (pr.HAS_JOINT | pr.DISABLED)).any()
    assert (split["adis_steps_left"] != b["adis_steps_left"]).any()       # the seed did the bookkeeping
    pr.step_forces(b, split, H)
    for k in alone:
        assert np.array_equal(alone[k].view(np.uint8), split[k].view(np.uint8)), k


def test_seed_puts_to_sleep_and_wake_clears_the_flag_alone():
    n = 6
    b = synth.capsule_bodies(n, box=4.0, seed=3, resting_frac=1.0)
    b["lvel"][:] = b["avel"][:] = 0
    b["bflags"][:] |= pr.HAS_JOINT | pr.AUTO_DISABLE
    b["adis_steps_left"][:] = 1
    b["lvel"][5] = [3.0, 0, 0]                                             # 5 moves: its counters are reset
    st = pr.step_state(b)
    island, woken = ir.islands(st, [[0, 1], [1, 5], [2, 3]], [1, 2, 1])
    assert island.tolist() == [0, 0, 2, 2, 4, 0] and woken == 2
    assert (st["bflags"] & pr.DISABLED).astype(bool).tolist() == [False, False, True, True, True, False]
    assert st["adis_steps_left"].tolist() == [0, 0, 0, 0, 0, 30] and not st["lvel"][:5].any()
    assert not (st["bflags"] & pr.HAS_JOINT).any()


def test_abi_and_frame_descriptor():
    assert _lib.ABI_VERSION >= 37
    assert {"island_scratch", "island", "island_woken"} <= {f[0] for f in _lib.FrameDesc._fields_}
    assert "clapgpu_bodies_islands" in _lib.SYMBOLS and "clapgpu_bodies_islands_scratch_bytes" in _lib.SYMBOLS
