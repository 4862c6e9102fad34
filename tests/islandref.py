"""The island pass of dWorldQuickStep (ODE 0.16 util.cpp, dxProcessIslands) restated in numpy: what
clapgpu_bodies_islands is compared with, bit for bit.  seed() is the auto-disable bookkeeping of pushref's step (taken
from it, not written again), components() a plain sequential union-find, wake() the flag alone.  Nothing here imports
the device code.  ODE is absent from the reference: PARITY UNPINNED like the rest of the rigid-body block."""
import numpy as np

import pushref as pr

DISABLED, AUTO_DISABLE, HAS_JOINT = pr.DISABLED, pr.AUTO_DISABLE, pr.HAS_JOINT
CONTACT_DEEP = 0x80000000


def seed(st, world=pr.WORLD, h=1.0 / 120.0):
    """dInternalHandleAutoDisabling of every enabled body with the flag and a joint, then HAS_JOINT cleared on EVERY body.
    pushref's step does that bookkeeping before it integrates and writes nothing but bflags, the counters and the
    velocities of a body it puts to sleep: run on a copy, those are taken over.  st is changed in place."""
    n = len(st["bflags"])
    b = dict(n=n, mass=np.ones(n), adis_average_samples=1)
    tmp = {k: np.array(v) for k, v in st.items() if k in ("pos", "quat", "lvel", "avel", "bflags", "adis_steps_left",
                                                          "adis_time_left")}
    tmp["bflags"] = tmp["bflags"].astype(np.uint32)
    tmp["facc"] = np.zeros((n, 3))
    before = tmp["bflags"].copy()
    pr.step_forces(b, tmp, h, world)
    slept = ((tmp["bflags"] & DISABLED) != 0) & ((before & DISABLED) == 0)
    st["adis_steps_left"][:] = tmp["adis_steps_left"]
    st["adis_time_left"][:] = tmp["adis_time_left"]
    st["lvel"][slept] = 0
    st["avel"][slept] = 0
    st["bflags"][slept] |= np.uint32(DISABLED)
    st["bflags"][:] &= ~np.uint32(HAS_JOINT)
    return slept


def components(n, pairs, nc, total=None, capacity=None):
    """island[i] = the smallest index of i's component.  Pair k < min(total, capacity) links when nc[k] without the DEEP
    bit is at least 1; self pairs and pairs with an index >= n are ignored."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    k_max = len(pairs) if total is None else min(int(total), len(pairs))
    if capacity is not None:
        k_max = min(k_max, int(capacity))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for k in range(k_max):
        if (int(nc[k]) & ~CONTACT_DEEP & 0xffffffff) < 1:
            continue
        a, b = int(pairs[k, 0]), int(pairs[k, 1])
        if a >= n or b >= n or a == b or a < 0 or b < 0:
            continue
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)], np.uint32)


def wake(st, island):
    """a DISABLED body whose component holds an enabled body loses the flag; nothing else changes.  Returns the count."""
    fl = st["bflags"]
    awake = np.zeros(len(fl), bool)
    awake[island[(fl & DISABLED) == 0]] = True
    w = ((fl & DISABLED) != 0) & awake[island]
    fl[w] &= ~np.uint32(DISABLED)
    return int(w.sum())


def islands(st, pairs, nc, world=pr.WORLD, h=1.0 / 120.0, total=None, capacity=None):
    """seed, components, wake: (island, woken)"""
    seed(st, world, h)
    island = components(len(st["bflags"]), pairs, nc, total, capacity)
    return island, wake(st, island)
