"""Chosen inputs for the pose kernel (clap_amd/csrc/pose.hip, pose_math_dev.h, pose_pack.hip): frame times on and beside
every key, channel lengths on both sides of every size at which the key search or the launch decides, and rotation key
pairs whose inner product sits on the slerp's thresholds.

Key grids.  All channels of one length share one grid of strictly increasing float32 key times (and one entry of the
times pool), so a single character time lands on a key of every channel of that length at once.  Lengths are spread
over the joints so that neighbouring joints and the three paths of one joint differ (wherever the model has three
lengths to choose from): a lane's three searches end at different `lo`.  The first key is above 0 and the last one
below time_end.  The longest grid of a model holds two keys that are adjacent floats.

Frame times, per model: every key of every grid, the float below and the float above it, one time inside every interval,
one below the first and one above the last key of every grid, 0, time_end, -inf and +inf, shuffled.  No NaN (the
reference's answer for it depends on its search cursor).  Every animation of the model plays every time: character i
plays animation i % n_anims at times[i // n_anims].

Models: both sides of every size decision -- the search's row count kp (a power of two above the longest channel), and
key times staged in LDS or read through L2 -- see MODELS.  A separate model (slerp_edges) carries the rotation pairs.

Everything is built on the CPU, is deterministic, and uses no GPU.  tests/test_pose_edges.py checks that the cases are
what they claim.
"""
import functools

import numpy as np

from clap_amd import synth

F32 = np.float32
INF = F32(np.inf)
TIME_END = F32(2.0)


# ------------------------------------------------------------------------------------------------- the size rules
# PosePack::of (clap_amd/csrc/pose_pack.h:34-39), pose_lanes (pose_pack.h:29) and clapgpu_pose_update's
# `times_lds = lay.head_floats() <= POSE_TIMES_LDS_MAX * (lay.lanes / 64)` (pose.hip:655, pose_pack.h:41-47, pose.hip:56),
# restated once
POSE_TIMES_LDS_MAX = 6400


def pose_kp(max_keys):
    kp = 2
    while kp <= max_keys:
        kp <<= 1
    return kp


def pose_lanes(nr_joints):
    return (nr_joints + 63) // 64 * 64


def times_lds_rule(n_anims, kp, nr_joints):
    lanes = pose_lanes(nr_joints)
    head_floats = n_anims * 3 * kp * lanes + n_anims * 3 * lanes
    return head_floats <= POSE_TIMES_LDS_MAX * (lanes // 64)


def program_passes_wanted(n_levels, nr_joints):
    """pose_launch's `want` (pose.hip:567).  Where the program does not fit beside the key times in LDS the launch takes
    the times through L2 (pose.hip:570-571): what the 256-lane kernel always does."""
    q = pose_lanes(nr_joints) // 4
    return n_levels + (nr_joints + q - 1) // q + 1


# ------------------------------------------------------------------------------------------------- the models
def lengths_up_to(longest):
    """1, 2, 3 and every 2^m - 1, 2^m, 2^m + 1 up to the longest channel, and the longest"""
    s = {1, 2, 3, longest}
    m = 2
    while (1 << m) - 1 <= longest:
        s.update(((1 << m) - 1, 1 << m, (1 << m) + 1))
        m += 1
    return tuple(sorted(k for k in s if k <= longest))


def anim_longest(n_anims, longest):
    """The longest channel of each animation of a model: they differ as far as `longest` leaves room"""
    return tuple(longest - a % longest for a in range(n_anims))


# name: (n_anims, longest channel, joints, missing channels, times in LDS as the head_floats rule gives it)
MODELS = {}
for _k in (1, 3, 7, 8, 31, 32, 63, 64, 127):                                  # the search's sizes: kp 2 .. 128
    MODELS[f"search_{_k}"] = (1, _k, 64, False, _k <= 31)
for _n, _k, _lds in ((2, 7, True), (2, 8, False), (4, 3, True), (4, 4, False), (11, 1, True), (12, 1, False)):
    MODELS[f"anims_{_n}x{_k}"] = (_n, _k, 64, False, _lds)                    # n_anims * (kp + 1) <= 33 and above
MODELS["missing_lds"] = (2, 7, 64, True, True)
MODELS["missing_l2"] = (1, 32, 64, True, False)
for _j in (100, 200):                                                         # 128 and 256 lanes per character
    MODELS[f"search_31_{_j}j"] = (1, 31, _j, False, True)
    MODELS[f"search_64_{_j}j"] = (1, 64, _j, False, False)
    MODELS[f"anims_2x7_{_j}j"] = (2, 7, _j, False, True)
MODELS["search_31_150j"] = (1, 31, 150, False, True)                          # 192 lanes
MODELS["slerp_edges"] = (1, 5, 64, False, True)
CASE_NAMES = tuple(MODELS)


def grid(k, time_end=TIME_END, adjacent=False):
    """k strictly increasing float32 key times inside (0, time_end); with `adjacent`, keys (k - 1) // 2 and the one after
    it are adjacent floats"""
    rng = np.random.Generator(np.random.PCG64(7000 + k))
    t = (0.05 + 0.9 * (np.arange(k) + 0.1 + 0.8 * rng.uniform(0, 1, k)) / k) * float(time_end)
    t = t.astype(F32)
    if adjacent and k >= 2:
        m = (k - 1) // 2
        t[m + 1] = np.nextafter(t[m], INF)
    assert (t[1:] > t[:-1]).all() and t[0] > 0 and t[-1] < time_end
    return t


def frame_times(grids, time_end=TIME_END, seed=1):
    """The list of the module docstring for these grids, as float32, each value once, shuffled"""
    out = [F32(0.0), F32(time_end), -INF, INF]
    for t in grids.values():
        out += list(t) + list(np.nextafter(t, -INF)) + list(np.nextafter(t, INF))
        mid = ((t[1:].astype(np.float64) + t[:-1]) / 2).astype(F32)
        out += list(mid[(mid > t[:-1]) & (mid < t[1:])])                      # nothing lies inside the adjacent pair
        out += [F32(t[0] / 2), F32((float(t[-1]) + float(time_end)) / 2)]
    bits = np.unique(np.asarray(out, F32).view(np.uint32))
    times = bits.view(F32).copy()
    np.random.Generator(np.random.PCG64(seed)).shuffle(times)
    return times


def bracket_kinds(t, time):
    """What the time is to the keys t of one channel: the names the coverage test and the mismatch message use"""
    k, kinds = len(t), []
    on = np.flatnonzero(t == time)
    if time < t[0]:
        kinds.append("before the first key")
    if time > t[-1]:
        kinds.append("past the last key")
    for i in on:
        kinds.append("on the first key" if i == 0 else "on the last key" if i == k - 1 else f"on interior key {i}")
    for i in np.flatnonzero(np.nextafter(t, INF) == time):
        kinds.append(f"one float above key {i}")
    for i in np.flatnonzero(np.nextafter(t, -INF) == time):
        kinds.append(f"one float below key {i}")
    if not kinds:
        kinds.append(f"inside interval {int(np.searchsorted(t, time)) - 1}")
    return tuple(kinds)


def _quats(rng, k):
    ang = rng.uniform(-1.2, 1.2, (k, 3))
    d = synth.quat_from_euler_xyz(ang[:, 0], ang[:, 1], ang[:, 2]).astype(F32)
    flip = rng.uniform(0, 1, k) < 0.3                                         # inner products below 0
    d[flip] = -d[flip]
    near = rng.uniform(0, 1, k) < 0.1                                         # equal neighbours: inner product 1
    d[1:][near[1:]] = d[:-1][near[1:]]
    return d


def _values(rng, path, k):
    if path == 1:
        return _quats(rng, k)
    return (rng.uniform(-0.5, 0.5, (k, 3)) if path == 0 else rng.uniform(0.8, 1.25, (k, 3))).astype(F32)


def _animation(J, chan_len, grids, time_end, rng, fixed=None):
    """One animation in the layout of synth.animation.  chan_len[j][p]: keys of (joint, path), 0 = no channel; every
    channel of a length points at that length's one grid in the times pool.  fixed[(j, p)]: key values given."""
    t_off, pool, at = {}, [], 0
    for k in sorted(grids):
        t_off[k] = at
        pool.append(grids[k])
        at += k
    tgt, path, nr, toff, doff, data, d_at = [], [], [], [], [], [], 0
    for j in range(J):
        for p in range(3):
            k = int(chan_len[j][p])
            if not k:
                continue
            d = fixed[(j, p)] if fixed and (j, p) in fixed else _values(rng, p, k)
            assert d.shape == (k, 4 if p == 1 else 3) and d.dtype == F32
            tgt.append(j); path.append(p); nr.append(k); toff.append(t_off[k]); doff.append(d_at)
            data.append(d.ravel())
            d_at += d.size
    return dict(n_channels=len(tgt), ch_target=np.asarray(tgt, np.uint32), ch_path=np.asarray(path, np.uint32),
                ch_nr=np.asarray(nr, np.uint32), ch_time_off=np.asarray(toff, np.uint32),
                ch_data_off=np.asarray(doff, np.uint32), times=np.concatenate(pool).astype(F32),
                data=np.concatenate(data).astype(F32), time_end=F32(time_end))


def spread(J, lengths, shift=0):
    """chan_len[j][p]: neighbouring joints and the three paths of a joint get different lengths (given three to choose from)"""
    n = len(lengths)
    return np.asarray([[lengths[(j + p + shift) % n] for p in range(3)] for j in range(J)], np.int32)


def _finish(name, sk, anims, chan_len, grids, time_end, adjacent, seed, extra=None):
    J, n_anims = sk["nr_joints"], len(anims)
    times = frame_times(grids, time_end, seed)
    n = n_anims * len(times)
    ch = synth.characters(n, J, seed=seed)
    longest = int(max(cl.max() for cl in chan_len))
    kp = pose_kp(longest)
    c = dict(name=name, sk=sk, anims=anims, n_anims=n_anims, J=J, n_chars=n, times=times,
             which=(np.arange(n) % n_anims).astype(np.int32), t=times[np.arange(n) // n_anims].copy(),
             trs0=ch["trs0"], char_mx=ch["char_mx"], chan_len=chan_len, grids=grids, time_end=F32(time_end),
             longest=longest, kp=kp, lanes=pose_lanes(J), times_lds=times_lds_rule(n_anims, kp, J),
             missing=bool(any((cl == 0).any() for cl in chan_len)), adjacent=adjacent)
    c.update(extra or {})
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(sk, anims, which, t, trs0, char_mx, ...) of one model of MODELS: what animation.SkinnedModel / CharacterBatch and
    ob.pose take, with the model's grids, its channel lengths chan_len[anim][joint][path] and the sizes the rules give"""
    if name == "slerp_edges":
        return _slerp_case()
    n_anims, longest, J, missing, _lds = MODELS[name]
    seed = 500 + CASE_NAMES.index(name)
    rng = np.random.Generator(np.random.PCG64(seed))
    sk = synth.skeleton(J, 6 if J <= 64 else 8, seed=seed)
    per_anim = anim_longest(n_anims, longest)
    grids = {k: grid(k, adjacent=(k == longest)) for k in lengths_up_to(longest)}
    for la in per_anim:
        for k in lengths_up_to(la):
            grids.setdefault(k, grid(k))
    chan_len = []
    for a, la in enumerate(per_anim):
        cl = spread(J, lengths_up_to(la), shift=a)
        if missing:
            # every eighth joint: a path without a channel beside a one-key path and a longest path, in all three rotations;
            # joint 5 has no channel at all, joint 13 a single one
            for j in range(3, J, 8):
                r = (j // 8 + a) % 3
                cl[j, r], cl[j, (r + 1) % 3], cl[j, (r + 2) % 3] = 0, 1, la
            cl[5] = 0
            cl[13] = (0, la, 0)
        chan_len.append(cl)
    anims = [_animation(J, cl, {k: grids[k] for k in set(cl.ravel()) - {0}}, TIME_END, rng) for cl in chan_len]
    return _finish(name, sk, anims, chan_len, grids, TIME_END, (longest, (longest - 1) // 2) if longest >= 2 else None, seed)


# ------------------------------------------------------------------------------------------------- slerp edges
# quat_slerp (oracle/lm.h:280-303) decides twice on dot = quat_inner_product(a, b): `dot < 0.0` (negate b) and
# `dot > 0.9995` (normalised lerp, no acos), both against double literals.  With a = (0, 0, 0, 1) and b = (s, 0, 0, c)
# the float sum 0 + s*0 + 0*0 + 0*0 + c*1 is c exactly (a -0 becomes the +0 the sum opens with).
C9995 = F32(0.9995)                              # below the double 0.9995: NOT above the literal
TINY, DENORMAL = F32(np.finfo(np.float32).tiny), F32(1.0e-41)
# (c, the branch the reference takes, b negated)
SLERP_C = (
    (C9995, "acos", False), (np.nextafter(C9995, F32(2)), "nlerp", False),
    (F32(1.0), "nlerp", False), (np.nextafter(F32(1), F32(0)), "nlerp", False),
    (F32(0.0), "acos", False), (F32(-0.0), "acos", False),
    (TINY, "acos", False), (-TINY, "acos", True), (DENORMAL, "acos", False), (-DENORMAL, "acos", True),
    (-C9995, "acos", True), (np.nextafter(-C9995, F32(-2)), "nlerp", True),
    (F32(-1.0), "nlerp", True),
    (np.nextafter(C9995, F32(0)), "acos", False), (np.nextafter(F32(0), F32(1)), "acos", False),
    (np.nextafter(F32(0), F32(-1)), "acos", True), (F32(0.5), "acos", False),
)
UNIT_A = np.asarray([0, 0, 0, 1], F32)


def unit_b(c):
    return np.asarray([np.sqrt(max(0.0, 1.0 - float(c) ** 2)), 0, 0, c], F32)


def slerp_pairs():
    """[(a, b, branch, negated, what)]: the pairs of SLERP_C, then the pairs that are not unit quaternions"""
    out = [(UNIT_A, unit_b(c), br, neg, f"c = {float(c)!r}") for c, br, neg in SLERP_C]
    out.append((F32(2) * UNIT_A, F32(0.4) * unit_b(F32(0.75)), "acos", False, "2a with 0.4b, c = 0.75"))
    out.append((F32(2) * UNIT_A, UNIT_A.copy(), "nlerp", False, "inner product 2"))
    return out


SLERP_TIME_END = F32(3.0)
SLERP_GRID2 = np.asarray([0.5, 1.5], F32)                 # a time of 1.0 is fac 0.5 exactly
SLERP_GRID3 = np.asarray([0.5, 1.5, 2.5], F32)


def _slerp_case():
    """64 joints.  Joint q < len(pairs): a two-key rotation channel (a, b) of pair q.  The next joints: three-key rotation
    channels (b of pair 2r, a, b of pair 2r + 1) -- both intervals have the pairs' inner products, the wrap's is whatever
    the two b give.  The other joints and paths carry ordinary random channels of 1 to 5 keys."""
    J, seed = 64, 900
    rng = np.random.Generator(np.random.PCG64(seed))
    pairs = slerp_pairs()
    unit = [q for q, p in enumerate(pairs) if p[0] is UNIT_A]                # indices of the unit pairs
    grids = {1: grid(1, SLERP_TIME_END), 2: SLERP_GRID2, 3: SLERP_GRID3, 4: grid(4, SLERP_TIME_END),
             5: grid(5, SLERP_TIME_END, adjacent=True)}
    cl = spread(J, (1, 2, 3, 4, 5))
    fixed, rot_pairs = {}, {}
    for q, (a, b, *_r) in enumerate(pairs):
        cl[q, 1] = 2
        fixed[(q, 1)] = np.stack([a, b]).astype(F32)
        rot_pairs[q] = [(0, q)]                                              # interval 0 of joint q is pair q
    for r in range(len(unit) // 2):
        j = len(pairs) + r
        cl[j, 1] = 3
        fixed[(j, 1)] = np.stack([pairs[unit[2 * r]][1], UNIT_A, pairs[unit[2 * r + 1]][1]]).astype(F32)
        rot_pairs[j] = [(0, unit[2 * r]), (1, unit[2 * r + 1])]
    assert len(pairs) + len(unit) // 2 <= J
    sk = synth.skeleton(J, 6, seed=seed)
    an = _animation(J, cl, grids, SLERP_TIME_END, rng, fixed)
    return _finish("slerp_edges", sk, [an], [cl], grids, SLERP_TIME_END, (5, 2), seed,
                   extra=dict(pairs=pairs, rot_pairs=rot_pairs))


def frames(c):
    """The two frames every case runs: its times, then the list rotated by one character (stored T / R / S of paths without
    a channel carry over)"""
    return [(c["t"], c["which"]), (np.roll(c["t"], 1), c["which"])]


def channel_times(c, a, j, p):
    k = int(c["chan_len"][a][j][p])
    return c["grids"][k] if k else None


PATHS = ("T", "R", "S")


def first_difference(c, f, t, out, trs, jt, jp, reach, trs_on):
    """Names the model, the character's time, the joint, the path and the bracket kind of the first differing value"""
    u = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    if trs_on:
        bad = np.argwhere(u(out["trs"]) != u(trs))
        if bad.size:
            i, j, comp = (int(x) for x in bad[0])
            p = 0 if comp < 3 else 1 if comp < 7 else 2
            a = int(c["which"][i])
            g = channel_times(c, a, j, p)
            kind = "no channel: the stored value" if g is None else f"{len(g)} keys, " + ", ".join(bracket_kinds(g, t[i]))
            lo = (0, 3, 7)[p]
            return (f"model {c['name']} frame {f}: character {i} (animation {a}) at time {t[i]!r}, joint {j}, path {PATHS[p]}: "
                    f"{kind}; kernel {out['trs'][i, j, lo:lo + (4 if p == 1 else 3)]!r}, oracle {trs[i, j, lo:lo + (4 if p == 1 else 3)]!r}")
    for what, got, exp in (("joint_transforms", out["joint_transforms"], jt), ("joint_pos", out["joint_pos"], jp)):
        bad = np.argwhere(u(got[:, reach]) != u(exp[:, reach]))
        if bad.size:
            i, j = int(bad[0][0]), int(reach[int(bad[0][1])])
            return (f"model {c['name']} frame {f}: character {i} (animation {int(c['which'][i])}) at time {t[i]!r}, joint {j}: "
                    f"{what} differs" + ("" if trs_on else " (T / R / S not written in this run)"))
    return f"model {c['name']} frame {f}"
