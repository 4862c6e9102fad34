"""CPU: the chosen pose cases of tests/posecases.py are what they claim.  Conditions on the INPUTS, checked with the oracle
and with Python restatements of the two bracket rules; no kernel runs here (tests/test_pose_edges_gpu.py does that).

  * the kernel's stated rule -- lo = #{t[k] < time} by the probe steps kp/2 .. 1 over rows padded with +INF, then finish()
    (clap_amd/csrc/pose.hip:94-124) -- gives the (prev, next, fac) bits of channel_time_to_idx WITH its cursor
    (oracle/pose.c:15-33, 51-57) for every channel of every character of every case, both frames;
  * every bracket kind occurs for every channel length of every model, and the models have the sizes they were built for;
  * five wrong rules each change a bracket on every model they can affect: the cases can fail;
  * a wrong bracket on a key is invisible in T and S (lerp(a, b, 1) and lerp(b, c, 0) are both b) and visible in R where
    slerp(a, b, 1) differs from b in bits -- the share of such results is measured with the oracle and held above 1 in 4;
  * the slerp pairs take the branches they were built for.
"""
import functools

import numpy as np
import pytest

import posecases as pc
from oracle import binding as ob

F32 = np.float32


# ------------------------------------------------------------------------------------------------- the two rules
def reference_brackets(t, times, cursor=0):
    """oracle/pose.c:15-33 time_to_idx and the cursor update of pose.c:52, for one channel with keys t over a sequence of
    frame times; fac as pose.c:53-57.  Returns (prev, next, fac, the cursor afterwards)."""
    nr, tl = len(t), [float(x) for x in t]
    prev, nxt = np.zeros(len(times), np.int32), np.zeros(len(times), np.int32)
    for q, time in enumerate(float(x) for x in times):
        start = cursor
        tail = time < tl[0]
        if not tail:
            if time < tl[start]:
                start = 0
            i = start
            while i < nr and time > tl[i]:
                i += 1
            tail = i == nr
        if tail:
            p, n = nr - 1, 0
        else:
            p = max(i - 1, 0)
            n = min(p + 1, nr - 1)
        prev[q], nxt[q] = p, n
        cursor = min(p, n)
    times = np.asarray(times, F32)
    pt, nt = t[prev], t[nxt]
    with np.errstate(invalid="ignore", divide="ignore"):
        quot = ((times - pt) / (nt - pt)).astype(F32)
    fac = np.where(pt > nt, np.where(times < nt, F32(1), F32(0)), np.where(pt < nt, quot, F32(0))).astype(F32)
    return prev, nxt, fac, cursor


WRONG_RULES = ("t <= time", "no top probe step", "wrap without time < tp", "outside always 0", "next not clamped")


def kernel_brackets(t, kp, times, wrong=None):
    """pose_gather_keys' search and finish() (pose.hip:94-124) for one channel: rows [kp], +INF past the last key"""
    nr = len(t)
    assert kp > nr and kp & (kp - 1) == 0
    rows = np.full(kp + 1, np.inf, F32)                    # (+ a row for the unclamped wrong rule's read)
    rows[:nr] = t
    times = np.asarray(times, F32)
    lo = np.zeros(len(times), np.int32)
    step = kp >> (2 if wrong == "no top probe step" else 1)
    while step > 0:
        a = rows[lo + step - 1]
        lo += np.where((a <= times) if wrong == "t <= time" else (a < times), step, 0).astype(np.int32)
        step >>= 1
    lo = np.minimum(lo, nr)
    pn = np.where(lo > 0, lo - 1, 0)
    nn = pn + 1 if wrong == "next not clamped" else np.where(pn + 1 < nr - 1, pn + 1, nr - 1)
    tp, tn = rows[pn], rows[nn]
    wrap = (lo == nr) | ((lo == 0) & ((times < tp) | (wrong == "wrap without time < tp")))
    with np.errstate(invalid="ignore", divide="ignore"):
        q = ((times - tp) / (tn - tp)).astype(F32)
    inside = np.where(tp < tn, q, F32(0))
    outside = np.where((lo == 0) & (nr > 1) & (wrong != "outside always 0"), F32(1), F32(0))
    prev = np.where(wrap, nr - 1, pn).astype(np.int32)
    nxt = np.where(wrap, 0, nn).astype(np.int32)
    fac = np.where(wrap, outside, inside).astype(F32)
    return prev, nxt, fac, lo


def same(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x[:2], y[:2])) and np.array_equal(x[2].view(np.uint32), y[2].view(np.uint32))


@functools.lru_cache(maxsize=None)
def _reference_cached(t_bytes, times_bytes):
    return reference_brackets(np.frombuffer(t_bytes, F32), np.frombuffer(times_bytes, F32))[:3]


def channel_runs(c):
    """(frame, animation, length, keys, the time sequence the animation's characters bring, in character order): all
    channels of one length of one animation see the same grid and the same sequence, so one run stands for them all"""
    for f, (t, which) in enumerate(pc.frames(c)):
        for a in range(c["n_anims"]):
            seq = np.ascontiguousarray(t[which == a])
            for k in sorted(set(c["chan_len"][a].ravel().tolist()) - {0}):
                yield f, a, k, c["grids"][k], seq


def reference_of(grid, seq):
    return _reference_cached(grid.tobytes(), seq.tobytes())


# ------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_kernel_rule_is_the_references_bracket(name):
    """The kernel's claim, before any GPU run: count-the-keys-below and finish() equal channel_time_to_idx, whose cursor is
    carried here from character to character (harsher than the per-character cursors of ob.pose: every start state
    occurs), as bits of (prev, next, fac)."""
    c = pc.case(name)
    runs = 0
    for f, a, k, grid, seq in channel_runs(c):
        ref = reference_of(grid, seq)
        got = kernel_brackets(grid, c["kp"], seq)
        bad = np.flatnonzero((ref[0] != got[0]) | (ref[1] != got[1]) | (ref[2].view(np.uint32) != got[2].view(np.uint32)))
        assert bad.size == 0, (f"{name} frame {f} animation {a}, channels of {k} keys, time {seq[bad[0]]!r} "
                               f"({pc.bracket_kinds(grid, seq[bad[0]])}): the reference has "
                               f"{(ref[0][bad[0]], ref[1][bad[0]], ref[2][bad[0]])}, the kernel's rule {(got[0][bad[0]], got[1][bad[0]], got[2][bad[0]])}")
        assert np.isfinite(got[2]).all() and (got[2] >= 0).all() and (got[2] <= 1).all()
        runs += 1
    assert runs >= 2 * c["n_anims"]


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_every_bracket_kind_occurs_for_every_length(name):
    c = pc.case(name)
    t, which = pc.frames(c)[0]
    for a in range(c["n_anims"]):
        seq = np.ascontiguousarray(t[which == a])
        for k in sorted(set(c["chan_len"][a].ravel().tolist()) - {0}):
            g = c["grids"][k]
            prev, nxt, fac = reference_of(g, seq)
            what = f"{name} animation {a}, {k} keys"

            def at(time):
                q = np.flatnonzero(seq.view(np.uint32) == np.asarray(time, F32).view(np.uint32))
                assert q.size == 1, f"{what}: time {time!r} is played {q.size} times"
                return int(prev[q[0]]), int(nxt[q[0]]), float(fac[q[0]])
            before = seq[seq < g[0]]
            assert (before > 0).any() and np.isneginf(before).any() and (before == 0).any(), what
            for time in before:                                            # wrap; fac 1, or 0 for a single key
                assert at(time) == (k - 1, 0, 1.0 if k > 1 else 0.0), what
            past = seq[seq > g[-1]]
            assert np.isposinf(past).any() and (past == c["time_end"]).any() and (past < c["time_end"]).any(), what
            for time in past:
                assert at(time) == (k - 1, 0, 0.0), what
            assert at(g[0]) == (0, min(1, k - 1), 0.0), what + ": on the first key"
            for i in range(1, k):                                          # on every interior key and on the last one
                assert at(g[i]) == (i - 1, i, 1.0), f"{what}: on key {i}"
            for i in range(k):                                             # one float above and below every key
                up, dn = np.nextafter(g[i], pc.INF), np.nextafter(g[i], -pc.INF)
                p, n, fc = at(up)
                if i + 1 < k and g[i + 1] == up:
                    assert (p, n, fc) == (i, i + 1, 1.0), what + ": the adjacent pair's upper key"
                else:
                    assert (p, n) == ((i, i + 1) if i + 1 < k else (k - 1, 0)) and (0.0 < fc < 1e-3 if i + 1 < k else fc == 0.0), what
                p, n, fc = at(dn)
                if i > 0 and g[i - 1] == dn:
                    assert (p, n, fc) == ((i - 2, i - 1, 1.0) if i > 1 else (0, 1, 0.0)), what + ": the adjacent pair's lower key"
                else:
                    assert (p, n) == ((i - 1, i) if i > 0 else (k - 1, 0)) and (1.0 - 1e-3 < fc <= 1.0 if i > 0 else fc == (1.0 if k > 1 else 0.0)), what   # (the quotient may round to 1)
            for i in range(k - 1):                                         # a time strictly inside every interval
                if np.nextafter(g[i], pc.INF) == g[i + 1]:
                    continue
                inside = seq[(seq > np.nextafter(g[i], pc.INF)) & (seq < np.nextafter(g[i + 1], -pc.INF))]
                got = [at(x) for x in inside]                               # (other grids' keys fall in here too)
                assert got and all(b[:2] == (i, i + 1) and 0 < b[2] <= 1 for b in got), f"{what}: interval {i}"
                assert any(0.1 < b[2] < 0.9 for b in got), f"{what}: interval {i}"
    if c["adjacent"]:
        k, m = c["adjacent"]
        g = c["grids"][k]
        assert np.nextafter(g[m], pc.INF) == g[m + 1] and any((cl == k).any() for cl in c["chan_len"])
    else:
        assert c["longest"] == 1


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_models_have_the_sizes_they_were_built_for(name):
    c = pc.case(name)
    n_anims, longest, J, missing, lds = pc.MODELS[name]
    assert (c["n_anims"], c["longest"], c["J"], c["missing"], c["times_lds"]) == (n_anims, longest, J, missing, lds)
    assert c["kp"] == pc.pose_kp(longest) and c["kp"] // 2 <= longest < c["kp"]
    assert c["times_lds"] == (n_anims * (c["kp"] + 1) <= 33)              # what the head_floats rule works out to
    assert 9 <= c["n_chars"] <= 2200 and len(np.unique(c["which"])) == n_anims
    per_anim = [int(cl.max()) for cl in c["chan_len"]]
    assert len(set(per_anim)) == min(n_anims, longest), "the animations' longest channels differ as far as there is room"
    assert not np.isnan(c["t"]).any()
    for a, cl in enumerate(c["chan_len"]):
        lengths = sorted(set(cl.ravel().tolist()) - {0})
        assert lengths == list(pc.lengths_up_to(per_anim[a])), (a, lengths)
        if len(lengths) >= 3 and not missing and name != "slerp_edges":
            assert (cl[:, 0] != cl[:, 1]).all() and (cl[:, 1] != cl[:, 2]).all() and (cl[:, 0] != cl[:, 2]).all()
            assert (cl[1:] != cl[:-1]).all()
        an = c["anims"][a]
        assert an["n_channels"] == int((cl > 0).sum())
        for ch in range(an["n_channels"]):                                 # a length's channels share its grid in the pool
            k, off = int(an["ch_nr"][ch]), int(an["ch_time_off"][ch])
            assert np.array_equal(an["times"][off:off + k], c["grids"][k])
    if missing:
        cl = c["chan_len"][0]
        assert any(sorted(r) == [0, 1, per_anim[0]] for r in cl.tolist()) and (cl == 0).all(axis=1).any()
        assert {int(np.flatnonzero(r == 0)[0]) for r in cl if sorted(r.tolist()) == [0, 1, per_anim[0]]} == {0, 1, 2}
    # the longest channel's final lo: 0, nr, and kp / 2 and kp - 1 where the channel is that long
    g = c["grids"][longest]
    lo = kernel_brackets(g, c["kp"], c["times"])[3]
    want = {v for v in (0, longest, c["kp"] // 2, c["kp"] - 1) if v <= longest}
    assert want <= set(lo.tolist()) and set(lo.tolist()) == set(range(longest + 1))


def test_the_models_stand_on_both_sides_of_every_size_decision():
    by = {(m[0], m[1]): (pc.pose_kp(m[1]), m[4]) for n, m in pc.MODELS.items() if m[2] == 64 and not m[3] and n != "slerp_edges"}
    assert by == {(1, 1): (2, True), (1, 3): (4, True), (1, 7): (8, True), (1, 8): (16, True), (1, 31): (32, True),
                  (1, 32): (64, False), (1, 63): (64, False), (1, 64): (128, False), (1, 127): (128, False),
                  (2, 7): (8, True), (2, 8): (16, False), (4, 3): (4, True), (4, 4): (8, False), (11, 1): (2, True),
                  (12, 1): (2, False)}
    assert {pc.pose_lanes(m[2]) for m in pc.MODELS.values()} == {64, 128, 192, 256}
    assert {(m[4]) for m in pc.MODELS.values() if m[3]} == {True, False}, "missing channels on both times paths"
    # the least the level program asks of a skeleton of four wavefronts: more than the 256-lane kernel's LDS leaves it
    assert min(pc.program_passes_wanted(1, J) for J in range(193, 257)) == 6


def can_affect(wrong, c):
    """`t <= time`, the wrap rules and `outside` are the same answer on a single key; without its top step a search of one
    step (kp 2) still finds a single key's only bracket; every model has one-key channels."""
    return {"t <= time": c["longest"] >= 2, "no top probe step": c["kp"] >= 4, "wrap without time < tp": c["longest"] >= 2,
            "outside always 0": c["longest"] >= 2, "next not clamped": True}[wrong]


@pytest.mark.parametrize("wrong", WRONG_RULES)
def test_the_cases_can_fail(wrong):
    for name in pc.CASE_NAMES:
        c = pc.case(name)
        changed = 0
        for f, a, k, grid, seq in channel_runs(c):
            if f == 0:
                changed += int(not same(reference_of(grid, seq), kernel_brackets(grid, c["kp"], seq, wrong)))
        assert (changed > 0) == can_affect(wrong, c), f"{name}: the rule '{wrong}' changes {changed} runs of channels"


# ------------------------------------------------------------------------------------------------- on-key results
@functools.lru_cache(maxsize=None)
def oracle_trs(name):
    """The oracle's T / R / S of the case's first frame"""
    c = pc.case(name)
    trs = np.ascontiguousarray(np.tile(c["trs0"], (c["n_chars"], 1, 1)))
    for a, an in enumerate(c["anims"]):
        sel = np.flatnonzero(c["which"] == a)
        sub = trs[sel].copy()
        ob.pose(c["sk"], an, c["t"][sel], c["char_mx"][sel], sub)
        trs[sel] = sub
    return trs


def on_key_results(c, trs):
    """(rotation results on a key >= 1 that differ from the key's own bits, of how many, the same for T and S)"""
    index = {int(b): q for q, b in enumerate(c["times"].view(np.uint32))}
    rot, lerp = [0, 0], [0, 0]
    for a, an in enumerate(c["anims"]):
        for ch in range(an["n_channels"]):
            j, p, k, off = (int(an[f][ch]) for f in ("ch_target", "ch_path", "ch_nr", "ch_data_off"))
            w = 4 if p == 1 else 3
            g = c["grids"][k]
            lo = (0, 3, 7)[p]
            for m in range(1, k):
                i = index[int(g[m].view(np.uint32))] * c["n_anims"] + a
                diff = not np.array_equal(trs[i, j, lo:lo + w].view(np.uint32), an["data"][off + w * m:off + w * m + w].view(np.uint32))
                tally = rot if p == 1 else lerp
                tally[0] += int(diff)
                tally[1] += 1
    return rot, lerp


def test_a_wrong_bracket_on_a_key_shows_in_the_rotations(capsys):
    """On key i >= 1 the reference takes (i - 1, i) with fac 1; a search that took (i, i + 1) with fac 0 would return key i's
    own value.  T and S cannot tell: lerp(a, b, 1) == b in bits.  R can wherever slerp(a, b, 1) != b in bits.

    Measured with the oracle alone (never the kernel), first frame, on-key rotation results that differ from the key's own
    bits / all of them, and the same for T and S:
        search_3 46/64 (72 %), search_7 103/170 (61 %), search_8 132/208 (63 %), search_31 322/540 (60 %),
        search_32 442/685 (65 %), search_63 600/934 (64 %), search_64 744/1176 (63 %), search_127 938/1528 (61 %),
        anims_2x7 209/334 (63 %), anims_2x8 245/383 (64 %), anims_4x3 118/160 (74 %), anims_4x4 118/193 (61 %),
        missing_lds 207/326 (63 %), missing_l2 442/689 (64 %), search_31_100j 547/858 (64 %),
        search_64_100j 1114/1774 (63 %), anims_2x7_100j 325/520 (62 %), search_31_200j 1119/1741 (64 %),
        search_64_200j 2258/3573 (63 %), anims_2x7_200j 682/1031 (66 %), search_31_150j 817/1295 (63 %),
        slerp_edges 73/112 (65 %); T and S: 0 of every model's (between 128 and 7 146 results).
    Held: at least one in four per model that has rotation channels of three or more keys."""
    lines = []
    for name in pc.CASE_NAMES:
        c = pc.case(name)
        if not any((cl[:, 1] >= 3).any() for cl in c["chan_len"]):
            continue
        rot, lerp = on_key_results(c, oracle_trs(name))
        lines.append(f"{name} {rot[0]}/{rot[1]} ({100 * rot[0] / rot[1]:.0f} %) lerp {lerp[0]}/{lerp[1]}")
        assert rot[1] >= 50 and 4 * rot[0] >= rot[1], lines[-1]
        assert lerp[0] == 0 and lerp[1] >= 100, lines[-1]
    with capsys.disabled():
        print("\non-key results that differ from the key's own bits (oracle): " + ", ".join(lines))
    assert len(lines) == len(pc.CASE_NAMES) - 3                          # all but search_1, anims_11x1 and anims_12x1


# ------------------------------------------------------------------------------------------------- slerp edges
def rot_const_branch(a, b):
    """rot_const (clap_amd/csrc/pose_pack.hip:20-42) / quat_slerp (oracle/lm.h:280-293) up to the two decisions: the float
    sum in index order from +0, the comparisons against double literals.  Returns (dot, branch, negated)."""
    dot = F32(0)
    for i in range(4):
        dot = F32(dot + F32(b[i] * a[i]))
    negated = float(dot) < 0.0
    if negated:
        dot = F32(-dot)
    return dot, ("nlerp" if float(dot) > 0.9995 else "acos"), negated


def test_slerp_pairs_take_the_branches_they_were_built_for():
    c = pc.case("slerp_edges")
    pairs = c["pairs"]
    got = {}
    for q, (a, b, branch, negated, what) in enumerate(pairs):
        dot, br, neg = rot_const_branch(a, b)
        assert (br, neg) == (branch, negated), f"{what}: {br}, negated {neg}"
        assert rot_const_branch(b, a) == (dot, br, neg)                 # the three-key channels hold the pair as (b, a)
        got[q] = (float(dot), br, neg)
    for q, (cv, branch, negated) in enumerate(pc.SLERP_C):               # the inner product IS c; the sum opens with +0
        assert np.array_equal(np.asarray(abs(cv), F32).view(np.uint32), np.asarray(got[q][0], F32).view(np.uint32))
    val = {float(cv): (br, neg) for cv, br, neg in pc.SLERP_C}
    c9 = pc.C9995
    assert float(c9) < 0.9995 < float(np.nextafter(c9, F32(2)))
    # the two neighbours of every threshold take different branches
    assert val[float(c9)][0] == "acos" and val[float(np.nextafter(c9, F32(2)))][0] == "nlerp"
    assert val[float(-c9)] == ("acos", True) and val[float(np.nextafter(-c9, F32(-2)))] == ("nlerp", True)
    assert val[float(np.nextafter(F32(0), F32(1)))][1] is False and val[float(np.nextafter(F32(0), F32(-1)))][1] is True
    assert val[0.0] == ("acos", False) and not np.signbit(rot_const_branch(pc.UNIT_A, pc.unit_b(F32(-0.0)))[0])
    assert got[len(pc.SLERP_C)][1] == "acos" and got[len(pc.SLERP_C)][0] == 2 * float(F32(0.4) * F32(0.75))
    assert got[len(pc.SLERP_C) + 1] == (2.0, "nlerp", False)
    # the channels hold the pairs, and every pair stands in a two-key channel; all but the last unit pair in a three-key one
    an = c["anims"][0]
    chan = {(int(an["ch_target"][ch]), int(an["ch_path"][ch])): ch for ch in range(an["n_channels"])}
    in3 = set()
    for j, ivs in c["rot_pairs"].items():
        ch = chan[(j, 1)]
        keys = an["data"][int(an["ch_data_off"][ch]):][:4 * int(an["ch_nr"][ch])].reshape(-1, 4)
        for iv, q in ivs:
            a, b = pairs[q][0], pairs[q][1]
            assert rot_const_branch(keys[iv], keys[iv + 1]) == rot_const_branch(a, b)
            if len(keys) == 2:
                assert np.array_equal(keys.view(np.uint32), np.stack([a, b]).view(np.uint32))
            else:
                in3.add(q)
    assert sorted(j for j, v in c["rot_pairs"].items() if len(v) == 1) == list(range(len(pairs)))
    assert len(in3) == 16
    # fac at the frame times: 0, 1, 0.5 and the values beside 0 and 1 that a time beside a key gives
    for g in (pc.SLERP_GRID2, pc.SLERP_GRID3):
        prev, nxt, fac = reference_of(g, c["times"])
        for iv in range(len(g) - 1):
            f = fac[(prev == iv) & (nxt == iv + 1)]
            assert {0.0, 0.5, 1.0} <= set(f.tolist()) if iv == 0 else {0.5, 1.0} <= set(f.tolist())
            assert ((f > 0) & (f < 1e-6)).any() and ((f < 1) & (f > 1 - 1e-6)).any()
    # the oracle's results: finite for every pair at every time (no pair is built to be otherwise)
    trs = oracle_trs("slerp_edges")
    assert np.isfinite(trs).all()
    # theta_0 at both ends of the acos path's range
    assert float(np.arccos(np.float64(c9))) < 0.0317 and float(F32(np.arccos(0.0))) > np.pi / 2


def test_a_difference_is_named_by_model_time_joint_path_and_bracket_kind():
    """What tests/test_pose_edges_gpu.py adds to a mismatch, on outputs with one value changed on purpose"""
    c = pc.case("missing_lds")
    trs = oracle_trs("missing_lds")
    n, J, a = c["n_chars"], c["J"], 1
    j = int(np.flatnonzero(c["chan_len"][a][:, 1] >= 3)[0])
    g = pc.channel_times(c, a, j, 1)
    i = int(np.flatnonzero((c["t"] == g[1]) & (c["which"] == a))[0])
    jt, jp = np.zeros((n, J, 16), F32), np.zeros((n, J, 4), F32)
    reach = c["sk"]["order"]
    out = dict(trs=trs.copy(), joint_transforms=jt.copy(), joint_pos=jp.copy())
    out["trs"][i, j, 4] = np.nextafter(out["trs"][i, j, 4], F32(9))
    msg = pc.first_difference(c, 0, c["t"], out, trs, jt, jp, reach, True)
    for part in ("model missing_lds frame 0", f"character {i} (animation 1)", repr(c["t"][i]), f"joint {j}, path R",
                 f"{len(g)} keys", "on interior key 1" if len(g) > 2 else "on the last key"):
        assert part in msg, (part, msg)
    out = dict(trs=trs.copy(), joint_transforms=jt.copy(), joint_pos=jp.copy())
    out["trs"][7, 5, 9] = 3.0                                            # joint 5 of this model has no channel
    assert "joint 5, path S: no channel" in pc.first_difference(c, 1, np.roll(c["t"], 1), out, trs, jt, jp, reach, True)
    out["joint_pos"][3, reach[2], 1] = 1.0                               # T / R / S unwritten: only the palette and positions speak
    msg = pc.first_difference(c, 0, c["t"], out, trs, jt, jp, reach, False)
    assert f"character 3 (animation 1) at time {c['t'][3]!r}, joint {int(reach[2])}: joint_pos differs" in msg
