"""Chosen inputs for the particle kernels (clap_amd/csrc/particles.hip): respawn sets chosen bit by bit, and particles
one float32 step on either side of the respawn threshold.

Chosen respawn patterns.  Velocities are zero and every particle sits on its system's centre, so nothing respawns; the
chosen particles are moved two radii out, so the first frame's respawn set is exactly the chosen one.  That drives the
ranking of k_particles_respawn_rp -- group counts, popcount bytes, the 256-entry LDS list and the row-by-row walk past
it -- through every edge by construction and not by luck.  From frame 1 on the respawned particles fly and the frames
run free.

Threshold edges.  dd > radius_squared is a double comparison of a float32 sum of three products; the pairs here lie on
either side of it, adjacent floats, so one fused multiply-add decides differently.

Everything is built on the CPU, is deterministic, and uses no GPU.  tests/test_particle_edges.py checks with the oracle
that the cases are what they claim.
"""
import functools

import numpy as np

from clap_amd import synth

F32 = np.float32
PARKED = F32(1.0e6)                  # where the padded lanes of a system's last row stand: far outside every sphere
GROUP_ROWS, WAVE_ROWS, LIST_MAX = 1024, 64, 256      # particles.hip: PART_GROUP_ROWS, a wave's rows, PART_RESPAWN_LIST


def layout(counts, dists=(synth.PART_DIST_LIN, synth.PART_DIST_SQRT, synth.PART_DIST_CBRT), radius=2.0, velocity=0.3,
           centers=None):
    """Systems of the given particle counts in the layout of synth.particle_systems: every system starts a 64-particle
    row.  Centres and radii are exact in float32, so centre + 2 radius is."""
    n_sys = len(counts)
    sys = np.zeros(n_sys, synth.PSYS_DTYPE)
    sys["center"] = centers if centers is not None else [(16.0 * s - 8.0, 4.0 - 2.0 * s, 3.0 + s) for s in range(n_sys)]
    sys["count"] = counts
    sys["radius"] = radius
    sys["min_radius"] = 0.0
    sys["velocity"] = velocity
    sys["dist"] = [dists[s % len(dists)] for s in range(n_sys)]
    sys["radius_squared"] = sys["radius"] * sys["radius"]
    rows = (sys["count"].astype(np.int64) + 63) // 64
    first_row = np.concatenate([[0], np.cumsum(rows)])
    sys["first"] = (first_row[:-1] * 64).astype(np.uint32)
    return dict(sys=sys, n=int(first_row[-1]) * 64, n_real=int(sys["count"].sum()),
                row_sys=np.repeat(np.arange(n_sys, dtype=np.uint32), rows))


# three groups of 1024 rows; the systems end in rows 999 and 2036: inside a wave, and not where a group ends
LAYOUT_FULL = (1000 * 64 - 17, 1037 * 64 - 40, 1035 * 64)
# 3045 rows: the last wave has 37 rows, and the last row 5 padded lanes
LAYOUT_PARTIAL = (1000 * 64 - 17, 1037 * 64 - 40, 1008 * 64 - 5)


@functools.lru_cache(maxsize=None)
def layouts():
    return dict(full=layout(LAYOUT_FULL), partial=layout(LAYOUT_PARTIAL))


def live_mask(ps):
    live = np.zeros(ps["n"], bool)
    for f, c in zip(ps["sys"]["first"], ps["sys"]["count"]):
        live[int(f):int(f) + int(c)] = True
    return live


def at_rest(ps, chosen):
    """(pos, vel): every live particle on its centre without velocity, the chosen ones two radii out along +x, the padded
    lanes parked."""
    n = ps["n"]
    pos = np.full((n, 3), PARKED, F32)
    vel = np.zeros((n, 3), F32)
    sys_of = ps["row_sys"][np.arange(n) >> 6]
    live = live_mask(ps)
    pos[live] = ps["sys"]["center"][sys_of[live]]
    chosen = np.asarray(chosen, np.int64)
    assert live[chosen].all(), "a chosen particle is a padded lane"
    pos[chosen, 0] += (2.0 * ps["sys"]["radius"][sys_of[chosen]]).astype(F32)
    return pos, vel


def mask_words(n, chosen):
    """The respawn mask u64[n / 64] with the chosen bits"""
    bits = np.zeros(n, np.uint8)
    bits[np.asarray(chosen, np.int64)] = 1
    return np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).ravel()


# ------------------------------------------------------------------------------------------------- the patterns
def _rows(rows, lanes=range(64)):
    return [r * 64 + l for r in rows for l in lanes]


def _thin(wave, count):
    """`count` respawns spread over the 64 rows of a wave: four in each row, one more or less in row 9"""
    r0 = wave * WAVE_ROWS
    out = [(r0 + r) * 64 + (7 * r + 16 * j) % 64 for r in range(64) for j in range(4)]
    if count == 255:
        out.remove((r0 + 9) * 64 + (7 * 9) % 64)
    elif count == 257:
        out.append((r0 + 9) * 64 + (7 * 9 + 5) % 64)
    return out


def _thick(wave, count):
    """`count` respawns of a wave as four full rows, one lane less, or one more in a fifth row"""
    r0 = wave * WAVE_ROWS
    out = _rows([r0 + 3, r0 + 17, r0 + 40, r0 + 62])
    if count == 255:
        out.remove((r0 + 17) * 64 + 30)
    elif count == 257:
        out.append((r0 + 50) * 64 + 11)
    return out


WAVE_IN_GROUP_0, WAVE_IN_GROUP_1 = 0, 20


def patterns(ps):
    """name -> sorted particle indices, for a layout of three groups"""
    n, rows = ps["n"], ps["n"] // 64
    live = np.flatnonzero(live_mask(ps))
    waves = (rows + WAVE_ROWS - 1) // WAVE_ROWS
    last_wave_rows = rows - (waves - 1) * WAVE_ROWS
    p = {
        "none": [],
        "all": live.tolist(),
        "particle_0": [0],
        "last_live": [int(live[-1])],
        "lane_63_of_the_last_full_row": [int(live[live % 64 == 63][-1])],
        "one_full_row": _rows([5]),
        "rows_1023_and_1024": [1023 * 64 + l for l in (0, 31, 63)] + [1024 * 64 + l for l in (0, 5, 63)],
        "group_2_only": [r * 64 + (r * 13) % 64 for r in range(2 * GROUP_ROWS + 1, rows, 37)],
        "group_0_only": [r * 64 + (r * 13) % 64 for r in range(0, GROUP_ROWS, 37) if r != 999] + [1023 * 64 + 63],
        "x5555_in_every_row_of_a_wave": _rows(range(WAVE_IN_GROUP_1 * 64, WAVE_IN_GROUP_1 * 64 + 64), range(0, 64, 2)),
        "one_bit_per_wave": [(w * 64 + (w * 11) % (last_wave_rows if w == waves - 1 else 64)) * 64 + (w * 5) % 48
                             for w in range(waves)],
    }
    for wave, tag in ((WAVE_IN_GROUP_0, "wave_0"), (WAVE_IN_GROUP_1, "wave_20")):
        for count in (255, 256, 257):
            p[f"{count}_thin_in_{tag}"] = _thin(wave, count)
            p[f"{count}_as_rows_in_{tag}"] = _thick(wave, count)
    return {k: np.unique(np.asarray(v, np.int64)) for k, v in p.items()}


PATTERN_NAMES = tuple(patterns(layout(LAYOUT_FULL)))
# what runs on the layout with a partial last wave, and through the view-block entry
PARTIAL_PATTERNS = ("none", "all", "last_live", "one_bit_per_wave", "group_2_only", "257_thin_in_wave_20")
VIEWS_PATTERNS = ("all", "particle_0", "256_thin_in_wave_0", "257_as_rows_in_wave_20", "one_bit_per_wave")
STATE0 = 0x00C0FFEE1234


# ------------------------------------------------------------------------------------------------- threshold edges
def outside(pos, center, r2):
    """particles.c / particle.c:109-110 in numpy: a float32 sum of three float32 products, compared in double"""
    d = (pos - center).astype(F32)
    dd = F32(0) + d[:, 0] * d[:, 0]
    dd = dd + d[:, 1] * d[:, 1]
    dd = dd + d[:, 2] * d[:, 2]
    assert dd.dtype == F32
    return dd.astype(np.float64) > r2


@functools.lru_cache(maxsize=None)
def threshold_case(pairs_per_sys=160, n_sys=4, seed=11):
    """n_sys systems of 2 * pairs_per_sys particles without velocity: particle 2j of a system lies inside its sphere and
    2j + 1 outside, both on one ray from the centre, one coordinate one float32 step apart.  A last system at the origin
    with a power of two as radius holds dd == radius^2 exactly (no respawn) and the next float out (respawn).
    Returns dict(ps, pos, vel, expect): expect = the particle indices that respawn in the first frame."""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = pairs_per_sys
    ps = layout([2 * m] * n_sys + [8], radius=1.0, velocity=0.2,
                centers=np.concatenate([rng.uniform(-50, 50, (n_sys, 3)), np.zeros((1, 3))]).astype(F32))
    sys = ps["sys"]
    sys["radius"][:n_sys] = rng.uniform(0.5, 30.0, n_sys)
    sys["radius"][n_sys] = 4.0
    sys["radius_squared"] = sys["radius"] * sys["radius"]
    which = np.repeat(np.arange(n_sys), m)
    c, r, r2 = sys["center"][which], sys["radius"][which], sys["radius_squared"][which]
    d = rng.normal(size=(n_sys * m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)

    def at(t):
        return (c.astype(np.float64) + t[:, None] * d).astype(F32)
    a, b = 0.5 * r, 2.0 * r                                 # inside, outside
    assert not outside(at(a), c, r2).any() and outside(at(b), c, r2).all()
    for _ in range(60):
        mid = (a + b) / 2.0
        out = outside(at(mid), c, r2)
        a, b = np.where(out, a, mid), np.where(out, mid, b)
    p, q = at(a), at(b)
    # from p to q one coordinate at a time: the coordinate at which the answer changes is bisected in float32
    ax_of = np.full(len(p), -1)
    lo, hi = np.zeros(len(p), F32), np.zeros(len(p), F32)
    for ax in range(3):
        nxt = p.copy()
        nxt[:, ax] = q[:, ax]
        flips = outside(nxt, c, r2) & (ax_of < 0)
        ax_of[flips], lo[flips], hi[flips] = ax, p[flips, ax], q[flips, ax]
        p = np.where((ax_of < 0)[:, None], nxt, p)
    assert (ax_of >= 0).all()
    rows = np.arange(len(p))
    for _ in range(64):
        mid = ((lo.astype(np.float64) + hi.astype(np.float64)) / 2.0).astype(F32)
        open_ = (mid != lo) & (mid != hi)
        if not open_.any():
            break
        trial = p.copy()
        trial[rows, ax_of] = mid
        out = outside(trial, c, r2)
        lo, hi = np.where(open_ & ~out, mid, lo), np.where(open_ & out, mid, hi)
    inside_pos, outside_pos = p.copy(), p.copy()
    inside_pos[rows, ax_of], outside_pos[rows, ax_of] = lo, hi

    pos = np.full((ps["n"], 3), PARKED, F32)
    vel = np.zeros((ps["n"], 3), F32)
    first = sys["first"].astype(np.int64)
    idx = first[which] + 2 * (np.arange(n_sys * m) % m)
    pos[idx], pos[idx + 1] = inside_pos, outside_pos
    e = int(first[n_sys])
    up = np.nextafter(F32(4.0), F32(8.0))
    pos[e:e + 8] = [(4, 0, 0), (0, -4, 0), (0, 0, 4), (up, 0, 0), (0, up, 0), (-4, 0, 0), (0, 0, -up), (0, 0, 0)]
    expect = np.sort(np.concatenate([idx + 1, [e + 3, e + 4, e + 6]]))
    return dict(ps=ps, pos=pos, vel=vel, expect=expect, inside=idx, outside=idx + 1, equal=np.asarray([e, e + 1, e + 2, e + 5]))


# ------------------------------------------------------------------------------------------------- the fixture's case
@functools.lru_cache(maxsize=None)
def fixture_case():
    """What tests/golden/particles_edges_wave.npz pins on the reference: 256 respawns in the 64 rows of one wave and 257 in
    the next one's, and the equality case.  Returns dict(ps, pos, vel, expect)."""
    ps = layout([64 * 64, 64 * 64 - 9, 8], centers=np.asarray([(8, 4, 3), (-8, 2, 4), (0, 0, 0)], F32))
    ps["sys"]["radius"][2] = 4.0
    ps["sys"]["radius_squared"] = ps["sys"]["radius"] * ps["sys"]["radius"]
    chosen = np.unique(np.asarray(_thin(0, 256) + _thick(1, 257), np.int64))
    pos, vel = at_rest(ps, chosen)
    e = int(ps["sys"]["first"][2])
    up = np.nextafter(F32(4.0), F32(8.0))
    pos[e:e + 8] = [(4, 0, 0), (0, -4, 0), (0, 0, 4), (up, 0, 0), (0, up, 0), (-4, 0, 0), (0, 0, -up), (0, 0, 0)]
    return dict(ps=ps, pos=pos, vel=vel, expect=np.sort(np.concatenate([chosen, [e + 3, e + 4, e + 6]])))
