"""The order of a crowd (include/clapgpu.h, clapgpu_characters_order), restated in numpy for the tests: the reach box of
every mover in the header's order of fp64 operations (bit for bit what k_order_reach writes), the conflicts by brute
force, the levels by a plain loop in list order.

  reach box   roff = ray_off - 0.05; ray_len = yoffset - roff + 1e-3; rl = ray_len > 0 ? ray_len : 0;
              start = (double)(float)(pos.y - roff); end = start - rl * 2;
              a0 = |vx| + |vy| + |vz|; A = a0 + |gravity_y| * dt (not finite: a0; still not: 0); B = 3 * (|dx| + |dz|)
              (not finite: 0); S = max(A, B); T = S * clamp(dt) (not finite: 0); pad = mag * 2^-20 + 1e-6;
              the body's box grown by T + pad in x and z, by rl + T + pad in y, and extended to the ray's two ends
  classes     OUT (level 0, no conflicts): body >= n_bodies, or a body listed more than once among the finite boxes;
              ALONE (conflicts with every other mover that is not OUT): a box that is not finite
  conflict    i < j, neither OUT, and (one of them ALONE, or their boxes overlap, closed)
  level       0 without an earlier conflicting mover, else 1 + the largest level among them
"""
import numpy as np

f64 = np.float64
LEVELED, OUT, ALONE = 0, 1, 2


def reach_boxes(body, ray_off, motion, velocity, aabb, pos, yoffset, gravity_y, dt):
    """reach [n, 6] float64; gravity_y: (float)w->gravity[1]"""
    body = np.asarray(body, np.int64)
    n, nb = len(body), len(aabb)
    out = np.full((n, 6), np.nan)
    ok = body < nb
    i = body[ok]
    with np.errstate(all="ignore"):
        bb = np.asarray(aabb, f64)[i]
        roff = np.asarray(ray_off, f64)[ok] - 0.05
        ray_len = np.asarray(yoffset, f64)[i] - roff + 1e-3
        rl = np.where(ray_len > 0.0, ray_len, 0.0)
        start = (np.asarray(pos, f64)[i, 1] - roff).astype(np.float32).astype(f64)
        end = start - rl * 2.0
        v = np.abs(np.asarray(velocity, np.float32)[ok].astype(f64))
        d = np.abs(np.asarray(motion, np.float32)[ok].astype(f64))
        dt = f64(dt)
        a0 = v[:, 0] + v[:, 1] + v[:, 2]
        A = a0 + abs(f64(np.float32(gravity_y))) * dt
        A = np.where(np.isfinite(A), A, a0)
        A = np.where(np.isfinite(A), A, 0.0)
        B = 3.0 * (d[:, 0] + d[:, 1])
        B = np.where(np.isfinite(B), B, 0.0)
        S = np.where(A > B, A, B)
        dtc = f64(0.0) if dt < 1e-6 else f64(1.0 / 30.0) if dt > 1.0 / 30.0 else dt
        T = S * dtc
        T = np.where(np.isfinite(T), T, 0.0)
        mag = T
        for a in range(6):
            mag = np.fmax(mag, np.abs(bb[:, a]))
        mag = np.fmax(np.fmax(np.fmax(mag, np.abs(start)), np.abs(end)), rl)
        pad = mag * 2.0 ** -20 + 1e-6
        gx, gy = T + pad, rl + T + pad
        low, ray_low = bb[:, 2] - gy, end - pad
        high, ray_high = bb[:, 3] + gy, start + pad
        box = np.stack([bb[:, 0] - gx, bb[:, 1] + gx, np.where(ray_low < low, ray_low, low),
                        np.where(ray_high > high, ray_high, high), bb[:, 4] - gx, bb[:, 5] + gx], 1)
    out[ok] = box
    return out


def classes(body, reach, n_bodies):
    body = np.asarray(body, np.int64)
    cls = np.full(len(body), LEVELED, np.uint8)
    cls[~np.isfinite(reach).all(1)] = ALONE
    cls[body >= n_bodies] = OUT
    leveled = cls == LEVELED
    ids, counts = np.unique(body[leveled], return_counts=True)
    cls[leveled & np.isin(body, ids[counts > 1])] = OUT
    return cls


def overlaps(reach):
    """[n, n] bool: closed overlap of the boxes (False wherever a NaN stands)"""
    lo, hi = reach[:, 0::2], reach[:, 1::2]
    with np.errstate(invalid="ignore"):
        return ((lo[:, None, :] <= hi[None, :, :]) & (hi[:, None, :] >= lo[None, :, :])).all(2)


def levels(body, reach, n_bodies, earlier=True):
    """(level [n] uint32, n_levels, pair_total).  earlier=False is a mutant for the tests: the rule with i > j"""
    n = len(body)
    cls = classes(body, reach, n_bodies)
    meet = overlaps(reach)
    searched = np.isfinite(reach).all(1) & (np.asarray(body, np.int64) < n_bodies)       # the rows the pair search is given
    pair_total = int(np.triu(meet & searched[:, None] & searched[None, :], 1).sum())
    level = np.zeros(n, np.uint32)
    order = range(n) if earlier else range(n - 1, -1, -1)
    done = []
    for j in order:
        if cls[j] != OUT:
            for i in done:
                if cls[i] != OUT and (cls[i] == ALONE or cls[j] == ALONE or meet[i, j]):
                    level[j] = max(level[j], level[i] + 1)
        done.append(j)
    return level, (int(level.max()) + 1 if n else 0), pair_total
