"""The camera controller's rule (include/clapgpu.h, "The camera controller on the device"), restated once in numpy scalars:
float32 and float64 where core/camera.c has them, its order of operations, nothing shared with csrc/lm_dev.h.

    camera_target (camera.c:174-206)      target, dist from the control entity
    rays          (camera.c:68-91, 51-57) one iteration's corners and rays
    decide        (camera.c:101-116)      min_scale, next dist
    update        (camera.c:226-242)      the loop with a caller's cast(ray) -> (hit[4], depth[4], flags[4])

and a brute-force float64 ray caster over spheres, capsules, boxes and triangles (closest hit, front faces only for
triangles), which the tests use to CHOOSE cases -- that a case pulls in three times, or that a triangle wins -- not to
compare values with: the values are held to clapgpu_ray_cast itself, bit for bit.
"""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cbrtf.restype, _libm.cbrtf.argtypes = ctypes.c_float, [ctypes.c_float]


def cbrtf(x):
    """libm's cbrtf, which the reference calls (model.c:1263); numpy's float32 cbrt is not it to the last bit"""
    return F(_libm.cbrtf(float(F(x))))


IS_CHARACTER, HAS_HEAD_JOINT = 1, 2
UNRESOLVED, CAPPED = 1, 2
RAY_INVALID, RAY_UNRESOLVED = 1, 2
ITER_MAX = 16384


def _f(v):
    return np.asarray(v, F)


def quat_mul_vec3(q, v):
    """linmath.h:939-958"""
    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    qx = [q[0], q[1], q[2]]
    t = [c * F(2) for c in cross(qx, v)]
    u = cross(qx, t)
    t = [c * q[3] for c in t]
    r = [v[i] + t[i] for i in range(3)]
    return [r[i] + u[i] for i in range(3)]


def orbit(quat, target, length):
    """transform.c:116-123"""
    r = quat_mul_vec3(quat, [F(0), F(0), F(length)])
    return _f([r[i] + target[i] for i in range(3)])


def from_quat(q):
    """linmath.h:959-987; m[c][r]"""
    a, b, c, d = q[3], q[0], q[1], q[2]
    a2, b2, c2, d2 = a * a, b * b, c * c, d * d
    two, z, one = F(2), F(0), F(1)
    return [[a2 + b2 - c2 - d2, two * (b * c + a * d), two * (b * d - a * c), z],
            [two * (b * c - a * d), a2 - b2 + c2 - d2, two * (c * d + a * b), z],
            [two * (b * d + a * c), two * (c * d - a * b), a2 - b2 - c2 + d2, z],
            [z, z, z, one]]


def mat_mul(a, b):
    """linmath.h:506-516"""
    out = [[F(0)] * 4 for _ in range(4)]
    for c in range(4):
        for r in range(4):
            s = F(0)
            for k in range(4):
                s = s + a[k][r] * b[c][k]
            out[c][r] = s
    return out


def view_matrix(pos, quat):
    """transform.c:132-138"""
    ident = [[F(1) if i == j else F(0) for j in range(4)] for i in range(4)]
    m = mat_mul(ident, from_quat(quat))
    t = [row[:] for row in m]
    for c in range(3):
        for r in range(3):
            t[c][r] = m[r][c]
    x, y, z = -pos[0], -pos[1], -pos[2]
    for i in range(4):                               # mat4x4_translate_in_place, linmath.h:525-534
        p = F(0)
        p = p + x * t[0][i]
        p = p + y * t[1][i]
        p = p + z * t[2][i]
        p = p + F(0) * t[3][i]
        t[3][i] = t[3][i] + p
    return t


def invert(m):
    """linmath.h:611-651"""
    s0 = m[0][0] * m[1][1] - m[1][0] * m[0][1]
    s1 = m[0][0] * m[1][2] - m[1][0] * m[0][2]
    s2 = m[0][0] * m[1][3] - m[1][0] * m[0][3]
    s3 = m[0][1] * m[1][2] - m[1][1] * m[0][2]
    s4 = m[0][1] * m[1][3] - m[1][1] * m[0][3]
    s5 = m[0][2] * m[1][3] - m[1][2] * m[0][3]
    c0 = m[2][0] * m[3][1] - m[3][0] * m[2][1]
    c1 = m[2][0] * m[3][2] - m[3][0] * m[2][2]
    c2 = m[2][0] * m[3][3] - m[3][0] * m[2][3]
    c3 = m[2][1] * m[3][2] - m[3][1] * m[2][2]
    c4 = m[2][1] * m[3][3] - m[3][1] * m[2][3]
    c5 = m[2][2] * m[3][3] - m[3][2] * m[2][3]
    idet = F(1) / (s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0)
    t = [[None] * 4 for _ in range(4)]
    t[0][0] = (m[1][1] * c5 - m[1][2] * c4 + m[1][3] * c3) * idet
    t[0][1] = (-m[0][1] * c5 + m[0][2] * c4 - m[0][3] * c3) * idet
    t[0][2] = (m[3][1] * s5 - m[3][2] * s4 + m[3][3] * s3) * idet
    t[0][3] = (-m[2][1] * s5 + m[2][2] * s4 - m[2][3] * s3) * idet
    t[1][0] = (-m[1][0] * c5 + m[1][2] * c2 - m[1][3] * c1) * idet
    t[1][1] = (m[0][0] * c5 - m[0][2] * c2 + m[0][3] * c1) * idet
    t[1][2] = (-m[3][0] * s5 + m[3][2] * s2 - m[3][3] * s1) * idet
    t[1][3] = (m[2][0] * s5 - m[2][2] * s2 + m[2][3] * s1) * idet
    t[2][0] = (m[1][0] * c4 - m[1][1] * c2 + m[1][3] * c0) * idet
    t[2][1] = (-m[0][0] * c4 + m[0][1] * c2 - m[0][3] * c0) * idet
    t[2][2] = (m[3][0] * s4 - m[3][1] * s2 + m[3][3] * s0) * idet
    t[2][3] = (-m[2][0] * s4 + m[2][1] * s2 - m[2][3] * s0) * idet
    t[3][0] = (-m[1][0] * c3 + m[1][1] * c1 - m[1][2] * c0) * idet
    t[3][1] = (m[0][0] * c3 - m[0][1] * c1 + m[0][2] * c0) * idet
    t[3][2] = (-m[3][0] * s3 + m[3][1] * s1 - m[3][2] * s0) * idet
    t[3][3] = (m[2][0] * s3 - m[2][1] * s1 + m[2][2] * s0) * idet
    return t


def camera_target(flags, pos_scale, lo, hi, center, head, far_plane):
    pos_scale, lo, hi, center = _f(pos_scale), _f(lo), _f(hi), _f(center)
    s = pos_scale[3]
    X, Y, Z = [np.abs(hi[a] - lo[a]) * s for a in range(3)]          # entity3d_aabb_X / Y / Z
    if flags & IS_CHARACTER:
        height = Y
        if flags & HAS_HEAD_JOINT:
            head = _f(head)
            target = [head[0] + F(0), head[1] + height * F(0.2), head[2] + F(0)]
        else:
            target = [pos_scale[0], pos_scale[1] + height * F(0.75), pos_scale[2]]
    else:
        target = [center[0], center[1], center[2]]
        height = Y / F(2)
    with np.errstate(all="ignore"):
        dist_cap = np.fmax(F(10), cbrtf(X * Y * Z))
        dist = np.fmin(height * F(3), np.fmin(dist_cap, F(far_plane) - F(10)))
    return _f(target), F(dist)


def rays(quat, target, dist, near_plane, aspect):
    quat, target = _f(quat), _f(target)
    w, h = F(near_plane), F(near_plane) / F(aspect)
    with np.errstate(all="ignore"):
        pos = orbit(quat, target, F(dist))
        inv = invert(view_matrix(pos, quat))
        corner, ray = np.zeros((4, 4), F), np.zeros((4, 8), np.float64)
        for k, (sx, sy) in enumerate(((1, 1), (-1, 1), (1, -1), (-1, -1))):
            r = [F(sx) * w, F(sy) * h, F(0), F(1)]
            for j in range(4):                       # mat4x4_mul_vec4, linmath.h:308-316
                t = F(0)
                for i in range(4):
                    t = t + inv[i][j] * r[i]
                corner[k, j] = t
            d = [corner[k, i] - target[i] for i in range(3)]
            p = F(0)
            for i in range(3):
                p = p + d[i] * d[i]
            ray[k, 0:3], ray[k, 3:6], ray[k, 6] = target, d, np.sqrt(F(p))
    return corner, ray


def decide(dist, hit, depth, ray):
    min_scale = np.float64(1.0)
    with np.errstate(all="ignore"):
        for k in range(4):
            if hit[k]:
                min_scale = np.fmin(min_scale, np.float64(depth[k]) / np.float64(ray[k][6]))
    if min_scale < 0.99:
        return False, min_scale, np.float64(F(dist)) * min_scale
    return True, min_scale, None


def update(quat, target, cdist, near_plane, aspect, has_physics, cast):
    """The loop and what follows it.  Returns a dict: pos, dist, updated, iterations, status, corner (None without an
    iteration), and the per-iteration records (corner, ray, hit, depth, min_scale, dist after)."""
    dist = np.float64(F(cdist))
    it, status, corner, trace = 0, 0, None, []
    while dist > 0.1:
        if it == ITER_MAX:
            status |= CAPPED
            break
        it += 1
        corner, ray = rays(quat, target, F(dist), near_plane, aspect)
        hit, depth = [False] * 4, [0.0] * 4
        if has_physics:
            h, d, f = cast(ray)
            for k in range(4):
                miss = bool(f[k] & RAY_INVALID) or not h[k]
                hit[k], depth[k] = not miss, (0.0 if miss else float(d[k]))
                if f[k] & RAY_UNRESOLVED:
                    status |= UNRESOLVED
        good, ms, nxt = decide(F(dist), hit, depth, ray)
        if not good:
            dist = nxt
        trace.append(dict(corner=corner, ray=ray, hit=hit, depth=depth, min_scale=ms, dist=dist))
        if good:
            break
    updated = int(np.float64(F(cdist)) != dist)
    with np.errstate(all="ignore"):
        out_dist = F(dist)
        pos = orbit(_f(quat), _f(target), out_dist)
    return dict(pos=pos, dist=out_dist, updated=updated, iterations=it, status=status, corner=corner, trace=trace)


# ---- a brute-force float64 scene: for choosing cases -------------------------------------------------
def _ray_sphere(s, u, L, c, r):
    oc = s - c
    b, cc = oc @ u, oc @ oc - r * r
    disc = b * b - cc
    if disc < 0:
        return None
    sq = np.sqrt(disc)
    t = -b - sq if cc > 0 else -b + sq               # inside: the exit
    return t if 0 <= t <= L else None


def _ray_capsule(s, u, L, pos, axis, r, length):
    """closest entry (or exit from inside) by sampling-free algebra: the two cap spheres and the cylinder between them"""
    a, b = pos - axis * (length / 2), pos + axis * (length / 2)

    def inside(p):
        t = np.clip((p - a) @ axis, 0, length)
        return np.linalg.norm(p - (a + axis * t)) < r
    ins = inside(s)
    best = None
    for c in (a, b):                                 # caps
        oc = s - c
        bb, cc = oc @ u, oc @ oc - r * r
        disc = bb * bb - cc
        if disc >= 0:
            for t in (-bb - np.sqrt(disc), -bb + np.sqrt(disc)):
                p = s + t * u
                k = (p - a) @ axis
                if 0 <= t <= L and (k <= 0 or k >= length):
                    if ((not ins) and (best is None or t < best)) or (ins and (best is None or t > best)):
                        best = t
    up, sp = u - axis * (u @ axis), (s - a) - axis * ((s - a) @ axis)       # cylinder
    A, B, Cc = up @ up, sp @ up, sp @ sp - r * r
    if A > 0 and B * B - A * Cc >= 0:
        for t in ((-B - np.sqrt(B * B - A * Cc)) / A, (-B + np.sqrt(B * B - A * Cc)) / A):
            k = (s + t * u - a) @ axis
            if 0 <= t <= L and 0 <= k <= length:
                if ((not ins) and (best is None or t < best)) or (ins and (best is None or t > best)):
                    best = t
    return best


def _ray_box(s, u, L, bb):
    lo, hi = np.array(bb[0::2]), np.array(bb[1::2])
    with np.errstate(all="ignore"):
        t0, t1 = (lo - s) / u, (hi - s) / u
    tn, tf = np.fmin(t0, t1), np.fmax(t0, t1)
    for a in range(3):
        if u[a] == 0:
            if not lo[a] <= s[a] <= hi[a]:
                return None
            tn[a], tf[a] = -np.inf, np.inf
    near, far = tn.max(), tf.min()
    if near > far or far < 0:
        return None
    t = near if near >= 0 else far                   # a start inside: the exit
    return t if 0 <= t <= L else None


def _ray_tri(s, u, L, v):
    e1, e2 = v[1] - v[0], v[2] - v[0]
    n = np.cross(e1, e2)
    den = n @ u
    if den >= 0:                                     # back face or parallel
        return None
    t = (n @ (v[0] - s)) / den
    if not 0 <= t <= L:
        return None
    p = s + t * u
    for i in range(3):
        if np.cross(v[(i + 1) % 3] - v[i], p - v[i]) @ n < 0:
            return None
    return t


def brute_cast(scene, ray, skip):
    """scene: dict(bodies=[geom], statics=[geom], tris={static: [T, 3, 3]}), geom a dict with kind in sphere / capsule /
    box / other.  Returns (hit [4] as clapgpu_ray_cast codes it, depth [4], flags [4], what [4]): what = "body", "static"
    or "tri"."""
    hit, depth, flags, what = [-1] * 4, [0.0] * 4, [0] * 4, [None] * 4
    for k in range(4):
        s, d, L = np.array(ray[k][0:3], np.float64), np.array(ray[k][3:6], np.float64), float(ray[k][6])
        if not np.isfinite(d).all() or not d.any() or np.isnan(s).any() or not L >= 0:
            flags[k] = RAY_INVALID
            continue
        u = d / np.linalg.norm(d)
        best, other = (np.inf, -1, None), np.inf
        for code, kindname, geoms in ((lambda i: i, "body", scene["bodies"]), (lambda i: -2 - i, "static", scene["statics"])):
            for i, g in enumerate(geoms):
                if code(i) == skip:
                    continue
                if kindname == "static" and i in scene.get("tris", {}):
                    ts = [t for t in (_ray_tri(s, u, L, np.asarray(v, np.float64)) for v in scene["tris"][i]) if t is not None]
                    t, w = (min(ts) if ts else None), "tri"
                elif g["kind"] == "sphere":
                    t, w = _ray_sphere(s, u, L, np.array(g["pos"], np.float64), g["radius"]), kindname
                elif g["kind"] == "capsule":
                    t, w = _ray_capsule(s, u, L, np.array(g["pos"], np.float64), np.array(g["axis"], np.float64), g["radius"],
                                        g["length"]), kindname
                elif g["kind"] == "box":
                    t, w = _ray_box(s, u, L, g["aabb"]), kindname
                else:                                # OTHER without a mesh: where the segment enters its box
                    lo, hi = np.array(g["aabb"][0::2]), np.array(g["aabb"][1::2])
                    if ((lo <= s) & (s <= hi)).all():
                        other = 0.0
                    else:
                        te = _ray_box(s, u, L, g["aabb"])
                        if te is not None:
                            other = min(other, te)
                    continue
                if t is not None and t < best[0]:
                    best = (t, code(i), w)
        if best[1] != -1 or best[0] < np.inf:
            if best[0] < np.inf:
                hit[k], depth[k], what[k] = best[1], best[0], best[2]
        if other <= L and (hit[k] == -1 or other <= depth[k]):
            flags[k] |= RAY_UNRESOLVED
    return hit, depth, flags, what
