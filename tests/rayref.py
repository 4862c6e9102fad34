"""Independent long-double truth for the ray casts (clapgpu_ray_cast): no formula shared with the kernel.

For a convex solid, f(t) = signed distance from p(t) = start + t * u to the solid is convex along the ray.  Its
minimum on [0, L] comes from a golden-section search; the entry is the first zero on [0, t_min] by bisection; a start
inside (f(0) < 0) exits at the zero after 0.  The normal is the distance gradient at the hit (central differences),
negated for an exit.  Capsules use geomref.point_segment; boxes have their own signed distance.
"""
import numpy as np

from geomref import LD, EPS, capsule_ends, ld, norm, point_segment


def sd_sphere(p, c, r):
    return norm(ld(p) - ld(c)) - LD(r)


def sd_capsule(p, pos, axis, r, length):
    a, b = capsule_ends(ld(pos), ld(axis), ld(length))
    return point_segment(ld(p), a, b)[1] - LD(r)


def sd_box(p, bb):
    bb = ld(bb)
    lo, hi = bb[0::2], bb[1::2]
    c, h = (lo + hi) / 2, (hi - lo) / 2
    q = np.abs(ld(p) - c) - h
    out = norm(np.maximum(q, 0))
    return out + min(q.max(), LD(0))


def sd_of(geom):
    k = geom["kind"]
    if k == "sphere":
        return lambda p: sd_sphere(p, geom["pos"], geom["radius"])
    if k == "capsule":
        return lambda p: sd_capsule(p, geom["pos"], geom["axis"], geom["radius"], geom["length"])
    return lambda p: sd_box(p, geom["aabb"])


def unit(d):
    d = ld(d)
    return d / norm(d)


def cast(geom, start, direction, length, iters=200):
    """(depth, pos, normal, inside) of the ray's hit, or None for a miss."""
    f0 = sd_of(geom)
    s, u, L = ld(start), unit(direction), LD(length)
    f = lambda t: f0(s + t * u)
    if f(LD(0)) < 0:                                             # inside: the zero after 0
        if f(L) < 0:
            return None
        a, b = LD(0), L
        for _ in range(iters):
            m = (a + b) / 2
            if f(m) < 0:
                a = m
            else:
                b = m
        t, inside = (a + b) / 2, True
    else:
        g = (np.sqrt(LD(5)) - 1) / 2                            # golden section for the minimum on [0, L]
        a, b = LD(0), L
        x1, x2 = b - g * (b - a), a + g * (b - a)
        f1, f2 = f(x1), f(x2)
        for _ in range(iters):
            if f1 < f2:
                b, x2, f2 = x2, x1, f1
                x1 = b - g * (b - a)
                f1 = f(x1)
            else:
                a, x1, f1 = x1, x2, f2
                x2 = a + g * (b - a)
                f2 = f(x2)
        tm = (a + b) / 2
        cands = [(f(LD(0)), LD(0)), (f(tm), tm), (f(L), L)]
        fm, tm = min(cands, key=lambda c: c[0])
        if fm > 0:
            return None
        a, b = LD(0), tm                                         # f(a) >= 0 >= f(b)
        for _ in range(iters):
            m = (a + b) / 2
            if f(m) > 0:
                a = m
            else:
                b = m
        t, inside = (a + b) / 2, False
    p = s + t * u
    scale = max(LD(1e-300), LD(geom.get("radius", 0) or 0), LD(1e-3))
    h = scale * LD(1e-6)
    grad = np.array([(f0(p + h * e) - f0(p - h * e)) / (2 * h) for e in np.eye(3, dtype=LD)], dtype=LD)
    n = grad / norm(grad)
    return t, p, (-n if inside else n), inside


def tolerance(geom, start, direction, length, hit):
    """Depth tolerance for the kernel against cast(): rounding of coordinates of size `scale`, divided by how steeply
    the ray meets the surface; grazing hits (|cos| < 1e-4) get sqrt(eps) * scale."""
    scale = float(max(np.abs(ld(start)).max(), float(length) if np.isfinite(length) else 0.0,
                      np.abs(ld(geom.get("pos", np.zeros(3)))).max() if "pos" in geom else np.abs(ld(geom["aabb"])).max(),
                      1.0))
    cos = abs(float((unit(direction) * hit[2]).sum()))
    if cos < 1e-4:
        return np.sqrt(EPS) * scale * 4, True
    return 256 * EPS * scale / cos, False
