"""Independent truth for ray casts against static triangle meshes (clapgpu_ray_cast with a mesh set): no formula shared with the
kernel (which shears the ray onto its dominant axis and takes three 2-D edge functions).

A ray p(t) = s + t u crosses triangle (v0, v1, v2) inside or on its boundary when the three signed volumes
c_k = u . ((v_k+1 - s) x (v_k+2 - s)) are all <= 0; their sum is u . n, n = (v1 - v0) x (v2 - v0), which is < 0 for a
front face.  The depth is ((v0 - s) . n) / (u . n) (Cramer's rule).  A vectorised long-double pass prefilters and
classifies; every candidate whose classification or depth lies within a margin of the rounding is decided again in
exact rational arithmetic (fractions.Fraction of the fp64 inputs).  The mesh bake (float scale, dQtoR pose) is
restated here from physics.c / ODE's rotation.cpp.
"""
from fractions import Fraction

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def q_to_R(q):
    """dQtoR of (w, x, y, z), fp64"""
    w, x, y, z = (float(v) for v in q)
    qq1, qq2, qq3 = 2 * x * x, 2 * y * y, 2 * z * z
    return np.array([[1 - qq2 - qq3, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - qq1 - qq3, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - qq1 - qq2]])


def bake(vx, idx, scale, pos, quat_xyzw):
    """World-space fp64 triangles [T, 3, 3] of one mesh: (double)(float)(scale * v) (-0 -> +0), then R v + pos."""
    v = np.asarray(vx, np.float32).reshape(-1, 3)
    ms = (np.float32(scale) * v + np.float32(0.0)).astype(np.float64)
    q = np.asarray(quat_xyzw, np.float32).astype(np.float64)
    R = q_to_R([q[3], q[0], q[1], q[2]])
    p = np.asarray(pos, np.float64)
    w = np.empty_like(ms)
    for a in range(3):                                      # R[a,0] x + R[a,1] y + R[a,2] z + p, left to right
        w[:, a] = ((R[a, 0] * ms[:, 0] + R[a, 1] * ms[:, 1]) + R[a, 2] * ms[:, 2]) + p[a]
    return w[np.asarray(idx, np.int64).reshape(-1, 3)]


def unit_dir(d):
    """dSafeNormalize3 (fp64), as dGeomRaySet normalises"""
    d = np.asarray(d, np.float64).copy()
    a = np.abs(d)
    i = int(np.argmax(a)) if a.max() > 0 else 0
    if a[1] > a[0]:
        i = 2 if a[2] > a[1] else 1
    elif a[2] > a[0]:
        i = 2
    else:
        i = 0
    d = d / a[i]
    return d * (1.0 / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))


def _fr(x):
    return [Fraction(float(v)) for v in x]


def _exact(tri, s, u):
    """(front and inside-or-on, depth) in exact rationals"""
    v = [_fr(tri[k]) for k in range(3)]
    S, U = _fr(s), _fr(u)
    d = [[v[k][a] - S[a] for a in range(3)] for k in range(3)]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    c = [dot(U, cross(d[(k + 1) % 3], d[(k + 2) % 3])) for k in range(3)]
    n = cross([v[1][a] - v[0][a] for a in range(3)], [v[2][a] - v[0][a] for a in range(3)])
    un = dot(U, n)
    if un >= 0 or any(ck > 0 for ck in c):
        return False, None
    return True, dot(d[0], n) / un


class Meshes:
    """All meshes of a set: triangles [T, 3, 3] fp64 with their static and triangle-of-mesh index."""

    def __init__(self, tris, static, local):
        self.tri = np.ascontiguousarray(tris, np.float64)
        self.static = np.asarray(static, np.int64)
        self.local = np.asarray(local, np.int64)
        self.lo, self.hi = self.tri.min(1), self.tri.max(1)
        self.n = np.cross(self.tri[:, 1] - self.tri[:, 0], self.tri[:, 2] - self.tri[:, 0])
        self.zero = ~self.n.any(1)                              # never hit
        self.scale = np.abs(self.tri).max((1, 2))

    @classmethod
    def from_list(cls, meshes):
        """meshes: [(static, tris [T, 3, 3])]"""
        tris = np.concatenate([t for _s, t in meshes]) if meshes else np.zeros((0, 3, 3))
        st = np.concatenate([np.full(len(t), s) for s, t in meshes]) if meshes else np.zeros(0)
        lo = np.concatenate([np.arange(len(t)) for _s, t in meshes]) if meshes else np.zeros(0)
        return cls(tris, st, lo)

    def cast(self, s, u, length, skip_static=None):
        """-> (static, triangle, depth, normal, margin, bound) of the closest front-face hit, or None.  margin: the
        winner is decided without an exact tie (identity comparable); bound: depth tolerance of the fp64 test."""
        s, u = np.asarray(s, np.float64), np.asarray(u, np.float64)
        e = s + u * length
        seg_lo, seg_hi = np.minimum(s, e), np.maximum(s, e)
        pad = 1e-9 * (1 + np.abs(seg_lo).max() + np.abs(seg_hi).max())
        cand = np.nonzero(np.all(self.lo <= seg_hi + pad, 1) & np.all(self.hi >= seg_lo - pad, 1) & ~self.zero)[0]
        if skip_static is not None:
            cand = cand[self.static[cand] != skip_static]
        if len(cand) == 0:
            return None
        T = self.tri[cand].astype(LD)
        S, U = s.astype(LD), u.astype(LD)
        d = T - S
        c = np.stack([np.einsum("j,ij->i", U, np.cross(d[:, (k + 1) % 3], d[:, (k + 2) % 3])) for k in range(3)], 1)
        n = self.n[cand].astype(LD)
        un = n @ U
        depth = np.einsum("ij,ij->i", d[:, 0], n) / np.where(un == 0, 1, un)
        sc = (self.scale[cand] + np.abs(s).max() + 1.0)
        tol_c = 64 * EPS * sc * sc                              # signed-volume rounding of the fp64 test, generously
        sure_in = np.all(c < -tol_c[:, None], 1) & (un < 0)
        sure_out = np.any(c > tol_c[:, None], 1) | (un >= 0)
        inr = (depth >= 0) & (depth <= LD(length))
        sure = np.nonzero(sure_in & inr)[0]
        hits = [(LD(depth[k]), int(self.static[cand[k]]), int(self.local[cand[k]]), int(cand[k]), False) for k in
                sure[np.argsort(depth[sure], kind="stable")][:8]]                 # the closest few decide
        for k in np.nonzero(~sure_in & ~sure_out)[0]:                             # near a margin: exact rationals
            ok, t = _exact(self.tri[cand[k]], s, u)
            if ok:
                t = LD(t.numerator) / LD(t.denominator)
                if LD(0) <= t <= LD(length):
                    hits.append((t, int(self.static[cand[k]]), int(self.local[cand[k]]), int(cand[k]), True))
        if not hits:
            return None
        hits.sort()
        t, st, lo, gi, exact = hits[0]
        nn = self.n[gi] / np.linalg.norm(self.n[gi])
        cos = abs(float(nn @ u))
        bound = 64 * EPS * (self.scale[gi] + np.abs(s).max() + float(t) + 1.0) / max(cos, 1e-300)
        margin = not exact and (len(hits) == 1 or float(hits[1][0] - t) > 2 * bound)
        return st, lo, float(t), nn, margin, bound
