"""Independent float64 / long-double geometry for the physics rows that no reference binary pins.

The narrowphase, the capsule sweep, the body step and skinning are compared byte for byte with oracle/physics2.c and
oracle/skin.c, which come from the same reading of ODE as the kernels.  This module restates what those rows compute
from the geometric definitions, with different algorithms:

  - closest points of two segments by exact minimisation of the convex quadratic over the unit square (interior
    critical point, else the best of the four clamped edge solutions), not by a region test;
  - closest points of a segment and an axis-aligned box by exact minimisation of the piecewise quadratic in t between
    the points where a coordinate crosses a slab, not by ODE's walk along the derivative;
  - contact records in ODE's convention derived from the closest points c1 (on g1) and c2 (on g2);
  - the time of impact of a translated capsule by bisection on the exact distance (convex in t);
  - the rigid-body step from its equations (the implicit gyroscopic update solved as a linear system);
  - skinning as a float64 sum.

Arithmetic is np.longdouble (80-bit on x86-64) where the inputs allow; the inputs are whatever the kernel had, in
float64.  Nothing here calls the oracle.
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)             # 2^-52
EPS32 = float(np.finfo(np.float32).eps)           # 2^-23
PARALLEL_TOL = 1e-5                               # the two-contact branch: 1 - (a.b)^2 below this
DEEP = 0x80000000                                 # a capsule axis meets the box: the record is flagged, nc = 0


def ld(a):
    return np.asarray(a, dtype=LD)


def dot(a, b):
    return (a * b).sum(axis=-1)


def norm(a):
    return np.sqrt(dot(a, a))


# ---------------------------------------------------------------------------------------------- closest points
def point_segment(p, a, b):
    """Closest point to p on segment [a, b] (arrays (..., 3)): (point, distance, parameter)."""
    p, a, b = ld(p), ld(a), ld(b)
    u = b - a
    uu = dot(u, u)
    t = np.where(uu > 0, dot(p - a, u) / np.where(uu > 0, uu, 1), 0)
    t = np.clip(t, 0, 1)
    c = a + t[..., None] * u
    return c, norm(p - c), t


def segment_segment(p0, p1, q0, q1):
    """Closest points of segments [p0, p1] and [q0, q1], shape (n, 3) each.

    f(s, t) = |p0 + s u - q0 - t v|^2 is a convex quadratic on [0, 1]^2: its minimum is the interior critical point
    when that exists and lies in the square, else it lies on an edge, where the one-parameter problem is solved
    exactly by clamping.  Every candidate is evaluated and the smallest kept.

    Returns dict(c1, c2, d, s, t, cond, unique, interior): cond = 1 - (a.b)^2 of the unit directions; unique is False
    only for parallel segments whose projections overlap over a positive length (then every pair on the overlap is
    closest); interior: both parameters free at the minimum (the solution whose error grows as 1 / cond)."""
    p0, p1, q0, q1 = ld(p0), ld(p1), ld(q0), ld(q1)
    u, v, w = p1 - p0, q1 - q0, p0 - q0
    a, b, c = dot(u, u), dot(u, v), dot(v, v)
    d, e = dot(u, w), dot(v, w)
    det = a * c - b * b
    one = LD(1)
    safe = lambda x: np.where(x > 0, x, one)
    cands = []
    ok = det > 0
    s_i = np.where(ok, (b * e - c * d) / safe(det), -one)
    t_i = np.where(ok, (a * e - b * d) / safe(det), -one)
    inside = ok & (s_i >= 0) & (s_i <= 1) & (t_i >= 0) & (t_i <= 1)
    cands.append((s_i, t_i, inside, True))
    for s_fix in (0, 1):                                    # edges s = 0, 1: t = (e + b s) / c clamped
        cands.append((np.full_like(a, s_fix), np.clip((e + b * s_fix) / safe(c), 0, 1), np.ones(a.shape, bool), False))
    for t_fix in (0, 1):                                    # edges t = 0, 1: s = (b t - d) / a clamped
        cands.append((np.clip((b * t_fix - d) / safe(a), 0, 1), np.full_like(a, t_fix), np.ones(a.shape, bool), False))
    best = np.full(a.shape, np.inf, dtype=LD)
    S, T = np.zeros_like(a), np.zeros_like(a)
    interior = np.zeros(a.shape, bool)
    for s, t, valid, is_int in cands:
        r = w + s[..., None] * u - t[..., None] * v
        f = np.where(valid, dot(r, r), np.inf)
        take = f < best
        best = np.where(take, f, best)
        S, T = np.where(take, s, S), np.where(take, t, T)
        interior = np.where(take, is_int, interior)
    c1 = p0 + S[..., None] * u
    c2 = q0 + T[..., None] * v
    cosab = b / np.sqrt(safe(a) * safe(c))
    cond = one - cosab * cosab
    # parallel: the projections of segment 2 on the line of segment 1 overlap over a positive length -> not unique
    lu = np.sqrt(safe(a))
    uh = u / lu[..., None]
    s0, s1 = dot(q0 - p0, uh), dot(q1 - p0, uh)
    overlap = np.minimum(lu, np.maximum(s0, s1)) - np.maximum(0, np.minimum(s0, s1))
    unique = (det > 0) | (overlap <= 0)
    return dict(c1=c1, c2=c2, d=norm(c1 - c2), s=S, t=T, cond=cond, unique=unique, interior=interior)


def segment_aabb(p0, p1, lo, hi):
    """Closest points of segment [p0, p1] and the box [lo, hi] (arrays (n, 3)).

    g(t) = sum_i dist_i(x_i(t))^2 with x(t) = p0 + t (p1 - p0) and dist_i the distance to the slab [lo_i, hi_i] is a
    quadratic in t between consecutive breakpoints (where some x_i(t) = lo_i or hi_i: at most 6 in (0, 1)).  Each
    piece's quadratic is minimised exactly (vertex clamped to the piece), the smallest piece minimum kept.

    Returns dict(c1 on the segment, c2 on the box, d, t, unique, curv): curv = sum of u_i^2 over the coordinates
    outside their slab at the minimum, over |u|^2 (0: the segment runs parallel to the face / edge it is nearest to,
    the minimum is flat); unique is False when a flat piece of positive length attains the minimum."""
    p0, p1, lo, hi = ld(p0), ld(p1), ld(lo), ld(hi)
    u = p1 - p0
    n = p0.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        bl = (lo - p0) / u
        bh = (hi - p0) / u
    bp = np.concatenate([bl, bh], axis=1)
    bp = np.where(np.isfinite(bp) & (bp > 0) & (bp < 1), bp, LD(2))
    knots = np.sort(np.concatenate([np.zeros((n, 1), LD), bp, np.ones((n, 1), LD)], axis=1), axis=1)
    knots = np.minimum(knots, 1)                          # unused slots collapse onto t = 1: empty pieces
    best = np.full(n, np.inf, dtype=LD)
    T = np.zeros(n, LD)
    curv_at = np.zeros(n, LD)
    pieces = []
    uu = dot(u, u)
    for k in range(knots.shape[1] - 1):
        ta, tb = knots[:, k], knots[:, k + 1]
        tm = 0.5 * (ta + tb)
        xm = p0 + tm[:, None] * u
        below, above = xm < lo, xm > hi
        bound = np.where(below, lo, np.where(above, hi, 0))
        act = below | above
        off = np.where(act, p0 - bound, 0)
        uc = np.where(act, u, 0)
        A = dot(uc, uc)                                     # g(t) = A t^2 + 2 B t + C on this piece
        B = dot(uc, off)
        t = np.where(A > 0, -B / np.where(A > 0, A, 1), ta)
        t = np.clip(t, ta, tb)
        x = p0 + t[:, None] * u
        r = x - np.clip(x, lo, hi)
        g = dot(r, r)
        pieces.append((A, ta, tb, g))
        take = g < best
        best, T = np.where(take, g, best), np.where(take, t, T)
        curv_at = np.where(take, A / np.where(uu > 0, uu, 1), curv_at)
    unique = np.ones(n, bool)
    for A, ta, tb, g in pieces:
        flat = (A == 0) & (tb > ta) & (g <= best * (1 + 64 * EPS))
        unique &= ~flat
    c1 = p0 + T[:, None] * u
    c2 = np.clip(c1, lo, hi)
    return dict(c1=c1, c2=c2, d=norm(c1 - c2), t=T, unique=unique, curv=curv_at)


# ---------------------------------------------------------------------------------------------- contact records
def contact_from_points(c1, c2, r1, r2):
    """ODE's sphere-sphere record for spheres (c1, r1) on g1 and (c2, r2) on g2: normal = (c1 - c2) / |c1 - c2| points
    into g1, depth = r1 + r2 - d, pos = c1 - normal (r1 - depth / 2) (the middle of the overlap); d = 0 gives the
    normal (1, 0, 0), depth r1 + r2 and pos = c1.  touch: d <= r1 + r2."""
    c1, c2, r1, r2 = ld(c1), ld(c2), ld(r1), ld(r2)
    diff = c1 - c2
    d = norm(diff)
    zero = d <= 0
    nrm = np.where(zero[..., None], ld([1, 0, 0]), diff / np.where(zero, 1, d)[..., None])
    depth = r1 + r2 - d
    pos = np.where(zero[..., None], c1, c1 - nrm * (r1 - depth / 2)[..., None])
    return dict(touch=d <= r1 + r2, normal=nrm, depth=depth, pos=pos, d=d)


def capsule_ends(pos, axis, length):
    """A capsule's core segment: pos +- axis * length / 2."""
    pos, axis, half = ld(pos), ld(axis), ld(length)[..., None] / 2
    return pos + axis * half, pos - axis * half


def capsule_capsule(pos1, ax1, r1, l1, pos2, ax2, r2, l2):
    """Capsule (g1) against capsule (g2), arrays over pairs.

    Near-parallel axes (1 - (a1.a2)^2 < 1e-5) are treated as parallel: axis 2 is flipped if it points against axis 1,
    and the overlap [lo, hi] of the two core segments is measured along axis 1 from g1's centre (g2's spans
    [c - l2/2, c + l2/2], c = a1.(pos2 - pos1)); the point of g2 at axial coordinate x is pos2 + (x - c) a2.  When the
    spheres at both ends of a proper overlap touch, the pair has two contacts (at lo and at hi); otherwise one contact
    from the spheres at the middle of the overlap.  Without overlap, and for all other axes, the contact comes from
    the segments' closest points.

    Returns dict(nc, pos, normal, depth, pos2, normal2, depth2, branch, seg) -- branch "two" / "mid" / "general";
    seg is the segment_segment() result for every pair (distance, conditioning, uniqueness)."""
    pos1, ax1, pos2, ax2 = ld(pos1), ld(ax1), ld(pos2), ld(ax2)
    r1, l1, r2, l2 = ld(r1), ld(l1), ld(r2), ld(l2)
    n = pos1.shape[0]
    a1, b1 = capsule_ends(pos1, ax1, l1)
    a2, b2 = capsule_ends(pos2, ax2, l2)
    seg = segment_segment(a1, b1, a2, b2)
    gen = contact_from_points(seg["c1"], seg["c2"], r1, r2)
    cosang = dot(ax1, ax2)
    par = (1 - cosang * cosang) < PARALLEL_TOL
    a2f = np.where((cosang < 0)[:, None], -ax2, ax2)
    cc = dot(ax1, pos2 - pos1)
    lo = np.maximum(-l1 / 2, cc - l2 / 2)
    hi = np.minimum(l1 / 2, cc + l2 / 2)
    at = lambda x: (pos1 + x[:, None] * ax1, pos2 + (x - cc)[:, None] * a2f)
    e_lo = contact_from_points(*at(lo), r1, r2)
    e_hi = contact_from_points(*at(hi), r1, r2)
    mid = contact_from_points(*at((lo + hi) / 2), r1, r2)
    two = par & (lo < hi) & e_lo["touch"] & e_hi["touch"]
    use_mid = par & (lo <= hi) & ~two
    general = ~(two | use_mid)
    out = dict(nc=np.zeros(n, np.int64), pos=np.zeros((n, 3), LD), normal=np.zeros((n, 3), LD), depth=np.zeros(n, LD),
               pos2=np.zeros((n, 3), LD), normal2=np.zeros((n, 3), LD), depth2=np.zeros(n, LD),
               branch=np.where(two, "two", np.where(use_mid, "mid", "general")), seg=seg, d=gen["d"])
    first = {k: np.where((two | use_mid)[:, None] if k != "depth" else (two | use_mid),
                         np.where(two[:, None] if k != "depth" else two, e_lo[k], mid[k]), gen[k])
             for k in ("pos", "normal", "depth")}
    touch = np.where(two, True, np.where(use_mid, mid["touch"], gen["touch"]))
    out["d"] = np.where(two, e_lo["d"], np.where(use_mid, mid["d"], gen["d"]))
    out["nc"] = np.where(two, 2, touch.astype(np.int64))
    for k in ("pos", "normal", "depth"):
        out[k] = first[k]
    out["pos2"], out["normal2"], out["depth2"] = (np.where(two[:, None], e_hi["pos"], 0), np.where(two[:, None], e_hi["normal"], 0),
                                                  np.where(two, e_hi["depth"], 0))
    out["d_lo"], out["d_hi"] = e_lo["d"], e_hi["d"]
    out["lo"], out["hi"], out["par"] = lo, hi, par
    return out


def capsule_sphere(cpos, cax, cr, cl, spos, sr):
    """Capsule (g1) against sphere (g2): c1 = the point of the core segment nearest the centre, c2 = the centre."""
    a, b = capsule_ends(cpos, cax, cl)
    c1, _d, _t = point_segment(spos, a, b)
    out = contact_from_points(c1, ld(spos), cr, sr)
    out["nc"] = out["touch"].astype(np.int64)
    return out


def sphere_capsule(spos, sr, cpos, cax, cr, cl):
    """Sphere (g1) against capsule (g2): the capsule-sphere record with the normal negated."""
    out = capsule_sphere(cpos, cax, cr, cl, spos, sr)
    out["normal"] = -out["normal"]
    return out


def sphere_sphere(p1, r1, p2, r2):
    out = contact_from_points(p1, p2, r1, r2)
    out["nc"] = out["touch"].astype(np.int64)
    return out


def capsule_box(cpos, cax, cr, cl, aabb):
    """Capsule (g1) against the axis-aligned box aabb = (minx, maxx, miny, maxy, minz, maxz) (g2): closest points of the
    core segment and the box; a segment that meets the box is the deep case (flag 0x80000000, no contact here), else
    the sphere-sphere record of (c1, r) and (c2, 0)."""
    aabb = ld(aabb)
    lo, hi = aabb[:, 0::2], aabb[:, 1::2]
    a, b = capsule_ends(cpos, cax, cl)
    sb = segment_aabb(a, b, lo, hi)
    out = contact_from_points(sb["c1"], sb["c2"], cr, 0)
    deep = sb["d"] == 0
    out["nc"] = np.where(deep, DEEP, out["touch"].astype(np.int64))
    out["seg"] = sb
    return out


def sphere_box(c, r, aabb):
    """Sphere (g1) against the axis-aligned box (g2), ODE's dCollideSphereBox convention.  Centre outside the box:
    c2 = the box point nearest the centre, normal = (c - c2) / |c - c2|, depth = r - |c - c2|, pos = c2.  Centre
    inside (or on the boundary): the face nearest the centre decides (the first axis among equals), normal = +-e_axis
    by the side of the box's centre the sphere's centre lies on (+ strictly above it), depth = distance to that face
    + r, pos = c."""
    c, r, aabb = ld(c), ld(r), ld(aabb)
    lo, hi = aabb[:, 0::2], aabb[:, 1::2]
    q = np.clip(c, lo, hi)
    diff = c - q
    d = norm(diff)
    inside = np.all((c >= lo) & (c <= hi), axis=1)
    n = c.shape[0]
    face = np.minimum(c - lo, hi - c)
    ax = np.argmin(face, axis=1)                          # argmin keeps the first of equal values
    side = np.where(c[np.arange(n), ax] > (lo[np.arange(n), ax] + hi[np.arange(n), ax]) / 2, 1, -1)
    n_in = np.zeros((n, 3), LD)
    n_in[np.arange(n), ax] = side
    n_out = diff / np.where(d > 0, d, 1)[:, None]
    return dict(inside=inside, nc=np.where(inside | (d <= r), 1, 0),
                normal=np.where(inside[:, None], n_in, n_out),
                depth=np.where(inside, face[np.arange(n), ax] + r, r - d),
                pos=np.where(inside[:, None], c, q), d=d, c2=q)


# ---------------------------------------------------------------------------------------------- distances for sweeps
def geom_distance(probe_pos, probe_axis, probe_length, ob):
    """Distance between the core of a probe capsule (a point when its length is 0) at probe_pos and the core of an
    obstacle (sphere: its centre, capsule: its segment, box: the box), arrays over n probes: (distance, c1, c2).
    ob: dict(kind (n,) 0 sphere / 1 capsule / 2 box, pos, axis, length, aabb)."""
    a, b = capsule_ends(probe_pos, probe_axis, probe_length)
    bb = ld(ob["aabb"])
    box = segment_aabb(a, b, bb[:, 0::2], bb[:, 1::2])
    e1, e2 = capsule_ends(ob["pos"], ob["axis"], ob["length"])       # a sphere: e1 = e2 = the centre
    seg = segment_segment(a, b, e1, e2)
    is_box = (np.asarray(ob["kind"]) == 2)
    pick = lambda x, y: np.where(is_box[:, None] if x.ndim == 2 else is_box, x, y)
    return pick(box["d"], seg["d"]), pick(box["c1"], seg["c1"]), pick(box["c2"], seg["c2"])


def time_of_impact(gp, delta, probe_axis, probe_length, probe_radius, ob, iters=72):
    """The first t in [0, 1] at which the probe translated by t * delta touches the obstacle (distance of the cores =
    r_probe + r_obstacle, a box having radius 0), arrays over n (probe, obstacle) pairs.  The distance between convex
    sets under a translation is convex in t, so the set where it is <= R is an interval: a golden-section search finds
    the minimum on [0, 1], bisection on [0, t_min] the interval's left end.
    Returns (t* (inf without contact), normal at t* in ODE's convention with the probe as g1: (c1 - c2) / |c1 - c2|)."""
    gp, delta = ld(gp), ld(delta)
    R = ld(probe_radius) + np.where(np.asarray(ob["kind"]) == 2, 0, ld(ob["radius"]))
    dist = lambda t: geom_distance(gp + t[:, None] * delta, probe_axis, probe_length, ob)[0]
    n = gp.shape[0]
    lo_, hi_ = np.zeros(n, LD), np.ones(n, LD)
    g = (np.sqrt(LD(5)) - 1) / 2
    for _ in range(iters):                                  # the minimum of the convex distance on [0, 1]
        m1, m2 = hi_ - g * (hi_ - lo_), lo_ + g * (hi_ - lo_)
        left = dist(m1) < dist(m2)
        hi_, lo_ = np.where(left, m2, hi_), np.where(left, lo_, m1)
    tmin = (lo_ + hi_) / 2
    dmin = np.minimum(dist(tmin), np.minimum(dist(np.zeros(n, LD)), dist(np.ones(n, LD))))
    tmin = np.where(dist(np.zeros(n, LD)) <= dmin, 0, np.where(dist(np.ones(n, LD)) <= dmin, 1, tmin))
    a_, b_ = np.zeros(n, LD), tmin.copy()                   # dist(a_) > R >= dist(b_) once contact exists
    for _ in range(iters):
        m = (a_ + b_) / 2
        out = dist(m) > R
        a_, b_ = np.where(out, m, a_), np.where(out, b_, m)
    b_ = np.where(dist(np.zeros(n, LD)) <= R, 0, b_)
    _d, c1, c2 = geom_distance(gp + b_[:, None] * delta, probe_axis, probe_length, ob)
    diff = c1 - c2
    dn = norm(diff)
    nrm = np.where((dn > 0)[:, None], diff / np.where(dn > 0, dn, 1)[:, None], ld([1, 0, 0]))
    hit = dmin <= R
    return np.where(hit, b_, np.inf).astype(np.float64), nrm.astype(np.float64)


# ---------------------------------------------------------------------------------------------- the rigid-body step
def quat_to_R(q):
    """Rotation matrices (n, 3, 3) of unit quaternions (w, x, y, z)."""
    q = ld(q)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def quat_mul(a, b):
    """Hamilton product a (x) b of (n, 4) quaternions (w, x, y, z)."""
    aw, ax, ay, az = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    bw, bx, by, bz = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def _solve3(M, r):
    """Batched 3x3 solve by Cramer's rule (long double; numpy's solvers stop at float64)."""
    def det(A):
        return (A[:, 0, 0] * (A[:, 1, 1] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 1])
                - A[:, 0, 1] * (A[:, 1, 0] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 0])
                + A[:, 0, 2] * (A[:, 1, 0] * A[:, 2, 1] - A[:, 1, 1] * A[:, 2, 0]))
    D = det(M)
    out = np.empty(r.shape, LD)
    for j in range(3):
        Mj = M.copy()
        Mj[:, :, j] = r
        out[:, j] = det(Mj) / D
    return out


def world_inertia(q, I_body):
    R = quat_to_R(q)
    return np.einsum("nij,nj,nkj->nik", R, ld(I_body), R)


def body_step(pos, quat, lvel, avel, bflags, h, gravity, inertia=None, radius=None, length=None,
              damping=0.0, damping_threshold_sq=0.0):
    """One step of a body without constraint rows, from the equations:
      v' = v + h g (unless no-gravity), p' = p + h v';
      with inertia, the implicit gyroscopic update when the flag is set: solve Iw w' - h (L x w') = L with L = Iw w and
      Iw = R I R^T from the pre-step orientation (without the flag, or without inertia, w' = w);
      q' = normalise((1, h w'/2) (x) q) -- the rotation by w' in the WORLD frame, on the left;
      v' *= (1 - damping) when |v'|^2 > threshold^2;
      the capsule axis R(q') y and its AABB: the two core endpoints +- r per coordinate (a sphere: pos +- r).
    Disabled bodies (flag 1) are returned unchanged.  Returns dict of long-double arrays (+ 'resid': the gyroscopic
    residual |Iw w' - h (L x w') - L| and 'Lnorm': |L|)."""
    pos, quat, lvel, avel = ld(pos).copy(), ld(quat).copy(), ld(lvel).copy(), ld(avel).copy()
    n = pos.shape[0]
    fl = np.asarray(bflags, np.uint32)
    live = (fl & 1) == 0
    grav = ((fl & 4) == 0)[:, None] * ld(gravity)[None]
    v = lvel + LD(h) * grav
    p = pos + LD(h) * v
    w = avel.copy()
    resid = np.zeros(n, LD)
    Lnorm = np.zeros(n, LD)
    if inertia is not None:
        Iw = world_inertia(quat, inertia)
        L = np.einsum("nij,nj->ni", Iw, avel)
        gyro = (fl & 8) != 0
        Lx = np.zeros((n, 3, 3), LD)                        # [L]x y = L x y
        Lx[:, 0, 1], Lx[:, 0, 2] = -L[:, 2], L[:, 1]
        Lx[:, 1, 0], Lx[:, 1, 2] = L[:, 2], -L[:, 0]
        Lx[:, 2, 0], Lx[:, 2, 1] = -L[:, 1], L[:, 0]
        M = Iw - LD(h) * Lx
        wg = _solve3(M, L)
        w = np.where(gyro[:, None], wg, avel)
        r = np.einsum("nij,nj->ni", Iw, w) - LD(h) * np.cross(L, w) - L
        resid = np.where(gyro, norm(r), 0)
        Lnorm = norm(L)
    dq = np.concatenate([np.ones((n, 1), LD), LD(h) / 2 * w], axis=1)
    q = quat_mul(dq, quat)
    q = q / norm(q)[:, None]
    s2 = dot(v, v)
    v = np.where((damping != 0) & (s2 > damping_threshold_sq)[:, None], v * (1 - LD(damping)), v)
    out = dict(pos=np.where(live[:, None], p, pos), quat=np.where(live[:, None], q, quat),
               lvel=np.where(live[:, None], v, lvel), avel=np.where(live[:, None], w, avel), resid=resid, Lnorm=Lnorm)
    out["axis"] = np.einsum("nij,j->ni", quat_to_R(out["quat"]), ld([0, 1, 0]))
    if radius is not None:
        half = (ld(length) if length is not None else np.zeros(n, LD)) / 2
        ext = np.abs(out["axis"]) * half[:, None] + ld(radius)[:, None]
        bb = np.empty((n, 6), LD)
        bb[:, 0::2], bb[:, 1::2] = out["pos"] - ext, out["pos"] + ext
        out["aabb"] = bb
    return out


def axis_angle_between(q0, q1):
    """The rotation q1 q0^-1 as (angle in [0, pi], unit axis)."""
    q0, q1 = ld(q0), ld(q1)
    inv = q0 * ld([1, -1, -1, -1])
    r = quat_mul(q1, inv)
    r = np.where((r[:, :1] < 0), -r, r)
    s = norm(r[:, 1:])
    return 2 * np.arctan2(s, r[:, 0]), r[:, 1:] / np.where(s > 0, s, 1)[:, None]


# ---------------------------------------------------------------------------------------------- skinning
def skin(position, normal, joints, weights, palette):
    """sum_i w_i M_i [p, 1] and sum_i w_i M_i [n, 0] in float64, M_i read as a column-major 4x4 (element (r, c) at
    4 c + r).  Returns (pos (n, 3), nor (n, 3), w (n,), bound_p (n, 4), bound_n (n, 4)) where bound_* = sum_i |w_i|
    sum_c |M_i(r, c)| |x_c| per output row: the magnitude an fp32 evaluation's rounding error is proportional to."""
    P = np.asarray(palette, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)     # [j, r, c]
    M = P[np.asarray(joints, np.int64)]                                           # [v, 4, r, c]
    W = np.asarray(weights, np.float64)
    x = np.concatenate([np.asarray(position, np.float64), np.ones((len(W), 1))], axis=1)
    y = np.concatenate([np.asarray(normal, np.float64), np.zeros((len(W), 1))], axis=1)
    tp = np.einsum("vi,virc,vc->vr", W, M, x)
    tn = np.einsum("vi,virc,vc->vr", W, M, y)
    bp = np.einsum("vi,virc,vc->vr", np.abs(W), np.abs(M), np.abs(x))
    bn = np.einsum("vi,virc,vc->vr", np.abs(W), np.abs(M), np.abs(y))
    return tp[:, :3], tn[:, :3], tp[:, 3], bp, bn
