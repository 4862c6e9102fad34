"""Independent truth for contacts of spheres and capsules against static triangles (clapgpu_contacts_meshes,
clapgpu_sweep_capsules).  It shares no formula with the kernel (tricontact_dev.h, which uses edge functions for
"inside", the crossing point of the plane and ODE's dClosestLineSegmentPoints):

* "projects into the closed triangle": barycentric coordinates from the Gram system of the two edges;
* "the segment meets the triangle": the signs of the three signed volumes det(b - a, v_k - a, v_k+1 - a);
* the closest points: the minimum over the endpoints' projections onto the face and the segment-vs-edge distances,
  each the minimum of a quadratic over [0, 1]^2 (the stationary point, or the best of the four clamped sides).

Everything is long double.  Each decision records how far its quantity lies from its threshold; a contact whose
decision lies within the margin of the fp64 rounding is flagged `margin` (either outcome is accepted).  The mesh bake is
trimeshref.bake.
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
MAX_CONTACTS = 16


def _v(x):
    return np.asarray(x, np.float64).astype(LD)


def _bary(v0, e1, e2, x):
    """(u, v, w) of x's projection: x ~ v0 + v e1 + w e2, u = 1 - v - w"""
    d = x - v0
    d00, d01, d11 = e1 @ e1, e1 @ e2, e2 @ e2
    d20, d21 = d @ e1, d @ e2
    den = d00 * d11 - d01 * d01
    v = (d11 * d20 - d01 * d21) / den
    w = (d00 * d21 - d01 * d20) / den
    return np.array([LD(1) - v - w, v, w])


def _seg_seg(a, b, c, d):
    """closest points of segments a-b and c-d (either may be a point): min over [0,1]^2 of |a + s u - c - t w|^2"""
    u, w, r = b - a, d - c, a - c
    A, B, Cc, D, E = u @ u, u @ w, w @ w, u @ r, w @ r
    cands = []
    den = A * Cc - B * B
    if den > 0:
        s, t = (B * E - Cc * D) / den, (A * E - B * D) / den
        if 0 <= s <= 1 and 0 <= t <= 1:
            cands.append((s, t))
    for s in (LD(0), LD(1)):                                            # the clamped sides
        t = (E + s * B) / Cc if Cc > 0 else LD(0)
        cands.append((s, min(max(t, LD(0)), LD(1))))
    for t in (LD(0), LD(1)):
        s = (t * B - D) / A if A > 0 else LD(0)
        cands.append((min(max(s, LD(0)), LD(1)), t))
    best = None
    for s, t in cands:
        p, q = a + s * u, c + t * w
        dd = (p - q) @ (p - q)
        if best is None or dd < best[0] or (dd == best[0] and s < best[1]):
            best = (dd, s, p, q)
    return best[2], best[3]


def collide(a, b, r, tri):
    """The rule of include/clapgpu.h for segment a-b (a == b: a sphere), radius r and one triangle [3, 3]:
    (contacts [(pos, normal, depth)], margin, rule) with rule in {0: none, 3: face, 4: parallel, 5: closest}"""
    a, b, r = _v(a), _v(b), LD(float(r))
    v = _v(tri)
    v0, e1, e2 = v[0], v[1] - v[0], v[2] - v[0]
    n = np.cross(e1, e2)
    if not n.any():
        return [], False, 0
    scale = LD(1) + max(abs(v).max(), abs(a).max(), abs(b).max(), r)
    tol = LD(2 ** 12 * EPS) * scale                                     # lengths: fp64 rounding of the kernel, generously
    nl = np.sqrt(n @ n)
    nh = n / nl
    sa, sb = (a - v0) @ nh, (b - v0) @ nh
    m = min(sa, sb)
    e = b if sb < sa else a
    point = bool(np.all(a == b))
    margin = False
    area = nl                                                           # |e1 x e2|
    btol = tol * scale / area                                           # barycentric tolerance

    def inside(x):
        nonlocal margin
        w = _bary(v0, e1, e2, x)
        if abs(w).min() <= btol:
            margin = True
        return bool(w.min() >= 0)

    # 3. the face
    if abs(sa) <= tol and abs(sb) <= tol and not point:
        margin = True                                                   # (near-)coplanar segments: not pinned here
    crosses = False
    if (sa <= 0 <= sb) or (sb <= 0 <= sa):
        if abs(sa) <= tol or abs(sb) <= tol:
            margin = True
        if point:
            crosses = inside(a)
        else:
            vols = [np.linalg.det(np.stack([b - a, v[k] - a, v[(k + 1) % 3] - a]).astype(np.float64)) for k in range(3)]
            vols = [LD(x) for x in vols]
            vt = tol * scale * scale
            if min(abs(x) for x in vols) <= vt:
                margin = True
            crosses = all(x >= 0 for x in vols) or all(x <= 0 for x in vols)
    face = crosses
    if not face and -r < m <= 0:
        if abs(m + r) <= tol or abs(m) <= tol:
            margin = True
        face = inside(e)
    elif not face and (abs(m + r) <= tol or abs(m) <= tol):
        margin = True
    if face:
        return [(e - m * nh, nh, r - m)], margin, 3
    # 4. parallel
    if not point and m > 0:
        L = np.sqrt((b - a) @ (b - a))
        lim = LD(1e-5) * L
        hi = max(sa, sb)
        if abs(abs(sa - sb) - lim) <= tol or abs(hi - r) <= tol:
            margin = True
        if abs(sa - sb) <= lim and hi <= r:
            ia, ib = inside(a), inside(b)
            if ia and ib:
                return [(a - sa * nh, nh, r - sa), (b - sb * nh, nh, r - sb)], margin, 4
    # 5. the closest points
    best = None
    for x, sx in ((a, sa), (b, sb)) if not point else ((a, sa),):
        w = _bary(v0, e1, e2, x)
        if w.min() >= 0:
            q = x - sx * nh
            dd = (x - q) @ (x - q)
            if best is None or dd < best[0]:
                best = (dd, x, q)
    for k in range(3):
        p, q = _seg_seg(a, b, v[k], v[(k + 1) % 3])
        dd = (p - q) @ (p - q)
        if best is None or dd < best[0]:
            best = (dd, p, q)
    _dd, p, q = best
    pq = p - q
    d = np.sqrt(pq @ pq)
    if abs(d - r) <= tol or d <= tol:
        margin = True
    side = (pq @ nh)
    if abs(side) <= tol:
        margin = True
    if d > 0 and d <= r and side > 0:
        return [(q, pq / d, r - d)], margin, 5
    return [], margin, 0


class Pair:
    """The truth of one (body, mesh) pair: records [(tri, contacts, margin)] in triangle order, the kept ones, capped."""

    def __init__(self, a, b, r, tris, lo=None, hi=None):
        a, b = np.asarray(a, float), np.asarray(b, float)
        blo, bhi = np.minimum(a, b) - r, np.maximum(a, b) + r
        tlo, thi = tris.min(1), tris.max(1)
        pad = 1e-9 * (1 + np.abs(blo).max() + np.abs(bhi).max() + r)
        cand = np.nonzero(np.all(tlo <= bhi + pad, 1) & np.all(thi >= blo - pad, 1))[0]
        self.records, self.near = [], []
        for t in cand:
            cs, mg, _rule = collide(a, b, r, tris[t])
            if cs:
                self.records.append((int(t), cs, mg))
            elif mg:
                self.near.append(int(t))
        # MAX_CONTACTS: deeper first (a record's depth: its deeper contact), then lower triangle; while they fit
        order = sorted(self.records, key=lambda rec: (-max(c[2] for c in rec[1]), rec[0]))
        used, kept = 0, []
        for rec in order:
            if used + len(rec[1]) > MAX_CONTACTS:
                break
            used += len(rec[1])
            kept.append(rec)
        self.kept = sorted(kept, key=lambda rec: rec[0])
        self.capped = len(kept) < len(self.records)


def segment_of(pos, axis, length):
    """a body geom's segment: a capsule's ends pos +- axis * length / 2 (a first), a sphere's centre twice"""
    pos = np.asarray(pos, float)
    if length == 0:
        return pos.copy(), pos.copy()
    h = np.asarray(axis, float) * (length * 0.5)
    return pos + h, pos - h


def sweep(gp, radius, length, axis, delta, tris):
    """phys_body_sweep_capsule (physics.c:559-670) in numpy float32 where the reference uses float, against one mesh
    candidate: its contacts at every step in ascending triangle index from collide(), 16 per step at most.
    -> (frac, normal[3], touched: a mesh contact was taken)"""
    f32 = np.float32
    delta = np.asarray(delta, f32)
    dl = np.sqrt(f32(delta[0] * delta[0] + delta[1] * delta[1]) + f32(delta[2] * delta[2]), dtype=f32)
    best_frac, best_n, hit = f32(1.0), np.array([0, 1, 0], f32), False
    if dl < f32(1e-6):
        return best_frac, best_n, hit
    k = f32(1.0) / dl
    dirv = (delta * k).astype(f32)
    nsteps = int(np.ceil(f32(float(dl) / (float(radius) * 0.5))))
    nsteps = max(nsteps, 2)
    for s in range(1, nsteps + 1):
        t = f32(f32(s) / f32(nsteps))
        pos = np.array([gp[i] + float(f32(delta[i] * t)) for i in range(3)])
        a, b = segment_of(pos, axis, length)
        p = Pair(a, b, radius, tris)
        taken = 0
        for _tri, cs, _mg in p.records:
            for c in cs:
                if taken >= MAX_CONTACTS:
                    break
                taken += 1
                cn = np.asarray(c[1], np.float64).astype(f32)
                ndot = f32(f32(f32(dirv[0] * cn[0]) + f32(dirv[1] * cn[1])) + f32(dirv[2] * cn[2]))
                if ndot > f32(-0.1):
                    continue
                backup = f32(float(c[2]) / -float(ndot))
                safe = f32(f32(t * dl) - backup)
                if safe < 0:
                    safe = f32(0)
                frac = f32(safe / dl)
                if frac < best_frac:
                    best_frac, best_n, hit = frac, cn, True
        if best_frac < t:
            break
    return best_frac, best_n, hit
