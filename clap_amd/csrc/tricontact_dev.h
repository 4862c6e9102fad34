// tricontact_dev.h -- a sphere or capsule against one static triangle, shared by the mesh contact pass and the capsule
// sweep against meshes (mesh_contacts.hip, contacts.hip), and the triangle normal every mesh kernel uses (tri_normal; ray_trimesh.hip too).
// fp64, no FMA contraction (the Makefile builds with -ffp-contract=off).
//
// The body geom is a segment a, b with radius r (a sphere: a == b); the triangle is (v0, v1, v2) as the mesh set bakes
// it (trimesh.hip).  This is the project's own contract: ODE's trimesh colliders (dCollideSTL / dCollideCCTL, OPCODE)
// live in an absent submodule of the reference and are not restated here.  The rule (include/clapgpu.h):
//   1. n = (v1 - v0) x (v2 - v0); n == 0: no contact; else n^ = n / |n|
//   2. sa, sb = (a - v0) . n^, (b - v0) . n^; m = min(sa, sb); e = the endpoint attaining m (a on a tie)
//   3. face: the segment meets the closed triangle, or -r < m <= 0 and e projects into the closed triangle:
//      one contact, normal n^, depth r - m, pos e - m n^
//   4. parallel: a != b, m > 0, |sa - sb| <= 1e-5 |b - a|, both endpoints project into the triangle, max(sa, sb) <= r:
//      two contacts at the endpoints' projections, normal n^, depths r - sa and r - sb (a's first)
//   5. otherwise the closest points p (segment) and q (triangle) at distance d: a contact when 0 < d <= r and
//      (p - q) . n > 0: normal (p - q) / d, depth r - d, pos q.  Behind the face: none (a neighbour's contact, or nothing)
// Normals point from the static towards the body, as in sphere-box.  Depth >= 0 is a contact.
#pragma once
#include "phys_dev.h"

namespace phd {

PHD void sub3(const double *x, const double *y, double (&o)[3]) { o[0] = x[0] - y[0]; o[1] = x[1] - y[1]; o[2] = x[2] - y[2]; }

PHD void cross3(const double (&x)[3], const double (&y)[3], double (&o)[3])
{
    o[0] = x[1] * y[2] - x[2] * y[1];
    o[1] = x[2] * y[0] - x[0] * y[2];
    o[2] = x[0] * y[1] - x[1] * y[0];
}

// n = (v1 - v0) x (v2 - v0) of a baked triangle v[9], not normalised: the one normal of the mesh rays (ray_trimesh.hip) and of
// the rule above
PHD void tri_normal(const double *v, double (&n)[3])
{
    double e1[3], e2[3];
    sub3(v + 3, v, e1);
    sub3(v + 6, v, e2);
    cross3(e1, e2, n);
}

// ((v_k+1 - v_k) x (x - v_k)) . n >= 0 for every edge: x (anywhere along n) projects into the closed triangle
PHD bool projects_inside(const double *v, const double (&n)[3], const double *x)
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int k1 = k == 2 ? 0 : k + 1;
        double ed[3], dx[3], c[3];
        sub3(v + 3 * k1, v + 3 * k, ed);
        sub3(x, v + 3 * k, dx);
        cross3(ed, dx, c);
        if (!(dot3(c, n) >= 0)) return false;
    }
    return true;
}

// segment a-b within the triangle's plane (sa == sb == 0) meets the closed triangle
PHD bool coplanar_meets(const double *v, const double (&n)[3], const double (&a)[3], const double (&b)[3])
{
    if (projects_inside(v, n, a) || projects_inside(v, n, b)) return true;
    double ab[3];
    sub3(b, a, ab);
    for (int k = 0; k < 3; k++) {
        const int k1 = k == 2 ? 0 : k + 1;
        double ed[3], d0[3], d1[3], da[3], db[3], c[3];
        sub3(v + 3 * k1, v + 3 * k, ed);
        sub3(v + 3 * k, a, d0);
        sub3(v + 3 * k1, a, d1);
        sub3(a, v + 3 * k, da);
        sub3(b, v + 3 * k, db);
        cross3(ab, d0, c); const double o1 = dot3(c, n);
        cross3(ab, d1, c); const double o2 = dot3(c, n);
        cross3(ed, da, c); const double o3 = dot3(c, n);
        cross3(ed, db, c); const double o4 = dot3(c, n);
        if (o1 == 0 && o2 == 0) continue;                       // collinear with the edge: the other edges decide
        if (((o1 <= 0 && o2 >= 0) || (o1 >= 0 && o2 <= 0)) && ((o3 <= 0 && o4 >= 0) || (o3 >= 0 && o4 <= 0))) return true;
    }
    return false;
}

// the segment a-b (a != b) and the edge v_k v_k+1: closest points (dClosestLineSegmentPoints); a sphere: the point
// against the edge
PHD void closest_to_edge(const double (&a)[3], const double (&b)[3], bool point, const double *p0, const double *p1,
                         double (&cp)[3], double (&cq)[3])
{
    const double e0[3] = { p0[0], p0[1], p0[2] }, e1[3] = { p1[0], p1[1], p1[2] };
    if (!point) {
        closest_segment_points(a, b, e0, e1, cp, cq);
        return;
    }
    double ed[3], d[3];
    sub3(p1, p0, ed);
    sub3(a, p0, d);
    double t = dot3(d, ed) / dot3(ed, ed);                        // the edge has length: n != 0
    t = t > 0 ? (t < 1 ? t : 1.0) : 0.0;
    for (int i = 0; i < 3; i++) { cp[i] = a[i]; cq[i] = p0[i] + t * ed[i]; }
}

// the rule above: 0, 1 or 2 contacts (c0, c1)
PHD int collide_segment_triangle(const double (&a)[3], const double (&b)[3], double r, const double *v, CGeom &c0, CGeom &c1)
{
    double n[3];
    tri_normal(v, n);
    if (n[0] == 0 && n[1] == 0 && n[2] == 0) return 0;
    const double nl = sqrt(dot3(n, n));
    const double nh[3] = { n[0] / nl, n[1] / nl, n[2] / nl };
    double da[3], db[3];
    sub3(a, v, da);
    sub3(b, v, db);
    const double sa = dot3(da, nh), sb = dot3(db, nh);
    const bool eb = sb < sa;
    const double m = eb ? sb : sa;
    const double *e = eb ? b : a;
    const bool point = a[0] == b[0] && a[1] == b[1] && a[2] == b[2];
    // 3. the face
    bool face;
    if ((sa > 0 && sb > 0) || (sa < 0 && sb < 0)) face = false;
    else if (sa == sb) face = coplanar_meets(v, n, a, b);                    // both 0
    else if (sa == 0) face = projects_inside(v, n, a);
    else if (sb == 0) face = projects_inside(v, n, b);
    else {
        const double t = sa / (sa - sb);
        const double x[3] = { a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), a[2] + t * (b[2] - a[2]) };
        face = projects_inside(v, n, x);
    }
    if (!face && -r < m && m <= 0) face = projects_inside(v, n, e);
    if (face) {
        for (int i = 0; i < 3; i++) { c0.normal[i] = nh[i]; c0.pos[i] = e[i] - m * nh[i]; }
        c0.depth = r - m;
        return 1;
    }
    // 4. parallel above the face
    if (!point && m > 0) {
        double ab[3];
        sub3(b, a, ab);
        const double ls = sqrt(dot3(ab, ab));
        const double hi = sa > sb ? sa : sb;
        if (fabs(sa - sb) <= 1e-5 * ls && hi <= r && projects_inside(v, n, a) && projects_inside(v, n, b)) {
            for (int i = 0; i < 3; i++) {
                c0.normal[i] = nh[i]; c0.pos[i] = a[i] - sa * nh[i];
                c1.normal[i] = nh[i]; c1.pos[i] = b[i] - sb * nh[i];
            }
            c0.depth = r - sa;
            c1.depth = r - sb;
            return 2;
        }
    }
    // 5. the closest points: an endpoint over the face, or the segment against an edge (the segment does not meet the
    // triangle here, so one of these attains the distance); strict < keeps the first of a tie
    double bp[3], bq[3], bd2 = INFINITY;
    for (int s = 0; s < (point ? 1 : 2); s++) {
        const double *x = s ? b : a;
        const double sx = s ? sb : sa;
        if (projects_inside(v, n, x)) {
            const double q[3] = { x[0] - sx * nh[0], x[1] - sx * nh[1], x[2] - sx * nh[2] };
            double dd[3];
            sub3(x, q, dd);
            const double d2 = dot3(dd, dd);
            if (d2 < bd2) { bd2 = d2; for (int i = 0; i < 3; i++) { bp[i] = x[i]; bq[i] = q[i]; } }
        }
    }
    for (int k = 0; k < 3; k++) {
        double cp[3], cq[3], dd[3];
        closest_to_edge(a, b, point, v + 3 * k, v + 3 * (k == 2 ? 0 : k + 1), cp, cq);
        sub3(cp, cq, dd);
        const double d2 = dot3(dd, dd);
        if (d2 < bd2) { bd2 = d2; for (int i = 0; i < 3; i++) { bp[i] = cp[i]; bq[i] = cq[i]; } }
    }
    double pq[3];
    sub3(bp, bq, pq);
    const double d = sqrt(dot3(pq, pq));
    if (!(d > 0 && d <= r && dot3(pq, n) > 0)) return 0;
    for (int i = 0; i < 3; i++) { c0.normal[i] = pq[i] / d; c0.pos[i] = bq[i]; }
    c0.depth = r - d;
    return 1;
}

// a body geom as the segment of the rule: a capsule's ends pos +- axis * length / 2 (ODE's p1, p2), a sphere's centre
// twice; false: a kind without a triangle collider here (boxes, OTHER)
PHD bool geom_segment(const Geom &g, double (&a)[3], double (&b)[3])
{
    if (g.kind == 0) {
        for (int i = 0; i < 3; i++) a[i] = b[i] = g.pos[i];
        return true;
    }
    if (g.kind != 1) return false;
    const double h = g.length * 0.5;
    for (int i = 0; i < 3; i++) { a[i] = g.pos[i] + g.axis[i] * h; b[i] = g.pos[i] - g.axis[i] * h; }
    return true;
}

} // namespace phd
