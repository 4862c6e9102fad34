// ray_colliders_dev.h -- a ray against one geom, for the scene cast (rays.hip).  Include it after ray_dev.h.
//
// The colliders restate ODE 0.16's ray.cpp (dCollideRaySphere + ray_sphere_helper, dCollideRayCapsule, dCollideRayBox)
// for the flags physics.c:485-487 sets; a box is its AABB.  ODE is an absent submodule of the reference: PARITY UNPINNED.
// One deliberate difference: a hit needs 0 <= depth <= length as written, so NaN geometry never hits.
// fp64 throughout, no FMA contraction.
#pragma once
#include "ray_dev.h"

namespace clapgpu {

// ray_sphere_helper (ray.cpp): mode = the ray starts inside the capsule this cap belongs to
__device__ __forceinline__ bool ray_sphere(const Ray &r, const double (&c)[3], double radius, bool mode, phd::CGeom &o)
{
    const double q[3] = { r.s[0] - c[0], r.s[1] - c[1], r.s[2] - c[2] };
    const double B = q[0] * r.u[0] + q[1] * r.u[1] + q[2] * r.u[2];
    const double C = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] - radius * radius;
    double k = B * B - C;                                // C <= 0: the start is inside the sphere
    if (k < 0) return false;
    k = sqrt(k);
    double alpha;
    if (mode && C >= 0) {
        alpha = -B + k;
        if (alpha < 0) return false;
    } else {
        alpha = -B - k;
        if (alpha < 0) {
            alpha = -B + k;                              // inside: the exit point
            if (alpha < 0) return false;
        }
    }
    if (!(alpha >= 0 && alpha <= r.len)) return false;
    for (int a = 0; a < 3; a++) o.pos[a] = r.s[a] + alpha * r.u[a];
    // from inside: the normal points into the solid.  The sign follows C (where the start is), not the root taken: a
    // start exactly on the surface (C == 0) moving outward hits at depth 0 with the OUTWARD normal (clapgpu.h)
    const double nsign = (C < 0 || mode) ? -1.0 : 1.0;
    double n[3] = { nsign * (o.pos[0] - c[0]), nsign * (o.pos[1] - c[1]), nsign * (o.pos[2] - c[2]) };
    phd::safe_normalize3(n);
    o.normal[0] = n[0]; o.normal[1] = n[1]; o.normal[2] = n[2];
    o.depth = alpha;
    return true;
}

// dCollideRayCapsule (ray.cpp); axis = column 2 of the geom's R, lz = the cylinder length
__device__ __forceinline__ bool ray_capsule(const Ray &r, const double (&p)[3], const double (&axis)[3], double radius, double lz,
                                           phd::CGeom &o)
{
    const double lz2 = lz * 0.5;
    const double cs[3] = { r.s[0] - p[0], r.s[1] - p[1], r.s[2] - p[2] };
    double k = axis[0] * cs[0] + axis[1] * cs[1] + axis[2] * cs[2];          // the start's position along the axis
    double q[3] = { k * axis[0] - cs[0], k * axis[1] - cs[1], k * axis[2] - cs[2] };
    const double C = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] - radius * radius;
    bool inside = false;                                                     // C < 0: inside the infinite cylinder
    if (C < 0) {
        if (k < -lz2) k = -lz2;
        else if (k > lz2) k = lz2;
        const double rr[3] = { p[0] + k * axis[0], p[1] + k * axis[1], p[2] + k * axis[2] };
        const double d[3] = { r.s[0] - rr[0], r.s[1] - rr[1], r.s[2] - rr[2] };
        if (d[0] * d[0] + d[1] * d[1] + d[2] * d[2] < radius * radius) inside = true;
    }
    if (!inside && C < 0) {
        k = k < 0 ? -lz2 : lz2;                                              // outside, within the cylinder: a cap only
    } else {
        const double uv = axis[0] * r.u[0] + axis[1] * r.u[1] + axis[2] * r.u[2];
        const double rv[3] = { uv * axis[0] - r.u[0], uv * axis[1] - r.u[1], uv * axis[2] - r.u[2] };
        double A = rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2];
        if (A == 0) {                                                        // parallel to the axis
            k = uv < 0 ? -lz2 : lz2;
        } else {
            const double B = 2 * (q[0] * rv[0] + q[1] * rv[1] + q[2] * rv[2]);
            k = B * B - 4 * A * C;
            if (k < 0) {
                if (!inside) return false;
                k = uv < 0 ? -lz2 : lz2;
            } else {
                k = sqrt(k);
                A = 1.0 / (2 * A);
                double alpha = (-B - k) * A;
                if (alpha < 0) {
                    alpha = (-B + k) * A;
                    if (alpha < 0) return false;
                }
                if (!(alpha >= 0 && alpha <= r.len)) return false;
                for (int a = 0; a < 3; a++) o.pos[a] = r.s[a] + alpha * r.u[a];
                for (int a = 0; a < 3; a++) q[a] = o.pos[a] - p[a];
                k = q[0] * axis[0] + q[1] * axis[1] + q[2] * axis[2];
                const double nsign = inside ? -1.0 : 1.0;
                if (k >= -lz2 && k <= lz2) {                                 // on the cylinder between the caps
                    double n[3];
                    for (int a = 0; a < 3; a++) n[a] = nsign * (o.pos[a] - (p[a] + k * axis[a]));
                    phd::safe_normalize3(n);
                    o.normal[0] = n[0]; o.normal[1] = n[1]; o.normal[2] = n[2];
                    o.depth = alpha;
                    return true;
                }
                k = k < 0 ? -lz2 : lz2;                                      // beyond a cap: that cap's sphere
            }
        }
    }
    const double c[3] = { p[0] + k * axis[0], p[1] + k * axis[1], p[2] + k * axis[2] };
    return ray_sphere(r, c, radius, inside, o);
}

// dCollideRayBox (ray.cpp) for a box given by its AABB (R = identity, position = centre, side = max - min)
__device__ __forceinline__ bool ray_box(const Ray &r, const double (&bb)[6], phd::CGeom &o)
{
    double s[3], v[3], sign[3], h[3];
    for (int a = 0; a < 3; a++) {
        s[a] = r.s[a] - (bb[2 * a] + bb[2 * a + 1]) * 0.5;
        v[a] = r.u[a];
        if (v[a] < 0) { s[a] = -s[a]; v[a] = -v[a]; sign[a] = 1; }      // mirrored so that v >= 0
        else sign[a] = -1;
        h[a] = 0.5 * (bb[2 * a + 1] - bb[2 * a]);
    }
    if ((s[0] < -h[0] && v[0] <= 0) || s[0] > h[0] || (s[1] < -h[1] && v[1] <= 0) || s[1] > h[1] ||
        (s[2] < -h[2] && v[2] <= 0) || s[2] > h[2] || (v[0] == 0 && v[1] == 0 && v[2] == 0))
        return false;
    double lo = -INFINITY, hi = INFINITY;
    int nlo = 0, nhi = 0;
    for (int a = 0; a < 3; a++) {
        if (v[a] != 0) {
            double k = (-h[a] - s[a]) / v[a];
            if (k > lo) { lo = k; nlo = a; }
            k = (h[a] - s[a]) / v[a];
            if (k < hi) { hi = k; nhi = a; }
        }
    }
    if (lo > hi) return false;
    double alpha;
    int n;
    if (lo >= 0) { alpha = lo; n = nlo; }
    else { alpha = hi; n = nhi; }                        // inside: the exit face, its normal times the entry sign
    if (!(alpha >= 0 && alpha <= r.len)) return false;
    for (int a = 0; a < 3; a++) o.pos[a] = r.s[a] + alpha * r.u[a];
    for (int a = 0; a < 3; a++) o.normal[a] = a == n ? sign[n] : 0.0;
    o.depth = alpha;
    return true;
}

// where the segment enters an AABB (slab test), or +inf if it does not reach it
__device__ __forceinline__ double segment_enters(const Ray &r, const double (&bb)[6])
{
    double t0 = 0.0, t1 = r.len;
    for (int a = 0; a < 3; a++) {
        if (r.u[a] == 0) {
            if (!(r.s[a] >= bb[2 * a] && r.s[a] <= bb[2 * a + 1])) return INFINITY;
        } else {
            double ta = (bb[2 * a] - r.s[a]) / r.u[a], tb = (bb[2 * a + 1] - r.s[a]) / r.u[a];
            if (ta > tb) { const double t = ta; ta = tb; tb = t; }
            if (ta > t0) t0 = ta;
            if (tb < t1) t1 = tb;
        }
    }
    return (t0 <= t1) ? t0 : INFINITY;                   // NaN: not entered
}

} // namespace clapgpu
