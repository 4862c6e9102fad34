// ray_tri_dev.h -- one ray against the triangles of a mesh set, as ray_trimesh.hip's k_ray_trimesh and camera.hip's
// k_camera_calc run it: the ray's shear, the pruned slab test of the BVH walk (trimesh_dev.h) and the watertight
// ray-triangle test.  The test and the tie rule are described at the head of ray_trimesh.hip.
#pragma once
#include "common.h"
#include "phys_dev.h"
#include "trimesh_dev.h"
#include "tricontact_dev.h"
#include "ray_dev.h"

namespace clapgpu {

constexpr uint32_t NO_SLOT = 0xffffffffu;

struct Shear {
    int kx, ky, kz;
    double Sx, Sy, Sz;
    double inv[3];
};

__device__ __forceinline__ double pick(const double (&v)[3], int k) { return k == 0 ? v[0] : k == 1 ? v[1] : v[2]; }

__device__ __forceinline__ void shear_of(const Ray &r, Shear &q)
{
    const double ax = fabs(r.u[0]), ay = fabs(r.u[1]), az = fabs(r.u[2]);
    q.kz = ax >= ay ? (ax >= az ? 0 : 2) : (ay >= az ? 1 : 2);
    q.kx = q.kz == 2 ? 0 : q.kz + 1;
    q.ky = q.kx == 2 ? 0 : q.kx + 1;
    const double uz = pick(r.u, q.kz);
    if (uz < 0) { const int t = q.kx; q.kx = q.ky; q.ky = t; }                 // keeps the winding
    q.Sx = pick(r.u, q.kx) / uz;
    q.Sy = pick(r.u, q.ky) / uz;
    q.Sz = 1.0 / uz;
    for (int a = 0; a < 3; a++) q.inv[a] = r.u[a] == 0 ? 0.0 : 1.0 / r.u[a];             // 0: see box_hit
}

// where the segment [0, tmax] enters a float box, conservatively: a box holding a hit point at t <= tmax passes.  An axis
// the ray does not move along is a containment test (a start on the slab's face is inside it)
__device__ __forceinline__ bool box_hit(const Ray &r, const Shear &q, const float *b, double tmax, double &tn)
{
    double lo = 0.0, hi = INFINITY;
    for (int a = 0; a < 3; a++) {
        const double ta = ((double)b[a] - r.s[a]) * q.inv[a], tb = ((double)b[3 + a] - r.s[a]) * q.inv[a];
        const bool in = (double)b[a] <= r.s[a] && r.s[a] <= (double)b[3 + a];
        const bool flat = r.u[a] == 0;
        lo = fmax(lo, flat ? (in ? -INFINITY : INFINITY) : fmin(ta, tb));
        hi = fmin(hi, flat ? (in ? INFINITY : -INFINITY) : fmax(ta, tb));
    }
    tn = lo;
    return lo * (1.0 - 0x1p-48) <= fmin(hi * (1.0 + 0x1p-48), tmax);
}

struct MeshBest { double t; uint32_t key, tri, slot; };

__device__ __forceinline__ void test_tri(const MeshSet &m, const Ray &r, const Shear &q, uint32_t slot, uint32_t skip_key,
                                         MeshBest &b)
{
    const uint2 kt = m.key[slot];
    const uint32_t key = KEY_STATIC | kt.x;
    if (key == skip_key) return;
    const double *v = m.tri + 9 * (size_t)slot;
    const double A[3] = { v[0] - r.s[0], v[1] - r.s[1], v[2] - r.s[2] };
    const double B[3] = { v[3] - r.s[0], v[4] - r.s[1], v[5] - r.s[2] };
    const double C[3] = { v[6] - r.s[0], v[7] - r.s[1], v[8] - r.s[2] };
    const double Az = pick(A, q.kz), Bz = pick(B, q.kz), Cz = pick(C, q.kz);
    const double Ax = pick(A, q.kx) - q.Sx * Az, Ay = pick(A, q.ky) - q.Sy * Az;
    const double Bx = pick(B, q.kx) - q.Sx * Bz, By = pick(B, q.ky) - q.Sy * Bz;
    const double Cx = pick(C, q.kx) - q.Sx * Cz, Cy = pick(C, q.ky) - q.Sy * Cz;
    const double U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if (!(U >= 0 && V >= 0 && W >= 0)) return;                              // outside, or a back face
    const double det = U + V + W;
    if (!(det > 0)) return;                                                   // edge-on or parallel
    const double T = U * (q.Sz * Az) + V * (q.Sz * Bz) + W * (q.Sz * Cz);
    const double t = T / det;
    if (!(t >= 0 && t <= r.len)) return;
    if (!(t < b.t || (t == b.t && (key < b.key || (key == b.key && kt.y < b.tri))))) return;
    double n[3];
    phd::tri_normal(v, n);
    if (n[0] == 0 && n[1] == 0 && n[2] == 0) return;                          // zero area: never a hit
    b.t = t; b.key = key; b.tri = kt.y; b.slot = slot;
}

} // namespace clapgpu
