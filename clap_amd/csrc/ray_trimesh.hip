// ray_trimesh.hip -- the mesh pass of the ray casts, for gfx950:
//
//   k_ray_trimesh   behind rays.hip's k_ray_cast (<false>) or k_ground_rays (<true>) when a mesh set is given: one lane
//                   per ray, the walk of the mesh set's BVH (trimesh_dev.h; built by trimesh.hip) and the watertight
//                   ray-triangle test, merged with the best hit the first pass found
//
// The rays, the hit keys, the ground ray's decision and the pass's arguments (MeshPass) are ray_dev.h's.
#include "common.h"
#include "phys_dev.h"
#include "trimesh_dev.h"
#include "tricontact_dev.h"
#include "ray_dev.h"

namespace clapgpu {

constexpr int RT = WAVE;                                // one wave per workgroup (the walk's LDS stack)

// The pass behind k_ray_cast / k_ground_rays when a mesh set is given: those wrote the best hit, the flags and `other`
// of every ray and left the statics that own a mesh alone.
//
// The test: ODE's dCollideRTL runs OPCODE's float ray-triangle test with ClosestHit = 1, BackfaceCull = 1 (physics.c:485-487).
// Here the triangles are tested in fp64 with the watertight test of Woop, Benthin and Wald (JCGT 2013): the ray's dominant
// axis is z, the other two are sheared onto it once per ray, and the three edge functions U, V, W of the projected
// triangle decide.  A shared edge gets the same edge function with opposite sign in both triangles (the products
// commute and the difference is negated exactly; no FMA contraction), so a ray through an edge or a vertex of front faces
// hits at least one of them: no ray falls through the terrain.  Front face: U, V, W >= 0 and det = U + V + W > 0, which is
// u . n < 0 for n = (v1 - v0) x (v2 - v0).  n == 0 never hits (ODE's dSafeNormalize3 fails there); a hit needs
// 0 <= depth <= length.  Contact: pos = start + depth * u, normal = n / |n| (dSafeNormalize3), pointing back towards the
// start.  Our reading is that dCollideRTL forms the reversed cross product and dCollide flips it again when it swaps
// (trimesh, ray) into (ray, trimesh); ODE is an absent submodule of the reference, so this is PARITY UNPINNED.
//
// Ties: the smallest depth, then bodies before statics, then the lower static index, then the lower triangle index of
// the mesh.  The walk prunes with the best depth so far inclusively (the ray's length while there is none), enters the
// nearer child first, and takes the minimum of (depth, key, triangle), which does not depend on the order the leaves
// are reached in.
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

template <bool GROUND>
__global__ __launch_bounds__(RT)
void k_ray_trimesh(MeshSet m, MeshPass p)
{
    __shared__ uint32_t stk[TM_STACK * RT];
    const uint32_t j = blockIdx.x * RT + threadIdx.x;
    if (j >= p.n) return;
    Ray r;
    double ray_len = 0;
    uint32_t i = 0, skip_key;
    if (GROUND) {
        i = p.body[j];
        if (i >= p.n_bodies || (p.flags[j] & CLAPGPU_RAY_INVALID)) return;   // decided by the first pass
        ground_ray(p.pos, p.yoffset, i, p.ray_off[j], r, ray_len);
        skip_key = i;
    } else {
        if (!make_ray(p.ray + 8 * (size_t)j, r)) return;
        skip_key = skip_key_of(p.skip ? p.skip[j] : -1);
    }
    MeshBest b;
    b.key = key_of(p.hit[j]);
    b.t = b.key == KEY_NONE ? r.len : p.dist[j];        // the walk stays within the segment (KEY_NONE: t == len still wins)
    b.tri = 0;
    b.slot = NO_SLOT;
    Shear q;
    shear_of(r, q);
    bvh_walk(m, stk + threadIdx.x,
             [&](const float *box, double &tn) { return box_hit(r, q, box, b.t, tn); },   // b.t tightens as leaves are visited
             [&](uint32_t slot) { test_tri(m, r, q, slot, skip_key, b); });
    const bool won = b.slot != NO_SLOT;
    double nrm[3] = { 0, 0, 0 };
    if (won) {
        phd::tri_normal(m.tri + 9 * (size_t)b.slot, nrm);
        phd::safe_normalize3(nrm);
    }
    const uint32_t f = p.other ? unresolved(p.other[j], r.len, b.key, b.t) : 0u;
    if (GROUND) {
        ground_decide(j, i, ray_len, b.key, b.t, nrm, won, f, p.grounded, p.grounded_out, p.normal, p.dist, p.hit,
                      p.flags, p.moved);
    } else {
        if (won) {                                       // k_ray_cast's (rays.hip) stores of the hit, restated
            p.hit[j] = hit_of(b.key);
            p.dist[j] = b.t;
            if (p.contact)
                for (int a = 0; a < 3; a++) {
                    p.contact[6 * (size_t)j + a] = r.s[a] + b.t * r.u[a];
                    p.contact[6 * (size_t)j + 3 + a] = nrm[a];
                }
        }
        if (p.flags) p.flags[j] = f;
    }
}

// the mesh pass over p.n > 0 rays (declared in ray_dev.h)
int mesh_pass(hipStream_t s, const clapgpu_trimesh *meshes, const MeshPass &p)
{
    const MeshSet m = trimesh_set(meshes);
    const dim3 grid((p.n + RT - 1) / RT);
    if (p.ray) hipLaunchKernelGGL(k_ray_trimesh<false>, grid, dim3(RT), 0, s, m, p);
    else hipLaunchKernelGGL(k_ray_trimesh<true>, grid, dim3(RT), 0, s, m, p);
    CLAPGPU_LAUNCH_CHECK("k_ray_trimesh");
    return CLAPGPU_OK;
}

} // namespace clapgpu
