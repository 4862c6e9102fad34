// ray_trimesh.hip -- the mesh pass of the ray casts, for gfx950:
//
//   k_ray_trimesh   behind rays.hip's k_ray_cast (<false>) or k_ground_rays (<true>) when a mesh set is given: one lane
//                   per ray, the walk of the mesh set's BVH (trimesh_dev.h; built by trimesh.hip) and the watertight
//                   ray-triangle test, merged with the best hit the first pass found
//
// The rays, the hit keys, the ground ray's decision and the pass's arguments (MeshPass) are ray_dev.h's; the shear, the
// slab test and the triangle test are ray_tri_dev.h's, which camera.hip's k_camera_calc runs too.
#include "common.h"
#include "ray_tri_dev.h"

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
