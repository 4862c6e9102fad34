// ray_dev.h -- what the scene cast (rays.hip) and the mesh pass behind it (ray_trimesh.hip) share: the ray as dGeomRaySet
// stores it, the hit keys, phys_body_ground_collide's ray and its decision, the UNRESOLVED rule, and the mesh pass's
// arguments and launcher.  fp64 throughout, no FMA contraction.
#pragma once
#include "common.h"
#include "phys_dev.h"

struct clapgpu_trimesh;

namespace clapgpu {

// ------------------------------------------------------------------------------------------------- rays and hit keys
constexpr uint32_t KEY_NONE = 0xffffffffu, KEY_STATIC = 0x80000000u;   // body i: i; static s: KEY_STATIC | s

struct Ray { double s[3], u[3], len; };

// the ray as dGeomRaySet stores it; false: CLAPGPU_RAY_INVALID
__device__ __forceinline__ bool make_ray(const double *in, Ray &r)
{
    double d[3] = { in[3], in[4], in[5] };
    r.s[0] = in[0]; r.s[1] = in[1]; r.s[2] = in[2];
    r.len = in[6];
    const bool finite_dir = isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]);
    if (!finite_dir || (d[0] == 0 && d[1] == 0 && d[2] == 0) || r.s[0] != r.s[0] || r.s[1] != r.s[1] || r.s[2] != r.s[2] ||
        !(r.len >= 0))
        return false;
    phd::safe_normalize3(d);                                                 // dNormalize3
    r.u[0] = d[0]; r.u[1] = d[1]; r.u[2] = d[2];
    return true;
}

__device__ __forceinline__ uint32_t skip_key_of(int32_t skip)
{
    return skip >= 0 ? (uint32_t)skip : skip <= -2 ? KEY_STATIC | (uint32_t)(-2 - skip) : KEY_NONE;
}

__device__ __forceinline__ int32_t hit_of(uint32_t key)
{
    return key == KEY_NONE ? -1 : (key & KEY_STATIC) ? -2 - (int32_t)(key & ~KEY_STATIC) : (int32_t)key;
}

__device__ __forceinline__ uint32_t key_of(int32_t hit)
{
    return hit == -1 ? KEY_NONE : hit >= 0 ? (uint32_t)hit : KEY_STATIC | (uint32_t)(-2 - hit);
}

// phys_body_ground_collide's ray for body i: start (float) below the body's position, straight down, 2 * ray_len long;
// false: CLAPGPU_RAY_INVALID
__device__ __forceinline__ bool ground_ray(const double *pos, const double *yoffset, uint32_t i, double ray_off, Ray &r,
                                           double &ray_len)
{
    double roff;
    ray_len = phd::ground_ray_len(ray_off, yoffset[i], roff);
    const double *p = pos + 3 * (size_t)i;
    const float start[3] = { (float)p[0], (float)(p[1] - roff), (float)p[2] };   // through a vec3
    r.s[0] = start[0]; r.s[1] = start[1]; r.s[2] = start[2];
    r.u[0] = 0.0; r.u[1] = -1.0; r.u[2] = 0.0;
    r.len = ray_len * 2;
    return r.len >= 0 && r.s[0] == r.s[0] && r.s[1] == r.s[1] && r.s[2] == r.s[2];
}

// ... and its decision on the (final) hit of ray j for body i: hit / dist / grounded_out / flags, the float normal (unless
// write_nrm is false: already written), and bit 0 of moved[i] when the apply launch is to move the body
__device__ __forceinline__ void ground_decide(uint32_t j, uint32_t i, double ray_len, uint32_t key, double depth,
                                              const double (&nrm)[3], bool write_nrm, uint32_t f, const uint8_t *grounded,
                                              uint8_t *grounded_out, float *normal,
                                              double *dist, int32_t *hit, uint32_t *flags, uint32_t *moved)
{
    bool res = false;
    hit[j] = hit_of(key);
    if (key != KEY_NONE && !f) {
        if (write_nrm)
            for (int a = 0; a < 3; a++) normal[3 * (size_t)j + a] = (float)nrm[a];
        float dy;
        bool mv;
        res = phd::ground_branch(depth, ray_len, grounded[j] != 0, dy, mv);
        if (mv) atomicOr(&moved[i], 1u);
    }
    if (key != KEY_NONE) dist[j] = depth;
    grounded_out[j] = res ? 1 : 0;
    flags[j] = f;
}

// the UNRESOLVED rule on a ray's final hit: the segment enters an OTHER static without a mesh (first entry `other`)
// before the hit, or there is no hit
__device__ __forceinline__ uint32_t unresolved(double other, double len, uint32_t key, double depth)
{
    return (other <= len && (key == KEY_NONE || other <= depth)) ? CLAPGPU_RAY_UNRESOLVED : 0u;
}

// ------------------------------------------------------------------------------------------------- the mesh pass
// Cast rays: ray / skip / dist / hit / contact / flags as clapgpu_ray_cast.  Ground rays (ray == NULL): the rays of
// clapgpu_bodies_ground_collide, and the decision on the merged hit.
struct MeshPass {
    uint32_t n;
    const double *ray;                   // cast rays [n][8]; NULL: ground rays
    const int32_t *skip;
    double *dist, *contact;
    int32_t *hit;
    uint32_t *flags;
    const double *other;                 // [n] first entry into an OTHER static without a mesh (first pass)
    // ground rays
    uint32_t n_bodies;
    const double *pos, *yoffset, *ray_off;
    const uint32_t *body;
    const uint8_t *grounded;
    uint8_t *grounded_out;
    float *normal;
    uint32_t *moved;
};

// ray_trimesh.hip: the mesh pass over p.n > 0 rays, behind the first pass on the same stream
__attribute__((visibility("hidden"))) int mesh_pass(hipStream_t s, const clapgpu_trimesh *meshes, const MeshPass &p);

} // namespace clapgpu
