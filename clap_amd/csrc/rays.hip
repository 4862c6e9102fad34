// rays.hip -- batched ray casts against the device physics scene, for gfx950:
//
//   k_ray_cast      __phys_ray_cast (physics.c:474-524): one dRay against the bodies and statics, the closest hit
//                   that is not the caster; one wavefront per ray, brute force or through an index of the broadphase
//                   grid (clapgpu_bp_index)
//   k_ground_rays   phys_body_ground_collide's ray and decision (physics.c:695-744) for a batch of bodies; the moves
//                   themselves are applied by bodies.hip's k_ground_apply (the device function the step writes
//                   geoms with lives there)
//
// and the entry points of both.  Given a mesh set, either is followed by the mesh pass (ray_trimesh.hip's mesh_pass),
// which merges the triangles of the statics that own a mesh into the best hit written here.  The ray, the hit keys and
// the ground ray's decision are ray_dev.h's, the colliders ray_colliders_dev.h's; one ray's cast on a wavefront (the
// scan, the grid walk, the reduction, cast_scene) is ray_cast_dev.h's, which camera.hip's k_camera_calc runs too.
// fp64 throughout, no FMA contraction.
//
// Grid path: the segment is clipped to the indexed boxes' bounds joined with the statics' (grown by a cell) and cut into
// pieces of at most one cell; the cell range of every piece's box, its blocks' statics and the large list are visited
// through grid_query_dev.h, which says why they hold every geom the piece touches.  Every candidate runs the same
// collider as the brute-force scan and the minimum of (depth, key) does not depend on the order or on duplicates, so
// both paths give the same bits.
#include <string.h>
#include <stdlib.h>
#include "common.h"
#include "ray_cast_dev.h"

namespace clapgpu {

constexpr int RB = 256;                                 // 4 rays per workgroup

// other: NULL, or [n] where a mesh pass follows: the first entry into an OTHER static without a mesh, for its flags
template <bool LEVELED>
__global__ __launch_bounds__(RB)
void k_ray_cast(CastK k, uint32_t n, const double *ray, const int32_t *skip, double *dist, int32_t *hit, double *contact,
                uint32_t *flags, double *other)
{
    const uint32_t i = blockIdx.x * (RB / WAVE) + threadIdx.x / WAVE;
    if (i >= n) return;                                                      // whole waves
    const int lane = lane_id();
    Ray r;
    if (!make_ray(ray + 8 * (size_t)i, r)) {
        if (lane == 0) { hit[i] = -1; if (flags) flags[i] = CLAPGPU_RAY_INVALID; }
        return;
    }
    Best b;
    const uint32_t f = cast<LEVELED>(k, r, skip_key_of(skip ? skip[i] : -1), b);
    if (lane == 0) {
        hit[i] = hit_of(b.key);
        if (b.key != KEY_NONE) {
            dist[i] = b.depth;
            if (contact)
                for (int a = 0; a < 3; a++) { contact[6 * (size_t)i + a] = b.pos[a]; contact[6 * (size_t)i + 3 + a] = b.normal[a]; }
        }
        if (flags) flags[i] = f;
        if (other) other[i] = b.other;
    }
}

// phys_body_ground_collide's cast for body[k] (ground_ray), the body skipped; outputs the hit and the decision.
// moved[body]: bit 0 = the apply launch will move it (unless it is listed twice), bits 1.. = rays cast for it.
// other != NULL: a mesh pass follows and decides; this launch writes the hit so far, its normal (when the flags so far are
// clear: the mesh pass can only clear them) and `other`
template <bool LEVELED>
__global__ __launch_bounds__(RB)
void k_ground_rays(CastK k, uint32_t n, const double *pos, const double *yoffset, const uint32_t *body, const double *ray_off,
                   const uint8_t *grounded, uint8_t *grounded_out, float *normal, double *dist, int32_t *hit, uint32_t *flags,
                   uint32_t *moved, double *other)
{
    const uint32_t j = blockIdx.x * (RB / WAVE) + threadIdx.x / WAVE;
    if (j >= n) return;
    const int lane = lane_id();
    const uint32_t i = body[j];
    if (i >= k.bodies.n) {                                                   // not a body of the set
        if (lane == 0) { hit[j] = -1; grounded_out[j] = 0; flags[j] = CLAPGPU_RAY_INVALID; }
        return;
    }
    if (lane == 0) atomicAdd(&moved[i], 2u);                                 // rays per body (bits 1..): a body listed twice
    Ray r;
    double ray_len;
    uint32_t f;
    Best b;
    if (!ground_ray(pos, yoffset, i, ray_off[j], r, ray_len)) {
        f = CLAPGPU_RAY_INVALID;
        b.key = KEY_NONE;
    } else {
        f = cast<LEVELED>(k, r, i, b);
    }
    if (lane == 0) {
        if (other && !(f & CLAPGPU_RAY_INVALID)) {                           // ground_decide's stores of the hit, restated
            hit[j] = hit_of(b.key);
            if (b.key != KEY_NONE) {
                dist[j] = b.depth;
                if (!f)
                    for (int a = 0; a < 3; a++) normal[3 * (size_t)j + a] = (float)b.normal[a];
            }
            flags[j] = f;
            other[j] = b.other;
        } else {
            ground_decide(j, i, ray_len, b.key, b.depth, b.normal, true, f, grounded, grounded_out, normal, dist, hit, flags, moved);
        }
    }
}

} // namespace clapgpu

using namespace clapgpu;


// ------------------------------------------------------------------------------------------------- the two passes
// `other` between the first pass and the mesh pass of a call over n > 0 rays: the caller's [n] doubles (move.hip), or
// stream-ordered memory of the call's own, freed behind the mesh pass
struct Between { double *other; bool own; };

// want: a mesh pass follows and reads `other`; given: the caller's, or NULL
static int take_between(hipStream_t s, bool want, uint32_t n, double *given, Between &b)
{
    b.other = want ? given : nullptr;
    b.own = want && !given;
    if (b.own) CLAPGPU_HIP(hipMallocAsync(reinterpret_cast<void **>(&b.other), (size_t)n * sizeof(double), s));
    return CLAPGPU_OK;
}

// ... and what follows the first launch (`first`: its name): its error is kept, not returned; if it launched and meshes
// are given, the mesh pass p over b.other; the call's own memory is freed behind whatever the stream holds, on the error
// paths too
static int second_pass(hipStream_t s, const clapgpu_trimesh *meshes, const char *first, MeshPass &p, const Between &b)
{
    int rc = CLAPGPU_OK;
    const hipError_t le = launch_error();
    if (le != hipSuccess) rc = hip_fail(le, first);
    if (!rc && meshes) {
        p.other = b.other;
        rc = mesh_pass(s, meshes, p);
    }
    if (b.own) {
        const hipError_t e = hipFreeAsync(b.other, s);
        if (!rc && e != hipSuccess) rc = hip_fail(e, "hipFreeAsync");
    }
    return rc;
}

extern "C" int clapgpu_ray_cast(void *stream, clapgpu_bp *bp, const clapgpu_geoms *bodies, const clapgpu_geoms *statics,
                                const clapgpu_trimesh *meshes, uint32_t n_rays, const double *ray, const int32_t *skip,
                                double *dist, int32_t *hit, double *contact, uint32_t *flags)
{
    if (!bodies || !statics || (n_rays && (!ray || !dist || !hit))) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    CastK k;
    int rc = cast_scene(k, bp, bodies, nullptr, statics, meshes);
    if (rc) return rc;
    if (n_rays == 0) return CLAPGPU_OK;
    hipStream_t s = as_stream(stream);
    Between b;
    rc = take_between(s, meshes && flags, n_rays, nullptr, b);              // no flags asked for: `other` is not needed
    if (rc) return rc;
    hipLaunchKernelGGL(leveled(k) ? k_ray_cast<true> : k_ray_cast<false>, dim3((n_rays + RB / WAVE - 1) / (RB / WAVE)), dim3(RB), 0,
                       s, k, n_rays, ray, skip, dist, hit, contact, flags, b.other);
    MeshPass p;
    memset(&p, 0, sizeof(p));
    p.n = n_rays; p.ray = ray; p.skip = skip; p.dist = dist; p.contact = contact; p.hit = hit; p.flags = flags;
    return second_pass(s, meshes, "k_ray_cast", p, b);
}

// clapgpu_bodies_ground_collide on the caller's memory (move.hip): other = [n] doubles for the mesh pass
// (meshes != NULL), so the call allocates nothing; cleared: the caller's own launch has zeroed scratch[0 .. b->n), so the
// call issues kernels only
__attribute__((visibility("hidden"))) int clapgpu_bodies_ground_collide_on(void *stream, clapgpu_bp *bp, const clapgpu_bodies *b,
                                                                           const clapgpu_geoms *statics,
                                                                           const clapgpu_trimesh *meshes, uint32_t n,
                                                                           const uint32_t *body, const double *ray_off,
                                                                           const uint8_t *grounded, uint8_t *grounded_out,
                                                                           float *normal, double *dist, int32_t *hit,
                                                                           uint32_t *flags, uint32_t *scratch, double *other,
                                                                           bool cleared)
{
    if (!b || !statics || !b->pos || !b->quat || !b->radius || !b->yoffset)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (n && (!body || !ray_off || !grounded || !grounded_out || !normal || !dist || !hit || !flags || !scratch))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    clapgpu_geoms g;
    if (!body_geoms(b, &g)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    CastK k;
    int rc = cast_scene(k, bp, &g, b->aabb, statics, meshes);
    if (rc) return rc;
    if (n == 0) return CLAPGPU_OK;
    hipStream_t s = as_stream(stream);
    if (!cleared) CLAPGPU_HIP(hipMemsetAsync(scratch, 0, (size_t)(b->n ? b->n : 1) * sizeof(uint32_t), s));
    Between bt;
    rc = take_between(s, meshes != nullptr, n, other, bt);
    if (rc) return rc;
    hipLaunchKernelGGL(leveled(k) ? k_ground_rays<true> : k_ground_rays<false>, dim3((n + RB / WAVE - 1) / (RB / WAVE)), dim3(RB), 0,
                       s, k, n, b->pos, b->yoffset, body, ray_off, grounded, grounded_out, normal, dist, hit, flags, scratch,
                       bt.other);
    MeshPass p;                                                              // the decision on the merged hit
    memset(&p, 0, sizeof(p));
    p.n = n; p.dist = dist; p.hit = hit; p.flags = flags;
    p.n_bodies = b->n; p.pos = b->pos; p.yoffset = b->yoffset; p.ray_off = ray_off; p.body = body; p.grounded = grounded;
    p.grounded_out = grounded_out; p.normal = normal; p.moved = scratch;
    rc = second_pass(s, meshes, "k_ground_rays", p, bt);
    if (rc) return rc;
    rc = clapgpu_bodies_ground_apply(stream, b, n, body, ray_off, grounded, grounded_out, dist, hit, flags, scratch);
    if (rc) return rc;
    if (bp) return clapgpu_bp_invalidate(stream, bp);                        // the moved boxes: the index is stale
    return CLAPGPU_OK;
}

extern "C" int clapgpu_bodies_ground_collide(void *stream, clapgpu_bp *bp, const clapgpu_bodies *b, const clapgpu_geoms *statics,
                                             const clapgpu_trimesh *meshes, uint32_t n, const uint32_t *body,
                                             const double *ray_off, const uint8_t *grounded, uint8_t *grounded_out, float *normal,
                                             double *dist, int32_t *hit, uint32_t *flags, uint32_t *scratch)
{
    return clapgpu_bodies_ground_collide_on(stream, bp, b, statics, meshes, n, body, ray_off, grounded, grounded_out, normal,
                                            dist, hit, flags, scratch, nullptr, false);
}
