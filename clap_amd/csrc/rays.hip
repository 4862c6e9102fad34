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
// the ground ray's decision are ray_dev.h's, the colliders ray_colliders_dev.h's.  fp64 throughout, no FMA contraction.
//
// Grid path: the segment is clipped to the indexed boxes' bounds joined with the statics' (grown by a cell) and cut into
// pieces of at most one cell; the cell range of every piece's box, its blocks' statics and the large list are visited
// through grid_query_dev.h, which says why they hold every geom the piece touches.  Every candidate runs the same
// collider as the brute-force scan and the minimum of (depth, key) does not depend on the order or on duplicates, so
// both paths give the same bits.
#include <string.h>
#include <stdlib.h>
#include "common.h"
#include "phys_dev.h"
#include "geoms_dev.h"
#include "grid_query_dev.h"
#include "trimesh_dev.h"
#include "ray_dev.h"
#include "ray_colliders_dev.h"

namespace clapgpu {

constexpr int RB = 256;                                 // 4 rays per workgroup

struct Best {
    double depth, pos[3], normal[3];
    uint32_t key;
    double other;                                        // first entry into a CLAPGPU_GEOM_OTHER box
};

// one geom of a set: the collider of its kind, or, for CLAPGPU_GEOM_OTHER, where the segment enters its AABB.  A static
// with a triangle mesh (meshed[s] >= 0) is left to the mesh pass (below)
__device__ __forceinline__ void test_geom(const Ray &r, const GeomsK &g, uint32_t i, uint32_t key, uint32_t skip_key, Best &b,
                                          const int32_t *meshed)
{
    if (i >= g.n || key == skip_key) return;
    if (meshed && (key & KEY_STATIC) && meshed[i] >= 0) return;
    phd::Geom ge;
    load_geom(g, i, ge);
    phd::CGeom c;
    bool hit = false;
    if (ge.kind == CLAPGPU_GEOM_SPHERE) hit = ray_sphere(r, ge.pos, ge.radius, false, c);
    else if (ge.kind == CLAPGPU_GEOM_CAPSULE) hit = ray_capsule(r, ge.pos, ge.axis, ge.radius, ge.length, c);
    else if (ge.kind == CLAPGPU_GEOM_BOX) hit = ray_box(r, ge.aabb, c);
    else {
        double bb[6];
        for (int a = 0; a < 6; a++) bb[a] = g.aabb ? g.aabb[6 * (size_t)i + a] : 0.0;
        const double t = g.aabb ? segment_enters(r, bb) : 0.0;             // no box known: it may be anywhere
        b.other = fmin(b.other, t);
        return;
    }
    if (hit && (c.depth < b.depth || (c.depth == b.depth && key < b.key))) {
        b.depth = c.depth; b.key = key;
        for (int a = 0; a < 3; a++) { b.pos[a] = c.pos[a]; b.normal[a] = c.normal[a]; }
    }
}

// the wave's minimum (depth, key); the winner's contact broadcast to every lane
__device__ __forceinline__ void reduce_best(Best &b)
{
    double d = b.depth, ot = b.other;
    uint32_t k = b.key;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(d, o);
        const uint32_t ok = __shfl_xor(k, o);
        if (od < d || (od == d && ok < k)) { d = od; k = ok; }
        ot = fmin(ot, __shfl_xor(ot, o));
    }
    const uint64_t win = __ballot(b.key == k && b.depth == d && k != KEY_NONE);
    const int w = win ? __builtin_ctzll(win) : 0;
    for (int a = 0; a < 3; a++) { b.pos[a] = __shfl(b.pos[a], w); b.normal[a] = __shfl(b.normal[a], w); }
    b.depth = d; b.key = k; b.other = ot;
}

struct CastK {
    GeomsK bodies, statics;
    bool grid;
    BpGridView g;
    const int32_t *meshed;               // NULL, or [statics.n]: the static's mesh in a clapgpu_trimesh set, or -1
};

__device__ __forceinline__ void scan_all(const CastK &k, const Ray &r, uint32_t skip_key, Best &b)
{
    const int lane = lane_id();
    for (uint32_t i = lane; i < k.bodies.n; i += WAVE) test_geom(r, k.bodies, i, i, skip_key, b, k.meshed);
    for (uint32_t s = lane; s < k.statics.n; s += WAVE) test_geom(r, k.statics, s, KEY_STATIC | s, skip_key, b, k.meshed);
}

// false: the clipped segment has more pieces than a scan of every geom has candidates per lane (far-flung boxes); the
// caller scans instead, which also bounds the time one wavefront can spend on a ray.
// LEVELED (g.levels > 1): the bounds are grown by the top level's cell, the large list of the statics' level is visited
// once, and every level cuts the clipped segment into pieces of at most ITS cell and visits its own cells along them,
// the statics on their level's pieces alone; the limit holds the pieces of all levels together.
template <bool LEVELED>
__device__ bool scan_grid(const CastK &k, const Ray &r, uint32_t skip_key, Best &b)
{
    const BpGridView &g = k.g;
    const uint32_t levels = grid_levels<LEVELED>(g);
    double top = g.cell;                                                     // the coarsest cell
    for (uint32_t L = 1; L < levels; L++) top *= 2.0;

    // the scene's bounds: indexed boxes joined with the registered statics, grown by a cell
    double bnd[6];
    for (int a = 0; a < 3; a++) {
        double lo = g.s_bounds[a], hi = g.s_bounds[3 + a];
        if (g.n && g.index[a] != ~0ull) {
            lo = fmin(lo, order_value(g.index[a]));
            hi = fmax(hi, order_value(~g.index[3 + a]));
        }
        bnd[2 * a] = lo - top;
        bnd[2 * a + 1] = hi + top;
    }
    const bool any = bnd[0] <= bnd[1] && bnd[2] <= bnd[3] && bnd[4] <= bnd[5];   // else: nothing but the large statics
    const double t0 = any ? segment_enters(r, bnd) : INFINITY;
    const bool pieces = t0 <= r.len;
    double t1 = r.len;                                                       // where the segment leaves the bounds
    for (int a = 0; a < 3; a++)
        if (r.u[a] != 0) t1 = fmin(t1, fmax((bnd[2 * a] - r.s[a]) / r.u[a], (bnd[2 * a + 1] - r.s[a]) / r.u[a]));
    if (t1 < t0) t1 = t0;
    const double span = pieces ? t1 - t0 : 0.0;
    double c = g.cell, np_d = ceil(span / c);
    for (uint32_t L = 1; L < levels; L++) { c *= 2.0; np_d += ceil(span / c); }
    // the bounds are finite (k_bp_index_bounds takes finite coordinates only), so is span; the limit keeps a ray through
    // a sparse, far-flung scene from costing more than the scan
    const double limit = 64.0 + (double)(k.bodies.n + k.statics.n) / 256.0;
    if (!(np_d <= limit)) return false;

    auto test = [&](bool valid, bool is_static, uint32_t i) {
        if (!valid) return;
        if (is_static) test_geom(r, k.statics, i, KEY_STATIC | i, skip_key, b, k.meshed);
        else test_geom(r, k.bodies, i, i, skip_key, b, k.meshed);
    };
    grid_visit_large<LEVELED>(g, test);
    c = g.cell;
    for (uint32_t L = 0; L < levels; L++, c *= 2.0) {
        const double npl_d = ceil(span / c);
        const uint32_t np = !pieces ? 0u : npl_d < 1.0 ? 1u : (uint32_t)npl_d;
        GridRange prev;                                                      // the previous piece's: none
        for (uint32_t j = 0; j < np; j++) {
            const double ta = t0 + span * ((double)j / np), tb = (j + 1 == np) ? t1 : t0 + span * ((double)(j + 1) / np);
            double lo[3], hi[3];
            for (int a = 0; a < 3; a++) {
                const double pa = r.s[a] + ta * r.u[a], pb = r.s[a] + tb * r.u[a];
                lo[a] = fmin(pa, pb); hi[a] = fmax(pa, pb);
            }
            const GridRange piece = grid_range(c, lo, hi);
            grid_visit<LEVELED>(g, L, grid_level_statics<LEVELED>(g, L), piece, &prev, test);   // what the last piece looked up is skipped
            prev = piece;
        }
    }
    return true;
}

// one ray on the whole wave: the best hit (every lane) and the ray's flags.  LEVELED: k.g is a leveled index (the host
// picks the kernel by it, so a one-level index and the scan run the code they ran)
template <bool LEVELED>
__device__ __forceinline__ uint32_t cast(const CastK &k, const Ray &r, uint32_t skip_key, Best &b)
{
    b.depth = INFINITY; b.key = KEY_NONE; b.other = INFINITY;
    for (int a = 0; a < 3; a++) { b.pos[a] = 0; b.normal[a] = 0; }
    // the grid, unless: no index; the index may not be used (grid_usable); or more pieces than the scan's work
    if (!k.grid || !grid_usable(k.g) || !scan_grid<LEVELED>(k, r, skip_key, b)) scan_all(k, r, skip_key, b);
    reduce_best(b);
    return unresolved(b.other, r.len, b.key, b.depth);
}

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

// what both passes of an entry point read: the geom sets, the statics the mesh pass owns, and bp's grid when it is
// indexed over these bodies (their boxes body_aabb, or NULL) and statics
static int cast_scene(CastK &k, clapgpu_bp *bp, const clapgpu_geoms *bodies, const double *body_aabb,
                      const clapgpu_geoms *statics, const clapgpu_trimesh *meshes)
{
    memset(&k, 0, sizeof(k));
    k.bodies = geoms_k(bodies); k.statics = geoms_k(statics);
    k.meshed = meshes ? trimesh_set(meshes).static_mesh : nullptr;
    return scene_grid(bp, bodies->n, body_aabb, statics->n, meshes, &k.g, &k.grid);
}

// the kernels of a leveled index are instantiations of their own: the others keep their code and their registers
static bool leveled(const CastK &k) { return k.grid && k.g.levels > 1; }

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
