// ray_cast_dev.h -- one ray against the bodies and statics of a scene on one wavefront, as rays.hip's k_ray_cast and
// k_ground_rays and camera.hip's k_camera_calc run it: the best hit and its reduction, the scan of every geom, the walk
// of the broadphase grid's index, and the host's view of the scene (cast_scene).  The ray, the hit keys and the
// UNRESOLVED rule are ray_dev.h's, the colliders ray_colliders_dev.h's.  fp64 throughout, no FMA contraction.
#pragma once
#include <string.h>
#include "common.h"
#include "phys_dev.h"
#include "geoms_dev.h"
#include "grid_query_dev.h"
#include "trimesh_dev.h"
#include "ray_dev.h"
#include "ray_colliders_dev.h"

namespace clapgpu {

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

} // namespace clapgpu

// what both passes of an entry point read: the geom sets, the statics the mesh pass owns, and bp's grid when it is
// indexed over these bodies (their boxes body_aabb, or NULL) and statics
static inline int cast_scene(clapgpu::CastK &k, clapgpu_bp *bp, const clapgpu_geoms *bodies, const double *body_aabb,
                             const clapgpu_geoms *statics, const clapgpu_trimesh *meshes)
{
    memset(&k, 0, sizeof(k));
    k.bodies = geoms_k(bodies); k.statics = geoms_k(statics);
    k.meshed = meshes ? clapgpu::trimesh_set(meshes).static_mesh : nullptr;
    return scene_grid(bp, bodies->n, body_aabb, statics->n, meshes, &k.g, &k.grid);
}

// the kernels of a leveled index are instantiations of their own: the others keep their code and their registers
static inline bool leveled(const clapgpu::CastK &k) { return k.grid && k.g.levels > 1; }
