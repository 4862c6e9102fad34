// rays.hip -- batched ray casts against the device physics scene, for gfx950:
//
//   k_ray_cast      __phys_ray_cast (physics.c:474-524): one dRay against the bodies and statics, the closest hit
//                   that is not the caster; one wavefront per ray, brute force or through an index of the broadphase
//                   grid (clapgpu_bp_index)
//   k_ground_rays   phys_body_ground_collide's ray and decision (physics.c:695-744) for a batch of bodies; the moves
//                   themselves are applied by bodies.hip's k_ground_apply (the device function the step writes
//                   geoms with lives there)
//   k_ray_trimesh   the mesh pass behind either of them: one lane per ray, the walk of the mesh set's BVH
//                   (trimesh_dev.h; built by trimesh.hip) and the watertight ray-triangle test, merged with the best
//                   hit the first pass found (see "mesh pass" below)
//
// The colliders restate ODE 0.16's ray.cpp (dCollideRaySphere + ray_sphere_helper, dCollideRayCapsule, dCollideRayBox)
// for the flags physics.c:485-487 sets; a box is its AABB.  ODE is an absent submodule of the reference: PARITY UNPINNED.
// One deliberate difference: a hit needs 0 <= depth <= length as written, so NaN geometry never hits.
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
#include "phys_dev.h"
#include "geoms_dev.h"
#include "grid_query_dev.h"
#include "trimesh_dev.h"
#include "tricontact_dev.h"

namespace clapgpu {

constexpr int RB = 256;                                 // 4 rays per workgroup
constexpr int RT = WAVE;                                // k_ray_trimesh: one wave per workgroup (the walk's LDS stack)

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

// ------------------------------------------------------------------------------------------------- bodies and statics
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
// caller scans instead, which also bounds the time one wavefront can spend on a ray
__device__ bool scan_grid(const CastK &k, const Ray &r, uint32_t skip_key, Best &b)
{
    const BpGridView &g = k.g;

    // the scene's bounds: indexed boxes joined with the registered statics, grown by a cell
    double bnd[6];
    for (int a = 0; a < 3; a++) {
        double lo = g.s_bounds[a], hi = g.s_bounds[3 + a];
        if (g.n && g.index[a] != ~0ull) {
            lo = fmin(lo, order_value(g.index[a]));
            hi = fmax(hi, order_value(~g.index[3 + a]));
        }
        bnd[2 * a] = lo - g.cell;
        bnd[2 * a + 1] = hi + g.cell;
    }
    const bool any = bnd[0] <= bnd[1] && bnd[2] <= bnd[3] && bnd[4] <= bnd[5];   // else: nothing but the large statics
    const double t0 = any ? segment_enters(r, bnd) : INFINITY;
    const bool pieces = t0 <= r.len;
    double t1 = r.len;                                                       // where the segment leaves the bounds
    for (int a = 0; a < 3; a++)
        if (r.u[a] != 0) t1 = fmin(t1, fmax((bnd[2 * a] - r.s[a]) / r.u[a], (bnd[2 * a + 1] - r.s[a]) / r.u[a]));
    if (t1 < t0) t1 = t0;
    const double span = pieces ? t1 - t0 : 0.0;
    const double np_d = ceil(span / g.cell);
    // the bounds are finite (k_bp_index_bounds takes finite coordinates only), so is span; the limit keeps a ray through
    // a sparse, far-flung scene from costing more than the scan
    const double limit = 64.0 + (double)(k.bodies.n + k.statics.n) / 256.0;
    if (!(np_d <= limit)) return false;
    const uint32_t np = !pieces ? 0u : np_d < 1.0 ? 1u : (uint32_t)np_d;

    auto test = [&](bool valid, bool is_static, uint32_t i) {
        if (!valid) return;
        if (is_static) test_geom(r, k.statics, i, KEY_STATIC | i, skip_key, b, k.meshed);
        else test_geom(r, k.bodies, i, i, skip_key, b, k.meshed);
    };
    grid_visit_large(g, test);
    GridRange prev;                                                          // the previous piece's: none
    for (uint32_t j = 0; j < np; j++) {
        const double ta = t0 + span * ((double)j / np), tb = (j + 1 == np) ? t1 : t0 + span * ((double)(j + 1) / np);
        double lo[3], hi[3];
        for (int a = 0; a < 3; a++) {
            const double pa = r.s[a] + ta * r.u[a], pb = r.s[a] + tb * r.u[a];
            lo[a] = fmin(pa, pb); hi[a] = fmax(pa, pb);
        }
        const GridRange piece = grid_range(g, lo, hi);
        grid_visit(g, piece, &prev, test);                                   // what the last piece looked up is skipped
        prev = piece;
    }
    return true;
}

// one ray on the whole wave: the best hit (every lane) and the ray's flags
__device__ __forceinline__ uint32_t cast(const CastK &k, const Ray &r, uint32_t skip_key, Best &b)
{
    b.depth = INFINITY; b.key = KEY_NONE; b.other = INFINITY;
    for (int a = 0; a < 3; a++) { b.pos[a] = 0; b.normal[a] = 0; }
    // the grid, unless: no index; the index may not be used (grid_usable); or more pieces than the scan's work
    if (!k.grid || !grid_usable(k.g) || !scan_grid(k, r, skip_key, b)) scan_all(k, r, skip_key, b);
    reduce_best(b);
    return unresolved(b.other, r.len, b.key, b.depth);
}

// other: NULL, or [n] where a mesh pass follows: the first entry into an OTHER static without a mesh, for its flags
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
    const uint32_t f = cast(k, r, skip_key_of(skip ? skip[i] : -1), b);
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
        f = cast(k, r, i, b);
    }
    if (lane == 0) {
        if (other && !(f & CLAPGPU_RAY_INVALID)) {
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

// ------------------------------------------------------------------------------------------------- mesh pass
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
        if (won) {
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

// scratch for `other` between the passes: stream-ordered, freed behind the mesh pass
static int mesh_scratch(hipStream_t s, const clapgpu_trimesh *meshes, uint32_t n, double **other)
{
    *other = nullptr;
    if (!meshes || n == 0) return CLAPGPU_OK;
    CLAPGPU_HIP(hipMallocAsync(reinterpret_cast<void **>(other), (size_t)n * sizeof(double), s));
    return CLAPGPU_OK;
}

// ... freed behind whatever the stream holds, on the error paths too; rc: the call's result so far
static int free_scratch(hipStream_t s, double *other, int rc)
{
    if (!other) return rc;
    const hipError_t e = hipFreeAsync(other, s);
    if (!rc && e != hipSuccess) return hip_fail(e, "hipFreeAsync");
    return rc;
}

// the mesh pass over p.n > 0 rays
static int mesh_pass(hipStream_t s, const clapgpu_trimesh *meshes, const MeshPass &p)
{
    const MeshSet m = trimesh_set(meshes);
    const dim3 grid((p.n + RT - 1) / RT);
    if (p.ray) hipLaunchKernelGGL(k_ray_trimesh<false>, grid, dim3(RT), 0, s, m, p);
    else hipLaunchKernelGGL(k_ray_trimesh<true>, grid, dim3(RT), 0, s, m, p);
    CLAPGPU_LAUNCH_CHECK("k_ray_trimesh");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_ray_cast_meshes(void *stream, clapgpu_bp *bp, const clapgpu_geoms *bodies, const clapgpu_geoms *statics,
                                       const clapgpu_trimesh *meshes, uint32_t n_rays, const double *ray, const int32_t *skip,
                                       double *dist, int32_t *hit, double *contact, uint32_t *flags)
{
    if (!bodies || !statics || (n_rays && (!ray || !dist || !hit))) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    CastK k;
    int rc = cast_scene(k, bp, bodies, nullptr, statics, meshes);
    if (rc) return rc;
    if (n_rays == 0) return CLAPGPU_OK;
    hipStream_t s = as_stream(stream);
    double *other;
    rc = mesh_scratch(s, flags ? meshes : nullptr, n_rays, &other);         // no flags asked for: `other` is not needed
    if (rc) return rc;
    hipLaunchKernelGGL(k_ray_cast, dim3((n_rays + RB / WAVE - 1) / (RB / WAVE)), dim3(RB), 0, s, k, n_rays, ray, skip, dist, hit,
                       contact, flags, other);
    const hipError_t le = launch_error();
    if (le != hipSuccess) rc = hip_fail(le, "k_ray_cast");
    if (!rc && meshes) {
        MeshPass p;
        memset(&p, 0, sizeof(p));
        p.n = n_rays; p.ray = ray; p.skip = skip; p.dist = dist; p.contact = contact; p.hit = hit; p.flags = flags; p.other = other;
        rc = mesh_pass(s, meshes, p);
    }
    return free_scratch(s, other, rc);
}

extern "C" int clapgpu_ray_cast(void *stream, clapgpu_bp *bp, const clapgpu_geoms *bodies, const clapgpu_geoms *statics,
                                uint32_t n_rays, const double *ray, const int32_t *skip, double *dist, int32_t *hit,
                                double *contact, uint32_t *flags)
{
    return clapgpu_ray_cast_meshes(stream, bp, bodies, statics, nullptr, n_rays, ray, skip, dist, hit, contact, flags);
}

// clapgpu_bodies_ground_collide_meshes on the caller's memory (move.hip): other = [n] doubles for the mesh pass
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
    const bool own = meshes && !other;                                       // stream-ordered, freed behind the mesh pass
    if (own) {
        rc = mesh_scratch(s, meshes, n, &other);
        if (rc) return rc;
    }
    if (!meshes) other = nullptr;
    hipLaunchKernelGGL(k_ground_rays, dim3((n + RB / WAVE - 1) / (RB / WAVE)), dim3(RB), 0, s, k, n, b->pos, b->yoffset, body,
                       ray_off, grounded, grounded_out, normal, dist, hit, flags, scratch, other);
    const hipError_t le = launch_error();
    if (le != hipSuccess) rc = hip_fail(le, "k_ground_rays");
    if (!rc && meshes) {                                                     // the decision on the merged hit
        MeshPass p;
        memset(&p, 0, sizeof(p));
        p.n = n; p.dist = dist; p.hit = hit; p.flags = flags; p.other = other;
        p.n_bodies = b->n; p.pos = b->pos; p.yoffset = b->yoffset; p.ray_off = ray_off; p.body = body; p.grounded = grounded;
        p.grounded_out = grounded_out; p.normal = normal; p.moved = scratch;
        rc = mesh_pass(s, meshes, p);
    }
    if (own) rc = free_scratch(s, other, rc);
    if (rc) return rc;
    rc = clapgpu_bodies_ground_apply(stream, b, n, body, ray_off, grounded, grounded_out, dist, hit, flags, scratch);
    if (rc) return rc;
    if (bp) return clapgpu_bp_invalidate(stream, bp);                        // the moved boxes: the index is stale
    return CLAPGPU_OK;
}

extern "C" int clapgpu_bodies_ground_collide_meshes(void *stream, clapgpu_bp *bp, const clapgpu_bodies *b,
                                                    const clapgpu_geoms *statics, const clapgpu_trimesh *meshes, uint32_t n,
                                                    const uint32_t *body, const double *ray_off, const uint8_t *grounded,
                                                    uint8_t *grounded_out, float *normal, double *dist, int32_t *hit,
                                                    uint32_t *flags, uint32_t *scratch)
{
    return clapgpu_bodies_ground_collide_on(stream, bp, b, statics, meshes, n, body, ray_off, grounded, grounded_out, normal,
                                            dist, hit, flags, scratch, nullptr, false);
}

extern "C" int clapgpu_bodies_ground_collide(void *stream, clapgpu_bp *bp, const clapgpu_bodies *b, const clapgpu_geoms *statics,
                                             uint32_t n, const uint32_t *body, const double *ray_off, const uint8_t *grounded,
                                             uint8_t *grounded_out, float *normal, double *dist, int32_t *hit, uint32_t *flags,
                                             uint32_t *scratch)
{
    return clapgpu_bodies_ground_collide_meshes(stream, bp, b, statics, nullptr, n, body, ray_off, grounded, grounded_out, normal,
                                                dist, hit, flags, scratch);
}
