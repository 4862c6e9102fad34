// rays.hip -- batched ray casts against the device physics scene, for gfx950:
//
//   k_ray_cast      __phys_ray_cast (physics.c:474-524): one dRay against the bodies and statics, the closest hit
//                   that is not the caster; one wavefront per ray, brute force or through an index of the broadphase
//                   grid (clapgpu_bp_index)
//   k_ground_rays   phys_body_ground_collide's ray and decision (physics.c:695-744) for a batch of bodies; the moves
//                   themselves are applied by physics2.hip's k_ground_apply (the device function the step writes
//                   geoms with lives there)
//
// The colliders restate ODE 0.16's ray.cpp (dCollideRaySphere + ray_sphere_helper, dCollideRayCapsule, dCollideRayBox)
// for the flags physics.c:485-487 sets; a box is its AABB.  ODE is an absent submodule of the reference: PARITY UNPINNED.
// One deliberate difference: a hit needs 0 <= depth <= length as written, so NaN geometry never hits.
// fp64 throughout, no FMA contraction.
//
// Grid path: the segment is clipped to the indexed boxes' bounds joined with the statics' (grown by a cell), cut into
// pieces of at most one cell, and every cell in cell_coord(piece lo - grow) .. cell_coord(piece hi + grow) is looked up,
// grow = cell / 2 * (1 + 1e-9).  A box edge is at most `cell` and a body is binned by its box centre, so a body the
// segment touches has its centre cell in that range (cell_coord is monotone).  The statics registered for the blocks of
// the range (their boxes grown by the same half cell at clapgpu_bp_create) and the large list complete the candidates.
// Every candidate runs the same collider as the brute-force scan and the minimum of (depth, key) does not depend on the
// order or on duplicates, so both paths give the same bits.
#include <string.h>
#include <stdlib.h>
#include "common.h"
#include "phys_dev.h"
#include "geoms_dev.h"
#include "bp_grid.h"
#include "rays_dev.h"

struct clapgpu_bp;
int clapgpu_bodies_ground_apply(void *stream, const clapgpu_bodies *b, uint32_t n, const uint32_t *body, const double *ray_off,
                                const uint8_t *grounded, uint8_t *grounded_out, const double *dist, const int32_t *hit,
                                uint32_t *flags, const uint32_t *moved);                                      // physics2.hip

namespace clapgpu {

constexpr int RB = 256;                                 // 4 rays per workgroup

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
// with a triangle mesh (meshed[s] >= 0) is left to the mesh pass (trimesh.hip)
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

__device__ __forceinline__ bool in_box3(const int32_t (&lo)[3], const int32_t (&hi)[3], int32_t x, int32_t y, int32_t z)
{
    return x >= lo[0] && x <= hi[0] && y >= lo[1] && y <= hi[1] && z >= lo[2] && z <= hi[2];
}

// false: the clipped segment has more pieces than a scan of every geom has candidates per lane (far-flung boxes); the
// caller scans instead, which also bounds the time one wavefront can spend on a ray
__device__ bool scan_grid(const CastK &k, const Ray &r, uint32_t skip_key, Best &b)
{
    const int lane = lane_id();
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
    const double grow = g.cell * 0.5 * (1.0 + 1e-9);

    for (uint32_t j = lane; j < g.n_large; j += WAVE)                       // the large statics: every ray
        test_geom(r, k.statics, g.s_lrecs[j].idx, KEY_STATIC | g.s_lrecs[j].idx, skip_key, b, k.meshed);

    int32_t pc_lo[3] = { 1, 1, 1 }, pc_hi[3] = { 0, 0, 0 }, pb_lo[3] = { 1, 1, 1 }, pb_hi[3] = { 0, 0, 0 };   // previous piece: none
    for (uint32_t j = 0; j < np; j++) {
        const double ta = t0 + span * ((double)j / np), tb = (j + 1 == np) ? t1 : t0 + span * ((double)(j + 1) / np);
        int32_t c_lo[3], c_hi[3], b_lo[3], b_hi[3];
        uint32_t ext[3], bext[3];
        for (int a = 0; a < 3; a++) {
            const double pa = r.s[a] + ta * r.u[a], pb = r.s[a] + tb * r.u[a];
            c_lo[a] = cell_coord(fmin(pa, pb) - grow, g.cell);
            c_hi[a] = cell_coord(fmax(pa, pb) + grow, g.cell);
            b_lo[a] = c_lo[a] >> 2; b_hi[a] = c_hi[a] >> 2;
            ext[a] = (uint32_t)(c_hi[a] - c_lo[a] + 1); bext[a] = (uint32_t)(b_hi[a] - b_lo[a] + 1);
        }
        const uint32_t ncell = g.n ? ext[0] * ext[1] * ext[2] : 0u, nblk = bext[0] * bext[1] * bext[2];
        const uint32_t items = ncell + nblk;
        for (uint32_t base = 0; base < items; base += WAVE) {
            // one lookup per lane: a cell of the piece's range (bodies) or a block (statics), unless the last piece had it
            const uint32_t it = base + lane;
            uint32_t first = 0, count = 0, isstat = 0;
            int32_t cx = 0, cy = 0, cz = 0;
            if (it < ncell) {
                cx = c_lo[0] + (int32_t)(it % ext[0]);
                cy = c_lo[1] + (int32_t)((it / ext[0]) % ext[1]);
                cz = c_lo[2] + (int32_t)(it / (ext[0] * ext[1]));
                if (!in_box3(pc_lo, pc_hi, cx, cy, cz)) {
                    const uint2 cr = g.cell_range[cell_slot(cx, cy, cz, g.mask)];
                    first = cr.x; count = cr.y;
                }
            } else if (it < items) {
                const uint32_t q = it - ncell;
                const int32_t bx = b_lo[0] + (int32_t)(q % bext[0]), by = b_lo[1] + (int32_t)((q / bext[0]) % bext[1]),
                              bz = b_lo[2] + (int32_t)(q / (bext[0] * bext[1]));
                if (!in_box3(pb_lo, pb_hi, bx, by, bz)) {
                    const uint32_t h = block_hash(bx, by, bz, g.mask);
                    first = g.s_start[h]; count = g.s_start[h + 1] - first;
                }
                isstat = 1;
            }
            uint32_t incl = count;
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                const uint32_t u = __shfl_up(incl, o);
                if (lane >= o) incl += u;
            }
            const uint32_t total = __shfl(incl, WAVE - 1), excl = incl - count;
            // the candidates of these lookups spread over the lanes: candidate q belongs to the first lane with incl > q
            for (uint32_t q0 = 0; q0 < total; q0 += WAVE) {
                const uint32_t q = q0 + lane;
                int o = 0;
#pragma unroll
                for (int step = 32; step > 0; step >>= 1) {
                    const uint32_t v = __shfl(incl, o + step - 1);
                    if (v <= q) o += step;
                }
                const uint32_t ofirst = __shfl(first, o), oexcl = __shfl(excl, o), ostat = __shfl(isstat, o);
                const int32_t ox = __shfl(cx, o), oy = __shfl(cy, o), oz = __shfl(cz, o);
                if (q < total) {
                    const uint32_t e = ofirst + (q - oexcl);
                    if (ostat) {
                        const uint32_t s = g.s_recs[e].idx;
                        test_geom(r, k.statics, s, KEY_STATIC | s, skip_key, b, k.meshed);
                    } else {
                        const int4 t = reinterpret_cast<const int4 *>(g.recs + e)[3];      // idx, cell coordinates
                        if (t.y == ox && t.z == oy && t.w == oz && (uint32_t)t.x < g.n)    // not a hash neighbour
                            test_geom(r, k.bodies, (uint32_t)t.x, (uint32_t)t.x, skip_key, b, k.meshed);
                    }
                }
            }
        }
        for (int a = 0; a < 3; a++) { pc_lo[a] = c_lo[a]; pc_hi[a] = c_hi[a]; pb_lo[a] = b_lo[a]; pb_hi[a] = b_hi[a]; }
    }
    return true;
}

// one ray on the whole wave: the best hit (every lane) and the ray's flags
__device__ __forceinline__ uint32_t cast(const CastK &k, const Ray &r, uint32_t skip_key, Best &b)
{
    b.depth = INFINITY; b.key = KEY_NONE; b.other = INFINITY;
    for (int a = 0; a < 3; a++) { b.pos[a] = 0; b.normal[a] = 0; }
    // the grid, unless: no index; a box too large for it; boxes binned again since the index (a replayed graph moved
    // them: the device's bin epoch differs); or more pieces than the scan's work
    const bool grid = k.grid && k.g.index[INDEX_OVERSIZE] == ~0ull &&
                      (k.g.n == 0 || k.g.ctrl[CTRL_BIN_EPOCH] == k.g.ctrl[CTRL_INDEX_EPOCH]);
    if (!grid || !scan_grid(k, r, skip_key, b)) scan_all(k, r, skip_key, b);
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

} // namespace clapgpu

using namespace clapgpu;

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

extern "C" int clapgpu_ray_cast_meshes(void *stream, clapgpu_bp *bp, const clapgpu_geoms *bodies, const clapgpu_geoms *statics,
                                       const clapgpu_trimesh *meshes, uint32_t n_rays, const double *ray, const int32_t *skip,
                                       double *dist, int32_t *hit, double *contact, uint32_t *flags)
{
    if (!bodies || !statics || (n_rays && (!ray || !dist || !hit))) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (meshes && trimesh_n_statics(meshes) != statics->n) return CLAPGPU_ERR_INVALID_ARGUMENTS;   // built for other statics
    CastK k;
    memset(&k, 0, sizeof(k));
    k.bodies = geoms_k(bodies); k.statics = geoms_k(statics);
    k.meshed = meshes ? trimesh_static_mesh(meshes) : nullptr;
    if (bp) {
        if (!clapgpu_bp_grid_view(bp, bodies->n, nullptr, &k.g) || k.g.n_static != statics->n)
            return CLAPGPU_ERR_INVALID_ARGUMENTS;                           // not indexed over these bodies and statics
        k.grid = true;
    }
    if (n_rays == 0) return CLAPGPU_OK;
    hipStream_t s = as_stream(stream);
    double *other;
    int rc = mesh_scratch(s, flags ? meshes : nullptr, n_rays, &other);     // no flags asked for: `other` is not needed
    if (rc) return rc;
    hipLaunchKernelGGL(k_ray_cast, dim3((n_rays + RB / WAVE - 1) / (RB / WAVE)), dim3(RB), 0, s, k, n_rays, ray, skip, dist, hit,
                       contact, flags, other);
    const hipError_t le = launch_error();
    if (le != hipSuccess) rc = hip_fail(le, "k_ray_cast");
    if (!rc && meshes) {
        MeshPass p;
        memset(&p, 0, sizeof(p));
        p.n = n_rays; p.ray = ray; p.skip = skip; p.dist = dist; p.contact = contact; p.hit = hit; p.flags = flags; p.other = other;
        rc = trimesh_pass(s, meshes, p);
    }
    return free_scratch(s, other, rc);
}

extern "C" int clapgpu_ray_cast(void *stream, clapgpu_bp *bp, const clapgpu_geoms *bodies, const clapgpu_geoms *statics,
                                uint32_t n_rays, const double *ray, const int32_t *skip, double *dist, int32_t *hit,
                                double *contact, uint32_t *flags)
{
    return clapgpu_ray_cast_meshes(stream, bp, bodies, statics, nullptr, n_rays, ray, skip, dist, hit, contact, flags);
}

extern "C" int clapgpu_bodies_ground_collide_meshes(void *stream, clapgpu_bp *bp, const clapgpu_bodies *b,
                                                    const clapgpu_geoms *statics, const clapgpu_trimesh *meshes, uint32_t n,
                                                    const uint32_t *body, const double *ray_off, const uint8_t *grounded,
                                                    uint8_t *grounded_out, float *normal, double *dist, int32_t *hit,
                                                    uint32_t *flags, uint32_t *scratch)
{
    if (!b || !statics || !b->pos || !b->quat || !b->radius || !b->yoffset)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (n && (!body || !ray_off || !grounded || !grounded_out || !normal || !dist || !hit || !flags || !scratch))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (meshes && trimesh_n_statics(meshes) != statics->n) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    clapgpu_geoms g;                                                         // the bodies' geoms, as PhysWorld.body_geoms
    memset(&g, 0, sizeof(g));
    g.n = b->n; g.pos = b->pos; g.axis = b->axis; g.radius = b->radius; g.length = b->length; g.records = b->geom_records;
    if (b->length && !b->axis && !b->geom_records) return CLAPGPU_ERR_INVALID_ARGUMENTS;   // capsules need their axis
    CastK k;
    memset(&k, 0, sizeof(k));
    k.bodies = geoms_k(&g); k.statics = geoms_k(statics);
    k.meshed = meshes ? trimesh_static_mesh(meshes) : nullptr;
    if (bp) {
        if (!clapgpu_bp_grid_view(bp, b->n, b->aabb, &k.g) || k.g.n_static != statics->n)
            return CLAPGPU_ERR_INVALID_ARGUMENTS;
        k.grid = true;
    }
    if (n == 0) return CLAPGPU_OK;
    hipStream_t s = as_stream(stream);
    CLAPGPU_HIP(hipMemsetAsync(scratch, 0, (size_t)(b->n ? b->n : 1) * sizeof(uint32_t), s));
    double *other;
    int rc = mesh_scratch(s, meshes, n, &other);
    if (rc) return rc;
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
        rc = trimesh_pass(s, meshes, p);
    }
    rc = free_scratch(s, other, rc);
    if (rc) return rc;
    rc = clapgpu_bodies_ground_apply(stream, b, n, body, ray_off, grounded, grounded_out, dist, hit, flags, scratch);
    if (rc) return rc;
    if (bp) return clapgpu_bp_invalidate(stream, bp);                        // the moved boxes: the index is stale
    return CLAPGPU_OK;
}

extern "C" int clapgpu_bodies_ground_collide(void *stream, clapgpu_bp *bp, const clapgpu_bodies *b, const clapgpu_geoms *statics,
                                             uint32_t n, const uint32_t *body, const double *ray_off, const uint8_t *grounded,
                                             uint8_t *grounded_out, float *normal, double *dist, int32_t *hit, uint32_t *flags,
                                             uint32_t *scratch)
{
    return clapgpu_bodies_ground_collide_meshes(stream, bp, b, statics, nullptr, n, body, ray_off, grounded, grounded_out, normal,
                                                dist, hit, flags, scratch);
}
