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

struct clapgpu_bp;
int clapgpu_bodies_ground_apply(void *stream, const clapgpu_bodies *b, uint32_t n, const uint32_t *body, const double *ray_off,
                                const uint8_t *grounded, uint8_t *grounded_out, const double *dist, const int32_t *hit,
                                uint32_t *flags, const uint32_t *moved);                                      // physics2.hip

namespace clapgpu {

constexpr int RB = 256;                                 // 4 rays per workgroup
constexpr uint32_t KEY_NONE = 0xffffffffu, KEY_STATIC = 0x80000000u;

struct Ray { double s[3], u[3], len; };

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

// one geom of a set: the collider of its kind, or, for CLAPGPU_GEOM_OTHER, where the segment enters its AABB
__device__ __forceinline__ void test_geom(const Ray &r, const GeomsK &g, uint32_t i, uint32_t key, uint32_t skip_key, Best &b)
{
    if (i >= g.n || key == skip_key) return;
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
};

__device__ __forceinline__ void scan_all(const CastK &k, const Ray &r, uint32_t skip_key, Best &b)
{
    const int lane = lane_id();
    for (uint32_t i = lane; i < k.bodies.n; i += WAVE) test_geom(r, k.bodies, i, i, skip_key, b);
    for (uint32_t s = lane; s < k.statics.n; s += WAVE) test_geom(r, k.statics, s, KEY_STATIC | s, skip_key, b);
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
        test_geom(r, k.statics, g.s_lrecs[j].idx, KEY_STATIC | g.s_lrecs[j].idx, skip_key, b);

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
                        test_geom(r, k.statics, s, KEY_STATIC | s, skip_key, b);
                    } else {
                        const int4 t = reinterpret_cast<const int4 *>(g.recs + e)[3];      // idx, cell coordinates
                        if (t.y == ox && t.z == oy && t.w == oz && (uint32_t)t.x < g.n)    // not a hash neighbour
                            test_geom(r, k.bodies, (uint32_t)t.x, (uint32_t)t.x, skip_key, b);
                    }
                }
            }
        }
        for (int a = 0; a < 3; a++) { pc_lo[a] = c_lo[a]; pc_hi[a] = c_hi[a]; pb_lo[a] = b_lo[a]; pb_hi[a] = b_hi[a]; }
    }
    return true;
}

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
    const bool hit = b.key != KEY_NONE;
    return (b.other <= r.len && (!hit || b.other <= b.depth)) ? CLAPGPU_RAY_UNRESOLVED : 0u;
}

__device__ __forceinline__ int32_t hit_of(uint32_t key)
{
    return key == KEY_NONE ? -1 : (key & KEY_STATIC) ? -2 - (int32_t)(key & ~KEY_STATIC) : (int32_t)key;
}

__global__ __launch_bounds__(RB)
void k_ray_cast(CastK k, uint32_t n, const double *ray, const int32_t *skip, double *dist, int32_t *hit, double *contact,
                uint32_t *flags)
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
    }
}

// phys_body_ground_collide's cast for body[k]: start (float) below the body's position, straight down, 2 * ray_len long,
// the body skipped; outputs the hit and the decision.  moved[body]: bit 0 = the apply launch will move it (unless it is
// listed twice), bits 1.. = rays cast for it
__global__ __launch_bounds__(RB)
void k_ground_rays(CastK k, uint32_t n, const double *pos, const double *yoffset, const uint32_t *body, const double *ray_off,
                   const uint8_t *grounded, uint8_t *grounded_out, float *normal, double *dist, int32_t *hit, uint32_t *flags,
                   uint32_t *moved)
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
    double roff;
    const double ray_len = phd::ground_ray_len(ray_off[j], yoffset[i], roff);
    const double *p = pos + 3 * (size_t)i;
    const float start[3] = { (float)p[0], (float)(p[1] - roff), (float)p[2] };   // through a vec3
    Ray r;
    r.s[0] = start[0]; r.s[1] = start[1]; r.s[2] = start[2];
    r.u[0] = 0.0; r.u[1] = -1.0; r.u[2] = 0.0;
    r.len = ray_len * 2;
    uint32_t f;
    Best b;
    if (!(r.len >= 0) || r.s[0] != r.s[0] || r.s[1] != r.s[1] || r.s[2] != r.s[2]) {
        f = CLAPGPU_RAY_INVALID;
        b.key = KEY_NONE;
    } else {
        f = cast(k, r, i, b);
    }
    if (lane == 0) {
        bool res = false;
        hit[j] = hit_of(b.key);
        if (b.key != KEY_NONE && !f) {
            normal[3 * (size_t)j] = (float)b.normal[0];
            normal[3 * (size_t)j + 1] = (float)b.normal[1];
            normal[3 * (size_t)j + 2] = (float)b.normal[2];
            float dy;
            bool mv;
            res = phd::ground_branch(b.depth, ray_len, grounded[j] != 0, dy, mv);
            if (mv) atomicOr(&moved[i], 1u);
        }
        if (b.key != KEY_NONE) dist[j] = b.depth;
        grounded_out[j] = res ? 1 : 0;
        flags[j] = f;
    }
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" int clapgpu_ray_cast(void *stream, clapgpu_bp *bp, const clapgpu_geoms *bodies, const clapgpu_geoms *statics,
                                uint32_t n_rays, const double *ray, const int32_t *skip, double *dist, int32_t *hit,
                                double *contact, uint32_t *flags)
{
    if (!bodies || !statics || (n_rays && (!ray || !dist || !hit))) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    CastK k;
    memset(&k, 0, sizeof(k));
    k.bodies = geoms_k(bodies); k.statics = geoms_k(statics);
    if (bp) {
        if (!clapgpu_bp_grid_view(bp, bodies->n, nullptr, &k.g) || k.g.n_static != statics->n)
            return CLAPGPU_ERR_INVALID_ARGUMENTS;                           // not indexed over these bodies and statics
        k.grid = true;
    }
    if (n_rays == 0) return CLAPGPU_OK;
    hipLaunchKernelGGL(k_ray_cast, dim3((n_rays + RB / WAVE - 1) / (RB / WAVE)), dim3(RB), 0, as_stream(stream), k, n_rays,
                       ray, skip, dist, hit, contact, flags);
    CLAPGPU_LAUNCH_CHECK("k_ray_cast");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_bodies_ground_collide(void *stream, clapgpu_bp *bp, const clapgpu_bodies *b, const clapgpu_geoms *statics,
                                             uint32_t n, const uint32_t *body, const double *ray_off, const uint8_t *grounded,
                                             uint8_t *grounded_out, float *normal, double *dist, int32_t *hit, uint32_t *flags,
                                             uint32_t *scratch)
{
    if (!b || !statics || !b->pos || !b->quat || !b->radius || !b->yoffset)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (n && (!body || !ray_off || !grounded || !grounded_out || !normal || !dist || !hit || !flags || !scratch))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    clapgpu_geoms g;                                                         // the bodies' geoms, as PhysWorld.body_geoms
    memset(&g, 0, sizeof(g));
    g.n = b->n; g.pos = b->pos; g.axis = b->axis; g.radius = b->radius; g.length = b->length; g.records = b->geom_records;
    if (b->length && !b->axis && !b->geom_records) return CLAPGPU_ERR_INVALID_ARGUMENTS;   // capsules need their axis
    CastK k;
    memset(&k, 0, sizeof(k));
    k.bodies = geoms_k(&g); k.statics = geoms_k(statics);
    if (bp) {
        if (!clapgpu_bp_grid_view(bp, b->n, b->aabb, &k.g) || k.g.n_static != statics->n)
            return CLAPGPU_ERR_INVALID_ARGUMENTS;
        k.grid = true;
    }
    if (n == 0) return CLAPGPU_OK;
    hipStream_t s = as_stream(stream);
    CLAPGPU_HIP(hipMemsetAsync(scratch, 0, (size_t)(b->n ? b->n : 1) * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_ground_rays, dim3((n + RB / WAVE - 1) / (RB / WAVE)), dim3(RB), 0, s, k, n, b->pos, b->yoffset, body,
                       ray_off, grounded, grounded_out, normal, dist, hit, flags, scratch);
    CLAPGPU_LAUNCH_CHECK("k_ground_rays");
    int rc = clapgpu_bodies_ground_apply(stream, b, n, body, ray_off, grounded, grounded_out, dist, hit, flags, scratch);
    if (rc) return rc;
    if (bp) return clapgpu_bp_invalidate(stream, bp);                        // the moved boxes: the index is stale
    return CLAPGPU_OK;
}
