// order.hip -- the order of a crowd: which movers of a clapgpu_characters_move batch can reach each other, the conflict
// level of each, and the move level by level, for gfx950.  The rule is stated in include/clapgpu.h
// (clapgpu_characters_order) and restated in tests/orderref.py.
//
//   k_order_reach   one lane per mover: its reach box (below), its class, level 0, and the row the pair search is given
//   (clapgpu_bp_collide over those rows: ascending (i, j), i < j -- the conflicts, oriented as the level rule reads them)
//   k_order_dups    one lane per pair: two listings of one body have one box, so they are a pair; both are taken out
//   k_order_round   one relaxation round: atomicMax(level[j], level[i] + 1) per pair; returns at once when the round
//                   before it raised nothing
//   k_order_alone   the same round for the movers whose box is not finite (they conflict with everybody); launched only
//                   when there is one
//   k_order_keys / (rocPRIM radix sort, stable) / k_order_first   the movers by (level, k) and where each level starts
//   k_order_gather / k_order_scatter   the clapgpu_move arrays into level-major copies and back
//
// Why the reach box of mover k holds everything its three stages read of another geom or write of its own body.
// Everything is measured from b->aabb[body], the body's box at the start of the call (rows 0..5 = min/max x, y, z).
//   The ray (ray_dev.h's ground_ray): starts at (float)pos.x, (float)(pos.y - roff), (float)pos.z and runs 2 * ray_len
//     straight down.  x and z are the body's own, inside its box, within a float rounding (the pad).  Both ends of the
//     segment in y, start and start - 2 * ray_len, are taken into the box explicitly, each with the pad.  A ray_len
//     that is negative or NaN makes the ray CLAPGPU_RAY_INVALID: the mover ends there, and its length counts as 0.
//   The snap (phd::ground_branch): dy = ray_len - dist or -(dist - ray_len) with 0 <= dist <= 2 * ray_len, so |dy| <=
//     ray_len, in y alone.
//   The slide (slide.hip's k_slide_decide): the deltas are velocity * dt with dt clamped to 1 / 30, the velocity being
//     what k_move_decide leaves.  Airborne: the given one with velocity[1] + (float)gravity[1] * dt_sec, |.|_1 <= A.
//     Walking: newx * sx + newz * sz with unit newx, newz and |sx| <= |dx|, |sz| <= |dz| (coef <= 1), every component
//     <= |dx| + |dz|, |.|_1 <= B; with a zero normal the given velocity stays, |.|_1 <= A.  A jump and a state below
//     IDLE do not slide.  One character_sweep_delta call travels frac * delta, then projects the remainder (1 - frac) *
//     delta on the plane of a unit normal, which does not lengthen it, at most three times: the running position and the
//     far end of every probe (position + remaining delta) stay within |delta|_2 <= |delta|_1 of where the call began, on
//     every axis.  The falling branch makes two calls whose deltas are the y part and the x, z part of velocity * dt:
//     together |.|_1 of the whole.  So every position the slide probes, and where it ends, is within T = S * dt of the
//     snapped position, S = max(A, B).  A delta that is not finite is CLAPGPU_SLIDE_INVALID and moves nothing, so a
//     branch whose bound is not finite counts as 0 (an infinite dt_sec keeps A's part without it: a walker on a zero
//     normal still travels the given velocity).
//   The boxes: a probe's swept box is the box of its geom at the running position united with that box moved by the
//     delta, grown by a relative 2^-40 (slide.hip's swept_box); a geom is a candidate when its own box meets it.  The
//     geom's box at position p is b->aabb moved by p - pos up to roundings.
//   pad = 2^-20 * (the largest magnitude among the box rows, the ray's ends, ray_len and T) + 1e-6 covers the float round
//     trips (the ray's start, phys_body_move's (double)step, the float products of the deltas and of the projection --
//     a handful of 2^-24 relative each) and the 2^-40.
// Hence: what mover k reads of another geom lies in a box that meets k's reach box, and what it writes of its own body
// keeps the body's box inside it.  Two movers whose reach boxes do not meet cannot see each other, before, between or
// after their moves.  Over-estimating costs levels; nothing here under-estimates.
// fp64 in a fixed order, no FMA contraction: numpy restates it bit for bit.
#include <rocprim/device/device_radix_sort.hpp>
#include <vector>
#include "common.h"
#include "move_dev.h"

namespace clapgpu {

constexpr int OB = 256;
constexpr uint32_t ORDER_CHUNK = 8;                     // relaxation rounds between two looks at the `changed` word
constexpr uint32_t ORDER_ROUND_BLOCKS = 2048;           // a round's grid at most: its lanes stride over the pairs
// the control words
constexpr int CTL_PAIRS = 0, CTL_CHANGED = 1 /* three: round r writes r % 3 */, CTL_ALONE = 4, CTL_MAX = 5, CTL_ROUNDS = 6,
              CTL_WORDS = 16;
constexpr uint8_t CLS_LEVELED = 0, CLS_OUT = 1 /* a body listed twice, or no body of the set: level 0, no conflicts */,
                  CLS_ALONE = 2 /* a box that is not finite: conflicts with every other leveled mover */;

struct ReachK {
    uint32_t n, n_bodies;
    const uint32_t *body;
    const double *ray_off;
    const float *motion, *velocity;
    const double *aabb, *pos, *yoffset;
    double gravity_y;                   // (double)(float)w->gravity[1]
    double dt;
    double *reach, *search;
    uint8_t *cls;
    uint32_t *level, *ctl;
};

__device__ __forceinline__ double finite_or_0(double v) { return isfinite(v) ? v : 0.0; }

__global__ __launch_bounds__(OB)
void k_order_reach(ReachK r)
{
    const uint32_t k = blockIdx.x * OB + threadIdx.x;
    if (k >= r.n) return;
    const uint32_t i = r.body[k];
    double out[6];
    uint8_t cls = CLS_LEVELED;
    if (i >= r.n_bodies) {
        for (int a = 0; a < 6; a++) out[a] = __builtin_nan("");
        cls = CLS_OUT;
    } else {
        double bb[6];
        for (int a = 0; a < 6; a++) bb[a] = r.aabb[6 * (size_t)i + a];
        // phd::ground_ray_len and ground_ray, the same operations
        const double roff = r.ray_off[k] - 0.05;
        const double ray_len = r.yoffset[i] - roff + 1e-3;
        const double rl = ray_len > 0.0 ? ray_len : 0.0;                     // a negative or NaN length casts no ray
        const double start = (double)(float)(r.pos[3 * (size_t)i + 1] - roff);
        const double end = start - rl * 2.0;
        const double vx = r.velocity[3 * (size_t)k], vy = r.velocity[3 * (size_t)k + 1], vz = r.velocity[3 * (size_t)k + 2];
        const double dx = r.motion[2 * (size_t)k], dz = r.motion[2 * (size_t)k + 1];
        const double a0 = fabs(vx) + fabs(vy) + fabs(vz);
        double A = a0 + fabs(r.gravity_y) * r.dt;
        if (!isfinite(A)) A = a0;
        A = finite_or_0(A);
        const double B = finite_or_0(3.0 * (fabs(dx) + fabs(dz)));
        const double S = A > B ? A : B;
        const double dtc = r.dt < 1e-6 ? 0.0 : r.dt > 1.0 / 30.0 ? 1.0 / 30.0 : r.dt;
        const double T = finite_or_0(S * dtc);
        double mag = T;
        for (int a = 0; a < 6; a++) mag = fmax(mag, fabs(bb[a]));
        mag = fmax(mag, fabs(start));
        mag = fmax(mag, fabs(end));
        mag = fmax(mag, rl);
        const double pad = mag * 0x1p-20 + 1e-6;
        const double gx = T + pad, gy = rl + T + pad;
        const double low = bb[2] - gy, ray_low = end - pad;
        out[0] = bb[0] - gx; out[1] = bb[1] + gx;
        const double high = bb[3] + gy, ray_high = start + pad;
        out[2] = ray_low < low ? ray_low : low; out[3] = ray_high > high ? ray_high : high;
        out[4] = bb[4] - gx; out[5] = bb[5] + gx;
        for (int a = 0; a < 6; a++)
            if (!isfinite(out[a])) cls = CLS_ALONE;
    }
    for (int a = 0; a < 6; a++) r.reach[6 * (size_t)k + a] = out[a];
    // the pair search takes finite boxes; a mover outside it gets a row that meets no row, not even its like: min above max
    if (cls != CLS_LEVELED) {
        out[0] = 0x1p1000; out[1] = -0x1p1000;
        for (int a = 2; a < 6; a++) out[a] = 0.0;
        if (cls == CLS_ALONE) atomicAdd(&r.ctl[CTL_ALONE], 1u);
    }
    for (int a = 0; a < 6; a++) r.search[6 * (size_t)k + a] = out[a];
    r.cls[k] = cls;
    r.level[k] = 0;
}

__global__ __launch_bounds__(OB)
void k_order_dups(uint32_t cap, const uint32_t *pairs, const uint32_t *ctl, const uint32_t *body, uint8_t *cls)
{
    const uint32_t total = ctl[CTL_PAIRS] < cap ? ctl[CTL_PAIRS] : cap;
    for (uint32_t p = blockIdx.x * OB + threadIdx.x; p < total; p += gridDim.x * OB) {
        const uint32_t i = pairs[2 * (size_t)p], j = pairs[2 * (size_t)p + 1];
        if (body[i] == body[j]) { cls[i] = CLS_OUT; cls[j] = CLS_OUT; }
    }
}

// Round r.  changed[r % 3] is this round's word (zero on entry: the round before zeroed it), changed[(r + 2) % 3] the
// word of the round before.  level[] only grows, and a value read stale only costs a round: the round that raises
// nothing has read every value as the launch boundary left it.
__device__ __forceinline__ bool round_runs(uint32_t r, uint32_t *ctl)
{
    return r == 0 || ctl[CTL_CHANGED + (r + 2) % 3] != 0;
}

__device__ __forceinline__ void raise(uint32_t r, uint32_t *ctl, uint32_t *level, uint32_t j, uint32_t want)
{
    if (level[j] >= want) return;
    atomicMax(&level[j], want);
    atomicMax(&ctl[CTL_MAX], want);
    ctl[CTL_CHANGED + r % 3] = 1;
}

__global__ __launch_bounds__(OB)
void k_order_round(uint32_t r, uint32_t cap, const uint32_t *pairs, uint32_t *ctl, const uint8_t *cls, uint32_t *level)
{
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (first) ctl[CTL_CHANGED + (r + 1) % 3] = 0;                           // nobody reads or writes it in this round
    if (!round_runs(r, ctl)) return;
    if (first) ctl[CTL_ROUNDS] = ctl[CTL_ROUNDS] + 1;
    const uint32_t total = ctl[CTL_PAIRS] < cap ? ctl[CTL_PAIRS] : cap;
    for (uint32_t p = blockIdx.x * OB + threadIdx.x; p < total; p += gridDim.x * OB) {
        const uint32_t i = pairs[2 * (size_t)p], j = pairs[2 * (size_t)p + 1];
        if (cls[i] | cls[j]) continue;
        raise(r, ctl, level, j, level[i] + 1);
    }
}

// ... and the conflicts no pair states: a mover that stands alone against every earlier leveled mover, every leveled
// mover against every earlier one that stands alone.  n lanes of up to n steps: the price of a box that is not finite.
__global__ __launch_bounds__(OB)
void k_order_alone(uint32_t r, uint32_t n, uint32_t *ctl, const uint8_t *cls, uint32_t *level)
{
    const uint32_t j = blockIdx.x * OB + threadIdx.x;
    if (j >= n || !round_runs(r, ctl)) return;
    const uint8_t cj = cls[j];
    if (cj == CLS_OUT) return;
    uint32_t want = 0;
    for (uint32_t i = 0; i < j; i++) {
        const uint8_t ci = cls[i];
        if (ci == CLS_OUT || (ci != CLS_ALONE && cj != CLS_ALONE)) continue;
        const uint32_t l = level[i] + 1;
        if (l > want) want = l;
    }
    if (want) raise(r, ctl, level, j, want);
}

__global__ __launch_bounds__(OB)
void k_order_keys(uint32_t n, const uint32_t *level, uint32_t *keys, uint32_t *vals)
{
    const uint32_t k = blockIdx.x * OB + threadIdx.x;
    if (k >= n) return;
    keys[k] = level[k];
    vals[k] = k;
}

// every level 0 .. n_levels - 1 has a mover (a level above 0 stands on a chain through all below it)
__global__ __launch_bounds__(OB)
void k_order_first(uint32_t n, const uint32_t *keys, uint32_t n_levels, uint32_t *level_first)
{
    const uint32_t p = blockIdx.x * OB + threadIdx.x;
    if (p >= n) return;
    if (p == 0) level_first[n_levels] = n;
    if (p == 0 || keys[p] != keys[p - 1]) level_first[keys[p]] = p;
}

// src of lane p: from[p] (gather: from = the sorted movers, rows p <- from[p]) or rows from[p] <- p (scatter)
template <typename T, int W>
__device__ __forceinline__ void copy_row(T *dst, size_t d, const T *src, size_t s)
{
    for (int a = 0; a < W; a++) dst[W * d + a] = src[W * s + a];
}

__global__ __launch_bounds__(OB)
void k_order_gather(uint32_t n, const uint32_t *order, clapgpu_move m, clapgpu_move lm)
{
    const uint32_t p = blockIdx.x * OB + threadIdx.x;
    if (p >= n) return;
    const uint32_t k = order[p];
    copy_row<uint32_t, 1>(const_cast<uint32_t *>(lm.body), p, m.body, k);
    copy_row<double, 1>(const_cast<double *>(lm.ray_off), p, m.ray_off, k);
    copy_row<float, 2>(const_cast<float *>(lm.motion), p, m.motion, k);
    copy_row<uint8_t, 1>(const_cast<uint8_t *>(lm.state), p, m.state, k);
    copy_row<uint8_t, 1>(const_cast<uint8_t *>(lm.jump), p, m.jump, k);
    copy_row<float, 2>(const_cast<float *>(lm.jump_params), p, m.jump_params, k);
    copy_row<float, 3>(lm.velocity, p, m.velocity, k);
    copy_row<float, 3>(lm.normal, p, m.normal, k);
    copy_row<uint8_t, 1>(lm.airborne, p, m.airborne, k);
    if (m.entity) {
        copy_row<uint32_t, 1>(const_cast<uint32_t *>(lm.entity), p, m.entity, k);
        copy_row<float, 4>(const_cast<float *>(lm.yaw_quat), p, m.yaw_quat, k);
    }
}

// the in/out and out arrays back to the caller's order, and the push's inputs of the level-major parts (lp) into
// list-order ones
__global__ __launch_bounds__(OB)
void k_order_scatter(uint32_t n, const uint32_t *order, clapgpu_move lm, clapgpu_move m, const uint32_t *l_body,
                     const uint32_t *l_flags, const float *l_given, uint32_t *o_body, uint32_t *o_flags, float *o_given)
{
    const uint32_t p = blockIdx.x * OB + threadIdx.x;
    if (p >= n) return;
    const uint32_t k = order[p];
    copy_row<float, 3>(m.velocity, k, lm.velocity, p);
    copy_row<float, 3>(m.normal, k, lm.normal, p);
    copy_row<uint8_t, 1>(m.airborne, k, lm.airborne, p);
    copy_row<uint8_t, 1>(m.request, k, lm.request, p);
    copy_row<uint8_t, 1>(m.applied, k, lm.applied, p);
    copy_row<int32_t, 1>(m.collision, k, lm.collision, p);
    copy_row<float, 2>(m.first_frac, k, lm.first_frac, p);
    copy_row<int32_t, 6>(m.push_hit, k, lm.push_hit, p);
    copy_row<uint32_t, 1>(m.flags, k, lm.flags, p);
    copy_row<uint32_t, 1>(o_body, k, l_body, p);
    copy_row<uint32_t, 1>(o_flags, k, l_flags, p);
    copy_row<float, 3>(o_given, k, l_given, p);
}

// ---------------------------------------------------------------------------------------------------- the scratch
struct OrderLayout { size_t search, cls, pairs, ctl, bytes; };

static OrderLayout order_layout(uint32_t n, uint32_t cap)
{
    OrderLayout l;
    Carve c;
    l.search = c.take((size_t)n * 6 * sizeof(double));
    l.cls = c.take(n);
    l.pairs = c.take((size_t)(cap ? cap : 1) * 2 * sizeof(uint32_t));
    l.ctl = c.take(CTL_WORDS * sizeof(uint32_t));
    l.bytes = c.bytes();
    return l;
}

struct OrderedLayout {
    size_t order, reach, level, keys0, keys1, vals0, vals1, sort, sort_bytes, level_first;
    size_t body, ray_off, motion, state, jump, jump_params, velocity, normal, airborne, request, applied, collision,
           first_frac, push_hit, flags, entity, yaw_quat;
    size_t o_body, o_flags, o_given, move, bytes;
};

static hipError_t ordered_layout(uint32_t n_bodies, uint32_t n, uint32_t cap, size_t move_bytes, OrderedLayout &l)
{
    Carve c;
    const size_t N = n;
    l.order = c.take(order_layout(n, cap).bytes);
    l.reach = c.take(N * 6 * sizeof(double));
    l.level = c.take(N * 4);
    l.keys0 = c.take(N * 4); l.keys1 = c.take(N * 4); l.vals0 = c.take(N * 4); l.vals1 = c.take(N * 4);
    rocprim::double_buffer<uint32_t> none(nullptr, nullptr);
    l.sort_bytes = 0;
    const hipError_t err = rocprim::radix_sort_pairs(nullptr, l.sort_bytes, none, none, N, 0, 32, nullptr);
    l.sort = c.take(l.sort_bytes);
    l.level_first = c.take((N + 1) * 4);
    l.body = c.take(N * 4); l.ray_off = c.take(N * 8); l.motion = c.take(N * 8); l.state = c.take(N); l.jump = c.take(N);
    l.jump_params = c.take(N * 8); l.velocity = c.take(N * 12); l.normal = c.take(N * 12); l.airborne = c.take(N);
    l.request = c.take(N); l.applied = c.take(N); l.collision = c.take(N * 4); l.first_frac = c.take(N * 8);
    l.push_hit = c.take(N * 24); l.flags = c.take(N * 4); l.entity = c.take(N * 4); l.yaw_quat = c.take(N * 16);
    l.o_body = c.take(N * 4); l.o_flags = c.take(N * 4); l.o_given = c.take(N * 12);
    l.move = c.take(move_bytes);
    l.bytes = c.bytes();
    return err;
}

struct OrderResult { uint32_t n_levels, pair_total, status, rounds; };

// what both entry points run: boxes, pairs, levels; CLAPGPU_ERR_TOO_LARGE with `out` filled when the pairs did not fit
// or a box was too large for order_bp.  Synchronises the stream.
static int order_levels(void *stream, clapgpu_bp *order_bp, const clapgpu_bodies *b, const clapgpu_world *w, double dt_sec,
                        const clapgpu_move *m, uint32_t cap, double *reach, uint32_t *level, void *scratch, OrderResult &out)
{
    const uint32_t n = m->n;
    const OrderLayout l = order_layout(n, cap);
    uint8_t *base = static_cast<uint8_t *>(scratch);
    double *search = reinterpret_cast<double *>(base + l.search);
    uint8_t *cls = base + l.cls;
    uint32_t *pairs = reinterpret_cast<uint32_t *>(base + l.pairs), *ctl = reinterpret_cast<uint32_t *>(base + l.ctl);
    hipStream_t s = as_stream(stream);
    CLAPGPU_HIP(hipMemsetAsync(ctl, 0, CTL_WORDS * sizeof(uint32_t), s));
    ReachK r;
    r.n = n; r.n_bodies = b->n; r.body = m->body; r.ray_off = m->ray_off; r.motion = m->motion; r.velocity = m->velocity;
    r.aabb = b->aabb; r.pos = b->pos; r.yoffset = b->yoffset; r.gravity_y = (double)(float)w->gravity[1]; r.dt = dt_sec;
    r.reach = reach; r.search = search; r.cls = cls; r.level = level; r.ctl = ctl;
    const dim3 grid((n + OB - 1) / OB);
    hipLaunchKernelGGL(k_order_reach, grid, dim3(OB), 0, s, r);
    CLAPGPU_LAUNCH_CHECK("k_order_reach");
    int rc = clapgpu_bp_collide(stream, order_bp, n, search, cap ? pairs : nullptr, cap, ctl + CTL_PAIRS, nullptr, 0, nullptr);
    if (rc) return rc;
    uint32_t blocks = (cap + OB - 1) / OB;
    blocks = blocks < 1 ? 1 : blocks > ORDER_ROUND_BLOCKS ? ORDER_ROUND_BLOCKS : blocks;
    hipLaunchKernelGGL(k_order_dups, dim3(blocks), dim3(OB), 0, s, cap, pairs, ctl, m->body, cls);
    CLAPGPU_LAUNCH_CHECK("k_order_dups");
    uint32_t host[CTL_WORDS];
    CLAPGPU_HIP(hipMemcpyAsync(host, ctl, sizeof(host), hipMemcpyDeviceToHost, s));
    if ((rc = clapgpu_bp_status(stream, order_bp, &out.status))) return rc;   // synchronises
    out.pair_total = host[CTL_PAIRS];
    out.n_levels = 0; out.rounds = 0;
    if (out.pair_total > cap || (out.status & 1u)) return CLAPGPU_ERR_TOO_LARGE;
    const bool alone = host[CTL_ALONE] != 0;
    // the longest path has at most n movers: n rounds raise every level, one more sees that nothing is left
    for (uint32_t round = 0;;) {
        for (uint32_t q = 0; q < ORDER_CHUNK; q++, round++) {
            hipLaunchKernelGGL(k_order_round, dim3(blocks), dim3(OB), 0, s, round, cap, pairs, ctl, cls, level);
            CLAPGPU_LAUNCH_CHECK("k_order_round");
            if (alone) {
                hipLaunchKernelGGL(k_order_alone, grid, dim3(OB), 0, s, round, n, ctl, cls, level);
                CLAPGPU_LAUNCH_CHECK("k_order_alone");
            }
        }
        CLAPGPU_HIP(hipMemcpyAsync(host, ctl, sizeof(host), hipMemcpyDeviceToHost, s));
        CLAPGPU_HIP(hipStreamSynchronize(s));
        if (host[CTL_CHANGED + (round - 1) % 3] == 0) break;
        if (round > n + ORDER_CHUNK) {
            set_last_error("clapgpu_characters_order: the levels did not settle");
            return CLAPGPU_ERR_UNKNOWN;
        }
    }
    out.n_levels = host[CTL_MAX] + 1;
    out.rounds = host[CTL_ROUNDS];
    return CLAPGPU_OK;
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" size_t clapgpu_characters_order_scratch_bytes(uint32_t n, uint32_t pair_capacity)
{
    return n ? order_layout(n, pair_capacity).bytes : 0;
}

extern "C" int clapgpu_characters_order(void *stream, clapgpu_bp *order_bp, const clapgpu_bodies *b, const clapgpu_world *w,
                                        double dt_sec, const clapgpu_move *m, uint32_t pair_capacity, double *reach,
                                        uint32_t *level, uint32_t *summary, void *scratch)
{
    if (!m || !b || !w || !order_bp || !summary) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!b->aabb || !b->pos || !b->yoffset) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (m->n && (!m->body || !m->ray_off || !m->motion || !m->velocity || !reach || !level)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (m->n && (!scratch || (reinterpret_cast<uintptr_t>(scratch) & 255u))) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    summary[0] = summary[1] = summary[2] = summary[3] = 0;
    if (m->n == 0) return CLAPGPU_OK;
    OrderResult out = { 0, 0, 0, 0 };
    const int rc = order_levels(stream, order_bp, b, w, dt_sec, m, pair_capacity, reach, level, scratch, out);
    summary[0] = out.n_levels; summary[1] = out.pair_total; summary[2] = out.status; summary[3] = out.rounds;
    return rc;
}

extern "C" size_t clapgpu_characters_move_ordered_scratch_bytes(uint32_t n_bodies, uint32_t n, uint32_t pair_capacity)
{
    const size_t move_bytes = clapgpu_characters_move_scratch_bytes(n_bodies, n);
    if (!move_bytes) return 0;                                               // n == 0, n too large, or no device to ask
    OrderedLayout l;
    if (ordered_layout(n_bodies, n, pair_capacity, move_bytes, l) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return l.bytes;
}

extern "C" int clapgpu_characters_move_ordered(void *stream, clapgpu_bp *bp, clapgpu_bp *order_bp, const clapgpu_bodies *b,
                                               const clapgpu_world *w, const clapgpu_geoms *statics, const clapgpu_trimesh *meshes,
                                               const clapgpu_entities *e, double dt_sec, const clapgpu_move *m,
                                               uint32_t pair_capacity, uint32_t *level, uint32_t *n_levels, void *scratch)
{
    int rc = move_check(bp, b, w, statics, e, m);
    if (rc) return rc;
    if (!order_bp || !b->aabb || !n_levels) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (m->n == 0) { *n_levels = 0; return CLAPGPU_OK; }
    if (!scratch || (reinterpret_cast<uintptr_t>(scratch) & 255u)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    *n_levels = 0;
    const uint32_t n = m->n;
    const size_t move_bytes = clapgpu_characters_move_scratch_bytes(b->n, n);
    if (!move_bytes) return n > (1u << 28) ? CLAPGPU_ERR_TOO_LARGE : CLAPGPU_ERR_UNKNOWN;
    OrderedLayout l;
    CLAPGPU_HIP(ordered_layout(b->n, n, pair_capacity, move_bytes, l));
    uint8_t *base = static_cast<uint8_t *>(scratch);
    auto u32 = [&](size_t at) { return reinterpret_cast<uint32_t *>(base + at); };
    auto f32 = [&](size_t at) { return reinterpret_cast<float *>(base + at); };
    if (!level) level = u32(l.level);
    hipStream_t s = as_stream(stream);

    // ---- the levels; nothing has moved when this refuses ----
    OrderResult res = { 0, 0, 0, 0 };
    rc = order_levels(stream, order_bp, b, w, dt_sec, m, pair_capacity, reinterpret_cast<double *>(base + l.reach), level,
                      base + l.order, res);
    if (rc) return rc;
    *n_levels = res.n_levels;

    // ---- the movers by (level, k): a stable sort of k by level ----
    const dim3 grid((n + OB - 1) / OB);
    rocprim::double_buffer<uint32_t> keys(u32(l.keys0), u32(l.keys1)), vals(u32(l.vals0), u32(l.vals1));
    hipLaunchKernelGGL(k_order_keys, grid, dim3(OB), 0, s, n, level, keys.current(), vals.current());
    CLAPGPU_LAUNCH_CHECK("k_order_keys");
    CLAPGPU_HIP(rocprim::radix_sort_pairs(base + l.sort, l.sort_bytes, keys, vals, (size_t)n, 0, bits_of(res.n_levels - 1), s));
    uint32_t *level_first = u32(l.level_first);
    hipLaunchKernelGGL(k_order_first, grid, dim3(OB), 0, s, n, keys.current(), res.n_levels, level_first);
    CLAPGPU_LAUNCH_CHECK("k_order_first");
    std::vector<uint32_t> first(res.n_levels + 1);
    CLAPGPU_HIP(hipMemcpyAsync(first.data(), level_first, first.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));

    // ---- level-major copies of the movers ----
    clapgpu_move lm;
    lm.n = n;
    lm.body = u32(l.body); lm.ray_off = reinterpret_cast<double *>(base + l.ray_off); lm.motion = f32(l.motion);
    lm.state = base + l.state; lm.jump = base + l.jump; lm.jump_params = f32(l.jump_params); lm.velocity = f32(l.velocity);
    lm.normal = f32(l.normal); lm.airborne = base + l.airborne; lm.request = base + l.request; lm.applied = base + l.applied;
    lm.collision = reinterpret_cast<int32_t *>(base + l.collision); lm.first_frac = f32(l.first_frac);
    lm.push_hit = reinterpret_cast<int32_t *>(base + l.push_hit); lm.flags = u32(l.flags);
    lm.entity = m->entity ? u32(l.entity) : nullptr; lm.yaw_quat = m->entity ? f32(l.yaw_quat) : nullptr;
    const uint32_t *order = vals.current();
    hipLaunchKernelGGL(k_order_gather, grid, dim3(OB), 0, s, n, order, *m, lm);
    CLAPGPU_LAUNCH_CHECK("k_order_gather");
    CLAPGPU_HIP(hipStreamSynchronize(s));                                    // level_first is here
    if (first[0] != 0 || first[res.n_levels] != n) {
        set_last_error("clapgpu_characters_move_ordered: the level starts do not cover the movers");
        return CLAPGPU_ERR_UNKNOWN;
    }
    for (uint32_t L = 0; L < res.n_levels; L++)
        if (first[L + 1] <= first[L] || first[L + 1] > n) {
            set_last_error("clapgpu_characters_move_ordered: an empty level");
            return CLAPGPU_ERR_UNKNOWN;
        }

    // ---- stages 1 to 5 without the push, level by level ----
    MoveParts p;
    if ((rc = move_parts(base + l.move, b->n, n, &p))) return rc;
    for (uint32_t L = 0; L < res.n_levels; L++)
        if ((rc = move_slice(stream, bp, b, w, statics, meshes, dt_sec, &lm, first[L], first[L + 1] - first[L], p, false)))
            return rc;
    // ---- the flags and the rotation hand-off, back to the caller's order, and the pushes of all movers in list order ----
    if ((rc = move_finish(stream, e, &lm, p))) return rc;
    hipLaunchKernelGGL(k_order_scatter, grid, dim3(OB), 0, s, n, order, lm, *m, p.slide_body, p.slide_flags, p.given,
                       u32(l.o_body), u32(l.o_flags), f32(l.o_given));
    CLAPGPU_LAUNCH_CHECK("k_order_scatter");
    if (!(dt_sec < 1e-6))
        return clapgpu_bodies_push(stream, b, w, n, u32(l.o_body), f32(l.o_given), m->push_hit, u32(l.o_flags), nullptr, p.push);
    return CLAPGPU_OK;
}
