// bp_restatic.hip -- clapgpu_bp_statics_update: the static boxes of a clapgpu_bp registered again, on the device, and the
// read-back of a statics image (clapgpu_bp_statics_sizes / _read).  The rule for one static on one level is bp_statics.h's,
// host and device: the host binning there and the kernels below both call it and make the same image array for array.  An
// object that is never updated runs none of this: the create-time image inside its first allocation stays what its kernels read.
//
// One update, four launches over the object's SECOND allocation (made on the first update, grown geometrically):
//   k_rs_count   one wavefront per (level, static): large or not; the blocks of a registered static, one per lane (at
//                most 64), hashed (both: the rule's); the first lane of each distinct bucket counts it; the bounds of
//                the registered boxes as order keys (atomicMax on zeroed words)
//   k_rs_scan    one workgroup: the bucket counts of all levels scanned end to end into the starts, the large flags
//                compacted per level, in static order, into the large list and its records; the totals for the host
//   -- the totals come to the host here (one copy, one synchronisation).  They fit the allocation's room, or a larger
//      allocation is made and the two launches run again (no second wait: the totals are known)
//   k_rs_fill    k_rs_count's enumeration again: a static index into its bucket's range, in the order the atomics took
//   k_rs_order   one lane per registration: its static index ranked among its bucket's (they are distinct: a static
//                enters a bucket once), written at that rank with its record -- the CSR order whatever order the fill took
// The allocation holds the work arrays and TWO image slots: an update builds into the slot the object does not point
// at, and the object's pointers and counts change only after everything has been issued, checked and waited for.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <vector>
#include "bp_object.h"
#include "bp_statics.h"

namespace clapgpu {

constexpr int RB = 256;                  // four wavefronts a workgroup in the per-wavefront kernels
constexpr int RS_SCAN = 1024;            // k_rs_scan's one workgroup

// what the first two launches leave for the host: bounds[0..2] ~order_key(min), [3..5] order_key(max) of the registered
// boxes, reduced by atomicMax from zero (zero: none; no double has the key zero or all ones but a NaN, and a registered
// box has none); the registrations of all levels; the large statics up to the end of each level.  No total is an atomic
// sum: one word added to by every wavefront of k_rs_count cost that kernel 0.09 of its 0.1 ms at 5 000 statics.
struct RsHead {
    unsigned long long bounds[6];
    uint32_t n_entries;
    uint32_t large_end[CLAPGPU_BP_LEVELS_MAX];
    uint32_t pad;
};

struct RsK {
    uint32_t n_static, levels, buckets;
    double cell;
    const double *aabb;                  // the new boxes [n_static][6]
    uint32_t *cnt;                       // [levels * buckets] statics per bucket (k_rs_count), then the fill's cursors
    uint8_t *flag;                       // [levels * n_static] 1: large on that level
    RsHead *head;
    uint32_t *tmp, *tmp_bucket;          // [cap_entries] static indices in bucket order, unordered inside a bucket; their level * buckets + bucket
    // the image being built (BpK's s_* arrays of the slot)
    uint32_t *start, *entries, *large;
    GridRec *recs, *lrecs;
    uint32_t cap_entries, cap_large;     // the slot's room: nothing is written past it (the host grows it before the fill)
    uint32_t n_entries;                  // by value from the host, for k_rs_order (0 before the totals are known)
};

__device__ __forceinline__ void store_rec(GridRec *r, const double (&bb)[6], uint32_t idx)
{
    double2 *o = reinterpret_cast<double2 *>(r);
    o[0] = make_double2(bb[0], bb[1]); o[1] = make_double2(bb[2], bb[3]); o[2] = make_double2(bb[4], bb[5]);
    reinterpret_cast<int4 *>(r)[3] = make_int4((int)idx, 0, 0, 0);      // the cell words of a static's record are zero
}

__device__ __forceinline__ void zero_rec(GridRec *r)
{
    const double z[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    store_rec(r, z, 0u);
}

// A static on level l as the whole wavefront sees it: large (wave-uniform), or lane u's block u of its <= 64 blocks:
// mine: the lane has a block and no lower lane's block falls in the same bucket h (the host's first-met test).
struct RsBlocks { bool large, mine; uint32_t h; };
__device__ __forceinline__ RsBlocks lane_block(const RsK &q, uint32_t l, const double (&bb)[6], int lane)
{
    const StaticBlocks b = static_blocks(bb, level_cell(q.cell, l));
    RsBlocks r = { b.large, false, 0u };
    if (r.large) return r;
    const bool has = (uint32_t)lane < b.nb;
    r.h = static_block_bucket(b, has ? (uint32_t)lane : 0u, q.buckets - 1);
    bool dup = false;
#pragma unroll
    for (int i = 0; i < WAVE - 1; i++) {                                 // all lanes shuffle; lane i's bucket against the lanes above it
        const uint32_t hi_ = __shfl(r.h, i);
        dup |= i < lane && (uint32_t)i < b.nb && hi_ == r.h;
    }
    r.mine = has && !dup;
    return r;
}

// (level, static) of this wavefront; false: none
__device__ __forceinline__ bool wave_item(uint32_t items, uint32_t per, uint32_t *l, uint32_t *i)
{
    const uint32_t item = blockIdx.x * (RB / WAVE) + threadIdx.x / WAVE;
    if (item >= items) return false;
    *l = item / per; *i = item - *l * per;
    return true;
}

// Launch 1
__global__ __launch_bounds__(RB)
void k_rs_count(RsK q)
{
    uint32_t l, s;
    if (!wave_item(q.levels * q.n_static, q.n_static, &l, &s)) return;
    const int lane = lane_id();
    double bb[6];
    load_box(q.aabb, s, bb);
    const RsBlocks r = lane_block(q, l, bb, lane);
    if (r.large) {
        if (lane == 0) q.flag[l * q.n_static + s] = 1;
        return;
    }
    if (r.mine) atomicAdd(&q.cnt[(size_t)l * q.buckets + r.h], 1u);
    if (lane < 6) {                                                      // lanes 0..2: the minimum corner, 3..5: the maximum corner
        const double v = lane == 0 ? bb[0] : lane == 1 ? bb[2] : lane == 2 ? bb[4] : lane == 3 ? bb[1] : lane == 4 ? bb[3] : bb[5];
        const unsigned long long key = lane < 3 ? ~order_key(v) : order_key(v);
        // most boxes do not move the bound: look before asking for the atomic (a stale look only costs the atomic)
        if (key > __hip_atomic_load(&q.head->bounds[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(&q.head->bounds[lane], key);
    }
}

// Launch 2: ONE workgroup.  The counts of all levels are one sequence (level l's starts are offset by what the levels
// before it hold: bp_statics_concat), so are the large flags.
__global__ __launch_bounds__(RS_SCAN)
void k_rs_scan(RsK q)
{
    __shared__ uint32_t wtot[RS_SCAN / WAVE];
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    auto block_incl = [&](uint32_t v, uint32_t *total) {                // every thread of the workgroup calls it
        const uint32_t incl = wave_prefix_sum(v);
        __syncthreads();                                                 // the round before has read wtot
        if (lane == WAVE - 1) wtot[wave] = incl;
        __syncthreads();
        uint32_t before = 0, t = 0;
        for (int w = 0; w < RS_SCAN / WAVE; w++) { const uint32_t x = wtot[w]; before += w < wave ? x : 0u; t += x; }
        *total = t;
        return incl + before;
    };
    const uint32_t G = q.levels * q.buckets, F = q.levels * q.n_static;
    uint32_t carry = 0, total;
    for (uint32_t base = 0; base < G; base += RS_SCAN) {
        const uint32_t g = base + threadIdx.x;
        const uint32_t c = g < G ? q.cnt[g] : 0u;
        const uint32_t incl = block_incl(c, &total);
        if (g < G) {
            q.cnt[g] = 0;                                                // the fill's cursor
            const uint32_t l = g / q.buckets, b = g - l * q.buckets;
            uint32_t *st = q.start + (size_t)l * (q.buckets + 1);
            st[b] = carry + incl - c;
            if (b == q.buckets - 1) st[q.buckets] = carry + incl;
        }
        carry += total;
    }
    const uint32_t n_entries = carry;
    carry = 0;
    for (uint32_t base = 0; base < F; base += RS_SCAN) {
        const uint32_t f = base + threadIdx.x;
        const uint32_t c = f < F ? q.flag[f] : 0u;
        const uint32_t incl = block_incl(c, &total);
        const uint32_t at = carry + incl - c;
        if (f < F && f % q.n_static == q.n_static - 1) q.head->large_end[f / q.n_static] = carry + incl;
        if (c && at < q.cap_large) {
            const uint32_t s = f % q.n_static;
            double bb[6];
            load_box(q.aabb, s, bb);
            q.large[at] = s;
            store_rec(q.lrecs + at, bb, s);
        }
        carry += total;
    }
    if (threadIdx.x == 0) {                                              // the host's placeholders of an empty list
        q.head->n_entries = n_entries;
        if (n_entries == 0) { q.entries[0] = 0; zero_rec(q.recs); }
        if (carry == 0) { q.large[0] = 0; zero_rec(q.lrecs); }
    }
}

// Launch 3
__global__ __launch_bounds__(RB)
void k_rs_fill(RsK q)
{
    uint32_t l, s;
    if (!wave_item(q.levels * q.n_static, q.n_static, &l, &s)) return;
    double bb[6];
    load_box(q.aabb, s, bb);
    const RsBlocks r = lane_block(q, l, bb, lane_id());
    if (r.large || !r.mine) return;
    const uint32_t at = q.start[(size_t)l * (q.buckets + 1) + r.h] + atomicAdd(&q.cnt[(size_t)l * q.buckets + r.h], 1u);
    if (at < q.cap_entries) { q.tmp[at] = s; q.tmp_bucket[at] = l * q.buckets + r.h; }
}

// Launch 4: one lane per registration.  Its rank among its bucket's static indices is its place: a lane walks its own
// bucket (a few entries on the fine levels; on the coarse ones a few buckets hold every static, and their walks are the
// same loads for the whole wavefront).  One wavefront per bucket took 0.86 ms of a six-level update of 5 000 statics, all
// of it in the 27 buckets of the top level.
__global__ __launch_bounds__(RB)
void k_rs_order(RsK q)
{
    const uint32_t e = blockIdx.x * RB + threadIdx.x;
    if (e >= q.n_entries) return;
    const uint32_t g = q.tmp_bucket[e], v = q.tmp[e];
    if (g >= q.levels * q.buckets || v >= q.n_static) return;            // never: the fill wrote every place below n_entries
    const uint32_t l = g / q.buckets;
    const uint32_t *st = q.start + (size_t)l * (q.buckets + 1) + (g - l * q.buckets);
    const uint32_t s0 = st[0], s1 = st[1] < q.n_entries ? st[1] : q.n_entries;
    uint32_t rank = 0;
    for (uint32_t f = s0; f < s1; f++) rank += q.tmp[f] < v ? 1u : 0u;
    if (s0 + rank >= s1) return;                                         // never
    double bb[6];
    load_box(q.aabb, v, bb);
    q.entries[s0 + rank] = v;
    store_rec(q.recs + s0 + rank, bb, v);
}

// The second allocation, carved as bp_create.hip carves the first, every array stated once: the work arrays (zeroed in front of
// every count, up to work_end), then two image slots of at's room.  No at.dev2: sized only; else q points into it, at at.slot.
struct RsCarved { RsK q; size_t work_end, bytes; };

static RsCarved rs_carve(const clapgpu_bp *bp, const BpStatics &at, const double *aabb)
{
    RsCarved y{};
    RsK &q = y.q;
    const uint32_t cap_e = q.cap_entries = at.cap_entries, cap_l = q.cap_large = at.cap_large;
    q.n_static = bp->n_static; q.levels = bp->levels; q.buckets = bp->buckets; q.cell = bp->cell; q.aabb = aabb;
    Carve c;
    auto arr = [&](auto *&member, size_t count) {
        const size_t off = c.take(sizeof(*member) * count);
        if (at.dev2) member = reinterpret_cast<std::remove_reference_t<decltype(member)>>(static_cast<char *>(at.dev2) + off);
    };
    arr(q.cnt, (size_t)bp->levels * bp->buckets);
    arr(q.flag, (size_t)bp->levels * bp->n_static);
    arr(q.head, 1);
    y.work_end = c.bytes();
    arr(q.tmp, cap_e);
    arr(q.tmp_bucket, cap_e);
    for (int i = 0; i < 2; i++) {
        RsK other{};                                                     // the slot that is not asked for: sized, not pointed at
        RsK &t = i == at.slot ? q : other;
        arr(t.start, (size_t)bp->levels * (bp->buckets + 1));
        arr(t.entries, cap_e);
        arr(t.large, cap_l);
        arr(t.recs, cap_e);
        arr(t.lrecs, cap_l);
    }
    y.bytes = c.bytes();
    return y;
}

static uint32_t wave_blocks(uint32_t items) { return (items + RB / WAVE - 1) / (RB / WAVE); }

// launches 1 and 2
static int launch_count(hipStream_t s, void *base, const RsCarved &y)
{
    CLAPGPU_HIP(hipMemsetAsync(base, 0, y.work_end, s));
    hipLaunchKernelGGL(k_rs_count, dim3(wave_blocks(y.q.levels * y.q.n_static)), dim3(RB), 0, s, y.q);
    CLAPGPU_LAUNCH_CHECK("k_rs_count");
    hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(RS_SCAN), 0, s, y.q);
    CLAPGPU_LAUNCH_CHECK("k_rs_scan");
    return CLAPGPU_OK;
}

// Everything of an update that can fail.  *nx (in: the object's, its slot the other one): the allocation, its room and
// the slot the new image stands in; the caller frees nx->dev2 when it is not the object's and this returns an error.
static int rebuild(hipStream_t s, const clapgpu_bp *bp, const double *aabb, BpStatics *nx, RsHead *head)
{
    auto room = [](uint32_t have, uint32_t need) { return need > have ? (need > 2 * have ? need : 2 * have) : have; };
    auto fresh = [&](uint32_t cap_e, uint32_t cap_l) {                   // the bytes of a fresh allocation: the image goes to its slot 0
        nx->dev2 = nullptr; nx->cap_entries = cap_e; nx->cap_large = cap_l; nx->slot = 0;
        return rs_carve(bp, *nx, aabb).bytes;
    };
    if (!nx->dev2)                                                       // the first update: room for an image like the current one
        CLAPGPU_HIP(hipMalloc(&nx->dev2, fresh(room(64, nx->n_entries + nx->n_entries / 2), room(64, nx->n_large + nx->n_large / 2))));
    RsCarved y = rs_carve(bp, *nx, aabb);
    int rc = launch_count(s, nx->dev2, y);
    if (rc) return rc;
    CLAPGPU_HIP(hipMemcpyAsync(head, y.q.head, sizeof(*head), hipMemcpyDeviceToHost, s));
    CLAPGPU_HIP(hipStreamSynchronize(s));
    const uint32_t n_large = head->large_end[bp->levels - 1];
    if (head->n_entries > nx->cap_entries || n_large > nx->cap_large) {  // grow: another allocation, counted again (no second wait: the counts are known)
        if (nx->dev2 != bp->st.dev2) { (void)hipFree(nx->dev2); }
        CLAPGPU_HIP(hipMalloc(&nx->dev2, fresh(room(nx->cap_entries, head->n_entries), room(nx->cap_large, n_large))));
        y = rs_carve(bp, *nx, aabb);
        rc = launch_count(s, nx->dev2, y);
        if (rc) return rc;
    }
    RsK &q = y.q;
    hipLaunchKernelGGL(k_rs_fill, dim3(wave_blocks(q.levels * q.n_static)), dim3(RB), 0, s, q);
    CLAPGPU_LAUNCH_CHECK("k_rs_fill");
    q.n_entries = head->n_entries;
    if (q.n_entries) {
        hipLaunchKernelGGL(k_rs_order, dim3((q.n_entries + RB - 1) / RB), dim3(RB), 0, s, q);
        CLAPGPU_LAUNCH_CHECK("k_rs_order");
    }
    if (aabb != bp->k.s_aabb)                                            // the last step: the object's own copy of the boxes
        CLAPGPU_HIP(hipMemcpyAsync(const_cast<double *>(bp->k.s_aabb), aabb, sizeof(double) * 6 * (size_t)bp->n_static,
                                   hipMemcpyDeviceToDevice, s));
    CLAPGPU_HIP(hipStreamSynchronize(s));
    return CLAPGPU_OK;
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" int clapgpu_bp_statics_update(void *stream, clapgpu_bp *bp, uint32_t n_static, const double *static_aabb)
{
    if (!bp || n_static != bp->n_static || (n_static && !static_aabb)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!n_static) return CLAPGPU_OK;
    if ((uint64_t)bp->levels * n_static * 64 > 0xffffffffull) return CLAPGPU_ERR_TOO_LARGE;      // the entry count is a uint32
    // the index describes the old statics (its view's s_* fields and bounds), an unconsumed prebin goes with it
    int rc = clapgpu_bp_invalidate(stream, bp);
    if (rc) return rc;
    BpStatics &st = bp->st, nx = st;
    nx.slot = st.dev2 ? 1 - st.slot : 0;
    RsHead rs;
    rc = rebuild(as_stream(stream), bp, static_aabb, &nx, &rs);
    if (rc) {
        if (nx.dev2 && nx.dev2 != st.dev2) (void)hipFree(nx.dev2);
        return rc;
    }
    // ---- nothing below fails: the object becomes the object of the new boxes
    if (st.dev2 && st.dev2 != nx.dev2) (void)hipFree(st.dev2);
    st = nx;                                                             // the allocation, its room and the slot; the rest: below
    double bounds[6];
    for (int a = 0; a < 3; a++) {
        bounds[a] = rs.bounds[a] ? order_value(~rs.bounds[a]) : INFINITY;
        bounds[3 + a] = rs.bounds[3 + a] ? order_value(rs.bounds[3 + a]) : -INFINITY;
    }
    const RsK q = rs_carve(bp, st, static_aabb).q;
    bp_adopt_statics(bp, q.start, q.entries, q.large, q.recs, q.lrecs, rs.n_entries, rs.large_end, bounds);
    return CLAPGPU_OK;
}

extern "C" int clapgpu_bp_statics_sizes(const clapgpu_bp *bp, uint32_t *buckets, uint32_t *n_entries, uint32_t *n_large,
                                        uint32_t large_start[CLAPGPU_BP_LEVELS_MAX + 1], double bounds[6])
{
    if (!bp) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (buckets) *buckets = bp->buckets;
    if (n_entries) *n_entries = bp->st.n_entries;
    if (n_large) *n_large = bp->st.n_large;
    if (large_start) memcpy(large_start, bp->st.large_start, sizeof(bp->st.large_start));
    if (bounds) memcpy(bounds, bp->st.bounds, sizeof(bp->st.bounds));
    return CLAPGPU_OK;
}

extern "C" int clapgpu_bp_statics_read(void *stream, const clapgpu_bp *bp, uint32_t *start, uint32_t *entries, uint32_t *large,
                                       double *entry_boxes, double *large_boxes)
{
    if (!bp) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    hipStream_t s = as_stream(stream);
    const BpK &k = bp->k;
    std::vector<uint32_t> idx[2] = { std::vector<uint32_t>(bp->st.n_entries), std::vector<uint32_t>(bp->st.n_large) };
    std::vector<GridRec> recs[2] = { std::vector<GridRec>(bp->st.n_entries), std::vector<GridRec>(bp->st.n_large) };
    const uint32_t *d_idx[2] = { k.s_entries, k.s_large };
    const GridRec *d_recs[2] = { k.s_recs, k.s_lrecs };
    if (start)
        CLAPGPU_HIP(hipMemcpyAsync(start, k.s_start, sizeof(uint32_t) * (size_t)bp->levels * (bp->buckets + 1), hipMemcpyDeviceToHost, s));
    for (int t = 0; t < 2; t++) {
        if (idx[t].empty()) continue;
        CLAPGPU_HIP(hipMemcpyAsync(idx[t].data(), d_idx[t], sizeof(uint32_t) * idx[t].size(), hipMemcpyDeviceToHost, s));
        CLAPGPU_HIP(hipMemcpyAsync(recs[t].data(), d_recs[t], sizeof(GridRec) * recs[t].size(), hipMemcpyDeviceToHost, s));
    }
    CLAPGPU_HIP(hipStreamSynchronize(s));
    uint32_t *out_idx[2] = { entries, large };
    double *out_box[2] = { entry_boxes, large_boxes };
    for (int t = 0; t < 2; t++)
        for (size_t e = 0; e < idx[t].size(); e++) {
            const GridRec &r = recs[t][e];
            if (r.idx != idx[t][e] || r.cell[0] || r.cell[1] || r.cell[2]) {
                set_last_error("clapgpu_bp_statics_read: a record does not carry its entry's index, or its cell words are not zero");
                return CLAPGPU_ERR_UNKNOWN;
            }
            if (out_idx[t]) out_idx[t][e] = idx[t][e];
            if (out_box[t]) memcpy(out_box[t] + 6 * e, r.bb, sizeof(r.bb));
        }
    return CLAPGPU_OK;
}
