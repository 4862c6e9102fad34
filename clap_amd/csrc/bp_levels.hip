// bp_levels.hip -- the broadphase over a multi-level hash grid (clapgpu_bp_create_levels), for gfx950: the bin, scatter,
// search and emit launches of clapgpu_bp_collide for an object with more than one level.  The rule, and why it finds
// every pair once: bp_levels.h.  The second launch (k_bp_cells) and the launch order are broadphase.hip's; a one-level
// object launches none of this.  fp64 boxes; PARITY UNPINNED like the rest of the broadphase.
#include "bp_object.h"
#include "scan_dev.h"

namespace clapgpu {

constexpr int PB = 256;
constexpr uint32_t BPL_STATUS_SCAN = 4u;  // CTRL_STATUS: a look-back word never arrived (broadphase.hip's BP_STATUS_SCAN)

// Launch 1: k_bp_bin with the level in the key
__global__ __launch_bounds__(PB)
void k_bpl_bin(BplK q)
{
    const BpK &k = q.k;
    const uint32_t i = blockIdx.x * PB + threadIdx.x;
    if (i == 0) k.ctrl[CTRL_EPOCH] = k.ctrl[CTRL_EPOCH] + 1;
    if (i >= k.n) return;
    double bb[6], c;
    load_box(k.aabb, i, bb);
    bool over;
    const uint32_t l = box_level(bb, k.cell, q.levels, &c, &over);
    if (over) atomicOr(&k.ctrl[CTRL_STATUS], 1u);                        // binned on the top level: pairs may be missing
    int32_t cx, cy, cz;
    box_cell(bb, c, cx, cy, cz);
    const uint32_t slot = level_slot(l, cx, cy, cz, k.mask);
    k.key[i] = slot | l << BPL_LEVEL_SHIFT;                              // slots end below 2^28 (bp_create.hip's buckets_for)
    k.rank[i] = atomicAdd(&k.cell_cnt[slot], 1u);
}

// Launch 3: k_bp_scatter; the record's cell is the centre's cell on the body's own level, its index carries the level
__global__ __launch_bounds__(PB)
void k_bpl_scatter(BplK q)
{
    const BpK &k = q.k;
    const uint32_t i = blockIdx.x * PB + threadIdx.x;
    if (i >= k.n) return;
    const uint32_t key = k.key[i], l = key >> BPL_LEVEL_SHIFT;
    const uint32_t at = k.cell_range[key & BPL_IDX].x + k.rank[i];
    k.entries[at] = i;
    double bb[6], c = k.cell;
    load_box(k.aabb, i, bb);
    for (uint32_t x = 0; x < l; x++) c *= 2.0;
    int32_t cx, cy, cz;
    box_cell(bb, c, cx, cy, cz);
    double2 *o = reinterpret_cast<double2 *>(k.recs + at);
    o[0] = make_double2(bb[0], bb[1]); o[1] = make_double2(bb[2], bb[3]); o[2] = make_double2(bb[4], bb[5]);
    reinterpret_cast<int4 *>(o)[3] = make_int4((int)(i | l << BPL_LEVEL_SHIFT), cx, cy, cz);
}

// Launch 4: one lane per body in cell order (neighbouring lanes walk the same cells).  Same level: own cell (larger
// index) + the 13 cells after it; every coarser level: the cells of the grown box (bp_levels.h); its own level's
// statics.  Every record is checked against the (level, cell) looked up.  Body hits go to the partner list of min(i, j)
// as in k_bp_search; only this lane writes its body's static list.
__global__ __launch_bounds__(PB)
void k_bpl_search(BplK q)
{
    const BpK &k = q.k;
    const uint32_t t = blockIdx.x * PB + threadIdx.x;
    if (t >= k.n) return;
    const GridRec me = k.recs[t];
    const uint32_t i = me.idx & BPL_IDX, l = me.idx >> BPL_LEVEL_SHIFT;

    auto visit = [&](uint32_t L, int32_t x, int32_t y, int32_t z, bool own) {
        const uint2 cr = k.cell_range[level_slot(L, x, y, z, k.mask)];
        for (uint32_t s = cr.x; s < cr.x + cr.y; s++) {
            const GridRec r = k.recs[s];
            if (r.idx >> BPL_LEVEL_SHIFT != L || r.cell[0] != x || r.cell[1] != y || r.cell[2] != z) continue;   // shares the slot only
            const uint32_t j = r.idx & BPL_IDX;
            if ((own && j <= i) || !boxes_overlap(me.bb, r.bb)) continue;
            const uint32_t lo = i < j ? i : j, hi = i < j ? j : i;
            const uint32_t at = atomicAdd(&k.cnt[lo], 1u);
            if (at < BP_LIST) k.partners[(size_t)lo * BP_LIST + at] = hi;
        }
    };
    for (int cq = 13; cq < 27; cq++)                                     // 13 = own cell, 14..26 = the cells after it
        visit(l, me.cell[0] - 1 + cq % 3, me.cell[1] - 1 + (cq / 3) % 3, me.cell[2] - 1 + cq / 9, cq == 13);
    double c = k.cell;
    for (uint32_t x = 0; x < l; x++) c *= 2.0;
    for (uint32_t L = l + 1; L < q.levels; L++) {
        c *= 2.0;
        int32_t lo[3], hi[3];
        for (int a = 0; a < 3; a++) coarse_cells(me.bb[2 * a], me.bb[2 * a + 1], c, &lo[a], &hi[a]);
        for (int32_t z = lo[2]; z <= hi[2]; z++)
            for (int32_t y = lo[1]; y <= hi[1]; y++)
                for (int32_t x = lo[0]; x <= hi[0]; x++) visit(L, x, y, z, false);
    }
    if (!k.n_static) return;
    uint32_t sc = 0;
    auto stat = [&](const GridRec &r) {
        if (!boxes_overlap(me.bb, r.bb)) return;
        if (sc < BP_LIST) k.spartners[(size_t)i * BP_LIST + sc] = r.idx;
        sc++;
    };
    const uint32_t *ss = k.s_start + (size_t)l * (k.mask + 2u) + block_hash(me.cell[0] >> 2, me.cell[1] >> 2, me.cell[2] >> 2, k.mask);
    for (uint32_t s = ss[0]; s < ss[1]; s++) stat(k.s_recs[s]);
    for (uint32_t s = q.large_start[l]; s < q.large_start[l + 1]; s++) stat(k.s_lrecs[s]);
    k.scnt[i] = sc;
}

// Launch 5: k_bp_emit's offsets and its ranked write of a list that fit its slot.  A list that did not fit is searched
// again, and k_bp_emit's walk of 27 cells does not reach a leveled body's partners: they sit on its own level, on the
// coarser ones and -- all of a large body's small partners, when its index is the smaller -- on the finer ones, where
// its grown box covers (edge / cell_f + 2)^3 cells.  The bound on that count is zero: the wavefront of the body scans
// every box of larger index in index order, 64 a round, and a ballot ranks the hits -- exact and ascending whatever
// the levels, n / 64 rounds a body.  Its statics likewise, over all of them.
__global__ __launch_bounds__(BP_EMIT_TILE)
void k_bpl_emit(BpK k)
{
    __shared__ uint32_t lds[2][BP_EMIT_TILE / WAVE];
    __shared__ uint32_t tile_excl[2];
    const uint32_t i = blockIdx.x * BP_EMIT_TILE + threadIdx.x;
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const bool with_statics = k.n_static != 0, live = i < k.n;
    uint32_t c[2] = { 0, 0 };
    if (live) {
        c[0] = k.cnt[i];
        k.cnt[i] = 0;                                                    // ready for the next frame's atomics
        if (with_statics) { c[1] = k.scnt[i]; k.scnt[i] = 0; }
    }
    uint32_t incl[2] = { c[0], c[1] };
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint32_t u0 = __shfl_up(incl[0], o), u1 = __shfl_up(incl[1], o);
        if (lane >= o) { incl[0] += u0; incl[1] += u1; }
    }
    if (lane == WAVE - 1) { lds[0][wave] = incl[0]; lds[1][wave] = incl[1]; }
    __syncthreads();
    if (wave < 2) {                                                      // wavefront 0: the body list's offsets; wavefront 1: the statics'
        uint32_t sum = 0;
        for (int qq = 0; qq < BP_EMIT_TILE / WAVE; qq++) sum += lds[wave][qq];
        uint32_t excl = 0;
        if (wave == 0 || with_statics)
            excl = lb_exclusive(wave ? k.lb_static : k.lb_body, blockIdx.x, sum, k.ctrl[CTRL_EPOCH], k.ctrl + CTRL_STATUS, BPL_STATUS_SCAN);
        if (lane == 0) {
            tile_excl[wave] = excl;
            if (blockIdx.x == gridDim.x - 1) {                           // the last tile's inclusive prefix is the total
                uint32_t *tot = wave ? k.spair_total : k.pair_total;
                if (tot) *tot = (wave == 0 || with_statics) ? excl + sum : 0u;
            }
        }
    }
    __syncthreads();
    uint32_t off[2] = { tile_excl[0] + incl[0] - c[0], tile_excl[1] + incl[1] - c[1] };
    for (int qq = 0; qq < wave; qq++) { off[0] += lds[0][qq]; off[1] += lds[1][qq]; }
    // a list of n <= BP_LIST entries, out in ascending order: the rank of an entry = the entries below it
    auto ranked = [&](const uint32_t *list, uint32_t n, uint32_t at, uint2 *out, uint32_t cap) __attribute__((always_inline)) {
        uint32_t v[BP_LIST];
        const uint4 *src = reinterpret_cast<const uint4 *>(list);
#pragma unroll
        for (int q4 = 0; q4 < BP_LIST / 4; q4++) {
            uint4 x = make_uint4(0, 0, 0, 0);
            if ((uint32_t)(4 * q4) < n) x = src[q4];
            v[4 * q4] = x.x; v[4 * q4 + 1] = x.y; v[4 * q4 + 2] = x.z; v[4 * q4 + 3] = x.w;
        }
#pragma unroll
        for (int e = 0; e < BP_LIST; e++) {
            if ((uint32_t)e < n) {
                uint32_t rank = 0;
#pragma unroll
                for (int f = 0; f < BP_LIST; f++) rank += ((uint32_t)f < n) & (v[f] < v[e]);
                if (at + rank < cap) out[at + rank] = make_uint2(i, v[e]);
            }
        }
    };
    // the wavefront's bodies whose list overflowed, one after the other: every box after `first`, 64 a round
    // (a list ends where its count ends: a body above the top level may have been counted short -- status bit 0)
    auto scan_all = [&](uint32_t count, uint32_t at, const double *boxes, uint32_t n_boxes, bool after_self, uint2 *out,
                        uint32_t cap) __attribute__((always_inline)) {
        unsigned long long todo = __ballot(count > (uint32_t)BP_LIST);
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint32_t bi = __shfl(i, src);
            uint32_t w = __shfl(at, src);
            const uint32_t end = w + __shfl(count, src) < cap ? w + __shfl(count, src) : cap;
            double a[6];
            load_box(k.aabb, bi, a);
            for (uint32_t base = after_self ? bi + 1 : 0; base < n_boxes && w < end; base += WAVE) {
                const uint32_t j = base + lane;
                bool hit = false;
                if (j < n_boxes) {
                    double b[6];
                    load_box(boxes, j, b);
                    hit = boxes_overlap(a, b);
                }
                const unsigned long long m = __ballot(hit);
                const uint32_t pos = w + __popcll(m & ((1ull << lane) - 1ull));
                if (hit && pos < end) out[pos] = make_uint2(bi, j);
                w += __popcll(m);
            }
        }
    };
    uint2 *out = reinterpret_cast<uint2 *>(k.pairs), *sout = reinterpret_cast<uint2 *>(k.spairs);
    if (c[0] && c[0] <= (uint32_t)BP_LIST) ranked(k.partners + (size_t)BP_LIST * i, c[0], off[0], out, k.capacity);
    if (c[1] && c[1] <= (uint32_t)BP_LIST) ranked(k.spartners + (size_t)BP_LIST * i, c[1], off[1], sout, k.scapacity);
    scan_all(c[0], off[0], k.aabb, k.n, true, out, k.capacity);
    if (with_statics) scan_all(c[1], off[1], k.s_aabb, k.n_static, false, sout, k.scapacity);
}

} // namespace clapgpu

using namespace clapgpu;

__attribute__((visibility("hidden"))) int clapgpu_bpl_bin(hipStream_t s, const BplK &q)
{
    hipLaunchKernelGGL(k_bpl_bin, dim3((q.k.n + PB - 1) / PB), dim3(PB), 0, s, q);
    CLAPGPU_LAUNCH_CHECK("k_bpl_bin");
    return CLAPGPU_OK;
}

__attribute__((visibility("hidden"))) int clapgpu_bpl_scatter(hipStream_t s, const BplK &q)
{
    hipLaunchKernelGGL(k_bpl_scatter, dim3((q.k.n + PB - 1) / PB), dim3(PB), 0, s, q);
    CLAPGPU_LAUNCH_CHECK("k_bpl_scatter");
    return CLAPGPU_OK;
}

__attribute__((visibility("hidden"))) int clapgpu_bpl_pairs(hipStream_t s, const BplK &q)
{
    const dim3 grid((q.k.n + PB - 1) / PB);
    const int rc = clapgpu_bpl_scatter(s, q);
    if (rc) return rc;
    hipLaunchKernelGGL(k_bpl_search, grid, dim3(PB), 0, s, q);
    CLAPGPU_LAUNCH_CHECK("k_bpl_search");
    hipLaunchKernelGGL(k_bpl_emit, dim3(q.k.n_tiles), dim3(BP_EMIT_TILE), 0, s, q.k);
    CLAPGPU_LAUNCH_CHECK("k_bpl_emit");
    return CLAPGPU_OK;
}
