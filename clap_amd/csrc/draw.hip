// draw.hip -- clapgpu_draw_records (include/clapgpu.h, "Draw records on the device"): one render pass's draws in the
// order _models_render (core/model.c:784, :959) issues them, one 192-byte record per draw, and every txmodel's range.
// An ordered compaction in RENDER-ORDER space plus a row gather, in three launches:
//   k_draw_masks   a lane per render position: order[r] read coalesced, the entity's bit gathered from the plane (n / 8
//                  bytes, cache-resident), the skip-shadow groups cleared; two ballots per 64 positions -- "drawn" and
//                  "drawn and counted as a character" -- each with its popcount byte, as the cull leaves vis_row_pop.
//                  What the host cannot see (order[r] >= n, a group_start that does not ascend) is found here.
//   k_draw_prefix  one workgroup: the verdict, one exclusive scan of the row counts, and per group the records and the
//                  drawn characters in front of it (group_first, and the base of the edge mode's ordinal).
//   k_draw_fill    on the plan of k_visible_expand_rp, a wavefront per word of render space (DRAW_ROWS): the drawn
//                  lanes resolve entity, group and ordinal and leave the record's scalar tail in wave-private LDS at
//                  their rank, then the wave moves the word's records as 16-byte pieces, twelve lanes a record, so every
//                  store instruction writes whole consecutive 64-byte lines.
// No atomics anywhere: the order is the result.  The decisions are draw_dev.h's, shared with the host twin.
#include <string.h>
#include "common.h"
#include "draw_dev.h"
#include "entities_args.h"

namespace clapgpu {

constexpr int DRAW_BLOCK = 256;                     // four wavefronts
constexpr int DRAW_WAVES = DRAW_BLOCK / WAVE;
// words of render space per wavefront of the fill.  16, the plan of k_visible_expand_rp, was built and measured first: a
// word's chain -- order, the group search, the inputs, LDS, the rows, the stores -- is a dozen dependent memory round trips,
// and sixteen of them one after the other per wavefront made the call 343 us at a million draws and 95 us in the 10 k
// testbed frame (profiles/draw_records/README.md).  The bases come from k_draw_prefix's scan, not from a byte sum that
// wants 16-byte alignment, so nothing ties a wavefront to more than one word.
constexpr int DRAW_ROWS = 1;
constexpr int DRAW_PREFIX_BLOCK = 1024;
constexpr int DRAW_PIECES = CLAPGPU_DRAW_RECORD_BYTES / 16;

struct DrawK {
    uint32_t n, n_order, n_groups, n_words, n_mask_blocks, capacity;
    const uint32_t *order, *group_start, *group_flags;
    const uint64_t *plane;                          // NULL: the pass without a view
    const uint32_t *flags;
    const int32_t *lod;
    const uint4 *mx, *inv_mx;
    clapgpu_draw_inputs in;
    clapgpu_draw_pass pass;
    uint4 *records;
    uint32_t *count, *group_first, *status;
    // scratch
    uint64_t *drawn, *chr;                          // [n_words] render-space masks
    uint8_t *pop_d, *pop_c;                         // [n_words] their popcounts
    uint32_t *pre_d, *pre_c;                        // [n_words] exclusive prefixes of the popcounts
    uint32_t *group_chr;                            // [n_groups + 1] drawn characters in front of group g
    uint32_t *block_bad;                            // [n_mask_blocks] k_draw_masks' verdict per workgroup
    uint32_t *invalid;                              // one word: k_draw_prefix's verdict, read by the fill
};

// the groups of a word's first and last position: one search each per wavefront; a lane searches between them only when
// the word straddles groups
struct WordGroups { uint32_t g0, g1; };
__device__ __forceinline__ WordGroups word_groups(const DrawK &a, uint32_t w)
{
    const uint32_t r0 = w * 64u, last = a.n_order - 1u;
    const uint32_t r1 = last - r0 < 63u ? last : r0 + 63u;
    WordGroups wg;
    wg.g0 = draw_group_of(a.group_start, 0, a.n_groups - 1u, r0);
    wg.g1 = wg.g0;                                  // rows rarely straddle groups: one load says so
    if (wg.g0 + 1u < a.n_groups && a.group_start[wg.g0 + 1u] <= r1)
        wg.g1 = draw_group_of(a.group_start, wg.g0 + 1u, a.n_groups - 1u, r1);
    return wg;
}

__global__ __launch_bounds__(DRAW_BLOCK)
void k_draw_masks(DrawK a)
{
    const int lane = lane_id();
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * DRAW_WAVES + threadIdx.x / WAVE);
    bool bad = false;
    const uint32_t tid = blockIdx.x * DRAW_BLOCK + threadIdx.x, threads = gridDim.x * DRAW_BLOCK;
    for (uint32_t g = tid; g < a.n_groups; g += threads)
        if (a.group_start[g] > a.group_start[g + 1]) bad = true;
    if (tid == 0 && (a.group_start[0] != 0u || a.group_start[a.n_groups] != a.n_order)) bad = true;

    if (w < a.n_words) {
        const WordGroups wg = word_groups(a, w);
        const uint32_t r = w * 64u + lane;
        bool drawn = false, chr = false;
        if (r < a.n_order) {
            const uint32_t i = a.order[r];
            if (i >= a.n) {
                bad = true;
            } else {
                const uint32_t g = wg.g0 == wg.g1 ? wg.g0 : draw_group_of(a.group_start, wg.g0, wg.g1, r);
                if (!draw_group_skipped(a.group_flags[g], a.pass.flags) && draw_entity_drawn(a.plane, a.flags, i)) {
                    drawn = true;
                    chr = draw_counts_character(a.in.draw_flags ? a.in.draw_flags[i] : 0u, a.pass.mq_nr_characters);
                }
            }
        }
        const uint64_t md = __ballot(drawn), mc = __ballot(chr);
        if (lane == 0) {
            a.drawn[w] = md; a.chr[w] = mc;
            a.pop_d[w] = (uint8_t)__popcll(md); a.pop_c[w] = (uint8_t)__popcll(mc);
        }
    }
    const int any_bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) a.block_bad[blockIdx.x] = any_bad ? 1u : 0u;
}

// the workgroup's inclusive prefix of v, and its total; scratch: one word per wavefront.  Every lane calls it.
__device__ __forceinline__ uint32_t block_prefix_sum(uint32_t v, uint32_t *wave_tot, uint32_t *total)
{
    const int lane = lane_id(), wv = threadIdx.x / WAVE;
    const uint32_t incl = wave_prefix_sum(v);        // (the callers' two arrays alternate: the other's barrier stands
    if (lane == WAVE - 1) wave_tot[wv] = incl;       //  between a trip's readers and the next trip's writers)
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < DRAW_PREFIX_BLOCK / WAVE; k++) {
        const uint32_t t = wave_tot[k];
        if (k < wv) before += t;
        all += t;
    }
    *total = all;
    return incl + before;
}

__global__ __launch_bounds__(DRAW_PREFIX_BLOCK)
void k_draw_prefix(DrawK a)
{
    __shared__ uint32_t tot_d[DRAW_PREFIX_BLOCK / WAVE], tot_c[DRAW_PREFIX_BLOCK / WAVE];
    const uint32_t t = threadIdx.x;
    bool bad = false;
    for (uint32_t b = t; b < a.n_mask_blocks; b += DRAW_PREFIX_BLOCK)
        if (a.block_bad[b]) bad = true;
    if (__syncthreads_or(bad)) {                     // nothing else is written
        for (uint32_t g = t; g <= a.n_groups; g += DRAW_PREFIX_BLOCK) a.group_first[g] = 0u;
        if (t == 0) { *a.count = 0u; *a.status = CLAPGPU_DRAW_INVALID; *a.invalid = 1u; }
        return;
    }
    uint32_t carry_d = 0, carry_c = 0;
    for (uint32_t w0 = 0; w0 < a.n_words; w0 += DRAW_PREFIX_BLOCK) {
        const uint32_t w = w0 + t;
        const uint32_t d = w < a.n_words ? a.pop_d[w] : 0u, c = w < a.n_words ? a.pop_c[w] : 0u;
        uint32_t all_d, all_c;
        const uint32_t incl_d = block_prefix_sum(d, tot_d, &all_d);
        const uint32_t incl_c = block_prefix_sum(c, tot_c, &all_c);
        if (w < a.n_words) { a.pre_d[w] = carry_d + incl_d - d; a.pre_c[w] = carry_c + incl_c - c; }
        carry_d += all_d; carry_c += all_c;
    }
    __syncthreads();                                 // pre_d / pre_c of every word, to every lane
    for (uint32_t g = t; g <= a.n_groups; g += DRAW_PREFIX_BLOCK) {
        const uint32_t r = a.group_start[g], w = r >> 6;
        uint32_t d = carry_d, c = carry_c;           // r == n_order on a word boundary: the totals
        if (w < a.n_words) {
            const uint64_t below = (1ull << (r & 63u)) - 1ull;
            d = a.pre_d[w] + __popcll(a.drawn[w] & below);
            c = a.pre_c[w] + __popcll(a.chr[w] & below);
        }
        a.group_first[g] = d;
        a.group_chr[g] = c;
    }
    if (t == 0) { *a.count = carry_d; *a.status = carry_d > a.capacity ? CLAPGPU_DRAW_CAPPED : 0u; *a.invalid = 0u; }
}

__global__ __launch_bounds__(DRAW_BLOCK)
void k_draw_fill(DrawK a)
{
    __shared__ uint32_t s_entity[DRAW_WAVES][WAVE];
    __shared__ uint4 s_tail[DRAW_WAVES][WAVE * 3];
    const int lane = lane_id(), wv = threadIdx.x / WAVE;
    const uint32_t row0 = __builtin_amdgcn_readfirstlane((blockIdx.x * DRAW_WAVES + wv) * DRAW_ROWS);
    if (row0 >= a.n_words || *a.invalid) return;

    const bool mine = lane < DRAW_ROWS && row0 + lane < a.n_words;      // lane k holds word row0 + k
    const uint64_t my_d = mine ? a.drawn[row0 + lane] : 0ull, my_c = mine ? a.chr[row0 + lane] : 0ull;
    const uint32_t my_pd = mine ? a.pre_d[row0 + lane] : 0u, my_pc = mine ? a.pre_c[row0 + lane] : 0u;
    uint32_t *ent = s_entity[wv];
    uint4 *tail = s_tail[wv];

    for (int k = 0; k < DRAW_ROWS; k++) {
        const uint64_t md = __shfl(my_d, k);
        if (md == 0) continue;                       // the same in every lane
        const uint64_t mc = __shfl(my_c, k);
        const uint32_t base = __shfl(my_pd, k), cbase = __shfl(my_pc, k);
        const uint32_t w = row0 + k;
        if ((md >> lane) & 1ull) {
            const WordGroups wg = word_groups(a, w);
            const uint32_t r = w * 64u + lane;
            const uint32_t rank = __popcll(md & ((1ull << lane) - 1ull));
            const uint32_t i = a.order[r];
            const uint32_t g = wg.g0 == wg.g1 ? wg.g0 : draw_group_of(a.group_start, wg.g0, wg.g1, r);
            // drawn characters of the group up to and including this draw (model.c:1013: the increment comes first)
            const uint32_t ordinal = cbase + __popcll(mc & ((2ull << lane) - 1ull)) - a.group_chr[g];
            const DrawTail t = draw_tail(a.in, a.pass, a.lod, i, g, ordinal);
            ent[rank] = i;
            tail[rank * 3 + 0] = make_uint4(t.w[0], t.w[1], t.w[2], t.w[3]);
            tail[rank * 3 + 1] = make_uint4(t.w[4], t.w[5], t.w[6], t.w[7]);
            tail[rank * 3 + 2] = make_uint4(t.w[8], t.w[9], t.w[10], t.w[11]);
        }
        wave_lds_fence();
        const uint32_t pieces = __popcll(md) * DRAW_PIECES;
        for (uint32_t c = lane; c < pieces; c += WAVE) {
            const uint32_t j = c / DRAW_PIECES, p = c - j * DRAW_PIECES;
            const uint32_t rec = base + j;
            if (rec >= a.capacity) continue;
            const size_t i = ent[j];
            uint4 v;
            if (p < 4) v = a.mx[i * 4 + p];
            else if (p < 8) v = a.inv_mx[i * 4 + (p - 4)];
            else if (p == 8) v = a.in.color ? reinterpret_cast<const uint4 *>(a.in.color)[i] : make_uint4(0, 0, 0, 0);
            else v = tail[j * 3 + (p - 9)];
            a.records[(size_t)rec * DRAW_PIECES + p] = v;
        }
        wave_lds_fence();                            // the next word writes the same LDS
    }
}

struct DrawScratch { size_t drawn, chr, pop_d, pop_c, pre_d, pre_c, group_chr, block_bad, invalid, bytes; };

static DrawScratch draw_scratch(uint32_t n_order, uint32_t n_groups)
{
    const size_t n_words = ((size_t)n_order + 63) / 64, n_blocks = (n_words + DRAW_WAVES - 1) / DRAW_WAVES;
    Carve c;
    DrawScratch s;
    s.drawn = c.take(n_words * 8); s.chr = c.take(n_words * 8);
    s.pop_d = c.take(n_words); s.pop_c = c.take(n_words);
    s.pre_d = c.take(n_words * 4); s.pre_c = c.take(n_words * 4);
    s.group_chr = c.take(((size_t)n_groups + 1) * 4);
    s.block_bad = c.take(n_blocks * 4);
    s.invalid = c.take(4);
    s.bytes = c.bytes();
    return s;
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" size_t clapgpu_draw_records_scratch_bytes(uint32_t n_order, uint32_t n_groups)
{
    return draw_scratch(n_order, n_groups).bytes;
}

extern "C" int clapgpu_draw_records(void *stream, const clapgpu_entities *e, const uint64_t *vis_mask, const int32_t *lod,
                                    const clapgpu_draw_order *o, const clapgpu_draw_inputs *inputs, const clapgpu_draw_pass *pass,
                                    clapgpu_draw_record *records, uint32_t capacity, uint32_t *count, uint32_t *group_first,
                                    uint32_t *status, void *scratch)
{
    int rc = draw_check(e, vis_mask, o, pass, records, capacity, count, group_first, status);
    if (rc) return rc;
    if (!scratch || (reinterpret_cast<uintptr_t>(scratch) & 255u) || !aligned16(e->mx) || !aligned16(e->inv_mx) ||
        (inputs && !aligned16(inputs->color)))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (o->n_order == 0 || e->n == 0) {              // nothing can be drawn: the outputs alone
        CLAPGPU_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), as_stream(stream)));
        CLAPGPU_HIP(hipMemsetAsync(status, 0, sizeof(uint32_t), as_stream(stream)));
        CLAPGPU_HIP(hipMemsetAsync(group_first, 0, ((size_t)o->n_groups + 1) * sizeof(uint32_t), as_stream(stream)));
        return CLAPGPU_OK;
    }
    const DrawScratch s = draw_scratch(o->n_order, o->n_groups);
    uint8_t *base = static_cast<uint8_t *>(scratch);
    DrawK a;
    memset(&a, 0, sizeof(a));
    a.n = e->n; a.n_order = o->n_order; a.n_groups = o->n_groups;
    a.n_words = (uint32_t)(((size_t)o->n_order + 63) / 64);
    a.n_mask_blocks = (a.n_words + DRAW_WAVES - 1) / DRAW_WAVES;
    a.capacity = capacity;
    a.order = o->order; a.group_start = o->group_start; a.group_flags = o->group_flags;
    a.plane = vis_mask; a.flags = e->flags; a.lod = lod;
    a.mx = reinterpret_cast<const uint4 *>(e->mx); a.inv_mx = reinterpret_cast<const uint4 *>(e->inv_mx);
    if (inputs) a.in = *inputs;
    a.pass = *pass;
    a.records = reinterpret_cast<uint4 *>(records);
    a.count = count; a.group_first = group_first; a.status = status;
    a.drawn = reinterpret_cast<uint64_t *>(base + s.drawn); a.chr = reinterpret_cast<uint64_t *>(base + s.chr);
    a.pop_d = base + s.pop_d; a.pop_c = base + s.pop_c;
    a.pre_d = reinterpret_cast<uint32_t *>(base + s.pre_d); a.pre_c = reinterpret_cast<uint32_t *>(base + s.pre_c);
    a.group_chr = reinterpret_cast<uint32_t *>(base + s.group_chr);
    a.block_bad = reinterpret_cast<uint32_t *>(base + s.block_bad);
    a.invalid = reinterpret_cast<uint32_t *>(base + s.invalid);
    hipLaunchKernelGGL(k_draw_masks, dim3(a.n_mask_blocks), dim3(DRAW_BLOCK), 0, as_stream(stream), a);
    CLAPGPU_LAUNCH_CHECK("k_draw_masks");
    hipLaunchKernelGGL(k_draw_prefix, dim3(1), dim3(DRAW_PREFIX_BLOCK), 0, as_stream(stream), a);
    CLAPGPU_LAUNCH_CHECK("k_draw_prefix");
    const uint32_t fill_waves = (a.n_words + DRAW_ROWS - 1) / DRAW_ROWS;
    hipLaunchKernelGGL(k_draw_fill, dim3((fill_waves + DRAW_WAVES - 1) / DRAW_WAVES), dim3(DRAW_BLOCK), 0, as_stream(stream), a);
    CLAPGPU_LAUNCH_CHECK("k_draw_fill");
    return CLAPGPU_OK;
}
