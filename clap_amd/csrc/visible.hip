// visible.hip -- render-pass glue over what the entity update left: the cull-only pass over stored boxes, the ordered
// compaction of the visibility mask into a list of ids, and the per-pass LOD pick of the entities on that list.
// Reads boxes and masks only; nothing here rebuilds a row.
#include <string.h>
#include <math.h>
#include "common.h"
#include "lm_dev.h"
#include "entities_row.h"
#include "entities_args.h"

namespace clapgpu {

// Cull-only pass over stored AABBs (one per render pass in the reference).
// XV: nothing, or the frame's further views (a trailing XViewsK): every view of the frame from one read of the boxes.
// With a trailing XViewsDevK (clapgpu_entities_cull_views) every frustum lies in the view block: the main view's is slot
// 0's and the argument `fr` is not read.  One body for the three, in the kernel itself: moved into a function the kernels
// share, the two instantiations the parent had came out with other instruction streams (tools/isa_hashes.sh).
__device__ __forceinline__ const lmd::FrustumK &main_frustum(const lmd::FrustumK &fr) { return fr; }
__device__ __forceinline__ const lmd::FrustumK &main_frustum(const lmd::FrustumK &fr, const XViewsK &) { return fr; }
__device__ __forceinline__ const lmd::FrustumK &main_frustum(const lmd::FrustumK &, const XViewsDevK &xv) { return view_frustum_k(xv.st, 0); }

template <class... XV>
__global__ __launch_bounds__(ENT_BLOCK)
void k_entities_cull(const uint32_t *flags, const float *aabb, uint64_t *vis_mask, uint8_t *vis_row_pop,
                     uint32_t n, lmd::FrustumK fr, XV... xv)
{
    const uint32_t i = blockIdx.x * ENT_BLOCK + threadIdx.x;
    const int lane = lane_id();
    bool base = false, vis = false;
    uint32_t fl = 0;
    float bb[6] = { 0, 0, 0, 0, 0, 0 };
    if (i < n) {
        fl = flags[i];
        base = (fl & CLAPGPU_E_ALIVE) && (fl & CLAPGPU_E_VISIBLE);
        vis = base;
        if (base && !(fl & CLAPGPU_E_SKIP_CULLING)) {
#pragma unroll
            for (int k = 0; k < 6; k++) bb[k] = aabb[6 * (size_t)i + k];
            vis = lmd::aabb_in_frustum_fast(main_frustum(fr, xv...), bb);
        }
    }
    // a wavefront past the end: with further views it leaves here, ahead of their ballots and mask words; without, the
    // test at the store is all it needs (and leaving here as well cost that kernel three instructions)
    if constexpr (sizeof...(XV) != 0)
        if ((i - lane) >= n) return;
    const uint64_t m = __ballot(vis);
    if (lane == 0 && (i - lane) < n) {
        vis_mask[i >> 6] = m;
        vis_row_pop[i >> 6] = (uint8_t)__popcll(m);
    }
    if constexpr (sizeof...(XV) != 0) cull_extra_views(xv..., base, fl, bb, i >> 6, lane);
}

// ---- ordered compaction of the visibility bitmask ----
// A group = 64 mask words = 4096 entities = one wave.
constexpr int GROUP_WORDS = 64;

__device__ __forceinline__ uint64_t load_mask_word(const uint64_t *vis_mask, uint32_t w, uint32_t n)
{
    const uint32_t nwords = (n + 63) / 64;
    if (w >= nwords)
        return 0;
    uint64_t v = vis_mask[w];
    const uint32_t rem = n - w * 64;                 // entities covered by this word
    if (rem < 64)
        v &= (1ull << rem) - 1ull;                   // bits past n are padding
    return v;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(WAVE)
void k_mask_group_count(const uint64_t *vis_mask, uint32_t n, uint32_t *group_count)
{
    const uint32_t w = blockIdx.x * GROUP_WORDS + threadIdx.x;
    const uint32_t c = wave_sum(__popcll(load_mask_word(vis_mask, w, n)));
    if (threadIdx.x == 0)
        group_count[blockIdx.x] = c;
}

__global__ __launch_bounds__(WAVE)
void k_visible_expand(const uint64_t *vis_mask, uint32_t n, const uint32_t *group_count,
                      uint32_t n_groups, uint32_t index_base, uint32_t *visible, uint32_t *count)
{
    const int lane = threadIdx.x;
    const uint32_t g = blockIdx.x;

    uint32_t pre = 0;                                 // visible entities in groups before g
    for (uint32_t j = lane; j < g; j += WAVE)
        pre += group_count[j];
    pre = wave_sum(pre);

    const uint64_t word = load_mask_word(vis_mask, g * GROUP_WORDS + lane, n);
    const uint32_t cnt = __popcll(word);
    uint32_t incl = cnt;                              // inclusive scan of per-word counts over lanes
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        uint32_t t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    const uint32_t excl = incl - cnt;

    // one mask word per iteration: lane l owns bit l, ranks come from the bits below it,
    // so the 4-byte stores of an iteration are contiguous and ascending.
    for (int k = 0; k < GROUP_WORDS; k++) {
        const uint64_t wk = __shfl(word, k);
        if (wk == 0) continue;                        // wave-uniform
        const uint32_t base = pre + __shfl(excl, k);
        if ((wk >> lane) & 1ull) {
            const uint32_t rank = __popcll(wk & ((1ull << lane) - 1ull));
            visible[base + rank] = index_base + (g * GROUP_WORDS + k) * 64u + lane;
        }
    }
    if (g == n_groups - 1 && lane == WAVE - 1)
        *count = pre + incl;
}

// ---- the same over a GATHERED mask: one segment of cap_words words per rank, rank r's slot i has global id base[r] + i ----
// (clapgpu_visible_compact_ranges: shards cut from one scene by clapgpu_shard_tile_range are uneven; every rank sends a
// mask of the common capacity, only its first n_words[r] words count)
constexpr int MAX_SEGMENTS = 64;
struct SegK { uint32_t cap_words, n_seg; uint32_t base[MAX_SEGMENTS], n_words[MAX_SEGMENTS]; };

__device__ __forceinline__ uint64_t load_seg_word(const uint64_t *mask, const SegK &sg, uint32_t w, uint32_t *id_base)
{
    const uint32_t r = w / sg.cap_words, lw = w - r * sg.cap_words;
    if (r >= sg.n_seg || lw >= sg.n_words[r]) { *id_base = 0; return 0ull; }
    *id_base = sg.base[r] + lw * 64u;
    return mask[w];
}

__global__ __launch_bounds__(WAVE)
void k_mask_group_count_seg(const uint64_t *mask, SegK sg, uint32_t *group_count)
{
    uint32_t idb;
    const uint32_t c = wave_sum(__popcll(load_seg_word(mask, sg, blockIdx.x * GROUP_WORDS + threadIdx.x, &idb)));
    if (threadIdx.x == 0)
        group_count[blockIdx.x] = c;
}

__global__ __launch_bounds__(WAVE)
void k_visible_expand_seg(const uint64_t *mask, SegK sg, const uint32_t *group_count, uint32_t n_groups, uint32_t *visible,
                          uint32_t *count)
{
    const int lane = threadIdx.x;
    const uint32_t g = blockIdx.x;
    uint32_t pre = 0;
    for (uint32_t j = lane; j < g; j += WAVE)
        pre += group_count[j];
    pre = wave_sum(pre);
    uint32_t idb;
    const uint64_t word = load_seg_word(mask, sg, g * GROUP_WORDS + lane, &idb);
    const uint32_t cnt = __popcll(word);
    uint32_t incl = cnt;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        uint32_t t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    const uint32_t excl = incl - cnt;
    for (int k = 0; k < GROUP_WORDS; k++) {
        const uint64_t wk = __shfl(word, k);
        if (wk == 0) continue;                        // wave-uniform
        const uint32_t base = pre + __shfl(excl, k), ids = __shfl(idb, k);
        if ((wk >> lane) & 1ull) {
            const uint32_t rank = __popcll(wk & ((1ull << lane) - 1ull));
            visible[base + rank] = ids + lane;
        }
    }
    if (g == n_groups - 1 && lane == WAVE - 1)
        *count = pre + incl;
}

// Single-launch compaction for up to RP_MAX_ROWS rows: the update / cull kernels leave one
// popcount byte per 64-entity row, so a wave gets the number of visible entities before its
// first row from at most RP_MAX_ROWS / 1024 16-byte loads per lane -- no separate count pass.
constexpr int RP_ROWS = 16;                 // rows (mask words) per wave; 16 keeps the byte prefix 16-B aligned
constexpr uint32_t RP_MAX_ROWS = 1u << 16;  // 4M entities; beyond that the two-pass path scales better

__device__ __forceinline__ uint32_t sum_bytes(uint32_t v, uint32_t acc)
{
    return __builtin_amdgcn_sad_u8(v, 0u, acc);      // v_sad_u8: acc + sum of the 4 bytes
}

__global__ __launch_bounds__(ENT_BLOCK)
void k_visible_expand_rp(const uint64_t *vis_mask, const uint8_t *row_pop, uint32_t n,
                         uint32_t index_base, uint32_t *visible, uint32_t *count)
{
    const int lane = lane_id();
    const uint32_t g = blockIdx.x * (ENT_BLOCK / WAVE) + threadIdx.x / WAVE;
    const uint32_t n_rows = (n + 63) / 64;
    const uint32_t row0 = g * RP_ROWS;
    if (row0 >= n_rows)
        return;

    // visible entities in rows [0, row0); row0 % 16 == 0
    const uint32_t pre = wave_byte_sum(row_pop, row0, lane);

    const uint64_t word = lane < RP_ROWS ? load_mask_word(vis_mask, row0 + lane, n) : 0ull;
    const uint32_t cnt = __popcll(word);
    uint32_t incl = cnt;
#pragma unroll
    for (int off = 1; off < RP_ROWS; off <<= 1) {
        uint32_t t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    const uint32_t excl = incl - cnt;
    const uint32_t lo = (uint32_t)word, hi = (uint32_t)(word >> 32);

#pragma unroll
    for (int k = 0; k < RP_ROWS; k++) {
        // readlane returns int: go through uint32_t or bit 31 sign-extends into the high half
        const uint64_t wk = (uint64_t)(uint32_t)__builtin_amdgcn_readlane(lo, k) |
                            ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(hi, k) << 32);
        if (wk == 0) continue;                        // scalar branch
        const uint32_t base = pre + (uint32_t)__builtin_amdgcn_readlane(excl, k);
        if ((wk >> lane) & 1ull) {
            const uint32_t rank = __popcll(wk & ((1ull << lane) - 1ull));
            visible[base + rank] = index_base + (row0 + k) * 64u + lane;
        }
    }
    if (row0 + RP_ROWS >= n_rows && lane == RP_ROWS - 1)
        *count = pre + incl;
}

// ---- per-pass LOD pick for the entities on the visible list (model.c:975-992) ----
struct LodK {                       // what the pick reads (model.c:975-992) and writes
    float cx, cy, cz;
    const float *aabb, *center;
    const float4 *pos_scale;
    const int32_t *model;
    const float4 *model_table;
    const int32_t *force_lod;
    int32_t *cur_lod;
    uint32_t n_models;
};

// the LOD entity i is drawn with; cur_lod[i] follows (entity3d_set_lod writes e->cur_lod)
__device__ __forceinline__ int32_t lod_pick(const LodK &k, uint32_t i)
{
    int32_t lod = k.cur_lod[i];
    const int32_t forced = k.force_lod ? k.force_lod[i] : -1;
    if (forced >= 0) {
        lod = forced;                                                   // model.c:976-977
    } else {
        const float *b = k.aabb + 6 * (size_t)i;
        const bool inside = k.cx >= b[0] && k.cx <= b[3] && k.cy >= b[1] && k.cy <= b[4] && k.cz >= b[2] && k.cz <= b[5];
        if (!inside) {                                                  // model.c:982-990
            const float *c = k.center + 3 * (size_t)i;
            const float dx = c[0] - k.cx, dy = c[1] - k.cy, dz = c[2] - k.cz;
            float dd = 0.f;
            dd += dx * dx;
            dd += dy * dy;
            dd += dz * dz;
            const int32_t mraw = k.model[i];
            const int32_t mi = (uint32_t)mraw < k.n_models ? mraw : 0;
            const float4 lo = k.model_table[2 * mi], hi = k.model_table[2 * mi + 1];
            const float s = k.pos_scale[i].w;
            const float X = fabsf(hi.x - lo.x) * s, Y = fabsf(hi.y - lo.y) * s, Z = fabsf(hi.z - lo.z) * s;
            const float side = lmd::cbrtf_glibc(X * Y * Z);                  // entity3d_aabb_avg_edge
            const float scale = (float)((double)fabsf(dd - side * side) / 3600.0);
            const uint32_t lm = __float_as_uint(hi.w);                  // lod_min | lod_max << 8
            const int lmin = (int)(lm & 0xffu), lmax = (int)((lm >> 8) & 0xffu);
            const int req = (int)scale;
            lod = req < lmin ? lmin : (req > lmax ? lmax : req);        // model3d_validate_lod
        }
    }
    k.cur_lod[i] = lod;
    return lod;
}

__device__ __forceinline__ void lod_pass(const uint32_t *visible, const uint32_t *count, const uint32_t index_base, const LodK &lk,
                                         int32_t *draw_lod, const uint32_t n)
{
    const uint32_t total = *count < n ? *count : n;                       // a count beyond the batch would walk off the list
    for (uint32_t k = blockIdx.x * ENT_BLOCK + threadIdx.x; k < total; k += gridDim.x * ENT_BLOCK) {
        const uint32_t i = visible[k] - index_base;
        if (i >= n) { draw_lod[k] = 0; continue; }                          // an id of another shard
        draw_lod[k] = lod_pick(lk, i);
    }
}

__global__ __launch_bounds__(ENT_BLOCK)
void k_entities_lod(const uint32_t *visible, const uint32_t *count, uint32_t index_base, LodK lk, int32_t *draw_lod, uint32_t n)
{
    lod_pass(visible, count, index_base, lk, draw_lod, n);
}

// clapgpu_entities_lod_views: the camera position is slot 0's of the view block
__global__ __launch_bounds__(ENT_BLOCK)
void k_entities_lod_views(const uint32_t *visible, const uint32_t *count, uint32_t index_base, LodK lk, int32_t *draw_lod, uint32_t n,
                          const clapgpu_views_state *st)
{
    lk.cx = st->slot[0].cam_pos[0]; lk.cy = st->slot[0].cam_pos[1]; lk.cz = st->slot[0].cam_pos[2];
    lod_pass(visible, count, index_base, lk, draw_lod, n);
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" int clapgpu_entities_cull(void *stream, const clapgpu_entities *e, const clapgpu_frustum *frustum)
{
    if (!e || !frustum || !e->flags || !e->aabb || !e->vis_mask || !e->vis_row_pop)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (e->n == 0)
        return CLAPGPU_OK;
    const lmd::FrustumK fr = make_frustum_k(frustum);
    XViewsK xv;
    if (!make_xviews_k(e, false, &xv)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    const dim3 grid((e->n + ENT_BLOCK - 1) / ENT_BLOCK), block(ENT_BLOCK);
    if (xv.n)
        hipLaunchKernelGGL(k_entities_cull<XViewsK>, grid, block, 0, as_stream(stream), e->flags, e->aabb, e->vis_mask,
                           e->vis_row_pop, e->n, fr, xv);
    else
        hipLaunchKernelGGL(k_entities_cull<>, grid, block, 0, as_stream(stream), e->flags, e->aabb, e->vis_mask,
                           e->vis_row_pop, e->n, fr);
    CLAPGPU_LAUNCH_CHECK("k_entities_cull");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_entities_cull_views(void *stream, const clapgpu_entities *e, const clapgpu_views_state *state)
{
    if (!view_block_ok(state) || !e || !e->flags || !e->aabb || !e->vis_mask || !e->vis_row_pop)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (e->n == 0)
        return CLAPGPU_OK;
    XViewsDevK xv;
    memset(&xv, 0, sizeof(xv));
    xv.st = state;
    if (const clapgpu_views *v = e->views) {                     // as make_xviews_k, without the frusta
        if (v->n > CLAPGPU_EXTRA_VIEWS_MAX) return CLAPGPU_ERR_INVALID_ARGUMENTS;
        xv.n = v->n;
        for (uint32_t k = 0; k < v->n; k++) {
            if (!v->vis_mask[k] || !v->vis_row_pop[k]) return CLAPGPU_ERR_INVALID_ARGUMENTS;
            xv.mask[k] = v->vis_mask[k]; xv.pop[k] = v->vis_row_pop[k];
        }
    }
    const lmd::FrustumK unread = {};                             // every frustum is read from the block
    hipLaunchKernelGGL(k_entities_cull<XViewsDevK>, dim3((e->n + ENT_BLOCK - 1) / ENT_BLOCK), dim3(ENT_BLOCK), 0, as_stream(stream),
                       e->flags, e->aabb, e->vis_mask, e->vis_row_pop, e->n, unread, xv);
    CLAPGPU_LAUNCH_CHECK("k_entities_cull<views>");
    return CLAPGPU_OK;
}

extern "C" size_t clapgpu_visible_scratch_bytes(uint32_t n)
{
    const uint32_t n_groups = (n + GROUP_WORDS * 64 - 1) / (GROUP_WORDS * 64);
    return (size_t)(n_groups ? n_groups : 1) * sizeof(uint32_t);
}

extern "C" int clapgpu_visible_compact(void *stream, const uint64_t *vis_mask, const uint8_t *vis_row_pop,
                                       uint32_t n, uint32_t index_base, uint32_t *visible, uint32_t *count,
                                       void *scratch)
{
    if (!count || (n && (!vis_mask || !visible)))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (n == 0) {
        CLAPGPU_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), as_stream(stream)));
        return CLAPGPU_OK;
    }
    const uint32_t n_rows = (n + 63) / 64;
    if (vis_row_pop && n_rows <= RP_MAX_ROWS && aligned16(vis_row_pop)) {
        const uint32_t waves = (n_rows + RP_ROWS - 1) / RP_ROWS, per_block = ENT_BLOCK / WAVE;
        hipLaunchKernelGGL(k_visible_expand_rp, dim3((waves + per_block - 1) / per_block), dim3(ENT_BLOCK), 0,
                           as_stream(stream), vis_mask, vis_row_pop, n, index_base, visible, count);
        CLAPGPU_LAUNCH_CHECK("k_visible_expand_rp");
        return CLAPGPU_OK;
    }
    if (!scratch)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    const uint32_t n_groups = (n + GROUP_WORDS * 64 - 1) / (GROUP_WORDS * 64);
    uint32_t *group_count = static_cast<uint32_t *>(scratch);
    hipLaunchKernelGGL(k_mask_group_count, dim3(n_groups), dim3(WAVE), 0, as_stream(stream), vis_mask, n, group_count);
    CLAPGPU_LAUNCH_CHECK("k_mask_group_count");
    hipLaunchKernelGGL(k_visible_expand, dim3(n_groups), dim3(WAVE), 0, as_stream(stream), vis_mask, n,
                       group_count, n_groups, index_base, visible, count);
    CLAPGPU_LAUNCH_CHECK("k_visible_expand");
    return CLAPGPU_OK;
}

static int check_ranges(uint32_t n_ranges, uint32_t cap_pad, const uint32_t *base, const uint32_t *n_pad)
{
    if (!n_ranges || n_ranges > (uint32_t)MAX_SEGMENTS || !cap_pad || (cap_pad & 63u) || !base) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    uint64_t end = 0;
    for (uint32_t r = 0; r < n_ranges; r++) {
        const uint32_t np = n_pad ? n_pad[r] : cap_pad;
        if ((np & 63u) || np > cap_pad || (base[r] & 63u) || base[r] < end) return CLAPGPU_ERR_INVALID_ARGUMENTS;   /* ascending, disjoint */
        end = (uint64_t)base[r] + np;
        if (end > 0x100000000ull) return CLAPGPU_ERR_TOO_LARGE;      /* end is one past the last id: 2^32 is the id 0xffffffff */
    }
    return CLAPGPU_OK;
}

extern "C" int clapgpu_visible_compact_ranges(void *stream, const uint64_t *gathered_mask, uint32_t n_ranges, uint32_t cap_pad,
                                              const uint32_t *base, const uint32_t *n_pad, uint32_t *visible, uint32_t *count,
                                              void *scratch)
{
    if (!gathered_mask || !visible || !count || !scratch) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    int rc = check_ranges(n_ranges, cap_pad, base, n_pad);
    if (rc) return rc;
    SegK sg = {};
    sg.cap_words = cap_pad / 64; sg.n_seg = n_ranges;
    for (uint32_t r = 0; r < n_ranges; r++) { sg.base[r] = base[r]; sg.n_words[r] = (n_pad ? n_pad[r] : cap_pad) / 64; }
    const uint64_t total_words = (uint64_t)sg.cap_words * n_ranges;
    if (total_words * 64 > 0xffffffffull) return CLAPGPU_ERR_TOO_LARGE;
    const uint32_t n_groups = (uint32_t)((total_words + GROUP_WORDS - 1) / GROUP_WORDS);
    uint32_t *group_count = static_cast<uint32_t *>(scratch);       // clapgpu_visible_scratch_bytes(n_ranges * cap_pad)
    hipLaunchKernelGGL(k_mask_group_count_seg, dim3(n_groups), dim3(WAVE), 0, as_stream(stream), gathered_mask, sg, group_count);
    CLAPGPU_LAUNCH_CHECK("k_mask_group_count_seg");
    hipLaunchKernelGGL(k_visible_expand_seg, dim3(n_groups), dim3(WAVE), 0, as_stream(stream), gathered_mask, sg, group_count, n_groups,
                       visible, count);
    CLAPGPU_LAUNCH_CHECK("k_visible_expand_seg");
    return CLAPGPU_OK;
}

// The same expansion on the host: what a rank without the device list needs, and the checker of the kernels above
// (tests/test_shard_cpu.py runs eight gloo ranks through it).  Returns the number of ids; writes at most `capacity`.
extern "C" uint32_t clapgpu_visible_expand_ranges_host(const uint64_t *gathered_mask, uint32_t n_ranges, uint32_t cap_pad,
                                                       const uint32_t *base, const uint32_t *n_pad, uint32_t *visible, uint32_t capacity)
{
    if (!gathered_mask || check_ranges(n_ranges, cap_pad, base, n_pad)) return 0;
    const uint32_t cap_words = cap_pad / 64;
    uint32_t cnt = 0;
    for (uint32_t r = 0; r < n_ranges; r++) {
        const uint32_t words = (n_pad ? n_pad[r] : cap_pad) / 64;
        for (uint32_t w = 0; w < words; w++) {
            uint64_t m = gathered_mask[(size_t)r * cap_words + w];
            while (m) {
                const uint32_t id = base[r] + w * 64u + (uint32_t)__builtin_ctzll(m);
                m &= m - 1;
                if (visible && cnt < capacity) visible[cnt] = id;
                cnt++;
            }
        }
    }
    return cnt;
}

static LodK lod_args(const clapgpu_entities *e, const float cam_pos[3], const int32_t *force_lod, int32_t *cur_lod)
{
    LodK k;
    k.cx = cam_pos[0]; k.cy = cam_pos[1]; k.cz = cam_pos[2];
    k.aabb = e->aabb; k.center = e->center;
    k.pos_scale = reinterpret_cast<const float4 *>(e->pos_scale);
    k.model = e->model;
    k.model_table = reinterpret_cast<const float4 *>(e->model_table);
    k.force_lod = force_lod; k.cur_lod = cur_lod;
    k.n_models = e->n_models ? e->n_models : 1;
    return k;
}

extern "C" int clapgpu_entities_lod(void *stream, const clapgpu_entities *e, const uint32_t *visible,
                                    const uint32_t *count, uint32_t index_base, const float cam_pos[3],
                                    const int32_t *force_lod, int32_t *cur_lod, int32_t *draw_lod)
{
    if (!e || !visible || !count || !cam_pos || !cur_lod || !draw_lod || !e->aabb || !e->center ||
        !e->pos_scale || !e->model || !e->model_table)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (e->n == 0)
        return CLAPGPU_OK;
    uint32_t blocks = (e->n + ENT_BLOCK - 1) / ENT_BLOCK;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_entities_lod, dim3(blocks), dim3(ENT_BLOCK), 0, as_stream(stream), visible, count, index_base,
                       lod_args(e, cam_pos, force_lod, cur_lod), draw_lod, e->n);
    CLAPGPU_LAUNCH_CHECK("k_entities_lod");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_entities_lod_views(void *stream, const clapgpu_entities *e, const uint32_t *visible, const uint32_t *count,
                                          uint32_t index_base, const clapgpu_views_state *state, const int32_t *force_lod,
                                          int32_t *cur_lod, int32_t *draw_lod)
{
    if (!view_block_ok(state) || !e || !visible || !count || !cur_lod || !draw_lod || !e->aabb || !e->center ||
        !e->pos_scale || !e->model || !e->model_table)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (e->n == 0)
        return CLAPGPU_OK;
    uint32_t blocks = (e->n + ENT_BLOCK - 1) / ENT_BLOCK;
    if (blocks > 2048) blocks = 2048;
    const float unread[3] = { 0.f, 0.f, 0.f };                   // the kernel takes the position from the block
    hipLaunchKernelGGL(k_entities_lod_views, dim3(blocks), dim3(ENT_BLOCK), 0, as_stream(stream), visible, count, index_base,
                       lod_args(e, unread, force_lod, cur_lod), draw_lod, e->n, state);
    CLAPGPU_LAUNCH_CHECK("k_entities_lod_views");
    return CLAPGPU_OK;
}

// clapgpu_visible_compact + clapgpu_entities_lod of this batch's own entities: the render pass's list and its LODs by one
// call.  Two launches: a single kernel that picks the LOD of every id as it writes it was built and measured (round 5,
// profiles/r05_experiments/lod_in_expand.md) -- the expansion walks sixteen mask rows per wavefront one after the other,
// and with the pick's chain of dependent loads under every row it took 42 us against 6 + 10 us for the two.
extern "C" int clapgpu_visible_compact_lod(void *stream, const clapgpu_entities *e, uint32_t index_base, const float cam_pos[3],
                                           const int32_t *force_lod, int32_t *cur_lod, uint32_t *visible, uint32_t *count,
                                           int32_t *draw_lod, void *scratch)
{
    if (!e || !count || !cam_pos || !cur_lod || !draw_lod || (e->n && (!e->vis_mask || !visible)) || !e->aabb || !e->center ||
        !e->pos_scale || !e->model || !e->model_table)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    const uint32_t n = e->n;
    int rc = clapgpu_visible_compact(stream, e->vis_mask, e->vis_row_pop, n, index_base, visible, count, scratch);
    if (rc) return rc;
    return clapgpu_entities_lod(stream, e, visible, count, index_base, cam_pos, force_lod, cur_lod, draw_lod);
}

extern "C" int clapgpu_visible_compact_lod_views(void *stream, const clapgpu_entities *e, uint32_t index_base,
                                                 const clapgpu_views_state *state, const int32_t *force_lod, int32_t *cur_lod,
                                                 uint32_t *visible, uint32_t *count, int32_t *draw_lod, void *scratch)
{
    if (!view_block_ok(state) || !e || !count || !cur_lod || !draw_lod || (e->n && (!e->vis_mask || !visible)) || !e->aabb ||
        !e->center || !e->pos_scale || !e->model || !e->model_table)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    int rc = clapgpu_visible_compact(stream, e->vis_mask, e->vis_row_pop, e->n, index_base, visible, count, scratch);
    if (rc) return rc;
    return clapgpu_entities_lod_views(stream, e, visible, count, index_base, state, force_lod, cur_lod, draw_lod);
}
