// entities.hip -- entity transform hierarchy -> inverse -> world AABB -> frustum cull
// for gfx950 (MI355X).  One lane per entity, one launch per hierarchy level.
//
// Replaces, per entity, the reference's default_update() transform branch
// (model.c:1649-1695), parent_transform_apply() jointless attachment
// (model.c:1594-1647), mat4x4_invert (linmath.h:611-651), entity3d_aabb_update
// (model.c:1200-1234) and the draw predicate of _models_render with
// view_entity_in_frustum (model.c:959-973, view.c:296-337).
//
// HBM-bound: ~276 algorithmic bytes / entity.  Inputs are read as
// coalesced float4 / dword streams, the parent matrix as 4 x 16 B per lane, and
// every output row block (64 entities x 64 / 64 / 24 / 12 B) is transposed through
// a wave-private LDS tile so each store instruction writes 1 KiB contiguous.
//
// This file holds the update only.  What a row is and how one is rebuilt: entities_row.h.  The host mirror's one-launch
// frame: entities_host.hip (its own translation unit, see entities_row.h).  Cull-only pass, visible list, LOD pick:
// visible.hip.  The verbs that rewrite or export rows between updates: entities_edit.hip.
#include <string.h>
#include <math.h>
#include <type_traits>
#include "common.h"
#include "lm_dev.h"
#include "entities_row.h"
#include "entities_args.h"

namespace clapgpu {

// The common row of a tile walk, as straight-line code: all 64 lanes alive and rebuilt, every parent in the
// previous row's registers (or none), no joint attachment, every model with a box (taken from the LDS copy `mt` of
// the model table), no camera query.  Same arithmetic as process_row; what differs is what the wavefront waits for.
// gfx950 has one counter for vector loads AND stores, retired in issue order: a wait for the newest load is a wait
// for every store before it.  process_row loads the model table (and, on its other paths, parents) between the
// previous row's stores and its own arithmetic, and its stores sit in branches, so the compiler can only wait for
// "everything" there and again before the row hand-over -- each row's 10 KB of stores was drained twice while the
// SIMD idled.  Here no vector load is issued between the prefetch of the next row and the hand-over, and the big
// stores are unconditional, so the hand-over waits for "all but the last N operations" and the stores stay in
// flight under the next row's arithmetic.
template <bool CULL, bool XV = false>
__device__ __forceinline__ void process_row_fast(const EntK &e, const RowIn &in, float4 *tile, const float4 *mt,
                                                 const int lane, const uint32_t row_first, const uint32_t mode,
                                                 const lmd::FrustumK &fr, const int src, const uint32_t parent_seq_now,
                                                 float (&carry_mx)[16], uint32_t &carry_seq, const XViewsK *xv = nullptr)
{
    const uint32_t i = row_first + lane;
    const uint32_t fl = in.fl;
    const int32_t p = in.p;
    uint32_t seq = in.sq & 0xffffu, pseq = in.sq >> 16;
    float pm[16];
#pragma unroll
    for (int k = 0; k < 16; k++) pm[k] = __shfl(carry_mx[k], src);
    if (p >= 0) pseq = parent_seq_now;

    const float4 lo = mt[2 * in.mi], hi = mt[2 * in.mi + 1];
    float mx[16], inv[16], bb[6], ctr[3], local_mx[16];
    lmd::trs(local_mx, in.ps.x, in.ps.y, in.ps.z, in.ps.w, in.q.x, in.q.y, in.q.z, in.q.w);
    if (p >= 0) {
        lmd::mul(mx, pm, local_mx);                              // model.c:1625
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++) mx[k] = local_mx[k];
    }
    row_inverse(inv, mx);
    row_box(bb, ctr, mx, lo, hi);
    seq = (seq + 1) & 0xffffu;
#pragma unroll
    for (int k = 0; k < 16; k++) carry_mx[k] = mx[k];
    carry_seq = seq;

    const size_t e0 = row_first;
    float4 *tile_a = tile, *tile_b = tile + 256;
    float *tile_f = reinterpret_cast<float *>(tile);
    float4 va[4], vb[4];
    stage_mat4(tile_a, mx, lane);
    stage_mat4(tile_b, inv, lane);
    wave_lds_fence();
    unstage_mat4(tile_a, va, lane);
    unstage_mat4(tile_b, vb, lane);
    store_mat4_rows(e.mx + 16 * e0, va, lane, WAVE);
    store_mat4_rows(e.inv_mx + 16 * e0, vb, lane, WAVE);
    e.seqs[i] = seq | (pseq << 16);
    wave_lds_fence();
    // every store below is issued by all 64 lanes, none under a lane test: a store in a branch is one the compiler
    // cannot count.  The row's 1536 B of boxes = one 16-byte and one 8-byte piece per lane; the centres are the
    // lanes' own 12 bytes in lane order already.
    stage_rows<6>(tile_f, bb, lane);
    wave_lds_fence();
    {
        float *ab = e.aabb + 6 * e0;
        store_stream(&reinterpret_cast<float4 *>(ab)[lane], reinterpret_cast<const float4 *>(tile_f)[lane]);
        const float2 t2 = reinterpret_cast<const float2 *>(tile_f + 4 * WAVE)[lane];
        const clapgpu_f2 v2 = { t2.x, t2.y };
        const clapgpu_f3 v3 = { ctr[0], ctr[1], ctr[2] };
        store_stream(reinterpret_cast<clapgpu_f2 *>(ab + 4 * WAVE) + lane, v2);
        store_stream(reinterpret_cast<clapgpu_f3 *>(e.center + 3 * (e0 + lane)), v3);   // sizeof(f3) is 16: index in floats
    }
    wave_lds_fence();
    if (!(mode & CLAPGPU_UPDATE_ALL_DIRTY) && (fl & CLAPGPU_E_DIRTY))
        e.flags[i] = fl & ~CLAPGPU_E_DIRTY;                      // transform_clear_updated
    if (e.rebuilt_mask && lane == 0) e.rebuilt_mask[row_first >> 6] = ~0ull;
    if (CULL) {
        bool vis = (fl & CLAPGPU_E_VISIBLE) != 0;                                      // model.c:959-965
        if (vis && !(fl & CLAPGPU_E_SKIP_CULLING))
            vis = lmd::aabb_in_frustum_fast(fr, bb);                                  // model.c:967-971
        const uint64_t m = __ballot(vis);
        e.vis_mask[e0 >> 6] = m;                                 // the same word from all 64 lanes: one request
        e.vis_row_pop[e0 >> 6] = (uint8_t)__popcll(m);
        if constexpr (XV) cull_extra_views(*xv, (fl & CLAPGPU_E_VISIBLE) != 0, fl, bb, (uint32_t)(e0 >> 6), lane);
    }
}

// model.c:1618-1622 + 1633-1639: local = TRS of the attached entity, joint_mx = joint_transforms[j] * bind[j],
// attach_local = joint_mx * local.  One lane per attachment (there are few).
__global__ __launch_bounds__(ENT_BLOCK)
void k_attach_prepare(EntK e)
{
    const uint32_t k = blockIdx.x * ENT_BLOCK + threadIdx.x;
    if (k >= e.n_attach) return;
    const clapgpu_attach at = e.attach[k];
    const float4 ps = e.pos_scale[at.entity], q = e.rot[at.entity];
    float local_mx[16], jt[16], bd[16], joint_mx[16], out[16];
    lmd::trs(local_mx, ps.x, ps.y, ps.z, ps.w, q.x, q.y, q.z, q.w);
    load_mat4(jt, e.jt_pool + 16 * (size_t)at.jt);
    load_mat4(bd, e.bind_pool + 16 * (size_t)at.bind);
    lmd::mul(joint_mx, jt, bd);
    lmd::mul(out, joint_mx, local_mx);
    float4 *d = reinterpret_cast<float4 *>(e.attach_local + 16 * (size_t)k);
#pragma unroll
    for (int c = 0; c < 4; c++)
        d[c] = make_float4(out[4 * c], out[4 * c + 1], out[4 * c + 2], out[4 * c + 3]);
}

// One launch per hierarchy level: every parent was written by an earlier launch.
// `first` is a multiple of 64, so each wave owns exactly one vis_mask word.
// XV: nothing, or the XViewsK of a launch that culls the frame's further views too -- a trailing kernel argument that
// exists only then.
template <bool CULL, class... XV>
__global__ __launch_bounds__(ENT_BLOCK)
void k_entities_level(EntK e, uint32_t first, uint32_t count, uint32_t mode, lmd::FrustumK fr, XV... xv)
{
    __shared__ float4 lds_tiles[ENT_BLOCK / WAVE][LDS_F4_PER_WAVE];
    const int lane = lane_id();
    const int wave = threadIdx.x / WAVE;
    const uint32_t wave_local0 = blockIdx.x * ENT_BLOCK + wave * WAVE;
    if (wave_local0 >= count)
        return;                                                  // whole wave; no block-level sync below
    const uint32_t row_count = count - wave_local0 < WAVE ? count - wave_local0 : WAVE;
    float carry_mx[16];
    uint32_t carry_seq = 0;
    bool carry_valid = false;
    const RowIn in = load_row(e, lane, first + wave_local0, row_count);
    process_row<CULL, false, false, sizeof...(XV) != 0>(e, in, lds_tiles[wave], lane, first + wave_local0, row_count, mode, fr,
                                                        false, 0, carry_mx, carry_seq, carry_valid, nullptr, nullptr, xviews_ptr(xv...));
}

// One launch for the whole forest: wave t walks tile t = rows [tile_row_start[t], tile_row_start[t+1]),
// row r = entities [64r, 64r+64) = one hierarchy level of the subtrees packed into the tile.
// The next row's inputs are in flight while the current row is computed.
constexpr int ENT_MT_CAP = 256;       // models whose table the tile kernel keeps in LDS (8 KiB); more: general loop only
constexpr int ENT_TILE_WAVES = 1;       // occupancy hint; 4 measured the same 44 us
// The frustum (63 dwords) is the FIRST kernel argument and is read where it is used, through the kernarg segment
// pointer, with the pointer laundered once per row: held in SGPRs across the row loop next to ~30 array pointers it
// cost 194 spilled SGPRs -- some 300 v_readlane / s_nop per row of a kernel that issues 850 vector instructions per row.
//
// XV as for k_entities_level.  The body stands HERE, in the kernel, for every instantiation, not in a device function the
// kernels share: called through a function the compiler scheduled k_entities_tiles<true> differently (57 instructions
// fewer, registers renumbered), and this kernel's store / wait structure is measured work that no other feature may move.
// As a template over the trailing argument all three instantiations keep their instruction streams (tools/isa_hashes.sh,
// profiles/entities_split); before that the body was a file included once per kernel.
template <bool CULL, class... XV>
__global__ __launch_bounds__(ENT_BLOCK, ENT_TILE_WAVES)
void k_entities_tiles(lmd::FrustumK fr_arg, EntK e, const uint32_t *tile_row_start, uint32_t n_tiles, uint32_t n,
                      uint32_t mode, XV... xv)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)fr_arg;                                                // read at kernarg offset 0: see the static_assert behind this kernel
    // kept in the constant address space through the laundering below: the planes then come through the scalar cache
    // (s_load, counted with LDS), not as flat loads, whose wait is a wait for every vector store before them
    typedef const __attribute__((address_space(4))) lmd::FrustumK *frustum_ptr;
    frustum_ptr frp = (frustum_ptr)__builtin_amdgcn_kernarg_segment_ptr();
#else
    typedef const lmd::FrustumK *frustum_ptr;
    frustum_ptr frp = &fr_arg;                                   // host pass of the compiler only
#endif
    __shared__ float4 lds_tiles[ENT_BLOCK / WAVE][LDS_F4_PER_WAVE];
    __shared__ float4 mt_lds[2 * ENT_MT_CAP];                    // the model table, for process_row_fast
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);   // uniform, and known to be: the row loops stay scalar
    const bool mt_cached = e.n_models <= (uint32_t)ENT_MT_CAP;
    if (mt_cached)
        for (uint32_t k = threadIdx.x; k < 2 * e.n_models; k += ENT_BLOCK) mt_lds[k] = e.model_table[k];
    __syncthreads();                                             // the only workgroup barrier: ahead of every return
    const uint32_t t = blockIdx.x * (ENT_BLOCK / WAVE) + wave;
    if (t >= n_tiles)
        return;
    const uint32_t n_rows = (n + WAVE - 1) / WAVE;
    uint32_t row = tile_row_start[t], row_end = tile_row_start[t + 1];
    if (row_end > n_rows) row_end = n_rows;                      // never walk past the arrays
    if (row >= row_end)
        return;

    float carry_mx[16];
#pragma unroll
    for (int k = 0; k < 16; k++) carry_mx[k] = 0.f;
    uint32_t carry_seq = 0;
    bool carry_valid = false;
    bool have_prev = false;

    uint32_t row_first = row * WAVE;
    uint32_t row_count = n - row_first < WAVE ? n - row_first : WAVE;
    RowIn cur = load_row(e, lane, row_first, row_count);

    // ---- rows that qualify for process_row_fast, until the first one that does not: the rest of the tile (and every
    // tile of a launch with a camera query or a model table too large for LDS) goes through the general loop below.
    // Two loops, not a branch inside one: the straight-line loop must never be re-entered from a path whose stores
    // the compiler cannot count.
    if (mt_cached && !e.bv_on) {
        // the first row's inputs are waited for HERE: left pending into the loop, their wait would sit inside it and,
        // on the way round, stand for "all but seven operations" -- the previous row's stores again
        asm volatile("" : : "v"(cur.ps.w), "v"(cur.q.w), "v"(cur.fl), "v"(cur.sq), "v"(cur.mi), "v"(cur.p));
        for (;;) {
            const uint32_t fl = cur.fl;
            const int32_t p = cur.p;
            const bool in_prev = have_prev && p >= 0 && (uint32_t)p >= row_first - WAVE && (uint32_t)p < row_first;
            const int src = in_prev ? (int)((uint32_t)p - (row_first - WAVE)) : lane;
            const uint32_t parent_seq_now = __shfl(carry_seq, src);
            const bool parent_ok = p < 0 || (in_prev && __shfl((int)carry_valid, src) != 0);
            const bool dirty = (mode & CLAPGPU_UPDATE_ALL_DIRTY) ? true : (fl & CLAPGPU_E_DIRTY) != 0;
            const bool rebuild = p >= 0 ? !((cur.sq >> 16) == parent_seq_now && !dirty) : dirty;
            const bool lane_ok = (fl & CLAPGPU_E_ALIVE) && rebuild && parent_ok &&
                                 !((fl & CLAPGPU_E_JOINT_ATTACHED) && e.n_attach) &&
                                 __float_as_uint(mt_lds[2 * cur.mi].w) == 0u;
            if (row_count != WAVE || __ballot(lane_ok) != ~0ull)
                break;
            const uint32_t next = row + 1;
            const bool more = next < row_end;
            const uint32_t nfirst = more ? next * WAVE : row_first;
            const uint32_t ncount = n - nfirst < WAVE ? n - nfirst : WAVE;
            const RowIn nxt = load_row(e, lane, nfirst, ncount);
            frustum_ptr frr = frp;
            asm volatile("" : "+s"(frr));
            process_row_fast<CULL, sizeof...(XV) != 0>(e, cur, lds_tiles[wave], mt_lds, lane, row_first, mode, *(const lmd::FrustumK *)frr,
                                                       src, parent_seq_now, carry_mx, carry_seq, xviews_ptr(xv...));
            carry_valid = true;
            if (!more)
                return;
            have_prev = true;
            cur = nxt;
            row = next;
            row_first = nfirst;
            row_count = ncount;
        }
    }
    for (;;) {
        const uint32_t next = row + 1;
        const bool more = next < row_end;
        const uint32_t nfirst = more ? next * WAVE : row_first;  // last row: harmless re-load
        const uint32_t ncount = n - nfirst < WAVE ? n - nfirst : WAVE;
        const RowIn nxt = load_row(e, lane, nfirst, ncount);     // in flight during process_row
        frustum_ptr frr = frp;
        asm volatile("" : "+s"(frr));                            // the planes are re-read (scalar cache) each row
        process_row<CULL, true, false, sizeof...(XV) != 0>(e, cur, lds_tiles[wave], lane, row_first, row_count, mode, *(const lmd::FrustumK *)frr,
                                                           have_prev, row_first - WAVE, carry_mx, carry_seq, carry_valid, nullptr, nullptr,
                                                           xviews_ptr(xv...));
        if (!more)
            break;
        have_prev = true;
        cur = nxt;
        row = next;
        row_first = nfirst;
        row_count = ncount;
    }
}

// k_entities_tiles reads its frustum through the kernarg segment pointer at offset 0.  The AMDGPU kernel ABI lays the
// explicit arguments out first and in declaration order, so that holds exactly as long as the frustum is the FIRST
// parameter: reordering the signature must not compile.
template <class F> struct first_param;
template <class R, class A0, class... A> struct first_param<R (*)(A0, A...)> { using type = A0; };
static_assert(std::is_same<first_param<decltype(&k_entities_tiles<true>)>::type, lmd::FrustumK>::value &&
              std::is_same<first_param<decltype(&k_entities_tiles<false>)>::type, lmd::FrustumK>::value,
              "k_entities_tiles: the frustum must stay the first kernel argument (it is read at kernarg offset 0)");
static_assert(std::is_same<first_param<decltype(&k_entities_tiles<true, XViewsK>)>::type, lmd::FrustumK>::value, "... with further views: the same");
static_assert(alignof(lmd::FrustumK) <= 8, "kernarg offset 0 holds for any alignment the segment start guarantees");

// clapgpu_entities.views for the kernels (entities_args.h)
bool make_xviews_k(const clapgpu_entities *e, bool hostio, XViewsK *out)
{
    memset(out, 0, sizeof(*out));
    const clapgpu_views *v = e->views;
    if (!v || !v->n) return true;
    if (v->n > CLAPGPU_EXTRA_VIEWS_MAX) return false;
    out->n = v->n;
    for (uint32_t k = 0; k < v->n; k++) {
        if (!v->vis_mask[k] || !v->vis_row_pop[k]) return false;
        out->mask[k] = v->vis_mask[k]; out->pop[k] = v->vis_row_pop[k];
        out->o_mask[k] = hostio ? v->host_vis_mask[k] : nullptr;
        out->fr[k] = make_frustum_k(&v->frustum[k]);
    }
    return true;
}

} // namespace clapgpu

using namespace clapgpu;

static int prepare_attachments(void *stream, const EntK &k)
{
    if (!k.n_attach)
        return CLAPGPU_OK;
    hipLaunchKernelGGL(k_attach_prepare, dim3((k.n_attach + ENT_BLOCK - 1) / ENT_BLOCK), dim3(ENT_BLOCK), 0,
                       as_stream(stream), k);
    CLAPGPU_LAUNCH_CHECK("k_attach_prepare");
    return CLAPGPU_OK;
}

static int launch_level(void *stream, const EntK &k, uint32_t first, uint32_t count, uint32_t mode,
                        const clapgpu_frustum *frustum, const XViewsK &xv)
{
    const lmd::FrustumK fr = make_frustum_k(frustum);
    const dim3 grid((count + ENT_BLOCK - 1) / ENT_BLOCK), block(ENT_BLOCK);
    if (frustum && xv.n)
        hipLaunchKernelGGL((k_entities_level<true, XViewsK>), grid, block, 0, as_stream(stream), k, first, count, mode, fr, xv);
    else if (frustum)
        hipLaunchKernelGGL(k_entities_level<true>, grid, block, 0, as_stream(stream), k, first, count, mode, fr);
    else
        hipLaunchKernelGGL(k_entities_level<false>, grid, block, 0, as_stream(stream), k, first, count, mode, fr);
    CLAPGPU_LAUNCH_CHECK("k_entities_level");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_entities_update_level(void *stream, const clapgpu_entities *e,
                                             uint32_t first, uint32_t count,
                                             uint32_t mode, const clapgpu_frustum *frustum)
{
    int rc = check_entities(e, frustum != nullptr);
    if (rc) return rc;
    if (first & 63u)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (first > e->n || count > e->n - first)
        return CLAPGPU_ERR_OUT_OF_BOUNDS;
    if (!count)
        return CLAPGPU_OK;
    const EntK k = to_kernel_args(e);
    XViewsK xv;
    if (!make_xviews_k(e, false, &xv)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    rc = prepare_attachments(stream, k);
    if (rc) return rc;
    return launch_level(stream, k, first, count, mode, frustum, xv);
}

extern "C" int clapgpu_entities_update(void *stream, const clapgpu_entities *e,
                                       const uint32_t *level_start, uint32_t n_levels,
                                       uint32_t mode, const clapgpu_frustum *frustum)
{
    int rc = check_entities(e, frustum != nullptr);
    if (rc) return rc;
    if (!level_start || (e->n && !n_levels))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (e->n == 0)
        return CLAPGPU_OK;
    if (level_start[0] != 0 || level_start[n_levels] != e->n)
        return CLAPGPU_ERR_OUT_OF_BOUNDS;
    for (uint32_t l = 0; l < n_levels; l++)
        if (level_start[l] > level_start[l + 1] || (level_start[l] & 63u))
            return CLAPGPU_ERR_INVALID_ARGUMENTS;

    const EntK k = to_kernel_args(e);
    XViewsK xv;
    if (!make_xviews_k(e, false, &xv)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (k.bv_result)
        CLAPGPU_HIP(hipMemsetAsync(k.bv_result, 0, sizeof(uint64_t), as_stream(stream)));
    rc = prepare_attachments(stream, k);
    if (rc) return rc;
    for (uint32_t l = 0; l < n_levels; l++) {
        const uint32_t first = level_start[l], count = level_start[l + 1] - first;
        if (!count)
            continue;
        rc = launch_level(stream, k, first, count, mode, frustum, xv);
        if (rc) return rc;
    }
    return CLAPGPU_OK;
}

extern "C" int clapgpu_entities_update_tiles(void *stream, const clapgpu_entities *e,
                                             const uint32_t *tile_row_start, uint32_t n_tiles,
                                             uint32_t mode, const clapgpu_frustum *frustum)
{
    int rc = check_entities(e, frustum != nullptr);
    if (rc) return rc;
    if (e->n == 0 || n_tiles == 0)
        return CLAPGPU_OK;
    if (!tile_row_start)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    const lmd::FrustumK fr = make_frustum_k(frustum);
    const EntK k = to_kernel_args(e);
    XViewsK xv;
    if (!make_xviews_k(e, false, &xv)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (k.bv_result)
        CLAPGPU_HIP(hipMemsetAsync(k.bv_result, 0, sizeof(uint64_t), as_stream(stream)));
    rc = prepare_attachments(stream, k);
    if (rc) return rc;
    const uint32_t per_block = ENT_BLOCK / WAVE;
    const dim3 grid((n_tiles + per_block - 1) / per_block), block(ENT_BLOCK);
    if (frustum && xv.n)
        hipLaunchKernelGGL((k_entities_tiles<true, XViewsK>), grid, block, 0, as_stream(stream), fr, k, tile_row_start, n_tiles, e->n, mode, xv);
    else if (frustum)
        hipLaunchKernelGGL(k_entities_tiles<true>, grid, block, 0, as_stream(stream), fr, k, tile_row_start, n_tiles,
                           e->n, mode);
    else
        hipLaunchKernelGGL(k_entities_tiles<false>, grid, block, 0, as_stream(stream), fr, k, tile_row_start, n_tiles,
                           e->n, mode);
    CLAPGPU_LAUNCH_CHECK("k_entities_tiles");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_entities_update_tiles_hostio(void *stream, const clapgpu_entities *e,
                                                    const uint32_t *tile_row_start, uint32_t n_tiles, uint32_t mode,
                                                    const clapgpu_frustum *frustum, const clapgpu_entities_hostio *io)
{
    int rc = check_entities(e, frustum != nullptr);
    if (rc) return rc;
    if (!io || !io->mx || !io->inv_mx || !io->aabb || !io->center || !io->rebuilt_mask || !io->counter || !io->done ||
        (frustum && !io->vis_mask) || (io->touched && (!io->pos_scale || !io->rot || !io->flags)) || (n_tiles && !tile_row_start))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!aligned16(io->mx) || !aligned16(io->inv_mx) || (reinterpret_cast<uintptr_t>(io->aabb) & 7u) ||
        (io->touched && (!aligned16(io->pos_scale) || !aligned16(io->rot))))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    const lmd::FrustumK fr = make_frustum_k(frustum);
    const EntK k = to_kernel_args(e);
    if (k.bv_result)
        CLAPGPU_HIP(hipMemsetAsync(k.bv_result, 0, sizeof(uint64_t), as_stream(stream)));
    rc = prepare_attachments(stream, k);
    if (rc) return rc;
    HostIO h;
    h.pos_scale = reinterpret_cast<const float4 *>(io->pos_scale); h.rot = reinterpret_cast<const float4 *>(io->rot);
    h.flags = io->flags; h.touched = io->touched;
    h.o_mx = io->mx; h.o_inv = io->inv_mx; h.o_aabb = io->aabb; h.o_center = io->center;
    h.o_vis = io->vis_mask; h.o_rebuilt = io->rebuilt_mask; h.o_inside = io->inside_mask;
    h.counter = io->counter; h.done = io->done; h.done_value = io->done_value;
    h.keep = io->keep_mask; h.o_exported = io->exported_mask; h.stale = io->stale_mask;
    h.late_ok = io->options & CLAPGPU_HOSTIO_EXPORT_STALE_READ;
    const uint32_t tiles = e->n ? n_tiles : 0;
    XViewsK xv;
    if (!make_xviews_k(e, true, &xv)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    rc = launch_entities_tiles_host(as_stream(stream), frustum != nullptr, fr, k, h, tile_row_start, tiles, e->n, mode, xv);
    if (rc) return rc;
    return CLAPGPU_OK;
}
