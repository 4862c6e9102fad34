// broadphase.hip -- the broadphase over explicit AABBs, for gfx950: dSpaceCollide2(ground, bodies) + dSpaceCollide(bodies)
// (physics.c:751-753) as ascending candidate-pair lists, and the same grid as an index for the ray cast (rays.hip).
// The six kernels and the entry points that launch them; the object itself is made in bp_create.hip (bp_object.h).
// An object of more than one level (clapgpu_bp_create_levels) runs bp_levels.hip's kernels around k_bp_cells instead.
// fp64 boxes.  ODE is an absent submodule of the reference: PARITY UNPINNED (oracle/physics2.c states what is restated).
#include "bp_object.h"
#include "scan_dev.h"

namespace clapgpu {

constexpr int PB = 256;

// ================================================================================== broadphase
// Hash grid over the AABB centres, cell >= the largest body AABB edge, so a body's partners have their centres in
// the 27 cells around its own.  Cells are grouped in 4x4x4 blocks: a cell's slot = (hash of its block) * 64 + its
// position inside the block, so the 64 cells of a block are neighbours in memory and the per-frame prefix work
// splits into a wave-sized piece per block (k_bp_cells) and a scan over the block totals.
// Five launches for BOTH passes of __phys_step (bodies x bodies and statics x bodies):
//   k_bp_bin      one atomic per body on its cell's counter (the return value is its rank in the cell)
//   k_bp_cells    one wavefront per block: exclusive prefix of its 64 cell counts; block starts by a single-pass scan
//                 with decoupled look-back over the workgroups' totals
//   k_bp_scatter  64-byte records (box, index, cell coordinates) into cell order
//   k_bp_search   one wavefront per tile of 16 bodies in cell order; candidates (own cell: partners with a larger
//                 index; the 13 cells after it; the statics registered for the block) listed once per DISTINCT cell /
//                 block bucket of the tile in an LDS work list and tested against the tile's boxes; hits go to the
//                 partner list of min(i, j); then the large statics from LDS
//   k_bp_emit     one thread per body in index order: offset = tile offset (look-back scan over the 256-body tiles) +
//                 scan inside the tile, its list written in ascending partner order, so the output is the canonical
//                 ascending list whatever order the atomics took
// Two different cells of one 3x3x3 neighbourhood never share a slot (same position inside a block means at least four
// cells apart), and a body from a far block that shares a slot cannot overlap (cell >= every edge), so candidates need
// no cell check beyond the box test.
// BP_LIST (partners kept per body in its fixed slot), BP_EMIT_TILE: bp_object.h
constexpr int BP_TILE = 16;            // bodies per wavefront of the search
constexpr int BP_WORK = 512;           // candidate entries listed per tile and round (256: spheres -2 us, capsules +5 us)
#ifndef BP_SEARCH_IN_FLIGHT
#define BP_SEARCH_IN_FLIGHT 1            // candidate records gathered per lane and round
#endif

// block_hash, cell_coord, cell_slot, box_cell, bin_body, the box helpers, the record and the control words: bp_grid.h
// BpK and bin_of: bp_object.h.  The look-back scan of k_bp_cells and k_bp_emit: scan_dev.h
constexpr uint32_t BP_STATUS_SCAN = 4u;  // CTRL_STATUS: a look-back word never arrived

// Launch 1 (skipped when the step before it has binned the boxes it wrote: clapgpu_bodies_step_prebin)
__global__ __launch_bounds__(PB)
void k_bp_bin(BpK k)
{
    const uint32_t i = blockIdx.x * PB + threadIdx.x;
    if (i == 0) k.ctrl[CTRL_EPOCH] = k.ctrl[CTRL_EPOCH] + 1;          // first launch of the frame; read by the later ones
    if (i >= k.n) return;
    double bb[6];
    load_box(k.aabb, i, bb);
    bin_body(bin_of(k), i, bb);
}

// Launch 2: wave w = block bucket w; a workgroup's BP_CELLS_BLOCK / 64 block totals enter the look-back scan as one tile
constexpr int BP_CELLS_BLOCK = 1024;   // 16 buckets a workgroup: 512 look-back words at 262 144 bodies (256: 2 048 words, +2 us)
__global__ __launch_bounds__(BP_CELLS_BLOCK)
void k_bp_cells(BpK k)
{
    __shared__ uint32_t tot[BP_CELLS_BLOCK / WAVE];
    __shared__ uint32_t excl_s;
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const uint32_t b = blockIdx.x * (BP_CELLS_BLOCK / WAVE) + wave;
    uint32_t block_total = 0, c = 0, before = 0;                        // this lane's cell: bodies, bodies of the block's cells before it
    if (b <= k.mask) {
        c = k.cell_cnt[(size_t)b * 64 + lane];
        k.cell_cnt[(size_t)b * 64 + lane] = 0;                          // ready for the next frame
        const uint32_t incl = wave_prefix_sum(c);
        before = incl - c;
        block_total = __shfl(incl, WAVE - 1);
    }
    if (lane == 0) tot[wave] = block_total;
    __syncthreads();
    if (wave == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (int q = 0; q < BP_CELLS_BLOCK / WAVE; q++) sum += tot[q];
        const uint32_t excl = lb_exclusive(k.lb_cells, blockIdx.x, sum, k.ctrl[CTRL_EPOCH], k.ctrl + CTRL_STATUS, BP_STATUS_SCAN);
        if (lane == 0) excl_s = excl;
    }
    __syncthreads();
    if (b <= k.mask) {
        uint32_t start = excl_s;
        for (int q = 0; q < wave; q++) start += tot[q];
        k.cell_range[(size_t)b * 64 + lane] = make_uint2(start + before, c);
    }
}

// Launch 3
__global__ __launch_bounds__(PB)
void k_bp_scatter(BpK k)
{
    const uint32_t i = blockIdx.x * PB + threadIdx.x;
    if (i >= k.n) return;
    const uint32_t slot = k.key[i];
    const uint32_t at = k.cell_range[slot].x + k.rank[i];
    k.entries[at] = i;
    const double2 *p = reinterpret_cast<const double2 *>(k.aabb + 6 * (size_t)i);
    double2 *o = reinterpret_cast<double2 *>(k.recs + at);
    const double2 b0 = p[0], b1 = p[1], b2 = p[2];
    o[0] = b0; o[1] = b1; o[2] = b2;
    // the cell coordinates travel with the record: the search would otherwise redo three fp64 divisions per body
    const int32_t cx = cell_coord((b0.x + b0.y) * 0.5, k.cell), cy = cell_coord((b1.x + b1.y) * 0.5, k.cell),
                  cz = cell_coord((b2.x + b2.y) * 0.5, k.cell);
    reinterpret_cast<int4 *>(o)[3] = make_int4((int)i, cx, cy, cz);
}

// Launch 4.  One wavefront per tile of BP_TILE bodies that are neighbours in cell order.  Bodies of one cell have the
// same 14 candidate cells, so the tile's candidates are listed per DISTINCT cell ("leader": the first body of each run
// of equal cell coordinates), each entry with the range of tile bodies it has to be tested against: a candidate record is
// gathered once per cell, not once per body, and the tile's own boxes are read back from LDS as broadcasts.  The
// statics registered for a block are listed the same way, once per distinct block bucket.  Steps that depend on memory:
// tile records (+ the large statics' records) -> cell / static ranges (up to four per lane, loaded together) -> the work
// list in LDS -> candidate records, two per lane and round -> hit atomics.  Hits on bodies go to the partner list of
// min(i, j) (global atomics); static hits count in LDS, because only this wavefront writes its bodies' static lists.
__global__ __launch_bounds__(PB)
void k_bp_search(BpK k)
{
    constexpr int WAVES = PB / WAVE, T = BP_TILE, LOOKUPS = 4;          // lookups per lane: T * 14 + T <= 64 * LOOKUPS
    constexpr uint32_t WL = BP_WORK, OWN = 0x80000000u, STAT = 0x40000000u, IDX = 0x3fffffffu;
    constexpr int LARGE_TILE = 32;                                      // large statics staged per round (LDS <= 26 KB: six workgroups per CU)
    constexpr uint32_t HITS = 64;                                       // body x body hits parked per round
    static_assert(T * 15 <= WAVE * LOOKUPS && T <= 16, "tile lookups");
    __shared__ __attribute__((aligned(8))) uint32_t work[WAVES][WL][2];  // (record | flags, a_lo | a_hi << 8)
    __shared__ double abox[WAVES][T][6];
    __shared__ uint32_t aidx[WAVES][T];
    __shared__ int32_t lead[WAVES][2 * T][4];                           // cell leaders: (cx, cy, cz, range); then block leaders: (bucket, -, -, range)
    __shared__ uint32_t shits[WAVES][T];
    __shared__ uint32_t hits[WAVES][HITS][2], nhits[WAVES];
    __shared__ GridRec large[LARGE_TILE];
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const uint32_t t0 = (blockIdx.x * WAVES + wave) * T;
    const uint32_t nA = t0 < k.n ? (k.n - t0 < (uint32_t)T ? k.n - t0 : (uint32_t)T) : 0;
    const bool statics = k.n_static != 0;

    const uint32_t m0 = statics ? (k.n_large < LARGE_TILE ? k.n_large : LARGE_TILE) : 0;
    if (threadIdx.x < m0) large[threadIdx.x] = k.s_lrecs[threadIdx.x];  // issued with the tile's own records: no extra step
    // ---- the tile's bodies, cell leaders and block leaders
    int32_t cx = 0, cy = 0, cz = 0;
    uint32_t ob = 0;
    const bool isA = (uint32_t)lane < nA;
    if (isA) {
        const GridRec me = k.recs[t0 + lane];
#pragma unroll
        for (int x = 0; x < 6; x++) abox[wave][lane][x] = me.bb[x];
        aidx[wave][lane] = me.idx;
        cx = me.cell[0]; cy = me.cell[1]; cz = me.cell[2];
        ob = block_hash(cx >> 2, cy >> 2, cz >> 2, k.mask);
    }
    if (lane < T) shits[wave][lane] = 0;
    if (lane == 0) nhits[wave] = 0;
    const int32_t px = __shfl_up(cx, 1), py = __shfl_up(cy, 1), pz = __shfl_up(cz, 1);
    const uint32_t pob = __shfl_up(ob, 1);
    const bool cell_leader = isA && (lane == 0 || px != cx || py != cy || pz != cz);
    const bool block_leader = isA && statics && (lane == 0 || pob != ob);
    const uint32_t cmask = (uint32_t)__ballot(cell_leader), bmask = (uint32_t)__ballot(block_leader);
    const uint32_t n_lead = __popc(cmask), n_blead = __popc(bmask);
    if (isA) {
        const uint32_t below = (1u << lane) - 1u;
        if (cell_leader) {
            const uint32_t above = cmask >> (lane + 1);
            const uint32_t hi = above ? lane + 1 + __builtin_ctz(above) : nA;
            int32_t *d = lead[wave][__popc(cmask & below)];
            d[0] = cx; d[1] = cy; d[2] = cz; d[3] = (int32_t)((uint32_t)lane | hi << 8);
        }
        if (block_leader) {
            const uint32_t above = bmask >> (lane + 1);
            const uint32_t hi = above ? lane + 1 + __builtin_ctz(above) : nA;
            int32_t *d = lead[wave][T + __popc(bmask & below)];
            d[0] = (int32_t)ob; d[3] = (int32_t)((uint32_t)lane | hi << 8);
        }
    }
    wave_lds_fence();
    // ---- candidate runs: (leader, cell) and (block leader) lookups, up to four per lane, loads in flight together
    const uint32_t n_cell_runs = n_lead * 14u, n_runs = n_cell_runs + n_blead;
    // All of a lane's lookups are addressed first and loaded together, under no lane test (a lookup that does not exist
    // reads entry 0 and is given length 0): written as "if cell run ... else if block run ..." per lookup, each of the
    // four became its own branch with its own waits -- eight dependent trips to L2 before the first candidate.
    uint32_t b0[LOOKUPS], len[LOOKUPS], rng[LOOKUPS], mylen = 0;
    uint32_t slot[LOOKUPS], sidx[LOOKUPS];
    bool is_cell[LOOKUPS], is_stat[LOOKUPS], own[LOOKUPS];
#pragma unroll
    for (int r = 0; r < LOOKUPS; r++) {
        const uint32_t u = lane + WAVE * r;
        is_cell[r] = u < n_cell_runs;
        is_stat[r] = !is_cell[r] && u < n_runs;
        const uint32_t l = is_cell[r] ? u / 14u : 0u, cq = 13u + u % 14u;           // 13 = own cell, 14..26 = the cells after it
        const int32_t *d = lead[wave][is_stat[r] ? T + (u - n_cell_runs) : l];
        const int32_t d0 = d[0], d1 = d[1], d2 = d[2];
        rng[r] = (is_cell[r] || is_stat[r]) ? (uint32_t)d[3] : 0u;
        own[r] = is_cell[r] && cq == 13u;
        slot[r] = is_cell[r] ? cell_slot(d0 - 1 + (int32_t)(cq % 3), d1 - 1 + (int32_t)((cq / 3) % 3), d2 - 1 + (int32_t)(cq / 9), k.mask) : 0u;
        sidx[r] = is_stat[r] ? (uint32_t)d0 : 0u;
    }
    uint2 v_cr[LOOKUPS];
    uint32_t v_s0[LOOKUPS], v_s1[LOOKUPS];
#pragma unroll
    for (int r = 0; r < LOOKUPS; r++) v_cr[r] = k.cell_range[slot[r]];
    if (statics) {                                                       // uniform
#pragma unroll
        for (int r = 0; r < LOOKUPS; r++) { v_s0[r] = k.s_start[sidx[r]]; v_s1[r] = k.s_start[sidx[r] + 1]; }
    } else {
#pragma unroll
        for (int r = 0; r < LOOKUPS; r++) { v_s0[r] = 0; v_s1[r] = 0; }
    }
#pragma unroll
    for (int r = 0; r < LOOKUPS; r++) {
        b0[r] = is_cell[r] ? (v_cr[r].x | (own[r] ? OWN : 0u)) : is_stat[r] ? (v_s0[r] | STAT) : 0u;
        len[r] = is_cell[r] ? v_cr[r].y : is_stat[r] ? v_s1[r] - v_s0[r] : 0u;
        mylen += len[r];
    }
    uint32_t incl = mylen;                                              // wave_prefix_sum (common.h) restated: calling it moves this kernel's code
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    const uint32_t total = __shfl(incl, WAVE - 1);
    const uint32_t first = incl - mylen;

    // A hit on another body needs one returning atomic on the partner count of min(i, j), ~2 us under load: hits are
    // parked in LDS while the candidates are tested and their atomics issued together once per round.
    auto append_partner = [&](uint32_t lo, uint32_t hi) {
        const uint32_t at = atomicAdd(&k.cnt[lo], 1u);
        if (at < BP_LIST) k.partners[(size_t)lo * BP_LIST + at] = hi;
    };
    auto flush_hits = [&]() {
        wave_lds_fence();
        const uint32_t nh = nhits[wave] < HITS ? nhits[wave] : HITS;
        for (uint32_t h = lane; h < nh; h += WAVE) append_partner(hits[wave][h][0], hits[wave][h][1]);
        wave_lds_fence();
        if (lane == 0) nhits[wave] = 0;
        wave_lds_fence();
    };
    auto test = [&](uint32_t w, uint32_t range, const GridRec &r) {
        const uint32_t j = r.idx, a_hi = range >> 8;
        for (uint32_t x = range & 0xffu; x < a_hi; x++) {
            const double2 *ab = reinterpret_cast<const double2 *>(abox[wave][x]);
            const double2 a01 = ab[0], a23 = ab[1], a45 = ab[2];         // all six before any compare: one LDS wait per body
            const bool apart = (a01.x > r.bb[1]) | (a01.y < r.bb[0]) | (a23.x > r.bb[3]) | (a23.y < r.bb[2]) |
                               (a45.x > r.bb[5]) | (a45.y < r.bb[4]);
            if (apart) continue;
            const uint32_t i = aidx[wave][x];
            if (w & STAT) {
                const uint32_t at = atomicAdd(&shits[wave][x], 1u);
                if (at < BP_LIST) k.spartners[(size_t)i * BP_LIST + at] = j;
            } else if (j != i && (!(w & OWN) || j > i)) {
                const uint32_t lo = i < j ? i : j, hi = i < j ? j : i;
                const uint32_t h = atomicAdd(&nhits[wave], 1u);
                if (h < HITS) { hits[wave][h][0] = lo; hits[wave][h][1] = hi; }
                else append_partner(lo, hi);                             // list full (a pile-up): straight to memory
            }
        }
    };

    for (uint32_t base = 0; base < total; base += WL) {                 // one round unless > WL candidates (total is wave-uniform)
        uint32_t off = first;
#pragma unroll
        for (int r = 0; r < LOOKUPS; r++) {
            for (uint32_t e = 0; __any(e < len[r]); e++) {
                if (e < len[r]) {
                    const uint32_t o = off + e - base;                  // wraps below base: then >= WL
                    if (o < WL) *reinterpret_cast<uint2 *>(work[wave][o]) = make_uint2(b0[r] + e, rng[r]);
                }
            }
            off += len[r];
        }
        wave_lds_fence();
        const uint32_t todo = total - base < WL ? total - base : WL;
#if BP_SEARCH_IN_FLIGHT == 2
        for (uint32_t e = lane; e < todo + lane; e += 2 * WAVE) {       // wave-uniform trip count; two records in flight per lane
            const bool v0 = e < todo, v1 = e + WAVE < todo;
            const uint2 e0 = v0 ? *reinterpret_cast<const uint2 *>(work[wave][e]) : make_uint2(0u, 0u);
            const uint2 e1 = v1 ? *reinterpret_cast<const uint2 *>(work[wave][e + WAVE]) : make_uint2(0u, 0u);
            const uint32_t w0 = e0.x, g0 = e0.y, w1 = e1.x, g1 = e1.y;
            GridRec r0, r1;
            if (v0) r0 = ((w0 & STAT) ? k.s_recs : k.recs)[w0 & IDX];
            if (v1) r1 = ((w1 & STAT) ? k.s_recs : k.recs)[w1 & IDX];
            if (v0) test(w0, g0, r0);
            if (v1) test(w1, g1, r1);
        }
#else
        for (uint32_t e = lane; e < todo; e += WAVE) {
            const uint2 e0 = *reinterpret_cast<const uint2 *>(work[wave][e]);
            const GridRec r0 = ((e0.x & STAT) ? k.s_recs : k.recs)[e0.x & IDX];
            test(e0.x, e0.y, r0);
        }
#endif
        flush_hits();
    }
    if (!statics) return;
    // ---- the large statics (tested by every body), staged through LDS for the whole workgroup
    for (uint32_t base = 0; base < k.n_large; base += LARGE_TILE) {
        const uint32_t m = k.n_large - base < LARGE_TILE ? k.n_large - base : LARGE_TILE;
        if (base) {
            __syncthreads();
            if (threadIdx.x < m) large[threadIdx.x] = k.s_lrecs[base + threadIdx.x];
        }
        __syncthreads();
        const uint32_t x = lane % T;                                    // tile body of this lane; the large list is strided by WAVE / T
        if (x < nA) {
            double a[6];
#pragma unroll
            for (int y = 0; y < 6; y++) a[y] = abox[wave][x][y];
            for (uint32_t e = lane / T; e < m; e += WAVE / T) {
                double bs[6];
#pragma unroll
                for (int y = 0; y < 6; y++) bs[y] = large[e].bb[y];
                if (boxes_overlap(a, bs)) {
                    const uint32_t at = atomicAdd(&shits[wave][x], 1u);
                    if (at < BP_LIST) k.spartners[(size_t)aidx[wave][x] * BP_LIST + at] = large[e].idx;
                }
            }
        }
    }
    wave_lds_fence();
    if (isA) k.scnt[aidx[wave][lane]] = shits[wave][lane];
}

// all partners of body i (larger index) in ascending order, for a body whose list did not fit its slot: one lane
// walks its 27 cells.  k_bp_emit's search over a body's statics restates the repeated minimum search with other
// candidates: one helper for both moved k_bp_emit's code and did not stay inside the parent's timing spread
// (profiles/bp_split/README.md).
template <typename F>
__device__ __forceinline__ void research_body(const BpK &k, uint32_t i, F &&emit_sorted)
{
    double a[6];
    load_box(k.aabb, i, a);
    int32_t cx, cy, cz;
    box_cell(a, k.cell, cx, cy, cz);
    uint32_t last = i;                                                   // partners > i, ascending: repeated minimum search
    for (;;) {
        uint32_t best = 0xffffffffu;
        for (int cq = 0; cq < 27; cq++) {
            const uint32_t slot = cell_slot(cx - 1 + cq % 3, cy - 1 + (cq / 3) % 3, cz - 1 + cq / 9, k.mask);
            const uint2 cr = k.cell_range[slot];
            const uint32_t s0 = cr.x, s1 = cr.x + cr.y;
            for (uint32_t s = s0; s < s1; s++) {
                const uint32_t j = k.entries[s];
                if (j <= last || j >= best) continue;
                double bj[6];
                load_box(k.aabb, j, bj);
                if (boxes_overlap(a, bj)) best = j;
            }
        }
        if (best == 0xffffffffu) break;
        emit_sorted(best);
        last = best;
    }
}

// Launch 5
__global__ __launch_bounds__(BP_EMIT_TILE)
void k_bp_emit(BpK k)
{
    __shared__ uint32_t lds[2][BP_EMIT_TILE / WAVE];
    __shared__ uint32_t tile_excl[2];
    const uint32_t i = blockIdx.x * BP_EMIT_TILE + threadIdx.x;
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    const bool with_statics = k.n_static != 0;
    uint32_t c[2] = { 0, 0 };
    if (i < k.n) {
        c[0] = k.cnt[i];
        k.cnt[i] = 0;                                                    // ready for the next frame's atomics
        if (with_statics) { c[1] = k.scnt[i]; k.scnt[i] = 0; }
    }
    // the lists travel while the offsets are scanned: their loads do not depend on the look-back
    uint4 pl[2][BP_LIST / 4];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int q = 0; q < BP_LIST / 4; q++) pl[t][q] = make_uint4(0, 0, 0, 0);
    if (c[0] && c[0] <= (uint32_t)BP_LIST) {
        const uint4 *src = reinterpret_cast<const uint4 *>(k.partners + (size_t)BP_LIST * i);
#pragma unroll
        for (int q = 0; q < BP_LIST / 4; q++) if ((uint32_t)(4 * q) < c[0]) pl[0][q] = src[q];
    }
    if (c[1] && c[1] <= (uint32_t)BP_LIST) {
        const uint4 *src = reinterpret_cast<const uint4 *>(k.spartners + (size_t)BP_LIST * i);
#pragma unroll
        for (int q = 0; q < BP_LIST / 4; q++) if ((uint32_t)(4 * q) < c[1]) pl[1][q] = src[q];
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
            excl = lb_exclusive(wave ? k.lb_static : k.lb_body, blockIdx.x, sum, k.ctrl[CTRL_EPOCH], k.ctrl + CTRL_STATUS, BP_STATUS_SCAN);
        if (lane == 0) {
            tile_excl[wave] = excl;
            if (blockIdx.x == gridDim.x - 1) {                           // the last tile's inclusive prefix is the total
                uint32_t *tot = wave ? k.spair_total : k.pair_total;
                if (tot) *tot = (wave == 0 || with_statics) ? excl + sum : 0u;
            }
        }
    }
    __syncthreads();
    uint32_t woff[2] = { 0, 0 };
    for (int qq = 0; qq < wave; qq++) { woff[0] += lds[0][qq]; woff[1] += lds[1][qq]; }
    if (i >= k.n) return;
    // a list of n <= BP_LIST entries, out in ascending order: the rank of an entry = the entries below it
    auto ranked = [&](const uint4 (&l4)[BP_LIST / 4], uint32_t n, uint32_t off, uint2 *out, uint32_t cap) {
        uint32_t v[BP_LIST];
#pragma unroll
        for (int q = 0; q < BP_LIST / 4; q++) { v[4 * q] = l4[q].x; v[4 * q + 1] = l4[q].y; v[4 * q + 2] = l4[q].z; v[4 * q + 3] = l4[q].w; }
#pragma unroll
        for (int e = 0; e < BP_LIST; e++) {
            if ((uint32_t)e < n) {
                uint32_t rank = 0;
#pragma unroll
                for (int f = 0; f < BP_LIST; f++) rank += ((uint32_t)f < n) & (v[f] < v[e]);
                if (off + rank < cap) out[off + rank] = make_uint2(i, v[e]);
            }
        }
    };
    if (c[0]) {
        const uint32_t off = tile_excl[0] + woff[0] + incl[0] - c[0];
        uint2 *out = reinterpret_cast<uint2 *>(k.pairs);
        if (c[0] <= (uint32_t)BP_LIST) ranked(pl[0], c[0], off, out, k.capacity);
        else {
            uint32_t w = 0;
            research_body(k, i, [&](uint32_t j) { if (off + w < k.capacity) out[off + w] = make_uint2(i, j); w++; });
        }
    }
    if (c[1]) {
        const uint32_t off = tile_excl[1] + woff[1] + incl[1] - c[1];
        uint2 *out = reinterpret_cast<uint2 *>(k.spairs);
        if (c[1] <= (uint32_t)BP_LIST) ranked(pl[1], c[1], off, out, k.scapacity);
        else {                                                           // every static of the block + the large ones, ascending
            double a[6];
            load_box(k.aabb, i, a);
            int32_t cx, cy, cz;
            box_cell(a, k.cell, cx, cy, cz);
            const uint32_t ob = block_hash(cx >> 2, cy >> 2, cz >> 2, k.mask);
            const uint32_t s0 = k.s_start[ob], nloc = k.s_start[ob + 1] - s0;
            uint32_t w = 0;
            int64_t last = -1;                                           // research_body's search, from "nothing emitted yet"
            for (;;) {
                uint32_t best = 0xffffffffu;
                for (uint32_t e = 0; e < nloc + k.n_large; e++) {
                    const uint32_t sidx = e < nloc ? k.s_entries[s0 + e] : k.s_large[e - nloc];
                    if ((int64_t)sidx <= last || sidx >= best) continue;
                    double bs[6];
                    load_box(k.s_aabb, sidx, bs);
                    if (boxes_overlap(a, bs)) best = sidx;
                }
                if (best == 0xffffffffu) break;
                if (off + w < k.scapacity) out[off + w] = make_uint2(i, best);
                w++;
                last = best;
            }
        }
    }
}

// clapgpu_bp_index's fourth launch: the indexed boxes' bounds and "an edge exceeds `limit`" into the index's own control
// words (bp_grid.h), which the host set to all ones in front of it.  limit: the cell of a one-level object, the top
// level's cell of a leveled one.  The sticky bit 0 of CTRL_STATUS is not this flag: it reports any oversized box since the
// object was made, this one the boxes of the current index only.
constexpr int BP_BOUNDS_BLOCKS = 512;
__global__ __launch_bounds__(PB)
void k_bp_index_bounds(BpK k, double limit)
{
    __shared__ double red[6][PB / WAVE];
    __shared__ uint32_t big[PB / WAVE];
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    double m[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };     // min xyz, max xyz
    uint32_t over = 0;
    for (uint32_t i = blockIdx.x * PB + threadIdx.x; i < k.n; i += gridDim.x * PB) {
        double bb[6];
        load_box(k.aabb, i, bb);
        if (box_oversized(bb, limit)) over = 1;
        // finite coordinates only: a geom at infinity or NaN never hits (ray_colliders_dev.h), and the bounds stay finite
        for (int a = 0; a < 3; a++) {
            if (isfinite(bb[2 * a])) m[a] = fmin(m[a], bb[2 * a]);
            if (isfinite(bb[2 * a + 1])) m[3 + a] = fmax(m[3 + a], bb[2 * a + 1]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        for (int a = 0; a < 3; a++) { m[a] = fmin(m[a], __shfl_xor(m[a], o)); m[3 + a] = fmax(m[3 + a], __shfl_xor(m[3 + a], o)); }
        over |= __shfl_xor(over, o);
    }
    if (lane == 0) {
        for (int a = 0; a < 6; a++) red[a][wave] = m[a];
        big[wave] = over;
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0)                             // the grid this index looked at (stream order: after its bins)
        k.ctrl[CTRL_INDEX_EPOCH] = k.ctrl[CTRL_EPOCH];
    if (threadIdx.x < 7) {
        unsigned long long *w = reinterpret_cast<unsigned long long *>(k.ctrl + CTRL_INDEX_WORD);
        const int a = threadIdx.x;
        if (a == INDEX_OVERSIZE) {
            uint32_t o = 0;
            for (int q = 0; q < PB / WAVE; q++) o |= big[q];
            if (o) atomicMin(&w[INDEX_OVERSIZE], 0ull);
        } else {
            double v = red[a][0];
            for (int q = 1; q < PB / WAVE; q++) v = a < 3 ? fmin(v, red[a][q]) : fmax(v, red[a][q]);
            if (a < 3 ? v < INFINITY : v > -INFINITY)                         // not the identity: this block has a box (NaN skipped)
                atomicMin(&w[a], a < 3 ? order_key(v) : ~order_key(v));
        }
    }
}

} // namespace clapgpu

using namespace clapgpu;

// ---------------------------------------------------------------------------------- launches, and the bookkeeping of struct clapgpu_bp (bp_object.h) they keep
// The boxes a step pre-binned were changed by somebody else (clapgpu_bodies_aabb, an upload, another body count): the cell
// counters go back to zero -- what k_bp_cells leaves between frames -- and the next collide bins for itself.
extern "C" int clapgpu_bp_invalidate(void *stream, clapgpu_bp *bp)
{
    if (!bp) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    bp->indexed = false;
    if (!bp->prebinned_aabb) return CLAPGPU_OK;
    bp->prebinned_aabb = nullptr; bp->prebinned_n = 0;
    CLAPGPU_HIP(hipMemsetAsync(bp->k.cell_cnt, 0, (size_t)bp->buckets * 64 * sizeof(uint32_t), as_stream(stream)));
    return CLAPGPU_OK;
}

// The object's kernel arguments for the n boxes of `aabb`
static BpK grid_k(const clapgpu_bp *bp, uint32_t n, const double *aabb)
{
    BpK k = bp->k;
    k.n = n; k.aabb = aabb; k.n_tiles = (n + BP_EMIT_TILE - 1) / BP_EMIT_TILE;
    return k;
}

static BplK bpl_k(const clapgpu_bp *bp, const BpK &k)
{
    BplK q;
    q.k = k; q.levels = bp->levels;
    for (uint32_t l = 0; l <= CLAPGPU_BP_LEVELS_MAX; l++) q.large_start[l] = bp->st.large_start[l];
    return q;
}

static int launch_bin(hipStream_t s, const BpK &k)
{
    hipLaunchKernelGGL(k_bp_bin, dim3((k.n + PB - 1) / PB), dim3(PB), 0, s, k);
    CLAPGPU_LAUNCH_CHECK("k_bp_bin");
    return CLAPGPU_OK;
}

// Launches 1 to 3: the grid of k's boxes in cell order.  Launch 1 is skipped when the step that wrote these boxes binned
// them (clapgpu_bodies_step_prebin; returned in *prebinned, and used up if `consume`: k_bp_cells zeroes the counters);
// a prebin for other boxes is undone first.
static int build_grid(void *stream, clapgpu_bp *bp, const BpK &k, bool consume, bool *prebinned)
{
    hipStream_t s = as_stream(stream);
    *prebinned = bp->prebinned_aabb == k.aabb && bp->prebinned_n == k.n;
    if (*prebinned) {
        if (consume) { bp->prebinned_aabb = nullptr; bp->prebinned_n = 0; }
    } else {
        if (bp->prebinned_aabb) {                                // binned for other boxes: undo
            int rc = clapgpu_bp_invalidate(stream, bp);
            if (rc) return rc;
        }
        int rc = launch_bin(s, k);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_bp_cells, dim3((bp->buckets + BP_CELLS_BLOCK / WAVE - 1) / (BP_CELLS_BLOCK / WAVE)), dim3(BP_CELLS_BLOCK), 0, s, k);
    CLAPGPU_LAUNCH_CHECK("k_bp_cells");
    hipLaunchKernelGGL(k_bp_scatter, dim3((k.n + PB - 1) / PB), dim3(PB), 0, s, k);
    CLAPGPU_LAUNCH_CHECK("k_bp_scatter");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_bp_collide(void *stream, clapgpu_bp *bp, uint32_t n, const double *aabb,
                                  uint32_t *pairs, uint32_t capacity, uint32_t *pair_total,
                                  uint32_t *static_pairs, uint32_t static_capacity, uint32_t *static_pair_total)
{
    if (!bp || !pair_total || (n && !aabb) || (capacity && !pairs) || (static_capacity && !static_pairs))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (n > bp->n_max) return CLAPGPU_ERR_TOO_LARGE;
    bp->indexed = false;                                         // collide rebins: an index it leaves behind is not kept
    hipStream_t s = as_stream(stream);
    const bool statics = bp->n_static && static_pair_total;
    if (n == 0) {
        CLAPGPU_HIP(hipMemsetAsync(pair_total, 0, sizeof(uint32_t), s));
        if (static_pair_total) CLAPGPU_HIP(hipMemsetAsync(static_pair_total, 0, sizeof(uint32_t), s));
        return clapgpu_bp_invalidate(stream, bp);
    }
    BpK k = grid_k(bp, n, aabb);
    k.pairs = pairs; k.capacity = capacity; k.pair_total = pair_total;
    k.spairs = static_pairs; k.scapacity = static_capacity; k.spair_total = static_pair_total;
    if (!statics) { k.n_static = 0; k.n_large = 0; if (static_pair_total) CLAPGPU_HIP(hipMemsetAsync(static_pair_total, 0, 4, s)); }
    if (bp->levels > 1) {                                        // bp_levels.hip's kernels around the shared k_bp_cells
        int rc = clapgpu_bpl_bin(s, bpl_k(bp, k));
        if (rc) return rc;
        hipLaunchKernelGGL(k_bp_cells, dim3((bp->buckets + BP_CELLS_BLOCK / WAVE - 1) / (BP_CELLS_BLOCK / WAVE)), dim3(BP_CELLS_BLOCK), 0, s, k);
        CLAPGPU_LAUNCH_CHECK("k_bp_cells");
        return clapgpu_bpl_pairs(s, bpl_k(bp, k));
    }
    bool prebinned;
    int rc = build_grid(stream, bp, k, true, &prebinned);
    if (rc) return rc;
    hipLaunchKernelGGL(k_bp_search, dim3((n + (PB / WAVE) * BP_TILE - 1) / ((PB / WAVE) * BP_TILE)), dim3(PB), 0, s, k);
    CLAPGPU_LAUNCH_CHECK("k_bp_search");
    hipLaunchKernelGGL(k_bp_emit, dim3(k.n_tiles), dim3(BP_EMIT_TILE), 0, s, k);
    CLAPGPU_LAUNCH_CHECK("k_bp_emit");
    return CLAPGPU_OK;
}

// bodies.hip's clapgpu_bodies_step_prebin (bp_grid.h)
__attribute__((visibility("hidden"))) int clapgpu_bp_prebin(void *stream, clapgpu_bp *bp, uint32_t n, const double *aabb, BinK *bin)
{
    if (n > bp->n_max) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (bp->levels > 1) {                                        // BinK bins one level: off, and no prebin recorded
        *bin = BinK{};
        return clapgpu_bp_invalidate(stream, bp);
    }
    *bin = bin_of(bp->k);
    if (n == 0) return CLAPGPU_OK;
    int rc = clapgpu_bp_invalidate(stream, bp);                  // the step moves the boxes and rebins: the index is stale; a step
    if (rc) return rc;                                           // binned already and no collide consumed it: start over
    bp->prebinned_aabb = aabb;
    bp->prebinned_n = n;
    return CLAPGPU_OK;
}

// The first three launches of clapgpu_bp_collide (the grid of the current boxes in cell order) and the bounds of those
// boxes: what clapgpu_ray_cast looks up.  The collide kernels are not run and keep their code.
// Boxes a step pre-binned are indexed WITHOUT using up the prebin: k_bp_cells zeroes the counters it reads, so the index
// bins the same boxes once more after its scatter.  The next collide -- eager, or captured in a graph whose collide has
// no bin launch (FrameLoop.capture with prebin) -- then finds the counters it expects.  Ranks inside a cell may come out
// in another order; the collide's lists are canonical whatever order the atomics took.
// A leveled object whose index is switched on (clapgpu_bp_leveled_index) runs the same four launches with bp_levels.hip's
// bin and scatter around k_bp_cells; it is never pre-binned, so nothing is binned back, and the bounds launch tests the
// edges against the top level's cell.  Switched off (as created) it launches nothing and the queries scan.
extern "C" int clapgpu_bp_index(void *stream, clapgpu_bp *bp, uint32_t n, const double *aabb)
{
    if (!bp || (n && !aabb)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (n > bp->n_max) return CLAPGPU_ERR_TOO_LARGE;
    bp->indexed = false;
    if (bp->levels > 1 && !bp->leveled_index) {                  // no index asked for: nothing is launched, queries scan
        bp->indexed = true; bp->indexed_aabb = aabb; bp->indexed_n = n;       // (clapgpu_bp_index_status: bit 2)
        return CLAPGPU_OK;
    }
    hipStream_t s = as_stream(stream);
    const BpK k = grid_k(bp, n, aabb);
    CLAPGPU_HIP(hipMemsetAsync(k.ctrl + CTRL_INDEX_WORD, 0xff, INDEX_WORDS * sizeof(uint64_t), s));
    const uint32_t bounds_blocks = (n + PB - 1) / PB < BP_BOUNDS_BLOCKS ? (n + PB - 1) / PB : BP_BOUNDS_BLOCKS;
    if (n && bp->levels > 1) {
        const BplK q = bpl_k(bp, k);
        int rc = clapgpu_bpl_bin(s, q);
        if (rc) return rc;
        hipLaunchKernelGGL(k_bp_cells, dim3((bp->buckets + BP_CELLS_BLOCK / WAVE - 1) / (BP_CELLS_BLOCK / WAVE)), dim3(BP_CELLS_BLOCK), 0, s, k);
        CLAPGPU_LAUNCH_CHECK("k_bp_cells");
        rc = clapgpu_bpl_scatter(s, q);
        if (rc) return rc;
        hipLaunchKernelGGL(k_bp_index_bounds, dim3(bounds_blocks), dim3(PB), 0, s, k, ldexp(bp->cell, (int)bp->levels - 1));
        CLAPGPU_LAUNCH_CHECK("k_bp_index_bounds");
    } else if (n) {
        bool prebinned;
        int rc = build_grid(stream, bp, k, false, &prebinned);
        if (rc) return rc;
        if (prebinned) {                                         // the counters back, as the prebinning step left them
            rc = launch_bin(s, k);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(k_bp_index_bounds, dim3(bounds_blocks), dim3(PB), 0, s, k, k.cell);
        CLAPGPU_LAUNCH_CHECK("k_bp_index_bounds");
    } else {
        int rc = clapgpu_bp_invalidate(stream, bp);              // no boxes: every cell is empty, as k_bp_cells leaves them
        if (rc) return rc;
    }
    bp->indexed = true; bp->indexed_aabb = aabb; bp->indexed_n = n;
    return CLAPGPU_OK;
}
