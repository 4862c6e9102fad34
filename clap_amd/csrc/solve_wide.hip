// solve_wide.hip -- the contact solve's sweep for a large island on gfx950: one 256-thread workgroup walks the island's
// rows in dependency levels instead of one lane walking them one by one (solve.hip; the rule: include/clapgpu.h).
//
// The canonical row order matters only between rows that share a body.  level = 1 + the highest level among the earlier
// rows of the island that name one of the row's bodies (0 when none does) makes rows of one level name disjoint bodies,
// and running level 1, 2, ... with a barrier between them gives every row exactly the operands the sequential walk
// gives it: the same statements (relax_row, solve_dev.h) on the same values, no sum reordered.
//   levels   the workgroup's first wavefront, 64 rows of the run at a time: one gather of last_level[] of the rows'
//            bodies, then 64 broadcasts (lane k's bodies and its by then final level) resolve the chunk's own
//            dependencies -- a later lane sharing a body raises its level, an earlier lane sharing a body gives up its
//            write-back -- and one write-back, the chunk's last row naming a body writing its level
//   buckets  rows per level counted, prefixed and the row ordinals scattered into level order inside the island's own
//            slice (the order within a level is free: its rows touch disjoint words)
//   sweeps   `iterations` times every level, the threads striding over the level's rows, __syncthreads() behind each
// a, lambda and the work arrays stay in global scratch.  The waves of a workgroup share one CU and its L1, so
// __syncthreads() -- a workgroup-scope fence and a barrier -- hands them over: no agent-scope fence, no flag, no polling,
// no word shared between workgroups (islands are disjoint in bodies and in their slices).  Every loop that holds a
// barrier takes its trip count from words the whole workgroup reads identically before it: the list's length, the
// run's length, the level count (through LDS, behind a barrier) and `iterations`.
// fp64, no FMA contraction (the Makefile builds with -ffp-contract=off).
#include "solve_dev.h"

namespace clapgpu {

// a word other threads change with atomics: read where the atomics act
__device__ __forceinline__ uint32_t load_word(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t lane_word(uint32_t v, uint32_t k)   // lane k's v, k the same in every lane
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)k);
}

// The levels of the run [start, start + len) of sorted keys, by one whole wavefront; returns the number of levels.
__device__ __forceinline__ uint32_t wave_levels(uint32_t start, uint32_t len, const uint64_t *keys, const SolveWide &w,
                                                uint32_t *row_level)
{
    const uint32_t lane = lane_id();
    uint32_t top = 0;
    uint32_t r = 0, b1 = NONE, b2 = NONE;                                   // this lane's row of the chunk and its bodies
    if (lane < len) {
        r = (uint32_t)keys[start + lane];
        const uint2 bb = w.row_bodies[r];
        b1 = bb.x; b2 = bb.y;
    }
    for (uint32_t c0 = 0; c0 < len; c0 += WAVE) {
        const uint32_t j = c0 + lane, m = len - c0 < WAVE ? len - c0 : WAVE;
        const bool in = j < len, more = j + WAVE < len && j + WAVE > j;
        const uint32_t nr = more ? (uint32_t)keys[start + j + WAVE] : 0u;   // the next chunk's rows wait for nothing of this one:
        uint32_t l = 0;                                                     // their two round trips pass under this chunk's work
        if (in) {
            l = w.last_level[b1];
            if (b2 != NONE) {
                const uint32_t l2 = w.last_level[b2];
                if (l2 > l) l = l2;
            }
            l += 1;
        }
        const uint2 nb = more ? w.row_bodies[nr] : make_uint2(NONE, NONE);
        bool keep1 = in, keep2 = in && b2 != NONE;                          // this row is the chunk's last to name the body
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t k1 = lane_word(b1, k), k2 = lane_word(b2, k), kl = lane_word(l, k);     // kl is final: lanes < k are done
            const bool s1 = b1 == k1 || (k2 != NONE && b1 == k2);
            const bool s2 = b2 != NONE && (b2 == k1 || b2 == k2);
            if (lane > k) {
                if ((s1 || s2) && kl + 1 > l) l = kl + 1;
            } else if (lane < k) {
                if (s1) keep1 = false;
                if (s2) keep2 = false;
            }
        }
        if (l > len) l = len;                                               // (cannot be: a level holds a row of the run)
        if (keep1) w.last_level[b1] = l;
        if (keep2) w.last_level[b2] = l;
        if (in) {
            w.level[start + j] = l;
            if (row_level) row_level[r] = l;
            if (l > top) top = l;
        }
        wave_lds_fence();                                                   // the write-back lands before the next gather
        r = nr; b1 = nb.x; b2 = nb.y;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(top, off);
        if (o > top) top = o;
    }
    return top;
}

__global__ __launch_bounds__(SB)
void k_solve_sweep_wide(uint32_t rows_capacity, uint32_t iterations, const uint32_t *ctl, const uint64_t *keys,
                        const SolveRow *__restrict__ rows, SolveWide w, double *lam, double *a, uint32_t *row_level,
                        uint32_t *wide_total)
{
    __shared__ uint32_t lds[SB / WAVE];
    __shared__ uint32_t s_levels;
    if (ctl[0] > rows_capacity) return;                                     // the whole workgroup, before its first barrier
    const uint32_t islands = ctl[1] < rows_capacity ? ctl[1] : rows_capacity;          // (an island has a row: it cannot be more)
    if (blockIdx.x == 0 && threadIdx.x == 0 && wide_total) *wide_total = islands;
    for (uint32_t isl = blockIdx.x; isl < islands; isl += gridDim.x) {
        const uint2 run = w.list[isl];
        const uint32_t start = run.x, len = run.y;
        if (start >= rows_capacity || len > rows_capacity - start) continue;                       // (cannot be: the list holds runs of keys)
        uint32_t *level = w.level + start, *cursor = w.cursor + start, *order = w.order + start;
        for (uint32_t j = threadIdx.x; j < len; j += SB) cursor[j] = 0;
        if (threadIdx.x < WAVE) {
            const uint32_t top = wave_levels(start, len, keys, w, row_level);
            if (threadIdx.x == 0) s_levels = top;
        }
        __syncthreads();
        const uint32_t levels = s_levels < len ? s_levels : len;            // (a level holds a row: it cannot be more)
        // rows per level, their prefix, the scatter
        for (uint32_t j = threadIdx.x; j < len; j += SB) atomicAdd(cursor + (level[j] - 1), 1u);
        __syncthreads();
        uint32_t base = 0;
        for (uint32_t tile = 0; tile < levels; tile += SB) {
            const uint32_t q = tile + threadIdx.x;
            const uint32_t c = q < levels ? load_word(cursor + q) : 0u;
            uint32_t tile_total;
            const uint32_t before = base + block_prefix(c, lds, tile_total);
            base += tile_total;
            if (q < levels) cursor[q] = before;
        }
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < len; j += SB) {
            const uint32_t at = atomicAdd(cursor + (level[j] - 1), 1u);
            if (at < len) order[at] = (uint32_t)keys[start + j];
        }
        __syncthreads();
        for (uint32_t q = threadIdx.x; q < levels; q += SB) level[q] = load_word(cursor + q);      // now: where level q + 1 ends
        __syncthreads();
        for (uint32_t it = 0; it < iterations; it++) {
            uint32_t from = 0;
            for (uint32_t q = 0; q < levels; q++) {
                uint32_t to = level[q];
                if (to > len) to = len;
                for (uint32_t j = from + threadIdx.x; j < to; j += SB) relax_row(rows, order[j], lam, a);
                __syncthreads();
                from = to;
            }
        }
    }
}

hipError_t solve_sweep_wide(hipStream_t s, uint32_t rows_capacity, uint32_t iterations, const uint32_t *ctl,
                            const uint64_t *keys, const SolveRow *rows, const SolveWide &w, double *lam, double *a,
                            uint32_t *row_level, uint32_t *wide_total)
{
    const uint32_t blocks = rows_capacity < SOLVE_WIDE_BLOCKS ? rows_capacity : SOLVE_WIDE_BLOCKS;
    hipLaunchKernelGGL(k_solve_sweep_wide, dim3(blocks), dim3(SB), 0, s, rows_capacity, iterations, ctl, keys, rows, w, lam, a,
                       row_level, wide_total);
    return launch_error();
}

} // namespace clapgpu
