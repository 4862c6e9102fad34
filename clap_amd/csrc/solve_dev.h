// solve_dev.h -- what the two sweeps of the contact solve share (solve.hip: one lane per island; solve_wide.hip: one
// workgroup per island, level by level): the row record, the update of one row -- stated here alone, so both paths run
// the same statements and give the same bits -- and the workgroup prefix.
#pragma once
#include "common.h"

namespace clapgpu {

constexpr int SB = 256;
constexpr uint32_t NONE = 0xffffffffu;
constexpr uint32_t SOLVE_WIDE_BLOCKS = CLAPGPU_SOLVE_WIDE_WORKGROUPS;     // the wide sweep's grid (include/clapgpu.h)

struct SolveRow {                                       // 240 bytes; b1 == NONE: dropped (d == 0)
    double J[12], iMJ[12];
    double rhs, Ad, cfmh, lo, hi;
    uint32_t b1, b2;                                    // b2 == NONE: a static or a mesh on the other side
};

// exclusive prefix of v over the workgroup; total: the workgroup's sum
__device__ __forceinline__ uint32_t block_prefix(uint32_t v, uint32_t *lds, uint32_t &total)
{
    const uint32_t incl = wave_prefix_sum(v);
    const int wave = threadIdx.x / WAVE;
    __syncthreads();
    if (lane_id() == WAVE - 1) lds[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < SB / WAVE; k++) {
        const uint32_t t = lds[k];
        if (k < wave) base += t;
        total += t;
    }
    return base + incl - v;
}

// One row of one sweep: delta from lambda and the a of its bodies, the clamp, a += iMJ dlambda.  It reads and writes
// lam[r] and the six doubles of the row's one or two bodies, nothing else.
__device__ __forceinline__ void relax_row(const SolveRow *__restrict__ rows, uint32_t r, double *lam, double *a)
{
    const SolveRow *R = rows + r;
    const uint32_t b1 = R->b1, b2 = R->b2;
    if (b1 == NONE) return;                                                 // dropped: lambda stays 0
    double *a1 = a + 6 * (size_t)b1, *a2 = a + 6 * (size_t)(b2 == NONE ? b1 : b2);
    double x[12], J[12], iMJ[12];
#pragma unroll
    for (int q = 0; q < 12; q++) { J[q] = R->J[q]; iMJ[q] = R->iMJ[q]; }
#pragma unroll
    for (int q = 0; q < 6; q++) { x[q] = a1[q]; x[6 + q] = a2[q]; }
    double Ja = J[0] * x[0];
#pragma unroll
    for (int q = 1; q < 6; q++) Ja += J[q] * x[q];
    if (b2 != NONE) {
#pragma unroll
        for (int q = 6; q < 12; q++) Ja += J[q] * x[q];
    }
    const double l = lam[r];
    const double delta = R->Ad * ((R->rhs - R->cfmh * l) - Ja);
    double nl = l + delta;
    if (nl < R->lo) nl = R->lo;
    if (nl > R->hi) nl = R->hi;
    const double dl = nl - l;
#pragma unroll
    for (int q = 0; q < 6; q++) a1[q] = x[q] + iMJ[q] * dl;
    if (b2 != NONE) {
#pragma unroll
        for (int q = 0; q < 6; q++) a2[q] = x[6 + q] + iMJ[6 + q] * dl;
    }
    lam[r] = nl;
}

// what the wide sweep works in, all inside the solve's scratch (solve.hip carves it)
struct SolveWide {
    const uint2 *row_bodies;                            // [rows] the bodies of every row, a dropped row's too (y == NONE: none)
    uint2 *list;                                        // [rows] (start, length) of every wide island's run of sorted keys
    uint32_t *last_level;                               // [n] the level of the latest row that named the body; 0: none yet
    uint32_t *level, *cursor, *order;                   // [rows] each, an island using the slice of its run
};

// solve_wide.hip: the islands k_solve_sweep listed (ctl[1] of them), each by one workgroup
__attribute__((visibility("hidden"))) hipError_t solve_sweep_wide(hipStream_t s, uint32_t rows_capacity, uint32_t iterations,
                                                                  const uint32_t *ctl, const uint64_t *keys, const SolveRow *rows,
                                                                  const SolveWide &w, double *lam, double *a, uint32_t *row_level,
                                                                  uint32_t *wide_total);

} // namespace clapgpu
