// bp_object.h -- struct clapgpu_bp and the kernel arguments made from it.  PRIVATE to the two broadphase translation
// units: bp_create.hip makes and hands out the object, broadphase.hip runs its kernels and keeps its bookkeeping.
// struct clapgpu_bp is written and read in those two files alone; others go through the hidden accessors of bp_grid.h.
#pragma once
#include "common.h"
#include "bp_grid.h"

namespace clapgpu {

constexpr int BP_LIST = 16;            // partners kept per body in its fixed slot
constexpr int BP_EMIT_TILE = 1024;     // bodies per tile of the pair-offset scan (= emit block; 256: +3 us, four times the look-back words)

struct BpK {
    uint32_t n;
    double cell;
    uint32_t mask;                       // block buckets - 1
    const double *aabb;
    uint32_t *cell_cnt;                  // [buckets * 64] the bin pass's counters, zero between frames
    uint2    *cell_range;                // [buckets * 64] (first position in cell order, bodies) of every cell: one load per lookup
    uint32_t *key, *rank;                // [n] cell slot and rank inside the cell
    uint32_t *entries;                   // [n] body indices in cell order
    GridRec *recs;                  // [n] the same with the boxes: what the search reads
    uint32_t *cnt, *scnt;                // [n] partners (larger index) / statics per body: atomics in the search
    uint32_t *partners, *spartners;      // [n][BP_LIST]
    uint64_t *lb_body, *lb_static;       // [tiles] look-back words of the pair-offset scan (k_bp_emit)
    uint64_t *lb_cells;                  // [buckets / 4] look-back words of the block-start scan (k_bp_cells)
    uint32_t *ctrl;                      // [CTRL_WORDS]
    uint32_t n_tiles;
    // statics (binned on the host at create time)
    const uint32_t *s_start;             // [buckets + 1]
    const uint32_t *s_entries;
    const double *s_aabb;
    const uint32_t *s_large;
    const GridRec *s_recs;          // s_entries with their boxes (what the search gathers)
    const GridRec *s_lrecs;         // the large statics with their boxes
    uint32_t n_large, n_static;
    // outputs
    uint32_t *pairs, capacity, *pair_total;
    uint32_t *spairs, scapacity, *spair_total;
};

// the words a bin pass works on: what k_bp_bin uses and what clapgpu_bp_prebin hands to the pre-binning body step
__host__ __device__ __forceinline__ BinK bin_of(const BpK &k) { return BinK{ k.cell, k.mask, k.key, k.rank, k.cell_cnt, k.ctrl }; }

} // namespace clapgpu

struct clapgpu_bp {
    uint32_t n_max, buckets, n_static, n_large, n_tiles;
    double cell;
    void *dev;                     // one allocation
    clapgpu::BpK k;                // device pointers filled in
    // clapgpu_bodies_step_prebin: the step that wrote these boxes has also binned them (key / rank / cell counters / epoch):
    // the next clapgpu_bp_collide over the same array skips its first launch
    const double *prebinned_aabb;
    uint32_t prebinned_n;
    // clapgpu_bp_index: the grid now describes these boxes (cleared by everything that bins again)
    bool indexed;
    const double *indexed_aabb;
    uint32_t indexed_n;
    double s_bounds[6];            // union of the statics registered per block (not the large list); min > max: none
};
