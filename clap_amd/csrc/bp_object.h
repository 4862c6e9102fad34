// bp_object.h -- struct clapgpu_bp and the kernel arguments made from it.  PRIVATE to the broadphase translation
// units: bp_create.hip makes and hands out the object, broadphase.hip runs its kernels and keeps its bookkeeping,
// bp_restatic.hip registers its static boxes again (clapgpu_bp_statics_update) and reads an image back, bp_levels.hip
// holds the kernels of a leveled object (it sees the kernel arguments, never the object).
// struct clapgpu_bp is written and read in the first three files alone; others go through the hidden accessors of bp_grid.h.
#pragma once
#include "common.h"
#include "bp_grid.h"
#include "bp_levels.h"

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
    // statics (binned on the host at create time; again on the device by clapgpu_bp_statics_update, which repoints these)
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

// A leveled object's kernel arguments (bp_levels.hip): BpK with one statics CSR per level laid end to end -- level l's
// starts are s_start[l * (buckets + 1) ..], already offset into the shared s_entries / s_recs -- and level l's large
// statics at s_large / s_lrecs[large_start[l] .. large_start[l + 1]).  k.cell is level 0's cell.
struct BplK {
    BpK k;
    uint32_t levels;
    uint32_t large_start[CLAPGPU_BP_LEVELS_MAX + 1];
};

// The statics image the object answers with (its arrays: the k.s_* but k.s_aabb), written by bp_adopt_statics alone ...
struct BpStatics {
    uint32_t n_entries, n_large;                   // of k.s_entries / k.s_recs and k.s_large / k.s_lrecs (n_large is k.n_large)
    uint32_t large_start[CLAPGPU_BP_LEVELS_MAX + 1];   // level l's large statics: [l] .. [l + 1]; ONE level: all zero (clapgpu.h)
    double bounds[6];                              // union of the registered (not large) boxes: min xyz, max xyz; min > max: none
    // ... and where clapgpu_bp_statics_update builds the next: its allocation (none until the first update; the create-time
    // image inside `dev` is then no longer pointed at), the allocation's room, and the slot of its two that k.s_* point into
    void *dev2;
    uint32_t cap_entries, cap_large;
    int slot;
};

} // namespace clapgpu

// bp_levels.hip, for clapgpu_bp_collide on a leveled object: launch 1 (bin), and launches 3 to 5 (scatter, search, emit);
// launch 2 in between is broadphase.hip's k_bp_cells, which reads slots and knows no level.  clapgpu_bp_index with the
// leveled index switched on runs launch 1, k_bp_cells and launch 3 alone (clapgpu_bpl_scatter).
__attribute__((visibility("hidden"))) int clapgpu_bpl_bin(hipStream_t s, const clapgpu::BplK &q);
__attribute__((visibility("hidden"))) int clapgpu_bpl_scatter(hipStream_t s, const clapgpu::BplK &q);
__attribute__((visibility("hidden"))) int clapgpu_bpl_pairs(hipStream_t s, const clapgpu::BplK &q);

struct clapgpu_bp {
    uint32_t n_max, buckets, n_static, n_tiles;
    uint32_t levels;               // 1: the one-level grid of broadphase.hip; more: bp_levels.hip's kernels
    bool leveled_index;            // clapgpu_bp_leveled_index: levels > 1 and clapgpu_bp_index builds an index (off: queries scan)
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
    clapgpu::BpStatics st;
};

// The object answers with this image (create's and every update's): its arrays, registrations, large ends per level, bounds
static inline void bp_adopt_statics(clapgpu_bp *bp, const uint32_t *start, const uint32_t *entries, const uint32_t *large,
                                    const clapgpu::GridRec *recs, const clapgpu::GridRec *lrecs, uint32_t n_entries,
                                    const uint32_t *large_end, const double *bounds)
{
    clapgpu::BpK &k = bp->k;
    k.s_start = start; k.s_entries = entries; k.s_large = large; k.s_recs = recs; k.s_lrecs = lrecs;
    bp->st.n_entries = n_entries;
    bp->st.n_large = k.n_large = large_end[bp->levels - 1];
    if (bp->levels > 1)                                                  // a one-level object keeps large_start all zero
        for (uint32_t l = 0; l < bp->levels; l++) bp->st.large_start[l + 1] = large_end[l];
    for (int a = 0; a < 6; a++) bp->st.bounds[a] = bounds[a];
}
