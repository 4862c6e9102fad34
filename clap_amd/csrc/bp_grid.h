// bp_grid.h -- the broadphase's hash grid as other translation units see it: the cell and slot functions and the bin step
// that the five k_bp_* launches (broadphase.hip) and the pre-binning body step (bodies.hip) bin with and the device
// queries look cells up with (grid_query_dev.h, for rays.hip and slide.hip), the record and the control words of a
// clapgpu_bp, a read-only view of an INDEXED clapgpu_bp (clapgpu_bp_index), and the hidden accessors of the broadphase
// code (broadphase.hip, bp_create.hip, bp_restatic.hip) that hand these out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace clapgpu {

__host__ __device__ __forceinline__ uint32_t block_hash(int32_t bx, int32_t by, int32_t bz, uint32_t mask)
{
    const uint32_t h = ((uint32_t)bx * 73856093u) ^ ((uint32_t)by * 19349663u) ^ ((uint32_t)bz * 83492791u);
    return (h ^ (h >> 15)) & mask;
}

__host__ __device__ __forceinline__ int32_t cell_coord(double x, double cell)
{
    double c = floor(x / cell);
    if (!(c > -5.0e8)) c = -5.0e8;                                       // also catches NaN
    if (c > 5.0e8) c = 5.0e8;
    return (int32_t)c;
}

// Half a cell and a relative margin against the rounding of the sums it enters: what a static's registration (bp_statics.h),
// a query's range (grid_query_dev.h) and a finer body's coarse lookup (bp_levels.h) grow a box by.  They must agree.
__host__ __device__ __forceinline__ double half_cell_grown(double c) { return c * 0.5 * (1.0 + 1e-9); }

__host__ __device__ __forceinline__ uint32_t cell_slot(int32_t cx, int32_t cy, int32_t cz, uint32_t mask)
{
    return block_hash(cx >> 2, cy >> 2, cz >> 2, mask) << 6 | (uint32_t)(cx & 3) | (uint32_t)(cy & 3) << 2 | (uint32_t)(cz & 3) << 4;
}

struct GridRec { double bb[6]; uint32_t idx; int32_t cell[3]; };    // 64 bytes; cell = the box centre's cell (dynamic records)

// Control words.  The broadphase's: the sticky status bits, the bin epoch (the frame counter
// lives on the device: a captured graph replays the same arguments; counted up by every bin pass, k_bp_bin or a
// pre-binning step) and [8..9]: clapgpu_contacts_geoms_both's ticket + counts, zero between launches.
constexpr int CTRL_STATUS = 2, CTRL_EPOCH = 3, CTRL_CONTACT_WORD = 8;
// The index's: seven 64-bit words, all reduced by atomicMin and set to all ones in front of the reduction: the indexed
// boxes' minimum corner as order keys, the maximum corner as complemented order keys, and a word that drops to 0 when
// a box edge exceeds `cell`.
constexpr int CTRL_INDEX_WORD = 16;
constexpr int INDEX_WORDS = 7, INDEX_OVERSIZE = 6;
// ... and the bin epoch the index saw last.  A graph replay bins without the host knowing; a differing epoch tells a
// query kernel the index is stale (grid_query_dev.h's grid_usable).
constexpr int CTRL_INDEX_EPOCH = CTRL_INDEX_WORD + 2 * INDEX_WORDS;       // word 30
constexpr int CTRL_WORDS = 160;                                           // clapgpu_bp.ctrl: every index above is below this
static_assert(CTRL_INDEX_EPOCH < CTRL_WORDS, "control words");

// One body into the grid: k_bp_bin's work per body, also done by the step that writes the box it would read
// (clapgpu_bodies_step_prebin).  key == nullptr: off.
struct BinK { double cell; uint32_t mask; uint32_t *key, *rank, *cell_cnt, *ctrl; };

__device__ __forceinline__ void box_cell(const double (&bb)[6], double cell, int32_t &cx, int32_t &cy, int32_t &cz)
{
    cx = cell_coord((bb[0] + bb[1]) * 0.5, cell);
    cy = cell_coord((bb[2] + bb[3]) * 0.5, cell);
    cz = cell_coord((bb[4] + bb[5]) * 0.5, cell);
}

__device__ __forceinline__ void load_box(const double *aabb, uint32_t i, double (&bb)[6])
{
    const double2 *p = reinterpret_cast<const double2 *>(aabb + 6 * (size_t)i);
    const double2 a = p[0], b = p[1], c = p[2];
    bb[0] = a.x; bb[1] = a.y; bb[2] = b.x; bb[3] = b.y; bb[4] = c.x; bb[5] = c.y;
}

__device__ __forceinline__ bool boxes_overlap(const double (&a)[6], const double (&b)[6])
{
    return !(a[0] > b[1] || a[1] < b[0] || a[2] > b[3] || a[3] < b[2] || a[4] > b[5] || a[5] < b[4]);
}

// an edge exceeds `cell`: the box's partners may lie outside the 27 cells around its own
__device__ __forceinline__ bool box_oversized(const double (&bb)[6], double cell)
{
    return bb[1] - bb[0] > cell || bb[3] - bb[2] > cell || bb[5] - bb[4] > cell;
}

__device__ __forceinline__ void bin_body(const BinK &bin, uint32_t i, const double (&bb)[6])
{
    if (box_oversized(bb, bin.cell))
        atomicOr(&bin.ctrl[CTRL_STATUS], 1u);
    int32_t cx, cy, cz;
    box_cell(bb, bin.cell, cx, cy, cz);
    const uint32_t slot = cell_slot(cx, cy, cz, bin.mask);
    bin.key[i] = slot;
    bin.rank[i] = atomicAdd(&bin.cell_cnt[slot], 1u);
}

__host__ __device__ __forceinline__ uint64_t order_key(double x)              // monotone in x (not for NaN)
{
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}

__host__ __device__ __forceinline__ double order_value(uint64_t k)
{
    return __builtin_bit_cast(double, (k >> 63) ? (k & ~(1ull << 63)) : ~k);
}

struct BpGridView {
    uint32_t n;                          // boxes indexed (0: the cell ranges are not written)
    uint32_t n_static;
    double cell;
    uint32_t mask;                       // block buckets - 1
    uint32_t n_large;
    const uint2 *cell_range;             // [buckets * 64] (first record, records) per cell slot
    const GridRec *recs;                 // the indexed boxes in cell order
    const uint32_t *s_start;             // [buckets + 1] statics registered per block bucket
    const GridRec *s_recs, *s_lrecs;     // their records; the large statics (tested by every ray)
    const uint64_t *index;               // INDEX_WORDS control words of the index
    const uint32_t *ctrl;                // the object's control words (epochs)
    double s_bounds[6];                  // union of the registered (not large) statics' boxes; min > max: none
    // a leveled object (bp_levels.h; 1: none of this is read): cell is level 0's, the bodies' records carry their level,
    // s_start holds one CSR of buckets + 1 starts per level, and the queries read level s_level's
    uint32_t levels, s_level;
    uint32_t large_first;                // the large statics are s_lrecs[large_first .. large_first + n_large) (level s_level's; one level: 0)
};

} // namespace clapgpu

// ---- the broadphase's hidden accessors: struct clapgpu_bp (bp_object.h) is written and read in broadphase.hip,
// bp_create.hip and bp_restatic.hip alone
struct clapgpu_bp;
// geoms_dev.h's scene_grid, for rays.hip and slide.hip: true when `bp` holds an index over exactly (n, aabb) (aabb == nullptr: any array of n boxes); fills *v
__attribute__((visibility("hidden"))) bool clapgpu_bp_grid_view(const clapgpu_bp *bp, uint32_t n, const double *aabb, clapgpu::BpGridView *v);
// ... and whether `bp` (not NULL) is a leveled object with its index switched off (clapgpu_bp_leveled_index): it never holds a view
__attribute__((visibility("hidden"))) bool clapgpu_bp_scans(const clapgpu_bp *bp);
// contacts.hip (k_contacts_geoms_both): the one-launch form keeps its ticket + counts in the object's control words
__attribute__((visibility("hidden"))) unsigned long long *clapgpu_bp_contact_ticket(clapgpu_bp *bp);
// bodies.hip: the bin arrays for a step that is about to write and bin the n boxes of `aabb`, recorded as pre-binned
// (an unconsumed prebin is undone first, an index dropped).  The caller launches that step or calls clapgpu_bp_invalidate.
__attribute__((visibility("hidden"))) int clapgpu_bp_prebin(void *stream, clapgpu_bp *bp, uint32_t n, const double *aabb, clapgpu::BinK *bin);
