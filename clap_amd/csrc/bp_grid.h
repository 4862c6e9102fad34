// bp_grid.h -- the broadphase's hash grid as other translation units see it: the cell and slot functions the five k_bp_*
// launches bin with (physics2.hip) and the ray cast looks cells up with (rays.hip), and a read-only view of an INDEXED
// clapgpu_bp (clapgpu_bp_index), handed out by a hidden accessor in physics2.hip.
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

__host__ __device__ __forceinline__ uint32_t cell_slot(int32_t cx, int32_t cy, int32_t cz, uint32_t mask)
{
    return block_hash(cx >> 2, cy >> 2, cz >> 2, mask) << 6 | (uint32_t)(cx & 3) | (uint32_t)(cy & 3) << 2 | (uint32_t)(cz & 3) << 4;
}

// physics2.hip's BpRec, field for field (static_assert there)
struct GridRec { double bb[6]; uint32_t idx; int32_t cell[3]; };

// Control words of the index (clapgpu_bp.ctrl has 160; the broadphase uses 2, 3, 8 and 9).  Seven 64-bit words, all
// reduced by atomicMin and set to all ones in front of the reduction: the indexed boxes' minimum corner as order keys,
// the maximum corner as complemented order keys, and a word that drops to 0 when a box edge exceeds `cell`.
constexpr int CTRL_BIN_EPOCH = 3;                 // physics2.hip's CTRL_EPOCH
constexpr int CTRL_INDEX_WORD = 16;
constexpr int INDEX_WORDS = 7, INDEX_OVERSIZE = 6;
// ... and the bin epoch (ctrl[3], counted up by every bin pass on the device, k_bp_bin or a prebinning step) the index
// saw last.  A graph replay bins without the host knowing; a differing epoch tells the ray kernel the index is stale.
constexpr int CTRL_INDEX_EPOCH = CTRL_INDEX_WORD + 2 * INDEX_WORDS;       // word 30

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
};

} // namespace clapgpu

struct clapgpu_bp;
// true when `bp` holds an index over exactly (n, aabb) (aabb == nullptr: any array of n boxes); fills *v
__attribute__((visibility("hidden"))) bool clapgpu_bp_grid_view(const clapgpu_bp *bp, uint32_t n, const double *aabb, clapgpu::BpGridView *v);
