// bp_levels.h -- the multi-level form of the broadphase's hash grid (clapgpu_bp_create_levels): the level of a box, the
// slot of a (level, cell) and the cells a finer body looks up on a coarser level.  Host and device; the kernels are
// bp_levels.hip's, the one-level grid (bp_grid.h, broadphase.hip) is not touched by any of this.
//
// Level l (0 .. levels - 1) has cell size cell * 2^l (exact in fp64).  A body lives on the LOWEST level whose cell is
// not smaller than its largest AABB edge, and is binned there by its box centre, as on the one-level grid.
//   same level     today's rule: the own cell (partners with a larger index) and the 13 cells after it
//   coarser level  a pair of different levels is owned by its FINER member, which looks up, on every coarser level L,
//                  the cells met by its own box grown by half of level L's cell, both ends inclusive.
// Why those cells hold every partner: a partner on level L has edges of at most cell_L and is binned by its centre, so
// its box lies within its centre's cell grown by cell_L / 2; a box that meets it therefore comes within cell_L / 2 of
// that cell.  The finer box has edges of at most cell_L / 2, so grown it spans at most 1.5 cells: 2 cells an axis in
// most positions and never more than 3.
// A slot is shared by cells of any level (slot = hash(level, block) << 6 | cell in block), and unlike on the one-level
// grid a record from another cell that shares the slot CAN overlap the searcher (a level-0 neighbour in the slot a
// level-2 lookup reads) and would then be found twice: every leveled lookup rejects records whose (level, cell) is not
// the cell looked up.  The level rides in the top four bits of GridRec::idx (and of the bin key): n_max <= 2^28.
#pragma once
#include "clapgpu.h"
#include "bp_grid.h"

namespace clapgpu {

constexpr uint32_t BPL_LEVEL_SHIFT = 28, BPL_IDX = (1u << BPL_LEVEL_SHIFT) - 1u;   // GridRec::idx = index | level << 28
static_assert(CLAPGPU_BP_LEVELS_MAX <= (1u << (32 - BPL_LEVEL_SHIFT)), "the level's bits");

// The level of a box and that level's cell size: compared level by level against cell * 2^l (no logarithm): an edge equal
// to cell * 2^l is level l, a NaN edge fits level 0.  *over: an edge exceeds the top level's cell (status bit 0).
__host__ __device__ __forceinline__ uint32_t box_level(const double (&bb)[6], double cell, uint32_t levels, double *cell_l, bool *over)
{
    const double ex = bb[1] - bb[0], ey = bb[3] - bb[2], ez = bb[5] - bb[4];
    uint32_t l = 0;
    double c = cell;
    while (l + 1 < levels && (ex > c || ey > c || ez > c)) { l++; c *= 2.0; }
    *cell_l = c;
    *over = ex > c || ey > c || ez > c;
    return l;
}

__host__ __device__ __forceinline__ uint32_t level_slot(uint32_t level, int32_t cx, int32_t cy, int32_t cz, uint32_t mask)
{
    const uint32_t h = ((uint32_t)(cx >> 2) * 73856093u) ^ ((uint32_t)(cy >> 2) * 19349663u) ^ ((uint32_t)(cz >> 2) * 83492791u) ^
                       (level * 2654435761u);
    return ((h ^ (h >> 15)) & mask) << 6 | (uint32_t)(cx & 3) | (uint32_t)(cy & 3) << 2 | (uint32_t)(cz & 3) << 4;
}

// The cells [lo, hi] of one axis that a finer body's extent [a0, a1] looks up on a coarser level of cell size c.  The
// half cell is half_cell_grown (bp_grid.h), the one the statics' registration grows a box by: a rounded centre cannot
// drop a touching partner.  Never more than 3 cells (above); the clamp only bounds the walk of a box that is not a number.
__host__ __device__ __forceinline__ void coarse_cells(double a0, double a1, double c, int32_t *lo, int32_t *hi)
{
    const double grow = half_cell_grown(c);
    *lo = cell_coord(a0 - grow, c);
    *hi = cell_coord(a1 + grow, c);
    if (*hi > *lo + 2) *hi = *lo + 2;
}

// The level S whose statics image the QUERIES through a leveled index read (grid_query_dev.h), counted down from the top
// level (an object of fewer levels: level 0).  0 would be the top level, whose cell is the one a one-level object for
// the same world would have been given, so the statics would cost a query what they cost it there: a block of 4^3 top
// cells holds many small statics, and a query walks them all.  Two below: at 262 144 mixed bodies on six levels and
// 5 000 statics of 0.1 .. 3 units, 65 536 ground rays take 862 us against 2 423 us, 65 536 sweeps 6.1 ms against 7.2 ms
// (one below: 1 114 us / 6.2 ms, three below: 838 us / 6.0 ms; profiles/bp_levels_index/).  The price: a static that
// spans more than 64 blocks of the finer level is in the large list, which every query tests.  Results do not depend on
// S (every visitor tests each candidate itself); change it only with a measurement (tools/bp_levels_index_time.py),
// written down there.
constexpr uint32_t BPL_QUERY_STATICS_BELOW_TOP = 2;
__host__ __device__ __forceinline__ uint32_t query_statics_level(uint32_t levels)
{
    return levels - 1u > BPL_QUERY_STATICS_BELOW_TOP ? levels - 1u - BPL_QUERY_STATICS_BELOW_TOP : 0u;
}

} // namespace clapgpu
