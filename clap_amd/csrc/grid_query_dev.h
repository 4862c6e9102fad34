// grid_query_dev.h -- reading an INDEXED broadphase grid (bp_grid.h's BpGridView, clapgpu_bp_index) on one wavefront:
// whether the index may be used, the cells and blocks a box asks for, and the one visit of their records that the ray
// cast (rays.hip) and the sweep's gather (slide.hip) share.
//
// Why the range of a box is complete.  An indexed body is binned by the centre of its box (box_cell) and, while
// grid_usable holds, no box edge exceeds `cell`: the centre of a body whose box meets [lo, hi] lies within cell / 2 of
// it on every axis.  cell_coord is monotone, so that centre's cell is one of cell_coord(lo - grow) ..
// cell_coord(hi + grow) with grow = half_cell_grown(cell) (bp_grid.h: its margin is against the rounding of the sums).  A
// static is registered (bp_statics.h's rule) in every block its box grown by the same half cell reaches, or, when those
// are too many, in the large list: the blocks of the range and the large list hold every static whose box meets
// [lo, hi].  Cells and blocks are hashed into buckets, so a lookup may return records of other cells (rejected here by
// the cell coordinates a body's record carries) and statics of other blocks, and a static comes once per block it is
// registered in: a visitor sees a superset of the candidates, some of them more than once, and tests each itself.
//
// A LEVELED index (g.levels > 1: clapgpu_bp_leveled_index; bp_levels.h).  Bodies: every level L = 0 .. levels - 1 is
// looked up with its own cell c_L = cell * 2^L: the cells cell_coord(lo - grow, c_L) .. cell_coord(hi + grow, c_L) with
// grow = half_cell_grown(c_L), each at level_slot(L, ...).  That range holds every candidate of level L for the reason
// bp_levels.h gives for a coarser partner: a body of level L has edges of at most c_L and is binned by its centre --
// while no box exceeds the top level's cell, which is what INDEX_OVERSIZE reports for a leveled index, and grid_usable
// is false then.  A slot is shared across levels, and a record of another level in the slot CAN be a candidate -- of
// its own level's lookup: a record counts only when its level bits are L, its cell is the cell looked up and its index
// (the level bits stripped) is below n, so no candidate arrives from a lookup that did not ask for it.  Statics: the
// image of ONE level, g.s_level (query_statics_level): the blocks of that level's cell range, its starts and its part
// of the large list; every static is registered on every level, so one level holds them all.
// The two forms are one function each with LEVELED as a compile-time switch, up to the kernels: the host launches the
// LEVELED instantiation of a query kernel for a view with levels > 1 (rays.hip, slide.hip), so the kernels of a one-level
// index keep their code and their registers.  (Both forms in one kernel behind a wave-uniform branch cost the one-level
// ground rays 4 % and every ray row 1 to 2 %: profiles/bp_levels_index/.)
#pragma once
#include "common.h"
#include "bp_grid.h"
#include "bp_levels.h"

namespace clapgpu {

// The index may be used by this wavefront now: no indexed box is larger than a cell (the top level's), and the boxes have not been binned
// again since the index was made (a replayed graph bins without the host knowing: the device's bin epoch differs).
__device__ __forceinline__ bool grid_usable(const BpGridView &g)
{
    return g.index[INDEX_OVERSIZE] == ~0ull && (g.n == 0 || g.ctrl[CTRL_EPOCH] == g.ctrl[CTRL_INDEX_EPOCH]);
}

struct GridRange {                                      // cells and blocks lo .. hi, inclusive; as constructed: none
    int32_t c_lo[3] = { 1, 1, 1 }, c_hi[3] = { 0, 0, 0 }, b_lo[3] = { 1, 1, 1 }, b_hi[3] = { 0, 0, 0 };
};

// the cells of size `cell`, and their blocks, that hold every candidate of the box [lo, hi] (see above)
__device__ __forceinline__ GridRange grid_range(double cell, const double (&lo)[3], const double (&hi)[3])
{
    const double grow = half_cell_grown(cell);
    GridRange r;
    for (int a = 0; a < 3; a++) {
        r.c_lo[a] = cell_coord(lo[a] - grow, cell);
        r.c_hi[a] = cell_coord(hi[a] + grow, cell);
        r.b_lo[a] = r.c_lo[a] >> 2; r.b_hi[a] = r.c_hi[a] >> 2;
    }
    return r;
}

// the lookups grid_visit makes for r, cells plus (with statics) blocks (a double: a far-flung or inverted box's count
// passes 32 bits)
__device__ __forceinline__ double grid_lookups(const BpGridView &g, const GridRange &r, bool statics)
{
    double ncell = g.n ? 1.0 : 0.0, nblk = statics ? 1.0 : 0.0;
    for (int a = 0; a < 3; a++) {
        ncell *= (double)(uint32_t)(r.c_hi[a] - r.c_lo[a] + 1);
        nblk *= (double)(uint32_t)(r.b_hi[a] - r.b_lo[a] + 1);
    }
    return ncell + nblk;
}

// A query's walk over the levels: level L's cell c (exact: a power of two times cell), and whether the statics are read
// on it.  One level: the walk is L = 0 alone, with the statics.
template <bool LEVELED>
__device__ __forceinline__ uint32_t grid_levels(const BpGridView &g) { return LEVELED ? g.levels : 1u; }
template <bool LEVELED>
__device__ __forceinline__ bool grid_level_statics(const BpGridView &g, uint32_t L) { return !LEVELED || L == g.s_level; }

__device__ __forceinline__ bool in_box3(const int32_t (&lo)[3], const int32_t (&hi)[3], int32_t x, int32_t y, int32_t z)
{
    return x >= lo[0] && x <= hi[0] && y >= lo[1] && y <= hi[1] && z >= lo[2] && z <= hi[2];
}

// The visit: every body record of the cells of r and every static registered for its blocks, spread over the lanes.
// visit(valid, is_static, idx) is called by every lane on every trip (a visitor may ballot); valid: idx is a body the
// index holds (is_static false) or a registered static.  prev: NULL, or a range whose cells and blocks the caller has
// visited already; they are not looked up again.  The caller keeps grid_lookups(r) small: the counts are 32-bit here.
// LEVELED: r is a range of level L's cells; the bodies of level L in them, and with `statics` the statics of its blocks.
template <bool LEVELED, typename V>
__device__ __forceinline__ void grid_visit(const BpGridView &g, uint32_t L, bool statics, const GridRange &r, const GridRange *prev,
                                           V &&visit)
{
    const uint32_t *s_start = LEVELED ? g.s_start + (size_t)g.s_level * (g.mask + 2u) : g.s_start;    // buckets + 1 a level
    const int lane = lane_id();
    uint32_t ext[3], bext[3];
    for (int a = 0; a < 3; a++) {
        ext[a] = (uint32_t)(r.c_hi[a] - r.c_lo[a] + 1); bext[a] = (uint32_t)(r.b_hi[a] - r.b_lo[a] + 1);
    }
    const uint32_t ncell = g.n ? ext[0] * ext[1] * ext[2] : 0u, nblk = statics ? bext[0] * bext[1] * bext[2] : 0u;
    const uint32_t items = ncell + nblk;
    for (uint32_t base = 0; base < items; base += WAVE) {
        // one lookup per lane: a cell of the range (bodies) or a block (statics)
        const uint32_t it = base + lane;
        uint32_t first = 0, count = 0, isstat = 0;
        int32_t cx = 0, cy = 0, cz = 0;
        if (it < ncell) {
            cx = r.c_lo[0] + (int32_t)(it % ext[0]);
            cy = r.c_lo[1] + (int32_t)((it / ext[0]) % ext[1]);
            cz = r.c_lo[2] + (int32_t)(it / (ext[0] * ext[1]));
            if (!prev || !in_box3(prev->c_lo, prev->c_hi, cx, cy, cz)) {
                const uint2 cr = g.cell_range[LEVELED ? level_slot(L, cx, cy, cz, g.mask) : cell_slot(cx, cy, cz, g.mask)];
                first = cr.x; count = cr.y;
            }
        } else if (it < items) {
            const uint32_t q = it - ncell;
            const int32_t bx = r.b_lo[0] + (int32_t)(q % bext[0]), by = r.b_lo[1] + (int32_t)((q / bext[0]) % bext[1]),
                          bz = r.b_lo[2] + (int32_t)(q / (bext[0] * bext[1]));
            if (!prev || !in_box3(prev->b_lo, prev->b_hi, bx, by, bz)) {
                const uint32_t h = block_hash(bx, by, bz, g.mask);
                first = s_start[h]; count = s_start[h + 1] - first;
            }
            isstat = 1;
        }
        const uint32_t incl = wave_prefix_sum(count);
        const uint32_t total = __shfl(incl, WAVE - 1), excl = incl - count;
        // the records of these lookups spread over the lanes: record q belongs to the first lane with incl > q
        for (uint32_t q0 = 0; q0 < total; q0 += WAVE) {
            const uint32_t q = q0 + lane;
            int o = 0;
#pragma unroll
            for (int step = 32; step > 0; step >>= 1) {
                const uint32_t v = __shfl(incl, o + step - 1);
                if (v <= q) o += step;
            }
            const uint32_t ofirst = __shfl(first, o), oexcl = __shfl(excl, o), ostat = __shfl(isstat, o);
            const int32_t ox = __shfl(cx, o), oy = __shfl(cy, o), oz = __shfl(cz, o);
            bool valid = q < total;
            uint32_t idx = 0;
            if (valid) {
                const uint32_t e = ofirst + (q - oexcl);
                if (ostat) {
                    idx = g.s_recs[e].idx;
                } else {
                    const int4 t = reinterpret_cast<const int4 *>(g.recs + e)[3];      // idx, cell coordinates
                    idx = LEVELED ? (uint32_t)t.x & BPL_IDX : (uint32_t)t.x;
                    valid = t.y == ox && t.z == oy && t.w == oz && idx < g.n;          // not a hash neighbour
                    if (LEVELED) valid = valid && (uint32_t)t.x >> BPL_LEVEL_SHIFT == L;  // ... nor another level's cell
                }
            }
            visit(valid, ostat != 0, idx);
        }
    }
}

// ... and the large statics (LEVELED: of the statics' level), which every query visits whatever its box
template <bool LEVELED, typename V>
__device__ __forceinline__ void grid_visit_large(const BpGridView &g, V &&visit)
{
    const GridRec *lrecs = LEVELED ? g.s_lrecs + g.large_first : g.s_lrecs;
    const int lane = lane_id();
    for (uint32_t base = 0; base < g.n_large; base += WAVE) {
        const uint32_t j = base + lane;
        const bool valid = j < g.n_large;
        visit(valid, true, valid ? lrecs[j].idx : 0u);
    }
}

} // namespace clapgpu
