// bp_statics.h -- the statics image of a clapgpu_bp.  First THE RULE for one static on one level, host and device, then
// the host binning at create time (host arithmetic only, no HIP call; bp_create.hip uploads the result, tests/c/ checks it
// alone).  It and the device binning of clapgpu_bp_statics_update (bp_restatic.hip) call the rule: one image by construction.
#pragma once
#include <math.h>
#include <string.h>
#include <utility>
#include <vector>
#include "bp_grid.h"

namespace clapgpu {

// Level l's cell: cell * 2^l by repeated doubling (exact in fp64)
__host__ __device__ __forceinline__ double level_cell(double cell, uint32_t l)
{
    for (uint32_t i = 0; i < l; i++) cell *= 2.0;
    return cell;
}

// A static binned with cell c is registered in every block (4^3 cells) that its box grown by half a cell reaches: the
// blocks whose own bodies could touch it.  More than 64 of them, or an edge that is inverted or not a number, make it
// LARGE: one of the list that every body tests.  Otherwise nb blocks from lo, nx by ny by nb / (nx * ny).
struct StaticBlocks { bool large; int32_t lo[3]; uint32_t nx, ny, nb; };

__host__ __device__ __forceinline__ StaticBlocks static_blocks(const double *bb, double c)
{
    const double grow = half_cell_grown(c);
    StaticBlocks r;
    r.large = false;                     // sticky
    int32_t hi[3];
    unsigned long long blocks = 1;       // checked after every axis: edges of 1e9 overflow it on the third, the flag set on the second
#pragma unroll
    for (int a = 0; a < 3; a++) {
        r.lo[a] = cell_coord(bb[2 * a] - grow, c) >> 2;
        hi[a] = cell_coord(bb[2 * a + 1] + grow, c) >> 2;
        if (!(bb[2 * a] <= bb[2 * a + 1])) r.large = true;                        // NaN / inverted: keep it in the tested-by-all list
        blocks *= (unsigned long long)(hi[a] - r.lo[a] + 1);
        if (blocks > 64) r.large = true;
    }
    r.nx = (uint32_t)(hi[0] - r.lo[0] + 1); r.ny = (uint32_t)(hi[1] - r.lo[1] + 1); r.nb = (uint32_t)blocks;
    return r;
}

// The bucket of its block u, 0 <= u < nb, x fastest; mask: block buckets - 1.  Blocks that share a bucket register once.
__host__ __device__ __forceinline__ uint32_t static_block_bucket(const StaticBlocks &b, uint32_t u, uint32_t mask)
{
    return block_hash(b.lo[0] + (int32_t)(u % b.nx), b.lo[1] + (int32_t)((u / b.nx) % b.ny), b.lo[2] + (int32_t)(u / (b.nx * b.ny)), mask);
}

// The image of one level, binned on the host: the registrations of the rule above as a CSR over the block buckets, and the large list.
struct __attribute__((visibility("hidden"))) StaticsImage {
    std::vector<uint32_t> start;         // [buckets + 1]
    std::vector<uint32_t> entries;       // static indices, ascending inside a bucket; one placeholder when none
    std::vector<uint32_t> large;         // n_large static indices, ascending; one placeholder when none
    std::vector<GridRec> recs, lrecs;    // entries / large with their boxes (placeholders: zero)
    uint32_t n_large;
    double bounds[6];                    // union of the registered (not large) boxes: min xyz, max xyz; min > max: none
};

__attribute__((visibility("hidden"))) inline StaticsImage bp_statics_image(uint32_t buckets, double cell, uint32_t n_static, const double *static_aabb)
{
    StaticsImage im;
    im.start.assign(buckets + 1, 0);
    std::vector<std::pair<uint32_t, uint32_t>> ins;                               // (bucket, static)
    for (int a = 0; a < 3; a++) { im.bounds[a] = INFINITY; im.bounds[3 + a] = -INFINITY; }
    for (uint32_t s = 0; s < n_static; s++) {
        const double *bb = static_aabb + 6 * (size_t)s;
        const StaticBlocks b = static_blocks(bb, cell);
        if (b.large) { im.large.push_back(s); continue; }
        for (int a = 0; a < 3; a++) {
            im.bounds[a] = fmin(im.bounds[a], bb[2 * a]);
            im.bounds[3 + a] = fmax(im.bounds[3 + a], bb[2 * a + 1]);
        }
        const size_t first = ins.size();
        for (uint32_t u = 0; u < b.nb; u++) {
            const uint32_t h = static_block_bucket(b, u, buckets - 1);
            bool dup = false;
            for (size_t e = first; e < ins.size(); e++) dup |= ins[e].first == h;
            if (!dup) ins.push_back({ h, s });
        }
    }
    for (auto &e : ins) im.start[e.first + 1]++;
    for (uint32_t b = 0; b < buckets; b++) im.start[b + 1] += im.start[b];
    im.entries.resize(ins.size() ? ins.size() : 1);
    {
        std::vector<uint32_t> cur(im.start.begin(), im.start.end() - 1);
        for (auto &e : ins) im.entries[cur[e.first]++] = e.second;                // ascending static index inside a bucket
    }
    im.n_large = (uint32_t)im.large.size();
    im.recs.resize(im.entries.size());                                            // zero: the cell words, the placeholders
    im.lrecs.resize(im.large.size() ? im.large.size() : 1);
    auto fill_rec = [&](GridRec &r, uint32_t sidx) { memcpy(r.bb, static_aabb + 6 * (size_t)sidx, sizeof(r.bb)); r.idx = sidx; };
    for (size_t e = 0; e < ins.size(); e++) fill_rec(im.recs[e], im.entries[e]);
    for (size_t e = 0; e < im.large.size(); e++) fill_rec(im.lrecs[e], im.large[e]);
    if (im.large.empty()) im.large.push_back(0);
    return im;
}

// A leveled object (bp_levels.h): one image per level, level l binned with level_cell(cell, l) -- a body tests the
// registrations of its own level, whose blocks are sized for bodies of that level.
__attribute__((visibility("hidden"))) inline std::vector<StaticsImage> bp_statics_level_images(uint32_t buckets, double cell, uint32_t levels,
                                                                                             uint32_t n_static, const double *static_aabb)
{
    std::vector<StaticsImage> ims;
    for (uint32_t l = 0; l < levels; l++) ims.push_back(bp_statics_image(buckets, level_cell(cell, l), n_static, static_aabb));
    return ims;
}

// ... laid end to end for one upload (bp_object.h's BplK): starts offset into the shared entries, the placeholders of
// the single images dropped; large_start[l] .. [l + 1]: level l's part of the large list.
__attribute__((visibility("hidden"))) inline StaticsImage bp_statics_concat(const std::vector<StaticsImage> &ims, std::vector<uint32_t> *large_start)
{
    StaticsImage all;
    all.n_large = 0;
    for (int a = 0; a < 3; a++) { all.bounds[a] = INFINITY; all.bounds[3 + a] = -INFINITY; }
    large_start->assign(1, 0u);
    for (const StaticsImage &im : ims) {
        const uint32_t base = (uint32_t)all.entries.size(), n = im.start.back();
        for (uint32_t s : im.start) all.start.push_back(base + s);
        all.entries.insert(all.entries.end(), im.entries.begin(), im.entries.begin() + n);
        all.recs.insert(all.recs.end(), im.recs.begin(), im.recs.begin() + n);
        all.large.insert(all.large.end(), im.large.begin(), im.large.begin() + im.n_large);
        all.lrecs.insert(all.lrecs.end(), im.lrecs.begin(), im.lrecs.begin() + im.n_large);
        all.n_large += im.n_large;
        large_start->push_back(all.n_large);
        for (int a = 0; a < 3; a++) {
            all.bounds[a] = fmin(all.bounds[a], im.bounds[a]);
            all.bounds[3 + a] = fmax(all.bounds[3 + a], im.bounds[3 + a]);
        }
    }
    GridRec zero;
    memset(&zero, 0, sizeof(zero));
    if (all.entries.empty()) { all.entries.push_back(0); all.recs.push_back(zero); }
    if (all.large.empty()) { all.large.push_back(0); all.lrecs.push_back(zero); }
    return all;
}

} // namespace clapgpu
