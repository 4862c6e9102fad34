// bp_create.hip -- the clapgpu_bp object: its statics binned on the host (bp_statics.h) and adopted (bp_object.h's
// bp_adopt_statics), its one device allocation carved into the arrays of BpK, and what the object hands out (status
// words, the ray cast's view of an index, the contact ticket).  No kernel: the launches are broadphase.hip's.
#include <stdlib.h>
#include <type_traits>
#include "bp_object.h"
#include "bp_statics.h"

using namespace clapgpu;

static uint32_t buckets_for(uint32_t n)
{
    uint32_t b = 1024;                                                  // block buckets: 64 cell slots each, about two slots per body
    while (b < n / 32 && b < (1u << 22)) b <<= 1;
    return b;
}

// One device allocation, carved.  Every array is stated once: member, elements and the host array uploaded into it
// (none: zero).  The list runs twice: with base == nullptr it only sizes the allocation, with the (zeroed) allocation it
// sets the pointers and uploads.  Returns the bytes; 0 when an upload failed.
static size_t carve(BpK &k, char *base, uint32_t n, uint32_t nb, uint32_t n_tiles, uint32_t n_static, const double *static_aabb,
                    const StaticsImage &im)
{
    size_t off = 0;
    bool ok = true;
    auto arr = [&](auto *&member, size_t count, const void *src = nullptr) {
        const size_t bytes = sizeof(*member) * count;
        if (base) {
            member = reinterpret_cast<std::remove_reference_t<decltype(member)>>(base + off);
            if (src && hipMemcpy(base + off, src, bytes, hipMemcpyHostToDevice) != hipSuccess) ok = false;
        }
        off += (bytes + 255) & ~(size_t)255;
    };
    arr(k.cell_cnt, (size_t)nb * 64);
    arr(k.cell_range, (size_t)nb * 64);
    arr(k.key, n);
    arr(k.rank, n);
    arr(k.entries, n);
    arr(k.recs, n);
    arr(k.cnt, n);
    arr(k.scnt, n);
    arr(k.partners, (size_t)BP_LIST * n);
    arr(k.spartners, (size_t)BP_LIST * n);
    arr(k.lb_body, n_tiles);
    arr(k.lb_static, n_tiles);
    arr(k.lb_cells, (size_t)nb / 4 + 1);
    arr(k.ctrl, CTRL_WORDS);
    arr(k.s_start, im.start.size(), im.start.data());
    arr(k.s_entries, im.entries.size(), im.entries.data());
    arr(k.s_large, im.large.size(), im.large.data());
    arr(k.s_aabb, 6 * (size_t)(n_static ? n_static : 1), n_static ? static_aabb : nullptr);
    arr(k.s_recs, im.recs.size(), im.recs.data());
    arr(k.s_lrecs, im.lrecs.size(), im.lrecs.data());
    return ok ? off : 0;
}

// levels == 1: the one-level object of clapgpu_bp_create.  More: the same arrays (the level is part of a cell's slot), one
// statics image per level laid end to end, and the level in four bits of a record's index: n_max <= 2^28.
static int create(clapgpu_bp **out, uint32_t n_max, double cell, uint32_t levels, uint32_t n_static, const double *static_aabb)
{
    if (!out || !(cell > 0.0) || (n_static && !static_aabb) || n_max > (levels > 1 ? BPL_IDX + 1u : 1u << 30) ||
        levels == 0 || levels > CLAPGPU_BP_LEVELS_MAX)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    clapgpu_bp *bp = static_cast<clapgpu_bp *>(calloc(1, sizeof(*bp)));
    if (!bp) return CLAPGPU_ERR_NOMEM;
    const uint32_t n = n_max ? n_max : 1, nb = buckets_for(n);
    bp->n_max = n_max; bp->buckets = nb; bp->cell = cell; bp->n_static = n_static;
    bp->n_tiles = (n + BP_EMIT_TILE - 1) / BP_EMIT_TILE;
    bp->levels = levels;
    std::vector<uint32_t> large_start{ 0u };
    const StaticsImage im = levels == 1 ? bp_statics_image(nb, cell, n_static, static_aabb)
                                        : bp_statics_concat(bp_statics_level_images(nb, cell, levels, n_static, static_aabb), &large_start);
    if (levels == 1) large_start.push_back(im.n_large);                  // [l + 1]: the large statics up to the end of level l

    BpK &k = bp->k;                                                      // zero: calloc
    k.cell = cell; k.mask = nb - 1; k.n_static = n_static;
    const size_t bytes = carve(k, nullptr, n, nb, bp->n_tiles, n_static, static_aabb, im);
    if (hipMalloc(&bp->dev, bytes) != hipSuccess) {
        (void)hipGetLastError();
        free(bp);
        return CLAPGPU_ERR_NOMEM;
    }
    if (hipMemset(bp->dev, 0, bytes) != hipSuccess ||
        !carve(k, static_cast<char *>(bp->dev), n, nb, bp->n_tiles, n_static, static_aabb, im)) {
        (void)hipGetLastError();
        (void)hipFree(bp->dev);
        free(bp);
        return CLAPGPU_ERR_UNKNOWN;
    }
    bp_adopt_statics(bp, k.s_start, k.s_entries, k.s_large, k.s_recs, k.s_lrecs, im.start.back(), large_start.data() + 1, im.bounds);
    *out = bp;
    return CLAPGPU_OK;
}

extern "C" int clapgpu_bp_create(clapgpu_bp **out, uint32_t n_max, double cell, uint32_t n_static, const double *static_aabb)
{
    return create(out, n_max, cell, 1, n_static, static_aabb);
}

extern "C" int clapgpu_bp_create_levels(clapgpu_bp **out, uint32_t n_max, double cell, uint32_t levels, uint32_t n_static,
                                        const double *static_aabb)
{
    return create(out, n_max, cell, levels, n_static, static_aabb);
}

extern "C" uint32_t clapgpu_bp_levels(const clapgpu_bp *bp) { return bp ? bp->levels : 0; }

extern "C" uint32_t clapgpu_bp_cell_slot(const clapgpu_bp *bp, uint32_t level, int32_t cx, int32_t cy, int32_t cz)
{
    if (!bp || level >= bp->levels) return 0xffffffffu;
    return bp->levels == 1 ? cell_slot(cx, cy, cz, bp->k.mask) : level_slot(level, cx, cy, cz, bp->k.mask);
}

// the switch of a leveled object's index; off as calloc leaves it.  Host state only: whatever index the object holds was
// made for the other setting and is dropped
extern "C" int clapgpu_bp_leveled_index(clapgpu_bp *bp, int on)
{
    if (!bp) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (bp->levels == 1) return CLAPGPU_OK;
    bp->leveled_index = on != 0;
    bp->indexed = false;
    return CLAPGPU_OK;
}

// geoms_dev.h's scene_grid: a leveled object whose index is switched off: queries through it scan, indexed or not
__attribute__((visibility("hidden"))) bool clapgpu_bp_scans(const clapgpu_bp *bp) { return bp->levels > 1 && !bp->leveled_index; }

extern "C" void clapgpu_bp_destroy(clapgpu_bp *bp)
{
    if (!bp) return;
    if (bp->dev) (void)hipFree(bp->dev);
    if (bp->st.dev2) (void)hipFree(bp->st.dev2);                 // clapgpu_bp_statics_update's images
    free(bp);
}

extern "C" const double *clapgpu_bp_static_aabb(const clapgpu_bp *bp) { return bp ? bp->k.s_aabb : nullptr; }

extern "C" int clapgpu_bp_status(void *stream, clapgpu_bp *bp, uint32_t *status)
{
    if (!bp || !status) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    CLAPGPU_HIP(hipMemcpyAsync(status, bp->k.ctrl + CTRL_STATUS, sizeof(uint32_t), hipMemcpyDeviceToHost, as_stream(stream)));
    CLAPGPU_HIP(hipStreamSynchronize(as_stream(stream)));
    return CLAPGPU_OK;
}

// contacts.hip's one-launch form (k_contacts_geoms_both) keeps its ticket + counts in this object's control words
__attribute__((visibility("hidden"))) unsigned long long *clapgpu_bp_contact_ticket(clapgpu_bp *bp)
{
    static_assert((CTRL_CONTACT_WORD * sizeof(uint32_t)) % 8 == 0, "the ticket word is a 64-bit atomic");
    return reinterpret_cast<unsigned long long *>(bp->k.ctrl + CTRL_CONTACT_WORD);
}

// rays.hip's view of an index (bp_grid.h)
__attribute__((visibility("hidden"))) bool clapgpu_bp_grid_view(const clapgpu_bp *bp, uint32_t n, const double *aabb,
                                                                 BpGridView *v)
{
    if (!bp || clapgpu_bp_scans(bp) || !bp->indexed || bp->indexed_n != n || (aabb && bp->indexed_aabb != aabb)) return false;
    v->n = n; v->n_static = bp->n_static; v->cell = bp->cell; v->mask = bp->k.mask;
    // a leveled object: the queries read the statics image of one level (bp_levels.h's query_statics_level)
    v->levels = bp->levels;
    v->s_level = query_statics_level(bp->levels);
    v->large_first = bp->levels > 1 ? bp->st.large_start[v->s_level] : 0u;
    v->n_large = bp->levels > 1 ? bp->st.large_start[v->s_level + 1] - v->large_first : bp->st.n_large;
    v->cell_range = bp->k.cell_range;
    v->recs = bp->k.recs;
    v->s_start = bp->k.s_start;
    v->s_recs = bp->k.s_recs;
    v->s_lrecs = bp->k.s_lrecs;
    v->index = reinterpret_cast<const uint64_t *>(bp->k.ctrl + CTRL_INDEX_WORD);
    v->ctrl = bp->k.ctrl;
    memcpy(v->s_bounds, bp->st.bounds, sizeof(v->s_bounds));
    return true;
}

extern "C" int clapgpu_bp_index_status(void *stream, clapgpu_bp *bp, uint32_t *status)
{
    if (!bp || !status || !bp->indexed) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    *status = clapgpu_bp_scans(bp) ? 4u : 0u;                            // leveled, switched off: no index was built, queries scan every geom
    if (!bp->indexed_n || clapgpu_bp_scans(bp)) return CLAPGPU_OK;
    uint64_t w = 0;
    uint32_t epochs[2] = { 0, 0 };
    hipStream_t s = as_stream(stream);
    CLAPGPU_HIP(hipMemcpyAsync(&w, bp->k.ctrl + CTRL_INDEX_WORD + 2 * INDEX_OVERSIZE, sizeof(w), hipMemcpyDeviceToHost, s));
    CLAPGPU_HIP(hipMemcpyAsync(&epochs[0], bp->k.ctrl + CTRL_EPOCH, 4, hipMemcpyDeviceToHost, s));
    CLAPGPU_HIP(hipMemcpyAsync(&epochs[1], bp->k.ctrl + CTRL_INDEX_EPOCH, 4, hipMemcpyDeviceToHost, s));
    CLAPGPU_HIP(hipStreamSynchronize(s));
    *status = (w != ~0ull ? 1u : 0u) | (epochs[0] != epochs[1] ? 2u : 0u);
    return CLAPGPU_OK;
}
