// skin_drawn.hip -- skinning that follows the cull and the LOD: clapgpu_skin_drawn (the rule: include/clapgpu.h).
//
// The reference skins in its vertex shader (shaders/model.vert:32-48), so only for entities that pass _models_render's
// draw predicate in some pass (model.c:959-973) and only for the vertices the bound index buffer model->index[e->cur_lod]
// references (model.c:993-997, 1042).  clapgpu_skin skins every vertex of every character; this call skins what is drawn.
//
// Three launches, no host synchronisation, nothing allocated:
//   k_skin_select     one lane per character: the bit of its entity slot in every mask plane, its LOD, skinned[], the
//                     range bits; a wavefront leaves one word of a "drawn" bit mask and that word's popcount in scratch
//   the compaction    clapgpu_visible_compact (visible.hip) over that mask: chars[] ascending, *count.  The mask has the
//                     shape of a visibility plane on purpose, so the ordered compaction is stated once in the library
//   k_skin_drawn      sized by n_chars; reads *count and chars[] on the device
//
// Mapping of k_skin_drawn: ONE WAVEFRONT PER DRAWN CHARACTER, up to four of them in a 256-lane workgroup, each with a
// palette region of its own in LDS (the 80-byte row pitch of skin.hip).  Why not skin.hip's workgroup per character:
//   - behind the cull and the LOD most characters are short.  The LOD rule puts everything beyond ~100 units at the
//     coarsest LOD, a few dozen vertices; for those the 64 * J bytes of the palette are the traffic (4 KiB at 64 joints
//     against 1.7 KiB for 25 vertices) and a 256-lane workgroup would hold 4 wavefront slots, a barrier and 5 KiB of LDS
//     for work that fills less than half of one wavefront;
//   - a wavefront that owns its character needs no workgroup barrier: it stages the palette, orders its own LDS writes
//     before its reads (wave_lds_fence) and streams its vertices 64 at a time, the next 64 requested before the current
//     ones are blended, as skin.hip does across its loop.  A 200-vertex character is four trips of one wavefront instead
//     of one trip of four (68-72 VGPRs: seven wavefronts per SIMD, 20 KiB of LDS per workgroup);
//   - the drawn characters are compacted in front of the launch, so workgroup g takes chars[4g .. 4g + 4): full
//     workgroups up to *count, and every workgroup behind it leaves on one scalar compare before it touches a palette.
// Several wavefronts per workgroup rather than 64-lane workgroups: a quarter of the workgroups to dispatch, and the CU's
// workgroup slots do not cap the resident wavefronts.  The workgroup holds as many wavefronts as palettes fit in 20 KiB
// (4 up to 64 joints, 2 up to 128, 1 up to 256), so eight workgroups stay resident per CU whatever the joint count.
// The per-vertex arithmetic, the non-temporal loads and stores and the palette pitch are skin.hip's: skin_dev.h.
// MEASURED (profiles/skin_drawn/README.md, 50 000 characters x 200 vertices, 64 joints): whole characters cost more this
// way -- everything drawn, no lists: 163 us against clapgpu_skin's 137 (k_skin_drawn 153, the two launches in front ~10)
// -- and the culled population (30 % drawn) 69 us.  Lists pay by the cache lines they leave untouched, not by their
// entries: every 8th vertex still touches every line (65 us), the first 25 of 200 do not (37 us).  Requesting two trips
// ahead instead of one (82 VGPRs, five wavefronts per SIMD) was no faster: 172 / 71 / 68 / 40 us for the same four.
#include "common.h"
#include "skin_dev.h"

namespace clapgpu {

constexpr int SD_BLOCK = 256;
constexpr uint32_t SD_NONE = 0xffffffffu;                  // a lane without a vertex this trip
constexpr int SD_PLANES = 1 + CLAPGPU_EXTRA_VIEWS_MAX;

struct SelK {
    uint32_t        n_chars, n_entities, n_planes, n_lods, n_rows, n_list;
    const uint64_t *plane[SD_PLANES];
    const uint32_t *entity;
    const int32_t  *cur_lod;
    const uint32_t *row, *lod_first, *lod_count, *list;
    uint8_t        *skinned;
    uint32_t       *chars, *count, *status;
    uint64_t       *mask;                                  // scratch: bit c = character c is drawn
    uint8_t        *pop;                                   // scratch: popcount of each mask word
};

__global__ __launch_bounds__(SD_BLOCK)
void k_skin_select(SelK s)
{
    const uint32_t c = blockIdx.x * SD_BLOCK + threadIdx.x;
    const int lane = lane_id();
    if ((c - lane) >= s.n_chars) return;                   // a wavefront past the end: no word of the mask is its own
    bool drawn = false;
    uint32_t bits = 0, lod = 0;
    if (c < s.n_chars) {
        const uint32_t e = s.entity ? s.entity[c] : c;
        if (e >= s.n_entities) {
            bits |= CLAPGPU_SKINSEL_ENTITY_RANGE;          // nothing is read outside the planes
        } else {
            for (uint32_t p = 0; p < s.n_planes; p++)
                drawn = drawn || ((s.plane[p][e >> 6] >> (e & 63u)) & 1ull);
            if (drawn && s.cur_lod) {
                const int32_t l = s.cur_lod[e];
                if (l < 0 || (uint32_t)l >= s.n_lods) bits |= CLAPGPU_SKINSEL_LOD_RANGE;
                else lod = (uint32_t)l;
            }
        }
        s.skinned[c] = drawn ? (uint8_t)lod : (uint8_t)CLAPGPU_SKIN_NOT_DRAWN;
    }
    if (bits) atomicOr(s.status, bits);
    const uint64_t m = __ballot(drawn);
    if (lane == 0) {
        s.mask[c >> 6] = m;
        s.pop[c >> 6] = (uint8_t)__popcll(m);
    }
}

template <bool W>                                          // W: also total_local_pos.w
__global__ __launch_bounds__(SD_BLOCK)
void k_skin_drawn(SkinArgs a, SelK s)
{
    extern __shared__ __attribute__((aligned(16))) float pal_all[];   // one palette of J rows per wavefront

    const uint32_t wave = threadIdx.x / WAVE, lane = (uint32_t)lane_id(), per_block = blockDim.x / WAVE;
    const uint32_t slot = blockIdx.x * per_block + wave;
    const uint32_t drawn = *s.count < a.n_chars ? *s.count : a.n_chars;   // a count beyond the batch would walk off the list
    if (slot >= drawn) return;                             // the whole workgroup when blockIdx.x * per_block >= drawn
    const uint32_t c = s.chars[slot];
    if (c >= a.n_chars) return;
    // the palette first: its address needs c alone, so its 64 * J bytes are in flight under the chain of dependent reads
    // below (the character's ranges -> its row of the tables -> the list -> the vertices)
    float *pal = pal_all + (size_t)wave * a.J * PAL_PITCH;
    stage_palette(pal, a.joint_transforms + (size_t)c * a.J * 4, a.J, lane, WAVE);
    const uint32_t vfirst = a.vert_first[c], vcount = a.vert_count[c], ofirst = a.out_first[c];
    uint32_t lod = s.skinned[c];
    if (lod >= s.n_lods) lod = 0;                          // (the select pass wrote it below n_lods: the tables are not read past a row)

    // the vertices it names: list[first .. first + cnt), or [0, vcount) without a list read
    uint32_t first = CLAPGPU_SKIN_LOD_ALL, cnt = vcount;
    bool bad = false;
    if (s.n_rows) {
        const uint32_t r = s.row ? s.row[c] : 0;
        if (r < s.n_rows) {
            first = s.lod_first[(size_t)r * s.n_lods + lod];
            if (first != CLAPGPU_SKIN_LOD_ALL) cnt = s.lod_count[(size_t)r * s.n_lods + lod];
        } else {
            bad = true;                                    // no such row: skinned whole
        }
    }
    const bool listed = first != CLAPGPU_SKIN_LOD_ALL;
    if (listed) {                                          // nothing is read outside the list
        if (first > s.n_list) { cnt = 0; bad = true; }
        else if (cnt > s.n_list - first) { cnt = s.n_list - first; bad = true; }
    }
    if (cnt) {
        // entry k of the range -> the local vertex it names, SD_NONE where the lane has none
        auto named = [&](uint32_t k) -> uint32_t {
            if (k >= cnt) return SD_NONE;
            const uint32_t v = listed ? s.list[(size_t)first + k] : k;
            if (v >= vcount) { bad = true; return SD_NONE; }      // a listed index past the mesh is skipped
            return v;
        };
        uint32_t k = lane, v = named(k);
        SkinVert cur;
        if (v != SD_NONE)
            cur = load_vert(a, (size_t)vfirst + v);
        wave_lds_fence();                                  // the wavefront's own palette: no workgroup barrier
        while (k < cnt) {
            if (v != SD_NONE)
                skin_vertex<W>(a, pal, cur, (size_t)ofirst + v);
            k += WAVE;
            v = named(k);
            if (v != SD_NONE)
                cur = load_vert(a, (size_t)vfirst + v);
        }
    }
    if (bad) atomicOr(s.status, CLAPGPU_SKINSEL_LIST_RANGE);
}

static uint32_t waves_per_block(uint32_t J) { return J <= 64 ? 4u : J <= 128 ? 2u : 1u; }

struct SelScratch { size_t mask, pop, groups, bytes; };
static SelScratch carve_select(uint32_t n_chars)
{
    const size_t words = ((size_t)n_chars + 63) / 64;
    Carve cv;
    SelScratch sc;
    sc.mask = cv.take(words * sizeof(uint64_t));
    sc.pop = cv.take(words);                               // 16-byte aligned: the compaction's byte prefix needs it
    sc.groups = cv.take(clapgpu_visible_scratch_bytes(n_chars));
    sc.bytes = cv.bytes();
    return sc;
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" size_t clapgpu_skin_select_scratch_bytes(uint32_t n_chars) { return carve_select(n_chars).bytes; }

extern "C" int clapgpu_skin_drawn(void *stream, const clapgpu_skin_batch *b, const clapgpu_skin_select *sel)
{
    if (!b || !sel)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (b->n_chars == 0)
        return CLAPGPU_OK;
    int rc = check_skin_batch(b);
    if (rc) return rc;
    if (sel->n_planes < 1 || sel->n_planes > (uint32_t)SD_PLANES || sel->n_lods > CLAPGPU_SKIN_LODS)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    for (uint32_t p = 0; p < sel->n_planes; p++)
        if (!sel->planes[p]) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (sel->n_rows && (sel->n_lods < 1 || !sel->lod_first || !sel->lod_count))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (sel->n_list && !sel->list)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!sel->skinned || !sel->chars || !sel->count || !sel->status)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!sel->scratch || ((uintptr_t)sel->scratch & 255u))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;

    const SelScratch sc = carve_select(b->n_chars);
    char *scratch = static_cast<char *>(sel->scratch);
    SelK s;
    s.n_chars = b->n_chars; s.n_entities = sel->n_entities; s.n_planes = sel->n_planes;
    s.n_lods = sel->n_lods ? sel->n_lods : CLAPGPU_SKIN_LODS;      // without rows 0 stands for all of them
    s.n_rows = sel->n_rows; s.n_list = sel->n_list;
    for (int p = 0; p < SD_PLANES; p++) s.plane[p] = (uint32_t)p < sel->n_planes ? sel->planes[p] : nullptr;
    s.entity = sel->entity; s.cur_lod = sel->cur_lod;
    s.row = sel->row; s.lod_first = sel->lod_first; s.lod_count = sel->lod_count; s.list = sel->list;
    s.skinned = sel->skinned; s.chars = sel->chars; s.count = sel->count; s.status = sel->status;
    s.mask = reinterpret_cast<uint64_t *>(scratch + sc.mask);
    s.pop = reinterpret_cast<uint8_t *>(scratch + sc.pop);

    hipLaunchKernelGGL(k_skin_select, dim3((b->n_chars + SD_BLOCK - 1) / SD_BLOCK), dim3(SD_BLOCK), 0, as_stream(stream), s);
    CLAPGPU_LAUNCH_CHECK("k_skin_select");
    rc = clapgpu_visible_compact(stream, s.mask, s.pop, b->n_chars, 0, s.chars, s.count, scratch + sc.groups);
    if (rc) return rc;
    const SkinArgs a = make_skin_args(b);
    const uint32_t per_block = waves_per_block(b->nr_joints);
    const dim3 grid((b->n_chars + per_block - 1) / per_block), block(per_block * WAVE);
    const size_t lds = (size_t)per_block * b->nr_joints * PAL_PITCH * sizeof(float);
    if (b->out_w)
        hipLaunchKernelGGL(k_skin_drawn<true>, grid, block, lds, as_stream(stream), a, s);
    else
        hipLaunchKernelGGL(k_skin_drawn<false>, grid, block, lds, as_stream(stream), a, s);
    CLAPGPU_LAUNCH_CHECK("k_skin_drawn");
    return CLAPGPU_OK;
}
