// draw_dev.h -- clapgpu_draw_records (include/clapgpu.h, "Draw records on the device"): every decision of
// _models_render's per-entity block (core/model.c:959-1050) stated once, for the kernels (draw.hip) and for the host twin
// (runtime.hip: clapgpu_draw_records_host), and what both entry points ask before anything else.
#pragma once
#include <math.h>
#include "common.h"
#include "lm_dev.h"

namespace clapgpu {

// model.c:786: `if (model->skip_shadow && opts->shader_override) continue;`
LMD bool draw_group_skipped(uint32_t group_flags, uint32_t pass_flags)
{
    return (group_flags & CLAPGPU_DRAW_GROUP_SKIP_SHADOW) && (pass_flags & CLAPGPU_DRAW_PASS_SHADOW);
}

// model.c:960-973 for entity i < n: the plane holds the whole predicate for its view; without a view (`view &&`,
// model.c:970) what is left is ALIVE && VISIBLE
LMD bool draw_entity_drawn(const uint64_t *plane, const uint32_t *flags, uint32_t i)
{
    if (plane) return (plane[i >> 6] >> (i & 63u)) & 1ull;
    const uint32_t f = flags[i];
    return (f & CLAPGPU_E_ALIVE) && (f & CLAPGPU_E_VISIBLE);
}

// the txmodel of render position r < n_order: the g with group_start[g] <= r < group_start[g + 1], searched between lo
// and hi (group_start[lo] <= r < group_start[hi + 1]); empty groups are stepped over.  At most 32 trips whatever the
// array holds, and no index outside lo .. hi
LMD uint32_t draw_group_of(const uint32_t *group_start, uint32_t lo, uint32_t hi, uint32_t r)
{
    while (lo < hi) {                                   // the last g in lo .. hi with group_start[g] <= r
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (group_start[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// model.c:1000-1008: `fabsf(v) > 1e-3` is a double comparison; `else if (ropts)`; otherwise the uniform is not set
LMD float draw_bloom(float entity_value, uint32_t pass_flags, float pass_value, bool *set)
{
    if ((double)fabsf(entity_value) > 1e-3) { *set = true; return entity_value; }
    if (pass_flags & CLAPGPU_DRAW_PASS_HAS_ROPTS) { *set = true; return pass_value; }
    *set = false;
    return 0.0f;
}

// model.c:1012: does this draw advance nr_characters
LMD bool draw_counts_character(uint32_t draw_flags, uint32_t mq_nr_characters)
{
    return (draw_flags & CLAPGPU_DRAW_IS_CHARACTER) && mq_nr_characters;
}

// model.c:1010-1015, shader_constants.h:57-62: EDGE_EXCLUDE = 1u << 7, EDGE_SOLID_MASK = 15, EDGE_SOLID_OFFSET = 0;
// ordinal: nr_characters behind the increment
LMD uint32_t draw_edge_mode(uint32_t draw_flags, uint32_t mq_nr_characters, uint32_t ordinal)
{
    uint32_t edge_mode = 0;
    if (draw_flags & CLAPGPU_DRAW_OUTLINE_EXCLUDE) edge_mode |= 1u << 7;
    if (draw_counts_character(draw_flags, mq_nr_characters)) edge_mode |= (ordinal & 15u) << 0;
    return edge_mode;
}

// the record's words behind mx / inv_mx / color (offsets 144 .. 191), from entity i at ordinal `ordinal` of group g
struct DrawTail { uint32_t w[12]; };

LMD uint32_t draw_f2u(float f) { union { float f; uint32_t u; } c; c.f = f; return c.u; }

LMD DrawTail draw_tail(const clapgpu_draw_inputs &in, const clapgpu_draw_pass &p, const int32_t *lod, uint32_t i, uint32_t g,
                       uint32_t ordinal)
{
    DrawTail t;
    bool set_i, set_t;
    const float bi = draw_bloom(in.bloom_intensity ? in.bloom_intensity[i] : 0.0f, p.flags, p.bloom_intensity, &set_i);
    const float bt = draw_bloom(in.bloom_threshold ? in.bloom_threshold[i] : 0.0f, p.flags, p.bloom_threshold, &set_t);
    const uint32_t df = in.draw_flags ? in.draw_flags[i] : 0u;
    t.w[0] = draw_f2u(bi);
    t.w[1] = draw_f2u(bt);
    t.w[2] = draw_edge_mode(df, p.mq_nr_characters, ordinal);
    t.w[3] = in.color_pt ? (uint32_t)in.color_pt[i] : 0u;
    t.w[4] = p.index_base + i;
    t.w[5] = lod ? (uint32_t)lod[i] : 0u;
    t.w[6] = g;
    t.w[7] = in.character ? (uint32_t)in.character[i] : 0xffffffffu;
    t.w[8] = (set_i ? CLAPGPU_DRAW_SET_BLOOM_INTENSITY : 0u) | (set_t ? CLAPGPU_DRAW_SET_BLOOM_THRESHOLD : 0u);
    t.w[9] = t.w[10] = t.w[11] = 0u;
    return t;
}

static inline int draw_check(const clapgpu_entities *e, const uint64_t *vis_mask, const clapgpu_draw_order *o,
                             const clapgpu_draw_pass *pass, const clapgpu_draw_record *records, uint32_t capacity,
                             const uint32_t *count, const uint32_t *group_first, const uint32_t *status)
{
    if (!e || !o || !pass || !count || !group_first || !status) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if ((!records && capacity) || (reinterpret_cast<uintptr_t>(records) & 63u)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!e->mx || !e->inv_mx || (!vis_mask && !e->flags)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (o->n_order && (!o->order || !o->n_groups)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (o->n_groups && (!o->group_start || !o->group_flags)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    return CLAPGPU_OK;
}

} // namespace clapgpu
