// views_dev.h -- the view block (include/clapgpu.h, "Views in device memory") as the kernels read it.  A slot of
// clapgpu_views_state begins with the cull's own lmd::FrustumK -- the frustum, then the constants k_views_calc left in
// the reserved words -- so a twin kernel hands the SAME functions (lmd::aabb_in_frustum_fast, cull_extra_views) a
// reference into the block where its original hands them a kernel argument.
#pragma once
#include <stddef.h>
#include "common.h"
#include "lm_dev.h"

namespace clapgpu {

static_assert(sizeof(lmd::Frustum) == sizeof(clapgpu_frustum) && offsetof(clapgpu_view_state, frustum) == 0 &&
              offsetof(clapgpu_view_state, cull) == offsetof(lmd::FrustumK, cmin) &&
              sizeof(lmd::FrustumK) <= offsetof(clapgpu_view_state, view_mx) && alignof(lmd::FrustumK) <= 16 &&
              sizeof(clapgpu_view_state) % 16 == 0,
              "a view slot begins with the cull's FrustumK");

__device__ __forceinline__ const lmd::FrustumK &view_frustum_k(const clapgpu_views_state *st, uint32_t slot)
{
    return *reinterpret_cast<const lmd::FrustumK *>(&st->slot[slot]);
}

// what every entry point asks of a block before any HIP call
static inline bool view_block_ok(const void *p) { return p && (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- clapgpu_lights_update ("Spotlights on the device"): what k_lights_update (lights.hip) and the host twin
//      (runtime.hip) decide per carrier, and what both entry points ask before anything else ----
// light.c:464-467: a valid active slot whose tracked transform was updated; no parent test
LMD bool spot_carrier_applies(int32_t l, uint32_t ent, uint32_t nr_lights, uint32_t n_entities, const uint32_t *active,
                              const uint32_t *flags, uint32_t mode)
{
    if (l < 0 || (uint32_t)l >= nr_lights || ent >= n_entities) return false;
    if (!active[l]) return false;
    return (mode & CLAPGPU_UPDATE_ALL_DIRTY) || (flags[ent] & CLAPGPU_E_DIRTY);
}

// a carrier's nonzero view slot names a pose slot of the source
LMD bool spot_view_slot_ok(uint32_t vs, const clapgpu_views_source *source)
{
    return vs < CLAPGPU_VIEW_SLOTS && (source->slot[vs].flags & CLAPGPU_VIEW_FROM_POSE);
}

static inline int spots_check(const clapgpu_entities *e, const clapgpu_spots *s, const clapgpu_lights *l,
                              const clapgpu_views_source *source)
{
    if (!e || !s || !l || !l->pos || !l->color || !l->attenuation || !l->is_dir || !l->active)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (l->nr_lights > CLAPGPU_LIGHTS_MAX)
        return CLAPGPU_ERR_TOO_LARGE;
    if (!e->pos_scale || !e->rot || !e->flags || !s->dir || !s->cutoff || !s->status)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (s->n && (!s->carrier_entity || !s->carrier_light || !s->carrier_off))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (s->carrier_view_slot && !view_block_ok(source))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    return CLAPGPU_OK;
}

} // namespace clapgpu
