// entities_args.h -- host side of the entity kernels' arguments: the checks of a clapgpu_entities and its translation
// into what the kernels take by value (entities_row.h).  Shared by entities.hip (the update), visible.hip (the render-pass
// glue) and entities_edit.hip; stated once, here.
#pragma once
#include "entities_row.h"

namespace clapgpu {

static inline EntK to_kernel_args(const clapgpu_entities *e)
{
    EntK k;
    k.pos_scale = reinterpret_cast<const float4 *>(e->pos_scale);
    k.rot = reinterpret_cast<const float4 *>(e->rot);
    k.parent = e->parent;
    k.model = e->model;
    k.model_table = reinterpret_cast<const float4 *>(e->model_table);
    k.flags = e->flags;
    k.seqs = e->seqs;
    k.mx = e->mx;
    k.inv_mx = e->inv_mx;
    k.aabb = e->aabb;
    k.center = e->center;
    k.vis_mask = e->vis_mask;
    k.vis_row_pop = e->vis_row_pop;
    k.n_attach = (e->attach && e->jt_pool && e->bind_pool && e->attach_local) ? e->n_attach : 0;
    k.attach = e->attach;
    k.attach_local = e->attach_local;
    k.jt_pool = e->jt_pool;
    k.bind_pool = e->bind_pool;
    k.n = e->n;
    k.n_models = e->n_models ? e->n_models : 1;
    k.bv_result = nullptr;
    k.bv_inside = nullptr;
    k.rebuilt_mask = e->rebuilt_mask;
    k.bv_has_ctl = k.bv_ctl_entity = k.bv_on = 0;
    for (int a = 0; a < 3; a++) k.bv_cam[a] = k.bv_ctl[a] = 0.f;
    if (e->bv && (e->bv->result || e->bv->inside_mask)) {
        k.bv_on = 1;
        memcpy(k.bv_cam, e->bv->cam_pos, 12);
        memcpy(k.bv_ctl, e->bv->ctl_pos, 12);
        k.bv_has_ctl = e->bv->has_ctl;
        k.bv_ctl_entity = e->bv->ctl_entity;
        k.bv_result = reinterpret_cast<unsigned long long *>(e->bv->result);
        k.bv_inside = e->bv->inside_mask;
    }
    return k;
}

// Kernel-side frustum of a host frustum: adds the cull's constants (lmd::frustum_constants, the statement k_views_calc
// shares).
static inline lmd::FrustumK make_frustum_k(const clapgpu_frustum *frustum)
{
    static_assert(sizeof(lmd::Frustum) == sizeof(clapgpu_frustum), "frustum layout");
    lmd::FrustumK k = {};
    if (!frustum)
        return k;
    memcpy(&k.f, frustum, sizeof(k.f));
    lmd::frustum_constants(k);
    return k;
}

static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// clapgpu_entities.views for the kernels; false: a count beyond the maximum, a missing plane.  Defined in entities.hip:
// an exported symbol of the library, so one definition in one object file, not an inline one.
bool make_xviews_k(const clapgpu_entities *e, bool hostio, XViewsK *out);

static inline int check_entities(const clapgpu_entities *e, bool need_mask)
{
    if (!e || !e->pos_scale || !e->rot || !e->parent || !e->model || !e->model_table || !e->flags ||
        !e->seqs || !e->mx || !e->inv_mx || !e->aabb || !e->center)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (need_mask && (!e->vis_mask || !e->vis_row_pop))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!aligned16(e->pos_scale) || !aligned16(e->rot) || !aligned16(e->model_table) || !aligned16(e->mx) ||
        !aligned16(e->inv_mx) || !aligned16(e->aabb) || !aligned16(e->center))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    return CLAPGPU_OK;
}

} // namespace clapgpu
