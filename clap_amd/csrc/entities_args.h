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

// Kernel-side frustum: adds the per-axis extremes of the frustum corners (NaN if any corner is
// NaN, so the comparison is false exactly when the reference's count cannot reach 8) and a flag
// telling whether every plane component is finite.
static inline lmd::FrustumK make_frustum_k(const clapgpu_frustum *frustum)
{
    static_assert(sizeof(lmd::Frustum) == sizeof(clapgpu_frustum), "frustum layout");
    lmd::FrustumK k = {};
    if (!frustum)
        return k;
    memcpy(&k.f, frustum, sizeof(k.f));
    for (int ax = 0; ax < 3; ax++) {
        float lo = INFINITY, hi = -INFINITY;
        bool nan = false;
        for (int i = 0; i < 8; i++) {
            const float c = k.f.corners[i][ax];
            nan = nan || (c != c);
            lo = c < lo ? c : lo;
            hi = c > hi ? c : hi;
        }
        k.cmin[ax] = nan ? NAN : lo;
        k.cmax[ax] = nan ? NAN : hi;
    }
    k.finite = 1;
    for (int i = 0; i < 6; i++)
        for (int c = 0; c < 4; c++)
            if (!(fabsf(k.f.planes[i][c]) <= 3.402823466e+38f))
                k.finite = 0;
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
