// cascades.hip -- the shadow cascades on the device, for gfx950: what scene_camera_calc (core/scene.c:1004-1048) does
// behind camera_update, as ONE launch that a frame graph can hold, and the bounding-volume pick it reads.
//
//   k_cascades_calc       the camera's cascade sub-frusta (view.c:11-37), near_backup from the bounding volume
//                         (scene.c:1021-1038), the shadow light's views fitted to those frusta (view.c:195-246) and the
//                         cascades' orthographic projections (view.c:129-146); the light's main view goes into its slot
//                         of the view block's source, where clapgpu_views_calc picks it up
//   k_entities_bv_views   default_update's bounding-volume pick (model.c:1703-1713) over the boxes the update stored, with
//                         the camera position read from the view block and the control's from pos_scale
//
// k_cascades_calc is one wavefront, a lane per fit: lane v < nr owns cascade v -- the camera sub-frustum under persp[v],
// the fit, the projection -- and lane 4 the light's main view from the camera's main frustum.  No lane needs another's
// values.  A few thousand flops: the launch is latency, not work; what it buys is that the shadow passes' cull follows the
// camera the device computed.  The arithmetic is lm_dev.h's, the statement the host twins below share.
// k_entities_bv_views is a bandwidth pass like the cull's: 24 B of box and 4 B of flags per entity; model, model_table and
// pos_scale.w are read only in a wavefront where some box holds a point.
#include <string.h>
#include <math.h>
#include "common.h"
#include "lm_dev.h"
#include "views_dev.h"
#include "entities_row.h"

namespace clapgpu {

static_assert(lmd::CASCADES_Z_REVERSE == CLAPGPU_CASCADES_Z_REVERSE && lmd::CASCADES_NDC_Z_ZERO_ONE == CLAPGPU_CASCADES_NDC_Z_ZERO_ONE &&
              lmd::CASCADES_NEAR_BACKUP_FROM_BV == CLAPGPU_CASCADES_NEAR_BACKUP_FROM_BV,
              "lm_dev.h restates the header's cascades constants");
static_assert(CLAPGPU_CASCADES_MAX == CLAPGPU_EXTRA_VIEWS_MAX && CLAPGPU_CASCADES_MAX + 1 <= WAVE, "a lane per fit");

// What the block and the source must hold before anything is written: nr (0 meaning 4) or 0 when invalid
__host__ __device__ __forceinline__ uint32_t cascades_valid(const clapgpu_cascades *c, const clapgpu_views_source *src)
{
    const uint32_t nr = c->nr_cascades ? c->nr_cascades : CLAPGPU_CASCADES_MAX;
    const uint32_t slot = c->light_slot;
    if (nr > CLAPGPU_CASCADES_MAX || slot < 1 || slot >= CLAPGPU_VIEW_SLOTS) return 0;
    if (src->slot[slot].flags & CLAPGPU_VIEW_FROM_POSE) return 0;
    return nr;
}

// One fit: `lane` < nr a cascade, CLAPGPU_CASCADES_MAX the light's main view.  Reads the block's inputs and slot 0 of the
// source; writes this fit's outputs and nothing else.
__host__ __device__ __forceinline__ void cascades_fit(clapgpu_cascades *c, clapgpu_views_source *src, uint32_t lane, float near_backup)
{
    const bool main_view = lane == CLAPGPU_CASCADES_MAX;
    const clapgpu_view_source &s0 = src->slot[0];
    const uint32_t flags = c->flags;
    float v[16], p[16], mvp[16];
    if (s0.flags & CLAPGPU_VIEW_FROM_POSE) {
        const float pos[3] = { s0.pos[0], s0.pos[1], s0.pos[2] }, q[4] = { s0.quat[0], s0.quat[1], s0.quat[2], s0.quat[3] };
        lmd::view_matrix(v, pos, q);
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) v[i] = s0.view_mx[i];
    }
    const float *pm = main_view ? s0.proj_mx : c->persp[lane];
#pragma unroll
    for (int i = 0; i < 16; i++) p[i] = pm[i];
    lmd::Frustum f;
    lmd::frustum_calc(f, mvp, v, p, (flags & CLAPGPU_CASCADES_NDC_Z_ZERO_ONE) != 0);
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int k = 0; k < 4; k++) c->cam_corners[lane][i][k] = f.corners[i][k];

    const float dir[3] = { c->light_dir[0], c->light_dir[1], c->light_dir[2] };
    float view[16], inv_view[16];
    lmd::cascade_fit(view, inv_view, f.corners, dir, near_backup);
    if (main_view) {
        float *slot_mx = src->slot[c->light_slot].view_mx;
#pragma unroll
        for (int i = 0; i < 16; i++) { c->view_mx[i] = view[i]; c->inv_view_mx[i] = inv_view[i]; slot_mx[i] = view[i]; }
        return;
    }
    float proj[16], inv_proj[16], far_plane;
    lmd::cascade_projection(proj, inv_proj, mvp, far_plane, view, f.corners, flags);
    clapgpu_cascade_view &o = c->cascade[lane];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        o.view_mx[i] = view[i]; o.inv_view_mx[i] = inv_view[i];
        o.proj_mx[i] = proj[i]; o.inv_proj_mx[i] = inv_proj[i];
        o.mvp[i] = mvp[i];
    }
    o.near_plane = 0.1f;
    o.far_plane = far_plane;
}

struct CascadesEntK {                                   // what near_backup reads of the frame's entities
    uint32_t n, n_models;
    const float4 *pos_scale;
    const int32_t *model;
    const float4 *model_table;
};

__global__ __launch_bounds__(WAVE)
void k_cascades_calc(clapgpu_cascades *c, clapgpu_views_source *src, CascadesEntK e, const unsigned long long *bv_result)
{
    const uint32_t lane = threadIdx.x;
    uint32_t nr = cascades_valid(c, src);
    // near_backup: every lane resolves it for itself (the same loads of the same few words)
    float nb = c->near_backup;
    uint32_t env = CLAPGPU_CASCADES_NO_ENTITY;
    if (nr && (c->flags & CLAPGPU_CASCADES_NEAR_BACKUP_FROM_BV)) {
        if (!bv_result) {
            nr = 0;
        } else {
            const unsigned long long key = *bv_result;
            nb = 0.0f;
            if (key) {
                env = 0xFFFFFFFFu - (uint32_t)key;
                if (env >= e.n) {
                    nr = 0;
                } else {
                    const float4 ps = e.pos_scale[env];
                    const int32_t mraw = e.model[env];
                    const int32_t mi = (uint32_t)mraw < e.n_models ? mraw : 0;      // as the pick reads the table (entities_row.h)
                    const float4 blo = e.model_table[2 * mi], bhi = e.model_table[2 * mi + 1];
                    const float lo[3] = { blo.x, blo.y, blo.z }, hi[3] = { bhi.x, bhi.y, bhi.z };
                    const float dir[3] = { c->light_dir[0], c->light_dir[1], c->light_dir[2] };
                    nb = lmd::near_backup(dir, lo, hi, ps.w);
                }
            }
        }
    }
    if (nr == 0) {
        if (lane == 0) c->status = CLAPGPU_CASCADES_INVALID;
        return;
    }
    if (lane == 0) {
        c->near_backup_used = lmd::one_nan(nb);
        c->bv_entity = env;
        c->status = 0;
    }
    if (lane < nr || lane == CLAPGPU_CASCADES_MAX)
        cascades_fit(c, src, lane, nb);
}

// model.c:1703-1713 as entities_row.h:443-471 has it, over stored boxes
__global__ __launch_bounds__(ENT_BLOCK)
void k_entities_bv_views(const uint32_t *flags, const float *aabb, const int32_t *model, const float4 *model_table,
                         const float4 *pos_scale, uint32_t n, uint32_t n_models, const clapgpu_views_state *st, uint32_t has_ctl,
                         uint32_t ctl_entity, unsigned long long *result, uint64_t *inside_words)
{
    const uint32_t i = blockIdx.x * ENT_BLOCK + threadIdx.x;
    const int lane = lane_id();
    if ((i - lane) >= n) return;                         // a wavefront past the end
    const bool in_range = i < n;
    const float cam[3] = { st->slot[0].cam_pos[0], st->slot[0].cam_pos[1], st->slot[0].cam_pos[2] };
    float ctl[3] = { 0.f, 0.f, 0.f };
    if (has_ctl && ctl_entity >= n) has_ctl = 0;
    if (has_ctl) {
        const float4 cp = pos_scale[ctl_entity];
        ctl[0] = cp.x; ctl[1] = cp.y; ctl[2] = cp.z;
    }
    uint32_t fl = 0;
    float bb[6] = { 0, 0, 0, 0, 0, 0 };
    if (in_range) {
        fl = flags[i];
#pragma unroll
        for (int k = 0; k < 6; k++) bb[k] = aabb[6 * (size_t)i + k];
    }
    bool inside = in_range && (fl & CLAPGPU_E_ALIVE) && point_in_box(cam, bb);
    if (!inside && has_ctl)
        inside = in_range && (fl & CLAPGPU_E_ALIVE) && point_in_box(ctl, bb);
    if (inside && has_ctl && i == ctl_entity)
        inside = false;
    const uint64_t inside_mask = __ballot(inside);
    if (inside_words && lane == 0) inside_words[i >> 6] = inside_mask;
    if (inside_mask && result) {                         // rare: almost no box contains the camera
        unsigned long long key = 0;
        if (inside) {
            int32_t mi = model[i];
            if ((uint32_t)mi >= n_models) mi = 0;
            const float4 lo = model_table[2 * mi], hi = model_table[2 * mi + 1];
            const float s = pos_scale[i].w;
            const float X = fabsf(hi.x - lo.x) * s, Y = fabsf(hi.y - lo.y) * s, Z = fabsf(hi.z - lo.z) * s;
            const float vol = X * Y * Z;
            key = ((unsigned long long)__float_as_uint(vol) << 32) | (0xFFFFFFFFu - i);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(key, off);
            key = o > key ? o : key;
        }
        if (lane == 0 && key)
            atomicMax(result, key);
    }
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" int clapgpu_cascades_calc(void *stream, clapgpu_cascades *c, clapgpu_views_source *source, const clapgpu_entities *e,
                                     const uint64_t *bv_result)
{
    if (!view_block_ok(c) || !view_block_ok(source) || !e) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (bv_result && (!e->pos_scale || !e->model || !e->model_table)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    CascadesEntK ek;
    ek.n = bv_result ? e->n : 0;
    ek.n_models = e->n_models ? e->n_models : 1;
    ek.pos_scale = reinterpret_cast<const float4 *>(e->pos_scale);
    ek.model = e->model;
    ek.model_table = reinterpret_cast<const float4 *>(e->model_table);
    hipLaunchKernelGGL(k_cascades_calc, dim3(1), dim3(WAVE), 0, as_stream(stream), c, source, ek,
                       reinterpret_cast<const unsigned long long *>(bv_result));
    CLAPGPU_LAUNCH_CHECK("k_cascades_calc");
    return CLAPGPU_OK;
}

extern "C" float clapgpu_cascades_near_backup(const float light_dir[3], const float env_box_lo[3], const float env_box_hi[3],
                                              float env_scale)
{
    float d[3], lo[3], hi[3];
    memcpy(d, light_dir, sizeof(d)); memcpy(lo, env_box_lo, sizeof(lo)); memcpy(hi, env_box_hi, sizeof(hi));
    return lmd::near_backup(d, lo, hi, env_scale);
}

extern "C" void clapgpu_cascades_calc_host(clapgpu_cascades *c, clapgpu_views_source *source, const float env_box_lo[3],
                                           const float env_box_hi[3], float env_scale, int has_env)
{
    const uint32_t nr = cascades_valid(c, source);
    if (nr == 0) { c->status = CLAPGPU_CASCADES_INVALID; return; }
    float nb = c->near_backup;
    uint32_t env = CLAPGPU_CASCADES_NO_ENTITY;
    if (c->flags & CLAPGPU_CASCADES_NEAR_BACKUP_FROM_BV) {
        nb = 0.0f;
        if (has_env) {
            env = 0;
            nb = clapgpu_cascades_near_backup(c->light_dir, env_box_lo, env_box_hi, env_scale);
        }
    }
    c->near_backup_used = lmd::one_nan(nb);
    c->bv_entity = env;
    c->status = 0;
    for (uint32_t v = 0; v < nr; v++) cascades_fit(c, source, v, nb);
    cascades_fit(c, source, CLAPGPU_CASCADES_MAX, nb);
}

// view.c:13-26: the splits; view.c:33: the projections
extern "C" void clapgpu_cascades_persp(float fov, float aspect, float near_plane, float far_plane, uint32_t nr_cascades,
                                       int ndc_z_zero_one, float persp[64])
{
    static const float dividers[CLAPGPU_CASCADES_MAX - 1] = { 15, 50, 150 };
    const uint32_t max = nr_cascades && nr_cascades <= CLAPGPU_CASCADES_MAX ? nr_cascades : CLAPGPU_CASCADES_MAX;
    float n = near_plane;
    for (uint32_t i = 0; i < max; i++) {
        const float f = i + 1 < max ? dividers[i] : far_plane;
        clapgpu_perspective(fov, aspect, n, f, ndc_z_zero_one, persp + 16 * i);
        n = f;
    }
}

extern "C" int clapgpu_entities_bv_views(void *stream, const clapgpu_entities *e, const clapgpu_views_state *state,
                                         uint32_t has_ctl, uint32_t ctl_entity, uint64_t *result, uint64_t *inside_mask)
{
    if (!view_block_ok(state) || !e || !e->flags || !e->aabb || !e->model || !e->model_table || !e->pos_scale)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!result && !inside_mask) return CLAPGPU_OK;      // nothing asked for: as the update with such a clapgpu_bv_query
    if (result)
        CLAPGPU_HIP(hipMemsetAsync(result, 0, sizeof(uint64_t), as_stream(stream)));
    if (e->n == 0) return CLAPGPU_OK;
    hipLaunchKernelGGL(k_entities_bv_views, dim3((e->n + ENT_BLOCK - 1) / ENT_BLOCK), dim3(ENT_BLOCK), 0, as_stream(stream),
                       e->flags, e->aabb, e->model, reinterpret_cast<const float4 *>(e->model_table),
                       reinterpret_cast<const float4 *>(e->pos_scale), e->n, e->n_models ? e->n_models : 1, state,
                       has_ctl, ctl_entity, reinterpret_cast<unsigned long long *>(result), inside_mask);
    CLAPGPU_LAUNCH_CHECK("k_entities_bv_views");
    return CLAPGPU_OK;
}
