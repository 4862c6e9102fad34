/*
 * gpu-scene-draw.c -- what the render passes ask of the entity binding (gpu-scene.c; shared declarations in
 * gpu-scene-internal.h): the registered views that ride the update's launch, the frustum verdict per entity, the LOD pick
 * and the draw lists (whole, and grouped by txmodel), and the scene dump for replay.
 */
#include "gpu-scene-internal.h"

/* the registered views ride the update's launch: their frusta to the mirror (those that are not the main view itself) */
int gs_views_before_update(struct gpu_scene *gs, struct view *view)
{
    clapgpu_frustum xfr[GPU_SCENE_EXTRA_VIEWS];
    uint32_t n = 0;
    for (uint32_t k = 0; k < gs->n_xview; k++) {
        gs->xslot[k] = -1;
        gs->xchecked[k] = gs->xok[k] = false;
        if (!view || gs->xview[k] == view) continue;
        frustum_of(gs->xview[k], &xfr[n]);
        memcpy(gs->xplanes[k], gs->xview[k]->main.frustum_planes, sizeof(gs->xplanes[k]));
        gs->xslot[k] = (int)n++;
    }
    gs->stats.views_culled = (view != NULL) + n;
    return clapgpu_scene_set_views(gs->scene, n, n ? xfr : NULL);
}

/* which registered view is `view` (and has a mask from the last update)?  -1: none */
static int xview_of(const struct gpu_scene *gs, const struct view *view)
{
    for (uint32_t k = 0; k < gs->n_xview; k++)
        if (gs->xview[k] == view) return gs->xslot[k] >= 0 ? (int)k : -1;
    return -1;
}

int gpu_scene_add_view(struct gpu_scene *gs, struct view *view)
{
    if (!gs || !view) return _CERR_INVALID_ARGUMENTS;
    for (uint32_t k = 0; k < gs->n_xview; k++) if (gs->xview[k] == view) return 0;
    if (gs->n_xview == GPU_SCENE_EXTRA_VIEWS) return _CERR_TOO_LARGE;
    gs->xview[gs->n_xview] = view;
    gs->xslot[gs->n_xview++] = -1;                               /* culled from the next update on */
    return 0;
}

void gpu_scene_remove_view(struct gpu_scene *gs, struct view *view)
{
    if (!gs) return;
    for (uint32_t k = 0; k < gs->n_xview; k++) {
        if (gs->xview[k] != view) continue;
        /* the mirror's planes keep their order until the next update: the others' slots stand */
        for (uint32_t j = k; j + 1 < gs->n_xview; j++) {
            gs->xview[j] = gs->xview[j + 1]; gs->xslot[j] = gs->xslot[j + 1];
            memcpy(gs->xplanes[j], gs->xplanes[j + 1], sizeof(gs->xplanes[j]));
            gs->xchecked[j] = gs->xchecked[j + 1]; gs->xok[j] = gs->xok[j + 1];
        }
        gs->n_xview--;
        return;
    }
}

/* view_calc_frustum() ran for `view` (view.c:291): the next verdict for it re-culls on the device if the planes changed */
void gpu_scene_view_changed(struct gpu_scene *gs, struct view *view)
{
    if (!gs) return;
    if (view == gs->culled_view) gs->cull_checked = false;
    for (uint32_t k = 0; k < gs->n_xview; k++)
        if (gs->xview[k] == view) gs->xchecked[k] = false;
}

/* The mask that answers for `view`, current for the planes the view holds NOW: the main view's (the one the last update
 * was given) or a registered view's own plane -- compared once per frustum, not per entity; planes that moved since the
 * launch that culled them cost one cull launch (every view of the frame for the main one, the one view alone otherwise).
 * NULL: the device has no answer for this view (not known to the last update, or the re-cull failed). */
static const uint64_t *mask_for_view(struct gpu_scene *gs, struct view *view)
{
    if (view == gs->culled_view) {
        if (!gs->cull_checked) {
            gs->cull_checked = true;
            gs->cull_ok = !memcmp(gs->culled_planes, view->main.frustum_planes, sizeof(gs->culled_planes));
            if (!gs->cull_ok) {
                clapgpu_frustum fr;
                frustum_of(view, &fr);
                gs->stats.cull_launches_after_update++;
                if (!clapgpu_scene_cull(gs->scene, &fr)) {
                    memcpy(gs->culled_planes, view->main.frustum_planes, sizeof(gs->culled_planes));
                    gs->cull_ok = true;
                    gs_consume_fetched(gs);                         /* GPU_SCATTER_DRAWN: what the new planes bring into view */
                }
            }
        }
        return gs->cull_ok ? gs->res.vis_mask : NULL;
    }
    const int k = xview_of(gs, view);
    if (k < 0) return NULL;
    if (!gs->xchecked[k]) {
        gs->xchecked[k] = true;
        gs->xok[k] = !memcmp(gs->xplanes[k], view->main.frustum_planes, sizeof(gs->xplanes[k]));
        if (!gs->xok[k]) {
            clapgpu_frustum fr;
            frustum_of(view, &fr);
            gs->stats.cull_launches_after_update++;
            if (!clapgpu_scene_cull_view(gs->scene, (uint32_t)gs->xslot[k], &fr)) {
                memcpy(gs->xplanes[k], view->main.frustum_planes, sizeof(gs->xplanes[k]));
                gs->xok[k] = true;
                gs_consume_fetched(gs);
            }
        }
    }
    return (gs->xok[k] && (uint32_t)gs->xslot[k] < gs->res.n_views) ? gs->res.view_mask[gs->xslot[k]] : NULL;
}

bool gpu_view_entity_in_frustum(struct gpu_scene *gs, struct view *view, entity3d *e)
{
    const uint64_t *mask = gs ? mask_for_view(gs, view) : NULL;
    if (mask) {
        if (gs->notify && gs->vis_cursor < gs->n_order && gs->vq_e[gs->vis_cursor] == e) {
            /* notification mode, asked in list order (model.c:958-973): the table answers */
            const uint32_t c = gs->vis_cursor;
            gs->vis_cursor = c + 1 < gs->n_order ? c + 1 : 0;
            if (gs->vq_ok[c])
                return (mask[gs->vq_slot[c] >> 6] >> (gs->vq_slot[c] & 63)) & 1;
        } else {
            /* _models_render asks in list order (model.c:958-973): try the next record of the walk first */
            uint32_t i;
            if (gs->vis_cursor < gs->n_order && gs->rec[gs->order[gs->vis_cursor]].e == e)
                i = gs->order[gs->vis_cursor];
            else
                i = rec_find(gs, e);
            const struct gs_rec *r = i != NO_REC ? &gs->rec[i] : NULL;
            if (r) gs->vis_cursor = r->order_pos + 1 < gs->n_order ? r->order_pos + 1 : 0;
            /* the mask bit is the draw predicate ALIVE && VISIBLE && (SKIP_CULLING || in frustum):
             * for an alive, visible, culled entity it is the frustum test itself */
            if (r && r->gen == gs->gen && r->cls == 1) {
                /* with notifications an untouched record's flags ARE the entity's: the 448-byte struct is not read at all */
                const uint32_t fl = (gs->notify && !r->pending) ? r->flags : (e->flags & (ENTITY3D_ALIVE | 0xffffu));
                if (fl == r->flags &&
                    (fl & (ENTITY3D_ALIVE | ENTITY3D_VISIBLE | ENTITY3D_SKIP_CULLING)) == (ENTITY3D_ALIVE | ENTITY3D_VISIBLE))
                    return (mask[r->slot >> 6] >> (r->slot & 63)) & 1;
            }
        }
    }
    /* the reference's test reads e->aabb: under GPU_SCATTER_DRAWN an entity nobody draws (hidden, or asked about out of
     * turn) may not have been shown its latest box yet */
    if (gs && gs->any_pend) gpu_scene_fetch(gs, e);
    return view_entity_in_frustum(view, e);
}

/*
 * _models_render's per-entity block (model.c:959-992) for one entity on the host -- the engine's own predicates,
 * entity3d_aabb_avg_edge and entity3d_set_lod around the five lines of glue between them -- for the entities the
 * device does not hold (foreign hooks, physics bodies, ...).  Returns whether the pass draws the entity.
 */
static bool lod_pick_host(struct view *view, entity3d *e, const float *cam_pos)
{
    if (!entity3d_matches(e, ENTITY3D_ALIVE) || !entity3d_matches(e, ENTITY3D_VISIBLE))
        return false;
    if (!entity3d_matches(e, ENTITY3D_SKIP_CULLING) && view && !view_entity_in_frustum(view, e))
        return false;
    if (cam_pos) {
        if (e->force_lod >= 0) {
            e->cur_lod = e->force_lod;
        } else if (!aabb_point_is_inside(e->aabb, cam_pos)) {       /* only when the camera is outside the box */
            vec3 dist;
            vec3_sub(dist, e->aabb_center, cam_pos);
            const float side = entity3d_aabb_avg_edge(e);
            const float scale = fabsf(vec3_mul_inner(dist, dist) - side * side) / 3600.0;
            entity3d_set_lod(e, (int)scale, false);
        }
    }
    return true;
}

static int draw_push(struct gpu_scene *gs, entity3d *e, int lod, uint32_t txm)
{
    if (gs->n_draw == gs->cap_draw) {
        const uint32_t cap = gs->cap_draw ? 2 * gs->cap_draw : 4096;
        entity3d **d = realloc(gs->draw, (size_t)cap * sizeof(*d));
        if (!d) return _CERR_NOMEM;
        gs->draw = d;
        int32_t *l = realloc(gs->draw_lod, (size_t)cap * sizeof(*l));
        if (!l) return _CERR_NOMEM;
        gs->draw_lod = l;
        uint16_t *t = realloc(gs->draw_txm, (size_t)cap * sizeof(*t));
        if (!t) return _CERR_NOMEM;
        gs->draw_txm = t;
        gs->cap_draw = cap;
    }
    if (txm == 0xffffffffu && (txm = txm_index(gs, e->txmodel)) == 0xffffffffu) return _CERR_NOMEM;
    gs->draw[gs->n_draw] = e;
    gs->draw_txm[gs->n_draw] = (uint16_t)txm;
    gs->draw_lod[gs->n_draw++] = lod;
    return 0;
}

static int draw_reserve(struct gpu_scene *gs, uint32_t n)
{
    if (n <= gs->cap_draw) return 0;
    uint32_t cap = gs->cap_draw ? gs->cap_draw : 4096;
    while (cap < n) cap *= 2;
    entity3d **d = realloc(gs->draw, (size_t)cap * sizeof(*d));
    if (d) gs->draw = d;
    int32_t *l = realloc(gs->draw_lod, (size_t)cap * sizeof(*l));
    if (l) gs->draw_lod = l;
    uint16_t *t = realloc(gs->draw_txm, (size_t)cap * sizeof(*t));
    if (t) gs->draw_txm = t;
    if (!d || !l || !t) return _CERR_NOMEM;
    gs->cap_draw = cap;
    return 0;
}

/* entries [lo, hi) of the device's draw list into the binding's (gpu_scene_select_lod, a list too long for one thread) */
struct draw_ctx { struct gpu_scene *gs; const clapgpu_scene_arrays *res; const uint32_t *slots; const int32_t *lods; uint32_t holes; };
static void draw_range(void *ctx, uint32_t lo, uint32_t hi)
{
    struct draw_ctx *dc = ctx;
    struct gpu_scene *gs = dc->gs;
    uint32_t holes = 0;
    for (uint32_t k = lo; k < hi; k++) {
        const uint32_t slot = dc->slots[k];
        const int32_t lod = dc->lods[k];
        entity3d *e = gs->slot_ent[slot];
        if (e && lod != gs->slot_lod[slot] && lod >= -128 && lod <= 127) {
            e->cur_lod = lod;                                    /* as model.c:977 / entity3d_set_lod leave it */
            gs->slot_lod[slot] = (int8_t)lod;
            const uint32_t tag = (uint32_t)(uintptr_t)dc->res->slot_user[slot];
            if (tag) gs->rec[tag - 1].lod_cur = lod;
            clapgpu_scene_lod_picked(gs->scene, slot, lod);
        }
        gs->draw[k] = e; gs->draw_lod[k] = lod; gs->draw_txm[k] = e ? gs->slot_txm[slot] : 0;
        holes += !e;
    }
    if (holes) __atomic_fetch_add(&dc->holes, holes, __ATOMIC_RELAXED);
}

void gpu_scene_lod_changed(struct gpu_scene *gs, entity3d *e)
{
    if (!gs || !e) return;
    const uint32_t i = rec_find(gs, e);
    if (i == NO_REC) return;
    struct gs_rec *r = &gs->rec[i];
    if (r->handle == CLAPGPU_NO_ENTITY || (e->force_lod == r->lod_force && e->cur_lod == r->lod_cur)) return;
    if (!clapgpu_scene_entity_lod(gs->scene, r->handle, e->force_lod, e->cur_lod)) {
        r->lod_force = e->force_lod; r->lod_cur = e->cur_lod;
        if (r->slot < gs->cap_slot_arrays) {
            if (e->cur_lod >= -128 && e->cur_lod <= 127) gs->slot_lod[r->slot] = (int8_t)e->cur_lod;
            else gs->cap_slot_arrays = 0;                        /* out of the byte's range: the record path */
        }
    }
}

int gpu_scene_select_lod(struct gpu_scene *gs, struct view *view, const float *cam_pos)
{
    if (!gs) return _CERR_INVALID_ARGUMENTS;
    gs->n_draw = 0;
    gs->groups_valid = false;
    /* entities came or went since the frame's update (notification mode knows): the list would miss what the reference's
     * walk of the txmodels draws -- this pass is the reference's */
    if (gs->notify && (gs->topology_pending || gs->n_created)) return _CERR_NOT_SUPPORTED;
    /* the mask that lists what the pass draws: the main view's or a registered view's own, re-culled if its planes moved; a
     * view the last update did not know takes the main view's place (one cull launch, and the main mask is its from now on) */
    uint32_t of_view = CLAPGPU_SCENE_MAIN_VIEW;
    if (view) {
        const int xk = view != gs->culled_view ? xview_of(gs, view) : -1;
        if (xk >= 0) {
            if (!mask_for_view(gs, view)) return _CERR_NOT_SUPPORTED;
            of_view = (uint32_t)gs->xslot[xk];
        } else if (view != gs->culled_view) {
            clapgpu_frustum fr;
            frustum_of(view, &fr);
            gs->stats.cull_launches_after_update++;
            CK(clapgpu_scene_cull(gs->scene, &fr));
            gs_consume_fetched(gs);                                 /* GPU_SCATTER_DRAWN: what the new planes bring into view */
            memcpy(gs->culled_planes, view->main.frustum_planes, sizeof(gs->culled_planes));
            gs->culled_view = view;
            gs->cull_checked = gs->cull_ok = true;
        } else if (!mask_for_view(gs, view)) {
            return _CERR_NOT_SUPPORTED;
        }
    }
    /* models whose LOD range moved since they were registered (model3d's mesh LODs are added at load time) */
    for (uint32_t k = 0; k < gs->n_models; k++) {
        struct gs_model *gm = &gs->models[k];
        if (gm->lod_min != gm->model->lod_min || gm->lod_max != gm->model->lod_max) {
            CK(clapgpu_scene_model_lods(gs->scene, gm->handle, gm->model->lod_min, gm->model->lod_max));
            gm->lod_min = gm->model->lod_min; gm->lod_max = gm->model->lod_max;
        }
    }
    /* a frame that is walked re-reads every batched entity's force_lod / cur_lod anyway (mirror()); in notification
     * mode the engine's entity3d_set_lod reports them (gpu-exports.inc.c -> gpu_scene_lod_changed) */
    uint32_t n = 0;
    bool device_ok = true;                                       /* false: no update has run on the device yet -- everything below by the host block */
    if (!view) {
        /* A pass without a view draws every ALIVE and VISIBLE entity (model.c:969-970: `view && !view_entity_in_frustum`);
         * the device's mask answers for the frustum of the last update, not for "no frustum": the reference's own block
         * for every entity, batched ones included (their mirrored LODs follow below), on current host fields */
        CK(gpu_scene_fetch_all(gs));
        device_ok = false;
    } else
    if (gs->n_batched) {
        const int rc = clapgpu_scene_select_lod_view(gs->scene, of_view, cam_pos, &n);
        if (rc && rc != CLAPGPU_ERR_NOT_SUPPORTED) return rc;
        device_ok = !rc;
    }
    clapgpu_scene_arrays res;
    const uint32_t *slots = NULL; const int32_t *lods = NULL;
    if (n && !clapgpu_scene_results(gs->scene, &res) && clapgpu_scene_draw_list(gs->scene, &slots, &lods) == n) {
        const bool by_slot = gs->cap_slot_arrays >= res.n_slots;
        if (by_slot && cam_pos && n >= GS_MIRROR_PAR_MIN && gs_par_threads() > 1 && !draw_reserve(gs, n)) {
            /* a long list: the gather on the workers (entry k -> draw[k]: nothing shared but the arrays) */
            struct draw_ctx dc = { gs, &res, slots, lods, 0 };
            gpu_scene_par_for(draw_range, &dc, n, gs_par_threads());
            gs->n_draw = n;
            if (dc.holes) {                                      /* lanes vacated since the update (gpu_scene_entity_deleting): out */
                uint32_t w = 0;
                for (uint32_t k = 0; k < n; k++) {
                    if (!gs->draw[k]) continue;
                    gs->draw[w] = gs->draw[k]; gs->draw_lod[w] = gs->draw_lod[k]; gs->draw_txm[w] = gs->draw_txm[k];
                    w++;
                }
                gs->n_draw = w;
            }
        } else
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t slot = slots[k];
            if (by_slot) {
                /* three arrays read in ascending slot order; an entity3d (and its record) only when the pick changed its LOD */
                entity3d *e = gs->slot_ent[slot];
                if (!e) continue;
                if (cam_pos && lods[k] != gs->slot_lod[slot] && lods[k] >= -128 && lods[k] <= 127) {
                    e->cur_lod = lods[k];                           /* as model.c:977 / entity3d_set_lod leave it */
                    gs->slot_lod[slot] = (int8_t)lods[k];
                    const uint32_t tag = (uint32_t)(uintptr_t)res.slot_user[slot];
                    if (tag) gs->rec[tag - 1].lod_cur = lods[k];
                    clapgpu_scene_lod_picked(gs->scene, slot, lods[k]);
                }
                CK(draw_push(gs, e, lods[k], gs->slot_txm[slot]));
                continue;
            }
            const uint32_t tag = (uint32_t)(uintptr_t)res.slot_user[slot];
            if (!tag) continue;
            struct gs_rec *r = &gs->rec[tag - 1];
            if (!r->e || r->gen != gs->gen || (r->cls != 1 && r->cls != 4)) continue;
            if (cam_pos && r->lod_cur != lods[k]) clapgpu_scene_lod_picked(gs->scene, slot, lods[k]);
            r->e->cur_lod = lods[k];                                /* as model.c:977 / entity3d_set_lod leave it */
            r->lod_cur = lods[k];
            CK(draw_push(gs, r->e, lods[k], 0xffffffffu));
        }
    }
    /* the entities the device does not hold, in list order, by the reference's own block: the host-class ones -- the two
     * lists the walk keeps of them (own hook now / behind the pose), merged by their place in the queue; NOT a scan of every
     * record for the few that are not batched (1 M records: 3-4 ms of a 5 ms call) */
    if (device_ok) {
        uint32_t a = 0, b = 0;
        while (a < gs->n_host || b < gs->n_deferred) {
            const uint64_t ka = a < gs->n_host ? gs->rec[gs->host_list[a]].order_key : UINT64_MAX;
            const uint64_t kb = b < gs->n_deferred ? gs->rec[gs->deferred[b]].order_key : UINT64_MAX;
            struct gs_rec *r = ka <= kb ? &gs->rec[gs->host_list[a++]] : &gs->rec[gs->deferred[b++]];
            if (!r->e || r->cls == 1 || r->cls == 4) continue;
            if (lod_pick_host(view, r->e, cam_pos))
                CK(draw_push(gs, r->e, r->e->cur_lod, 0xffffffffu));
        }
        return 0;
    }
    for (uint32_t k = 0; k < gs->n_order; k++) {
        struct gs_rec *r = &gs->rec[gs->order[k]];
        if (!r->e) continue;
        if (lod_pick_host(view, r->e, cam_pos))
            CK(draw_push(gs, r->e, r->e->cur_lod, 0xffffffffu));
        if ((r->cls == 1 || r->cls == 4) && r->handle != CLAPGPU_NO_ENTITY && r->e->cur_lod != r->lod_cur &&
            !clapgpu_scene_entity_lod(gs->scene, r->handle, r->e->force_lod, r->e->cur_lod)) {
            r->lod_force = r->e->force_lod; r->lod_cur = r->e->cur_lod;   /* the host block picked for a batched entity: the mirror follows */
            if (r->slot < gs->cap_slot_arrays && r->e->cur_lod >= -128 && r->e->cur_lod <= 127) gs->slot_lod[r->slot] = (int8_t)r->e->cur_lod;
        }
    }
    return 0;
}

uint32_t gpu_scene_visible(struct gpu_scene *gs, entity3d ***ents, const int32_t **lods)
{
    if (!gs) return 0;
    if (ents) *ents = gs->draw;
    if (lods) *lods = gs->draw_lod;
    return gs->n_draw;
}

/* the draw list grouped by txmodel (a stable counting sort, once per gpu_scene_select_lod and only when asked for) */
static int draw_group(struct gpu_scene *gs)
{
    if (gs->groups_valid) return 0;
    gs->n_groups = 0;
    if (gs->n_draw > gs->cap_draw_g) {
        entity3d **d = realloc(gs->draw_g, (size_t)gs->cap_draw * sizeof(*d));
        if (!d) return _CERR_NOMEM;
        gs->draw_g = d;
        int32_t *l = realloc(gs->draw_g_lod, (size_t)gs->cap_draw * sizeof(*l));
        if (!l) return _CERR_NOMEM;
        gs->draw_g_lod = l;
        gs->cap_draw_g = gs->cap_draw;
    }
    /* a stable counting sort over the entries' txmodel indices: the entities themselves are not read */
    if (gs->n_txms > gs->cap_groups) {
        struct gs_draw_group *q = realloc(gs->groups, (size_t)gs->n_txms * sizeof(*q));
        if (!q) return _CERR_NOMEM;
        gs->groups = q; gs->cap_groups = gs->n_txms;
    }
    gs->n_groups = gs->n_txms;
    for (uint32_t g = 0; g < gs->n_groups; g++) gs->groups[g] = (struct gs_draw_group){ .txm = gs->txms[g], .start = 0, .n = 0 };
    for (uint32_t k = 0; k < gs->n_draw; k++) gs->groups[gs->draw_txm[k]].n++;
    uint32_t at = 0;
    for (uint32_t g = 0; g < gs->n_groups; g++) { gs->groups[g].start = at; at += gs->groups[g].n; gs->groups[g].n = 0; }
    for (uint32_t k = 0; k < gs->n_draw; k++) {
        struct gs_draw_group *grp = &gs->groups[gs->draw_txm[k]];
        const uint32_t pos = grp->start + grp->n++;
        gs->draw_g[pos] = gs->draw[k];
        gs->draw_g_lod[pos] = gs->draw_lod[k];
    }
    gs->groups_valid = true;
    return 0;
}

uint32_t gpu_scene_visible_of(struct gpu_scene *gs, const model3dtx *txm, entity3d ***ents, const int32_t **lods)
{
    if (!gs || !txm || draw_group(gs)) return 0;
    for (uint32_t g = 0; g < gs->n_groups; g++)
        if (gs->groups[g].txm == txm) {
            if (ents) *ents = gs->draw_g + gs->groups[g].start;
            if (lods) *lods = gs->draw_g_lod + gs->groups[g].start;
            return gs->groups[g].n;
        }
    return 0;
}

int gpu_scene_snapshot_begin(struct gpu_scene *gs, const char *path, struct clapgpu_snapshot_writer **out)
{
    if (!gs || !path || !out) return _CERR_INVALID_ARGUMENTS;
    uint32_t n = 0;
    for (uint32_t k = 0; k < gs->n_order; k++) n += gs->rec[gs->order[k]].cls == 1;
    const uint32_t nm = gs->n_models ? gs->n_models : 1;
    uint32_t *index_of = malloc((size_t)(gs->n_rec ? gs->n_rec : 1) * 4);       /* record -> row of the dump */
    float *pos_scale = calloc((size_t)(n ? n : 1) * 4, 4), *rot = calloc((size_t)(n ? n : 1) * 4, 4);
    int32_t *parent = calloc(n ? n : 1, 4), *model = calloc(n ? n : 1, 4);
    uint32_t *flags = calloc(n ? n : 1, 4), *seqs = calloc(n ? n : 1, 4);
    float *maabb = calloc((size_t)nm * 6, 4);
    uint8_t *mskip = calloc(nm, 1);
    int rc = _CERR_NOMEM;
    clapgpu_snapshot_writer *w = NULL;
    if (!index_of || !pos_scale || !rot || !parent || !model || !flags || !seqs || !maabb || !mskip) goto done;
    uint32_t row = 0;
    for (uint32_t k = 0; k < gs->n_order; k++)
        if (gs->rec[gs->order[k]].cls == 1) index_of[gs->order[k]] = row++;
    for (uint32_t k = 0; k < gs->n_order; k++) {
        struct gs_rec *r = &gs->rec[gs->order[k]];
        if (r->cls != 1) continue;
        entity3d *e = r->e;
        const uint32_t i = index_of[gs->order[k]];
        memcpy(pos_scale + 4 * (size_t)i, transform_pos(&e->xform, NULL), 12);
        pos_scale[4 * (size_t)i + 3] = e->scale;
        memcpy(rot + 4 * (size_t)i, transform_rotation_quat(&e->xform), 16);
        parent[i] = e->parent ? (int32_t)index_of[parent_rec(gs, r)] : -1;
        flags[i] = (e->flags & (ENTITY3D_ALIVE | 0xffffu)) | CLAPGPU_E_DIRTY;     /* a replay rebuilds everything */
        for (uint32_t m = 0; m < gs->n_models; m++)
            if (gs->models[m].model == r->model) model[i] = (int32_t)m;
    }
    for (uint32_t m = 0; m < gs->n_models; m++) {
        const model3d *md = gs->models[m].model;
        const float a[6] = { md->aabb[0][0], md->aabb[0][1], md->aabb[0][2], md->aabb[1][0], md->aabb[1][1], md->aabb[1][2] };
        memcpy(maabb + 6 * (size_t)m, a, 24);
        mskip[m] = md->skip_aabb;
    }
    rc = clapgpu_snapshot_create(&w, path);
    if (rc) goto done;
    const int64_t n64 = n;
#define ADD(name, dt, nd, d0, d1, ptr) do { const uint64_t dims__[2] = { d0, d1 }; \
        if ((rc = clapgpu_snapshot_add(w, name, dt, nd, dims__, ptr))) { clapgpu_snapshot_abort(w); w = NULL; goto done; } } while (0)
    ADD("entities.n", CLAPGPU_DT_I64, 1, 1, 0, &n64);
    ADD("entities.pos_scale", CLAPGPU_DT_F32, 2, n, 4, pos_scale);
    ADD("entities.rot", CLAPGPU_DT_F32, 2, n, 4, rot);
    ADD("entities.parent", CLAPGPU_DT_I32, 1, n, 0, parent);
    ADD("entities.model", CLAPGPU_DT_I32, 1, n, 0, model);
    ADD("entities.flags", CLAPGPU_DT_U32, 1, n, 0, flags);
    ADD("entities.seqs", CLAPGPU_DT_U32, 1, n, 0, seqs);
    ADD("entities.model_aabb", CLAPGPU_DT_F32, 2, nm, 6, maabb);
    ADD("entities.model_skip", CLAPGPU_DT_U8, 1, nm, 0, mskip);
    if (gs->culled_view) {
        ADD("frustum.planes", CLAPGPU_DT_F32, 2, 6, 4, gs->culled_view->main.frustum_planes);
        ADD("frustum.corners", CLAPGPU_DT_F32, 2, 8, 4, gs->culled_view->main.frustum_corners);
    }
#undef ADD
    *out = w;
    rc = 0;
done:
    free(index_of); free(pos_scale); free(rot); free(parent); free(model); free(flags); free(seqs); free(maabb); free(mskip);
    return rc;
}
