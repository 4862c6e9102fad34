/*
 * gpu-scene-results.c -- the device's results into the engine's entity3d structs, for the entity binding (gpu-scene.c;
 * shared declarations in gpu-scene-internal.h).  In file order: the camera bounding-volume pick; scatter_one (step 5 for
 * one entity); the frame's second launch (joint riders) and gpu_scene_run_deferred; GPU_SCATTER_DRAWN's fetches and
 * standing readers; the mirror passes of a frame that is not walked (touched records, the address list); the write-back
 * passes on the workers; host hooks and bounding-volume picks merged in list order; gs_fast_frame (a NOTIFIED frame, or one
 * by the records: O(touched + rebuilt)) and gs_frame_results (the second half of every frame).
 */
#include "gpu-scene-internal.h"

/* model.c:1697-1713, for an entity whose aabb is current */
static void bv_pick(struct scene *scene, entity3d *e)
{
    struct camera *cam = scene->camera;
    if ((aabb_point_is_inside(e->aabb, transform_pos(&cam->xform, NULL)) ||
         (scene->control && aabb_point_is_inside(e->aabb, transform_pos(&scene->control->xform, NULL)))) &&
         e != scene->control) {
        float volume = entity3d_aabb_X(e) * entity3d_aabb_Y(e) * entity3d_aabb_Z(e);

        if (!cam->bv || volume > cam->bv_volume) {
            cam->bv = e;
            cam->bv_volume = volume;
        }
    }
}

/* A rebuilt entity WITHOUT a parent hands its position to the light it carries (model.c:1687-1692).  At most LIGHTS_MAX
 * entities do, each to its own slot, so this is safe from the scatter workers. */
static inline void light_hand_off(struct gpu_scene *gs, entity3d *e)
{
    if (e->parent || e->light_idx < 0 || !gs->hook_data) return;
    struct scene *scene = gs->hook_data;
    vec3 pos;
    transform_pos(&e->xform, pos);
    vec3_add(pos, pos, e->light_off);
    light_set_pos(&scene->light, e->light_idx, pos);
}

static void scatter_one(struct gpu_scene *gs, struct gs_rec *r, const clapgpu_scene_arrays *res, size_t slot, bool parent_seq)
{
    entity3d *e = r->e, *parent = e->parent;
    if (r->host_done) {                                          /* gpu_scene_host_updated(): the host wrote these fields itself */
        const uint8_t hd = r->host_done;                         /* 2: its transform was written again since (the mirror pass saw it) */
        r->host_done = 0;
        if (hd == 1 && !transform_is_updated(&e->xform) && !(parent && e->parent_seq != parent_seq_now(gs, r, parent))) {
            seq_shown(gs, slot, e->seq);                         /* the device has caught up with what the host did */
            return;
        }
        /* ... but it was touched again since (or its parent moved): an ordinary rebuild */
    }
    if (parent && parent_seq) e->parent_seq = parent_seq_now(gs, r, parent);   /* model.c:1613 (parents sit in lower slots: already advanced) */
    if (transform_is_updated(&e->xform)) transform_clear_updated(&e->xform);
    e->seq = (uint16_t)(e->seq + 1 + pend_of(gs, (uint32_t)slot));  /* model.c:1616, 1669 (+ the rebuilds it was not shown) */
    if (gs->any_pend && slot < gs->cap_pend) gs->pend[slot] = 0;
    seq_shown(gs, slot, e->seq);
    copy_rows(r, res, slot);
    light_hand_off(gs, e);
}

/* The frame's second entity launch: the subtrees riding a batched character's joint (class 4), now that the palettes of
 * the frame are in the entities (e->parent->joint_transforms[e->parent_joint], model.c:1633-1640). */
static int attached_pass(struct gpu_scene *gs, struct mq *mq)
{
    struct gpu_scene_stats *st = &gs->stats;
    uint32_t n_roots = 0;
    for (uint32_t k = 0; k < gs->n_att; k++) {
        const struct gs_rec *r = &gs->rec[gs->att_list[k]];
        n_roots += r->e && r->att;
    }
    if (!n_roots) return 0;
    if (n_roots > gs->cap_att_roots) {
        uint32_t cap = gs->cap_att_roots ? gs->cap_att_roots : 64;
        while (cap < n_roots) cap *= 2;
        uint32_t *h = realloc(gs->att_handles, (size_t)cap * 4);
        if (h) gs->att_handles = h;
        float *a = realloc(gs->att_jt, (size_t)cap * 64);
        if (a) gs->att_jt = a;
        float *b = realloc(gs->att_bind, (size_t)cap * 64);
        if (b) gs->att_bind = b;
        if (!h || !a || !b) return _CERR_NOMEM;
        gs->cap_att_roots = cap;
    }
    uint32_t q = 0;
    for (uint32_t k = 0; k < gs->n_att; k++) {
        const struct gs_rec *r = &gs->rec[gs->att_list[k]];
        if (!r->e || !r->att) continue;
        entity3d *e = r->e, *parent = e->parent;
        if (!parent || !parent->joint_transforms || e->parent_joint < 0 ||
            e->parent_joint >= (int)parent->txmodel->model->nr_joints) return _CERR_INVALID_ARGUMENTS;
        gs->att_handles[q] = r->handle;
        memcpy(gs->att_jt + 16 * (size_t)q, parent->joint_transforms[e->parent_joint], 64);
        memcpy(gs->att_bind + 16 * (size_t)q, parent->txmodel->model->joints[e->parent_joint].bind, 64);
        q++;
    }
    CK(clapgpu_scene_attached_update(gs->scene, q, gs->att_handles, gs->att_jt, gs->att_bind));
    clapgpu_scene_arrays res = { 0 };
    CK(clapgpu_scene_results(gs->scene, &res));
    gs->res = res;
    struct scene *scene = mq->priv;
    for (uint32_t k = 0; k < gs->n_att; k++) {                   /* list order, parents first */
        struct gs_rec *r = &gs->rec[gs->att_list[k]];
        if (!r->e || r->slot >= res.n_slots) continue;
        if ((res.rebuilt_mask[r->slot >> 6] >> (r->slot & 63)) & 1) {
            scatter_one(gs, r, &res, r->slot, true);
            st->written_back++;
        }
        if (scene) bv_pick(scene, r->e);                         /* default_update's pick, with this frame's box (model.c:1697-1713) */
        st->attached++;
    }
    return 0;
}

/* The joint-attached subtrees this frame's gpu_mq_update() held back (class 3), in list order, now that the parents'
 * joint transforms of the frame exist.  Called by gpu_anim_update(); a frame driver without it calls this itself. */
void gpu_scene_run_deferred(struct gpu_scene *gs, struct mq *mq)
{
    if (!gs || !mq) return;
    if (gs->n_att) {
        const int rc = attached_pass(gs, mq);
        if (rc) {
            /* the device pass could not run: the entities' own hooks keep the frame whole, and the failure is loud */
            fprintf(stderr, "gpu_scene: joint-attached pass failed (%d, %s): running %u hooks on the host\n", rc, clapgpu_last_error(), gs->n_att);
            gs->stats.attach_failures++;
            for (uint32_t k = 0; k < gs->n_att; k++) {
                struct gs_rec *r = &gs->rec[gs->att_list[k]];
                if (r->e && entity3d_matches(r->e, ENTITY3D_ALIVE)) entity3d_update(r->e, mq->priv);
            }
        }
    }
    for (uint32_t k = 0; k < gs->n_deferred; k++) {
        struct gs_rec *r = &gs->rec[gs->deferred[k]];
        if (r->e && !r->gone && entity3d_matches(r->e, ENTITY3D_ALIVE))
            entity3d_update(r->e, mq->priv);
    }
}

/* the rows the mirror's last call fetched (clapgpu_scene_arrays.fetched_mask) into their entity3d */
void gs_consume_fetched(struct gpu_scene *gs)
{
    clapgpu_scene_arrays res;
    if (clapgpu_scene_results(gs->scene, &res)) return;
    gs->res = res;
    if (!res.n_fetched || res.fetch_serial == gs->fetch_seen) return;   /* nothing new: an earlier fetch's rows may be older than the host's by now */
    gs->fetch_seen = res.fetch_serial;
    const uint32_t words = res.n_slots / 64;
    for (uint32_t w = 0; w < words; w++) {
        uint64_t m = res.fetched_mask[w];
        while (m) {
            const uint32_t slot = w * 64 + (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            const uintptr_t u = (uintptr_t)res.slot_user[slot];
            if (!u) continue;
            struct gs_rec *r = &gs->rec[u - 1];
            if (!r->e || (r->cls != 1 && r->cls != 4)) continue;
            scatter_fetched(gs, r, &res, slot);
            gs->stats.fetched++;
        }
    }
}

/* every stale row to the entity3d the queue's own lists still hold (not by the records: some may name freed memory) */
void gs_fetch_met_in_queue(struct gpu_scene *gs, struct mq *mq)
{
    uint32_t n_rows = 0;
    clapgpu_scene_arrays fr;
    if (clapgpu_scene_fetch(gs->scene, NULL, &n_rows) || !n_rows || clapgpu_scene_results(gs->scene, &fr)) return;
    gs->res = fr;
    gs->fetch_seen = fr.fetch_serial;
    model3dtx *txm;
    entity3d *e, *it;
    list_for_each_entry(txm, &mq->txmodels, entry) list_for_each_entry_iter(e, it, &txm->entities, entry) {
        if (!entity3d_matches(e, ENTITY3D_ALIVE)) continue;
        const uint32_t i = rec_find(gs, e);
        if (i == NO_REC) continue;
        struct gs_rec *r = &gs->rec[i];
        if (r->gone || r->e != e || (r->cls != 1 && r->cls != 4) || r->slot >= fr.n_slots) continue;
        if (!((fr.fetched_mask[r->slot >> 6] >> (r->slot & 63)) & 1)) continue;
        scatter_fetched(gs, r, &fr, r->slot);
        gs->stats.fetched++;
    }
    if (gs->pend) memset(gs->pend, 0, (size_t)gs->cap_pend * sizeof(*gs->pend));
    gs->any_pend = false;
}

void gpu_scene_set_scatter(struct gpu_scene *gs, int policy)
{
    if (!gs) return;
    const bool drawn = policy == GPU_SCATTER_DRAWN;
    if (gs->scatter_drawn && !drawn) gpu_scene_fetch_all(gs);    /* back to "everything is always current" */
    if (drawn && !gs->scatter_drawn) { gs->topology_pending = true; gs->shown_stale = true; }   /* its per-slot counters are laid out by a walk: the next frame is one */
    gs->scatter_drawn = drawn;
}

static inline bool slot_is_stale(const struct gpu_scene *gs, uint32_t slot)
{
    return gs->res.n_stale_words && gs->res.stale_mask && slot < gs->res.n_slots && ((gs->res.stale_mask[slot >> 6] >> (slot & 63)) & 1);
}

bool gpu_scene_entity_is_stale(struct gpu_scene *gs, entity3d *e)
{
    if (!gs || !gs->any_pend) return false;
    const uint32_t i = rec_find(gs, e);
    if (i == NO_REC || (gs->rec[i].cls != 1 && gs->rec[i].cls != 4)) return false;
    clapgpu_scene_arrays res;
    if (clapgpu_scene_results(gs->scene, &res)) return false;
    gs->res = res;
    return slot_is_stale(gs, gs->rec[i].slot);
}

int gpu_scene_fetch(struct gpu_scene *gs, entity3d *e)
{
    if (!gs || !e) return _CERR_INVALID_ARGUMENTS;
    if (!gs->any_pend) return 0;
    const uint32_t i = rec_find(gs, e);
    if (i == NO_REC) return 0;
    struct gs_rec *r = &gs->rec[i];
    if ((r->cls != 1 && r->cls != 4) || r->handle == CLAPGPU_NO_ENTITY) return 0;
    CK(clapgpu_scene_fetch_entity(gs->scene, r->handle));
    gs_consume_fetched(gs);
    return 0;
}

int gpu_scene_fetch_all(struct gpu_scene *gs)
{
    if (!gs) return _CERR_INVALID_ARGUMENTS;
    if (!gs->any_pend) return 0;
    /* entities were created or DELETED since the last update (gpu_scene_topology): a record may name freed memory, and only
     * the walk of the next gpu_mq_update() finds out which -- it fetches everything itself, as it meets the entities */
    if (gs->topology_pending) return _CERR_NOT_SUPPORTED;
    uint32_t n = 0;
    CK(clapgpu_scene_fetch(gs->scene, NULL, &n));
    gs_consume_fetched(gs);
    gs->any_pend = false;                                        /* every counter was consumed with its row */
    if (gs->verify)                                              /* the aid's own check: nothing is owed after a full fetch */
        for (uint32_t i = 0; i < gs->cap_pend; i++)
            if (gs->pend[i]) { fprintf(stderr, "gpu_scene: slot %u still owes %u seq steps after gpu_scene_fetch_all\n", i, gs->pend[i]); gs->pend[i] = 0; }
    return 0;
}

/* one line about e's record, for a checker's mismatch report */
void gpu_scene_describe(struct gpu_scene *gs, entity3d *e, char *buf, size_t len)
{
    const uint32_t i = gs ? rec_find(gs, e) : NO_REC;
    if (i == NO_REC) { snprintf(buf, len, "no record"); return; }
    const struct gs_rec *r = &gs->rec[i];
    clapgpu_scene_arrays res;
    const bool have = !clapgpu_scene_results(gs->scene, &res);
    if (have) gs->res = res;
    int n = snprintf(buf, len, "class %u slot %u keep %u user_keep %u host_child %u host_done %u pend %u stale %d parent_rec %d order_pos %u",
             r->cls, r->slot, r->keep, r->user_keep, r->host_child, r->host_done, pend_of(gs, r->slot),
             have ? (int)slot_is_stale(gs, r->slot) : -1, r->parent_rec == NO_REC ? -1 : (int)r->parent_rec, r->order_pos);
    if (have && n > 0 && (size_t)n < len && r->slot < res.n_slots && (r->cls == 1 || r->cls == 4)) {   /* the row the mirror holds, beside the entity3d's */
        const float *b = res.aabb + 6 * (size_t)r->slot;
        snprintf(buf + n, len - (size_t)n, "; mirror box %.9g %.9g %.9g %.9g %.9g %.9g vis %d rebuilt %d, entity3d box %.9g %.9g %.9g %.9g %.9g %.9g flags %x/%x",
                 b[0], b[1], b[2], b[3], b[4], b[5], (int)((res.vis_mask[r->slot >> 6] >> (r->slot & 63)) & 1),
                 (int)((res.rebuilt_mask[r->slot >> 6] >> (r->slot & 63)) & 1),
                 ((const float *)e->aabb)[0], ((const float *)e->aabb)[1], ((const float *)e->aabb)[2], ((const float *)e->aabb)[3],
                 ((const float *)e->aabb)[4], ((const float *)e->aabb)[5], (unsigned)r->flags, (unsigned)(e->flags & (ENTITY3D_ALIVE | 0xffffu)));
    }
}

void gpu_scene_keep(struct gpu_scene *gs, entity3d *e, bool keep)
{
    if (!gs || !e) return;
    const uint32_t i = rec_find(gs, e);
    if (i == NO_REC) return;
    struct gs_rec *r = &gs->rec[i];
    r->user_keep = keep;
    if (keep && !r->keep && r->handle != CLAPGPU_NO_ENTITY && !clapgpu_scene_entity_keep(gs->scene, r->handle, 1)) {
        r->keep = 1;
        gpu_scene_fetch(gs, e);                                  /* from now on it is always current: starting now */
    }
}

/* What a walk would decide an entity's class from, against what the last walk saw: its own criteria (hook, flags, animation:
 * self_ok; a plain entity that is host-class only because of where its parent stands in the list -- cls 2, self_ok 1 -- may be
 * touched without forcing a walk), its parent, whether it rides a joint, its model; a batched one must still be on the device */
static inline bool class_inputs_changed(const struct gpu_scene *gs, const struct gs_rec *r, entity3d *e)
{
    return !entity3d_matches(e, ENTITY3D_ALIVE) || self_batchable(gs, e) != (bool)r->self_ok || e->parent != r->parent_e ||
           (e->parent && e->parent_joint != JOINT_TYPE_MAX) != (bool)r->rides || entity_animated(e) != (bool)r->animated ||
           ((r->cls == 1 || r->cls == 4) && (r->model != e->txmodel->model || r->handle == CLAPGPU_NO_ENTITY));
}

static void *par_mirror(void *arg)
{
    struct par_job *j = arg;
    struct gpu_scene *gs = j->gs;
    for (uint32_t k = j->lo; k < j->hi; k++) {
        struct gs_rec *r = &gs->rec[gs->touched[k]];
        if (k + 8 < j->hi) {
            const struct gs_rec *a = &gs->rec[gs->touched[k + 8]];
            if (a->e) { __builtin_prefetch(&a->e->xform, 0, 1); __builtin_prefetch(&a->e->flags, 0, 1); }
        }
        r->pending = 0;
        r->xform_dirty = 0;
        if (!r->e) continue;
        entity3d *e = r->e;
        if (class_inputs_changed(gs, r, e)) {
            j->need_walk = 1;
            continue;
        }
        if (r->cls != 1 && r->cls != 4) continue;
        if (e->force_lod != r->lod_force || e->cur_lod != r->lod_cur)   /* entity3d_set_lod since (model.c:593-609): after the join, on one thread */
            if (push_u32(&j->deferred, &j->n_deferred, &j->cap_deferred, gs->touched[k])) j->rc = _CERR_NOMEM;
        const uint32_t flags = e->flags & (ENTITY3D_ALIVE | 0xffffu);
        const bool same_flags = flags == r->flags;
        r->flags = flags;
        if (gs->vq_ok && r->order_pos < gs->n_order) gs->vq_ok[r->order_pos] = verdict_ok(r);
        r->xform_dirty = transform_is_updated(&e->xform);
        if (r->host_done && r->xform_dirty) r->host_done = 2;
        if (!r->xform_dirty && !r->host_done && same_flags) continue;   /* (a frame that looks at EVERY record: most have nothing to say) */
        if (gs->drawn_now && r->xform_dirty) transform_clear_updated(&e->xform);
        const int rc = clapgpu_scene_entity_transform_mt(gs->scene, r->handle, transform_pos(&e->xform, NULL),
                                                         transform_rotation_quat(&e->xform), e->scale, flags, r->xform_dirty || r->host_done);
        if (rc) j->rc = rc;
        j->count++;
    }
    return NULL;
}

/* the mirror pass over [lo, hi) of the address list: table line asked for sixteen entries ahead, entity eight ahead */
struct xptr_ctx { struct gpu_scene *gs; int mt, rc; uint32_t pushed; };
static void xptr_range(void *ctx, uint32_t lo, uint32_t hi)
{
    struct xptr_ctx *xc = ctx;
    struct gpu_scene *gs = xc->gs;
    uint32_t ring[8];                                            /* table positions of entries k .. k + 7 */
    uint32_t pushed = 0;
    for (uint32_t k = lo; k < hi + 8; k++) {
        if (k + 8 < hi) __builtin_prefetch(&gs->ftab[ftab_home(gs, gs->xptr[k + 8])], 0, 1);
        if (k >= lo + 8) {                                       /* entry k - 8: resolved eight steps ago, its entity asked for then */
            const uint32_t h = ring[(k - 8) & 7];
            if (h != NO_REC) {
                const struct gs_fast *f = &gs->ftab[h];
                entity3d *e = (entity3d *)(uintptr_t)f->key;
                /* an entity moved twice this frame is on the list twice: between workers, whoever claims its slot first
                 * takes it (every entry would push the same, final, transform; two workers on one entity3d race) */
                const bool taken = xc->mt && f->slot < gs->cap_claim &&
                    ((__atomic_fetch_or(&gs->claim[f->slot >> 6], 1ull << (f->slot & 63), __ATOMIC_RELAXED) >> (f->slot & 63)) & 1);
                if (!taken) {
                    const bool upd = transform_is_updated(&e->xform);
                    const int rc = xc->mt ? clapgpu_scene_entity_xform_mt(gs->scene, f->handle, transform_pos(&e->xform, NULL),
                                                                          transform_rotation_quat(&e->xform), e->scale, upd)
                                          : (upd ? clapgpu_scene_entity_transform(gs->scene, f->handle, transform_pos(&e->xform, NULL),
                                                                                  transform_rotation_quat(&e->xform), e->scale) : 0);
                    if (rc) xc->rc = rc;
                    if (gs->drawn_now && upd) transform_clear_updated(&e->xform);   /* see mirror_one */
                    pushed++;
                }
            }
        }
        if (k < hi) {
            const entity3d *e = gs->xptr[k];
            uint32_t h = ftab_home(gs, e);
            while (gs->ftab[h].key && gs->ftab[h].key != (uint64_t)(uintptr_t)e) h = (h + 1) & gs->ftab_mask;
            if (gs->ftab[h].key && gs->ftab[h].handle != CLAPGPU_NO_ENTITY) {   /* ours, and on the device */
                ring[k & 7] = h;
                __builtin_prefetch(&e->xform, 1, 1);
                __builtin_prefetch((const char *)&e->xform + 32, 1, 1);  /* (transform_t + scale may straddle a line) */
                clapgpu_scene_entity_xform_prefetch(gs->scene, gs->ftab[h].handle, gs->ftab[h].slot);
            } else
                ring[k & 7] = NO_REC;                            /* another queue's entity, or a host-class one: its own hook reads the transform */
        }
    }
    __atomic_fetch_add(&xc->pushed, pushed, __ATOMIC_RELAXED);
}

/* A list-order chunk of the rebuilt entities.  A batched entity's parent precedes it in the list, so inside a chunk
 * parent_seq can be taken at once; a child whose parent lies in an EARLIER chunk (another thread) is noted and
 * finished after the join. */
static void *par_scatter(void *arg)
{
    struct par_job *j = arg;
    struct gpu_scene *gs = j->gs;
    const clapgpu_scene_arrays *res = j->res;
    for (uint32_t k = j->lo; k < j->hi; k++) {
        struct gs_rec *r = &gs->rec[gs->order[k]];
        if (k + 8 < j->hi) {
            const struct gs_rec *a = &gs->rec[gs->order[k + 8]];
            if (a->cls == 1 && a->slot < res->n_slots && ((j->scat[a->slot >> 6] >> (a->slot & 63)) & 1)) {
                prefetch_entity(a->e);
                __builtin_prefetch(res->mx + 16 * (size_t)a->slot, 0, 0);
                __builtin_prefetch(res->inverse_mx + 16 * (size_t)a->slot, 0, 0);
                __builtin_prefetch(res->aabb + 6 * (size_t)a->slot, 0, 0);
            }
        }
        if (r->cls != 1 || r->slot >= res->n_slots || !((j->scat[r->slot >> 6] >> (r->slot & 63)) & 1)) continue;
        if (r->host_done) {                                      /* see gs_frame_results: after the join, on one thread */
            if (push_u32(&j->whole, &j->n_whole, &j->cap_whole, gs->order[k])) j->rc = _CERR_NOMEM;
            continue;
        }
        bool here = true;
        if (r->e->parent) {
            const uint32_t pr = r->parent_rec;
            here = pr != NO_REC && gs->rec[pr].e == r->e->parent && gs->rec[pr].order_pos >= j->lo && !gs->rec[pr].host_done;
            if (!here && push_u32(&j->deferred, &j->n_deferred, &j->cap_deferred, gs->order[k])) j->rc = _CERR_NOMEM;
        }
        scatter_one(gs, r, res, r->slot, here);
        j->count++;
    }
    return NULL;
}

/* The same over a range of MASK WORDS (slots in ascending order: parents first): for a rebuilt set that is large enough for the
 * workers but a small part of the queue, where a pass over every record to find it costs more than the rows themselves
 * (1 M entities, 46 k rows to write: 80 MB of records read for 7 MB of rows). */
static void *par_scatter_mask(void *arg)
{
    struct par_job *j = arg;
    struct gpu_scene *gs = j->gs;
    const clapgpu_scene_arrays *res = j->res;
    for (uint32_t w = j->lo; w < j->hi; w++) {
        uint64_t m = j->scat[w];
        if (w + 1 < j->hi && j->scat[w + 1]) {                   /* the next word's first entity: its record's line */
            const uint32_t ns = (w + 1) * 64 + (uint32_t)__builtin_ctzll(j->scat[w + 1]);
            const uintptr_t nu = (uintptr_t)res->slot_user[ns];
            if (nu) __builtin_prefetch(&gs->rec[nu - 1], 0, 1);
        }
        while (m) {
            const uint32_t slot = w * 64 + (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            const uintptr_t u = (uintptr_t)res->slot_user[slot];
            if (!u) continue;
            struct gs_rec *r = &gs->rec[u - 1];
            if (r->cls != 1 || !r->e) continue;                  /* class 4: after the pose, from the second launch */
            if (r->host_done) {
                if (push_u32(&j->whole, &j->n_whole, &j->cap_whole, (uint32_t)(u - 1))) j->rc = _CERR_NOMEM;
                continue;
            }
            bool here = true;
            if (r->e->parent) {
                const uint32_t pr = r->parent_rec;
                here = pr != NO_REC && gs->rec[pr].e == r->e->parent && gs->rec[pr].slot >= j->lo * 64u && gs->rec[pr].slot < slot &&
                       !gs->rec[pr].host_done;
                if (!here && push_u32(&j->deferred, &j->n_deferred, &j->cap_deferred, (uint32_t)(u - 1))) j->rc = _CERR_NOMEM;
            }
            scatter_one(gs, r, res, slot, here);
            j->count++;
        }
    }
    return NULL;
}

static int rec_slot_cmp(const void *a, const void *b, void *ctx)
{
    const struct gpu_scene *gs = ctx;
    const uint32_t x = gs->rec[*(const uint32_t *)a].slot, y = gs->rec[*(const uint32_t *)b].slot;
    return x < y ? -1 : x > y;
}

static void *par_deferred(void *arg)
{
    struct par_job *j = arg;
    struct gpu_scene *gs = j->gs;
    for (uint32_t d = 0; d < j->n_deferred; d++) {
        if (d + 8 < j->n_deferred) {
            const entity3d *a = gs->rec[j->deferred[d + 8]].e;
            __builtin_prefetch(&a->parent_seq, 1, 1);
            __builtin_prefetch(&a->parent->seq, 0, 1);
        }
        const struct gs_rec *cr = &gs->rec[j->deferred[d]];
        entity3d *c = cr->e;
        c->parent_seq = parent_seq_now(gs, cr, c->parent);       /* model.c:1613: every parent is final by now */
    }
    return NULL;
}

/* GPU_SCATTER_DRAWN, after a fast frame's launch: every slot the device rebuilt without writing it back */
struct pend_ctx { struct gpu_scene *gs; const clapgpu_scene_arrays *res; uint32_t left; };
static void pend_range(void *ctx, uint32_t lo, uint32_t hi)
{
    struct pend_ctx *pc = ctx;
    struct gpu_scene *gs = pc->gs;
    const clapgpu_scene_arrays *res = pc->res;
    uint32_t left = 0;
    for (uint32_t w = lo; w < hi; w++) {
        uint64_t m = res->rebuilt_mask[w] & ~res->exported_mask[w];
        left += (uint32_t)__builtin_popcountll(m);
        while (m) {
            const uint32_t slot = w * 64 + (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            gs->pend[slot]++;
            if (gs->verify) {                                    /* a read nobody announced must show: poison what went stale */
                const uintptr_t u = (uintptr_t)res->slot_user[slot];
                if (u && gs->rec[u - 1].e) gs->rec[u - 1].e->mx[0][0] = __builtin_nanf("");
            }
        }
    }
    __atomic_fetch_add(&pc->left, left, __ATOMIC_RELAXED);
}

/* a host-class entity's own hook in a fast frame */
static void host_hook(struct gpu_scene *gs, struct mq *mq, struct gs_rec *hr)
{
    if (hr->gone || !hr->e) return;                              /* deleted by a hook that ran earlier in this frame */
    if (hr->lag) {
        /* listed before its batched parent: the reference has not updated that parent yet when this hook runs */
        struct lag_keep *kp = &gs->lag_keep[hr->lag - 1], now;
        entity3d *p = gs->rec[gs->lag_parent[hr->lag - 1]].e;
        memcpy(now.mx, p->mx, sizeof(mat4x4)); now.seq = p->seq;
        memcpy(p->mx, kp->mx, sizeof(mat4x4)); p->seq = kp->seq;
        entity3d_update(hr->e, mq->priv);
        memcpy(p->mx, now.mx, sizeof(mat4x4)); p->seq = now.seq;
    } else
        entity3d_update(hr->e, mq->priv);
}

static int cand_cmp(const void *a, const void *b)
{
    const struct gs_cand *x = a, *y = b;
    return x->key < y->key ? -1 : x->key > y->key;
}

/* The second half's last step: host-class entities' own hooks and the camera bounding-volume pick of the entities whose box holds
 * a query point (res->inside_mask), merged in list order.  *n_cand: the candidates of the pick. */
static int hooks_and_picks(struct gpu_scene *gs, struct mq *mq, const clapgpu_scene_arrays *res, uint32_t *n_cand_out)
{
    struct scene *scene = mq->priv;
    const uint32_t words = res->n_slots / 64;
    uint32_t n_cand = 0;
    if (gs->appended) {
        /* order[] is not the list any more (entities taken in since the walk stand at its end): the candidates -- few --
         * are sorted by their place in the queue instead, and merged with the host-class entities by that */
        if (scene && res->inside_mask)
            for (uint32_t w = 0; w < words; w++) {
                uint64_t m = res->inside_mask[w];
                while (m) {
                    const size_t slot = (size_t)w * 64 + (size_t)__builtin_ctzll(m);
                    m &= m - 1;
                    const uintptr_t u = (uintptr_t)res->slot_user[slot];
                    if (!u) continue;
                    if (n_cand == gs->cap_cands) {
                        const uint32_t cap = gs->cap_cands ? 2 * gs->cap_cands : 256;
                        struct gs_cand *q = realloc(gs->cands, (size_t)cap * sizeof(*q));
                        if (!q) return _CERR_NOMEM;
                        gs->cands = q; gs->cap_cands = cap;
                    }
                    gs->cands[n_cand++] = (struct gs_cand){ gs->rec[u - 1].order_key, (uint32_t)(u - 1) };
                }
            }
        if (n_cand > 1) qsort(gs->cands, n_cand, sizeof(*gs->cands), cand_cmp);
        *n_cand_out = n_cand;
        uint32_t hc = 0, ci = 0;
        for (;;) {
            const uint64_t ck = ci < n_cand ? gs->cands[ci].key : UINT64_MAX;
            const uint64_t hk = hc < gs->n_host ? gs->rec[gs->host_list[hc]].order_key : UINT64_MAX;
            if (ck == UINT64_MAX && hk == UINT64_MAX) break;
            if (hk < ck)
                host_hook(gs, mq, &gs->rec[gs->host_list[hc++]]);
            else {
                const struct gs_rec *cr = &gs->rec[gs->cands[ci++].rec];
                if (cr->cls == 1 && cr->e && !cr->gone) bv_pick(scene, cr->e);
            }
        }
        return 0;
    }
    /* candidates come off the mask in slot order; list order is restored through a bitmap over the walk's positions (one bit
     * per queue position: 125 KB per million entities), which the merge below scans upwards */
    const uint32_t pos_words = (gs->n_order + 63) / 64;
    if (scene && res->inside_mask) {
        if (pos_words > gs->cap_posmap) {
            uint64_t *pm = realloc(gs->posmap, (size_t)pos_words * 8);
            if (!pm) return _CERR_NOMEM;
            gs->posmap = pm; gs->cap_posmap = pos_words;
        }
        bool cleared = false;
        for (uint32_t w = 0; w < words; w++) {
            uint64_t m = res->inside_mask[w];
            while (m) {
                const size_t slot = (size_t)w * 64 + (size_t)__builtin_ctzll(m);
                m &= m - 1;
                const uintptr_t u = (uintptr_t)res->slot_user[slot];
                if (!u) continue;
                if (!cleared) { memset(gs->posmap, 0, (size_t)pos_words * 8); cleared = true; }
                const uint32_t op = gs->rec[u - 1].order_pos;
                gs->posmap[op >> 6] |= 1ull << (op & 63);
                n_cand++;
            }
        }
    }
    *n_cand_out = n_cand;
    uint32_t hc = 0, cw = 0;
    uint64_t cm = n_cand ? gs->posmap[0] : 0;
    for (;;) {
        while (n_cand && !cm && cw + 1 < pos_words) cm = gs->posmap[++cw];
        const uint32_t co = cm ? cw * 64 + (uint32_t)__builtin_ctzll(cm) : 0xffffffffu;
        const uint32_t ho = hc < gs->n_host ? gs->rec[gs->host_list[hc]].order_pos : 0xffffffffu;
        if (co == 0xffffffffu && ho == 0xffffffffu) break;
        if (ho < co) {
            host_hook(gs, mq, &gs->rec[gs->host_list[hc++]]);
        } else {
            cm &= cm - 1;
            if (gs->rec[gs->order[co]].cls == 1 && !gs->rec[gs->order[co]].gone)   /* class 4 boxes are last frame's until the second launch */
                bv_pick(scene, gs->rec[gs->order[co]].e);
        }
    }
    return 0;
}

/*
 * One frame in notification mode, nothing re-parented or re-hooked since the last walk (entities made or deleted since are
 * taken in / out in place where that is possible, gpu_scene_entity_created / _deleting):
 *   touched batched entities -> flags + transform to the mirror; the device; the slots the kernel reports as rebuilt
 *   -> back into their entity3d (ascending slot = parents first); host-class entities' own hooks and the camera
 *   bounding-volume pick of the few entities whose box contains a query point, merged in list order.
 * Returns 1 if the frame has to be done by the full walk after all (a touched entity changed class or parent).
 */
int gs_fast_frame(struct gpu_scene *gs, struct mq *mq, struct view *view)
{
    struct gpu_scene_stats *st = &gs->stats;
    struct scene *scene = mq->priv;
    const double t0 = now_ms();
    if (gs->n_created) {                                         /* entities made since the last frame: into the standing layout, or a walk */
        const int rc = gs_take_created(gs, mq);
        if (rc) return rc;
    }
    st->placed = gs->inc_placed; st->removed = gs->inc_removed;
    st->registered += gs->inc_placed; st->deleted += gs->inc_removed;
    gs->inc_placed = gs->inc_removed = 0;
    clapgpu_scene_set_export(gs->scene, gs->scatter_drawn && gs->notify ? CLAPGPU_SCENE_EXPORT_DRAWN : CLAPGPU_SCENE_EXPORT_ALL);   /* (the policy lives on notifications: gpu-scene.h) */
    gs->drawn_now = clapgpu_scene_export_is_drawn(gs->scene);
    if (gs->drawn_now && scene && scene->control != gs->last_control) {
        /* the control entity is read every frame (camera target, camera.c:191-205; the bounding-volume pick): a standing reader */
        gs->last_control = scene->control;
        if (scene->control) gpu_scene_keep(gs, scene->control, true);
    }
    /* batched characters: the host half of character_update (limbo teleport, motion reset), which may touch them */
    for (uint32_t k = 0; k < gs->n_char; k++) {
        struct gs_rec *r = &gs->rec[gs->char_list[k]];
        if (r->e && entity3d_matches(r->e, ENTITY3D_ALIVE)) gs->char_half(r->e, mq->priv);
    }
    static uint32_t mirror_par_min;
    if (!mirror_par_min) {
        const char *mp = getenv("GPU_SCENE_MIRROR_PAR_MIN");     /* tuning knob */
        mirror_par_min = mp && atoi(mp) > 0 ? (uint32_t)atoi(mp) : GS_MIRROR_PAR_MIN;
    }
    if (gs->n_touched >= mirror_par_min || (gs->replaying && gs_par_threads() > 1)) {
        struct par_job jobs[GS_MAX_THREADS] = { 0 };
        const int nt = gs_par_threads();
        for (int t = 0; t < nt; t++)
            jobs[t] = (struct par_job){ .gs = gs, .lo = (uint32_t)((uint64_t)gs->n_touched * t / nt),
                                        .hi = (uint32_t)((uint64_t)gs->n_touched * (t + 1) / nt) };
        gs_par_run(par_mirror, jobs, nt);
        int need_walk = 0, prc = 0;
        for (int t = 0; t < nt; t++) {
            need_walk |= jobs[t].need_walk; st->uploaded += jobs[t].count;
            if (jobs[t].rc) prc = jobs[t].rc;
            for (uint32_t d = 0; d < jobs[t].n_deferred && !prc; d++) {          /* LODs set since: the mirror's copy follows */
                struct gs_rec *r = &gs->rec[jobs[t].deferred[d]];
                if (!r->e || r->handle == CLAPGPU_NO_ENTITY) continue;
                prc = clapgpu_scene_entity_lod(gs->scene, r->handle, r->e->force_lod, r->e->cur_lod);
                r->lod_force = r->e->force_lod; r->lod_cur = r->e->cur_lod;
                if (r->slot < gs->cap_slot_arrays) {
                    if (r->lod_cur >= -128 && r->lod_cur <= 127) gs->slot_lod[r->slot] = (int8_t)r->lod_cur;
                    else gs->cap_slot_arrays = 0;
                }
            }
            free(jobs[t].deferred); jobs[t].deferred = NULL; jobs[t].n_deferred = jobs[t].cap_deferred = 0;
        }
        if (prc) return prc;
        clapgpu_scene_mark_all_dirty(gs->scene);
        if (need_walk) {
            if (gs->drawn_now)                                   /* the walk decides by xform.updated: give back what this pass cleared */
                for (uint32_t k = 0; k < gs->n_touched; k++) {
                    struct gs_rec *r = &gs->rec[gs->touched[k]];
                    if (r->e && r->xform_dirty) transform_set_updated(&r->e->xform);
                }
            gs->n_touched = 0;
            return 1;
        }
    } else
    for (uint32_t k = 0; k < gs->n_touched; k++) {
        struct gs_rec *r = &gs->rec[gs->touched[k]];
        r->pending = 0;
        r->xform_dirty = 0;
        if (!r->e) continue;
        entity3d *e = r->e;
        if (class_inputs_changed(gs, r, e)) {
            if (gs->drawn_now)                                   /* the walk decides by xform.updated: give back what this pass cleared */
                for (uint32_t j = 0; j < k; j++) {
                    struct gs_rec *q = &gs->rec[gs->touched[j]];
                    if (q->e && q->xform_dirty) transform_set_updated(&q->e->xform);
                }
            for (k++; k < gs->n_touched; k++) gs->rec[gs->touched[k]].pending = 0;
            gs->n_touched = 0;
            return 1;
        }
        if (r->cls == 1 || r->cls == 4) CK(mirror_one(gs, r));
        if (gs->vq_ok && r->order_pos < gs->n_order) gs->vq_ok[r->order_pos] = verdict_ok(r);
    }
    gs->n_touched = 0;
    if (gs->n_xptr) {
        struct xptr_ctx xc = { .gs = gs, .mt = gs->n_xptr >= mirror_par_min && gs_par_threads() > 1 };
        if (xc.mt) {
            const uint32_t need = clapgpu_scene_slot_count(gs->scene);
            if (need > gs->cap_claim) {
                uint64_t *q = realloc(gs->claim, ((size_t)need / 64 + 1) * 8);
                if (!q) return _CERR_NOMEM;
                gs->claim = q; gs->cap_claim = need;
            }
            memset(gs->claim, 0, ((size_t)gs->cap_claim / 64 + 1) * 8);
            gpu_scene_par_for(xptr_range, &xc, gs->n_xptr, gs_par_threads());
            clapgpu_scene_mark_all_dirty(gs->scene);
        } else
            xptr_range(&xc, 0, gs->n_xptr);
        gs->n_xptr = 0;
        if (xc.rc) return xc.rc;
        st->uploaded += xc.pushed;
    }
    if (scene && scene->camera)
        clapgpu_scene_set_bv_points(gs->scene, transform_pos(&scene->camera->xform, NULL),
                                    scene->control ? transform_pos(&scene->control->xform, NULL) : NULL, CLAPGPU_NO_ENTITY);
    else
        clapgpu_scene_set_bv_points(gs->scene, NULL, NULL, CLAPGPU_NO_ENTITY);
    const double t1 = now_ms();
    clapgpu_frustum fr;
    if (view) frustum_of(view, &fr);
    CK(gs_views_before_update(gs, view));
    CK(clapgpu_scene_mq_update(gs->scene, view ? &fr : NULL));
    gs->culled_view = view;
    gs->vis_cursor = 0;
    if (view) memcpy(gs->culled_planes, view->main.frustum_planes, sizeof(gs->culled_planes));
    gs->cull_checked = false;
    clapgpu_scene_arrays res = { 0 };
    if (clapgpu_scene_results(gs->scene, &res)) memset(&res, 0, sizeof(res));
    gs->res = res;
    return gs_frame_results(gs, mq, &res, t0, t1, now_ms());
}

/*
 * The second half of a frame whose device step did not re-tile: what the kernel rebuilt goes back into the entity3d structs
 * (by the device's masks, on the workers when there is much of it), then the host-class entities' own hooks and the camera
 * bounding-volume pick, merged in list order.  A notified frame ends here, and so does a WALKED one whose layout stood (a
 * frame without notifications, or one that only had to look at the queue again): the device rebuilds exactly what the
 * reference's own tests would (model.c:1609-1616, 1667: xform.updated, or a parent that was rebuilt), so its mask is the
 * walk's answer too -- instead of a second serial pass over every entity3d (1 M entities: 41-53 ms of a walked frame).
 */
int gs_frame_results(struct gpu_scene *gs, struct mq *mq, const clapgpu_scene_arrays *resp, double t0, double t1, double t2)
{
    struct gpu_scene_stats *st = &gs->stats;
    const clapgpu_scene_arrays res = *resp;
    for (uint32_t k = 0; k < gs->n_lag; k++) {                  /* last frame's bits of the parents some host child still has to see */
        const entity3d *p = gs->rec[gs->lag_parent[k]].e;
        memcpy(gs->lag_keep[k].mx, p->mx, sizeof(mat4x4));
        gs->lag_keep[k].seq = p->seq;
    }

    /* results: only what the kernel rebuilt.  Few of them: straight off the mask, in slot order (parents first), each
     * entity and its rows prefetched a few steps ahead.  Many: in LIST order -- the entity3d structs lie in memory in
     * creation order, a slot-order pass over most of them would miss the caches on every one. */
    const uint32_t words = res.n_slots / 64;
    /* GPU_SCATTER_DRAWN: the rows that came back are the ones somebody reads (exported_mask); a slot rebuilt without
     * coming back is owed one more seq step when its entity3d is next written */
    const uint64_t *scat = res.exported_mask ? res.exported_mask : res.rebuilt_mask;
    if (gs->drawn_now && res.rebuilt_mask && scat != res.rebuilt_mask) {
        if (res.n_slots > gs->cap_pend || !gs->shown) return _CERR_INVALID_ARGUMENTS;   /* laid out by the walk that made this layout */
        struct pend_ctx pc = { gs, &res };
        gpu_scene_par_for(pend_range, &pc, words, words >= 2048 ? gs_par_threads() : 1);
        st->left_stale = pc.left;
        if (pc.left) gs->any_pend = true;
    }
    const bool timing = getenv("GPU_SCENE_TIMING") != NULL;
    const double ts0 = timing ? now_ms() : 0;
    uint64_t n_rebuilt = 0;
    if (scat)
        for (uint32_t w = 0; w < words; w++) n_rebuilt += (uint64_t)__builtin_popcountll(scat[w]);
    const double ts1 = timing ? now_ms() : 0;
    static uint64_t scatter_par_min;
    if (!scatter_par_min) {
        const char *sp = getenv("GPU_SCENE_SCATTER_PAR_MIN");    /* tuning knob */
        scatter_par_min = sp && atoll(sp) > 0 ? (uint64_t)atoll(sp) : GS_SCATTER_PAR_MIN;
    }
    if (n_rebuilt >= scatter_par_min && gs_par_threads() > 1) {
        const int nt = gs_par_threads();
        struct par_job jobs[GS_MAX_THREADS] = { 0 };
        /* most of the queue: in LIST order (the entity3d structs lie in creation order); a small part of it: off the mask */
        const bool sparse = GS_SCATTER_SPARSE * n_rebuilt <= gs->n_order;
        const uint32_t span = sparse ? words : gs->n_order;
        for (int t = 0; t < nt; t++)
            jobs[t] = (struct par_job){ .gs = gs, .res = &res, .scat = scat, .lo = (uint32_t)((uint64_t)span * t / nt),
                                        .hi = (uint32_t)((uint64_t)span * (t + 1) / nt) };
        gs_par_run(sparse ? par_scatter_mask : par_scatter, jobs, nt);
        /* Entities updated on the host since the last frame (entity3d_update / _reset, instantiate_entity: few).  For them
         * scatter_one DECIDES by the parent's counters -- did the parent move on since, or has the device merely caught up? --
         * and that must not be read while another worker is half-way through writing them (found on the GPU box: the sum read
         * between the two stores said "not moved", and a rebuild was dropped).  So the workers leave them out (and mark their
         * children for the parent_seq pass below); here, with every other entity final, they follow on this thread, parents
         * first (ascending slot); then the children's parent_seq, which reads final counters only. */
        int rc = 0;
        uint32_t n_whole = 0;
        for (int t = 0; t < nt; t++) { if (jobs[t].rc) rc = jobs[t].rc; n_whole += jobs[t].n_whole; }
        if (n_whole && !rc) {
            uint32_t *all = malloc((size_t)n_whole * sizeof(*all)), at = 0;
            if (!all) rc = _CERR_NOMEM;
            for (int t = 0; t < nt && all; t++) {
                if (jobs[t].n_whole) memcpy(all + at, jobs[t].whole, (size_t)jobs[t].n_whole * sizeof(*all));
                at += jobs[t].n_whole;
            }
            if (all) {
                qsort_r(all, n_whole, sizeof(*all), rec_slot_cmp, gs);
                for (uint32_t k = 0; k < n_whole; k++) {
                    struct gs_rec *r = &gs->rec[all[k]];
                    scatter_one(gs, r, &res, r->slot, true);
                    st->written_back++;
                }
                free(all);
            }
        }
        if (!rc) gs_par_run(par_deferred, jobs, nt);
        for (int t = 0; t < nt; t++) {
            st->written_back += jobs[t].count;
            free(jobs[t].deferred); free(jobs[t].whole);
            if (jobs[t].rc) rc = jobs[t].rc;
        }
        if (rc) return rc;
    } else if (4 * n_rebuilt > gs->n_order) {
        /* a batched entity's parent precedes it in the list (else it would be host-class): one pass, parents first */
        for (uint32_t k = 0; k < gs->n_order; k++) {
            struct gs_rec *r = &gs->rec[gs->order[k]];
            if (k + 8 < gs->n_order) {
                const struct gs_rec *a = &gs->rec[gs->order[k + 8]];
                if (a->cls == 1 && a->slot < res.n_slots && ((scat[a->slot >> 6] >> (a->slot & 63)) & 1)) {
                    prefetch_entity(a->e);
                    __builtin_prefetch(res.mx + 16 * (size_t)a->slot, 0, 0);
                    __builtin_prefetch(res.inverse_mx + 16 * (size_t)a->slot, 0, 0);
                    __builtin_prefetch(res.aabb + 6 * (size_t)a->slot, 0, 0);
                }
            }
            if (r->cls != 1 || r->slot >= res.n_slots || !((scat[r->slot >> 6] >> (r->slot & 63)) & 1)) continue;
            scatter_one(gs, r, &res, r->slot, true);
            st->written_back++;
        }
    } else {
        /* the rebuilt slots off the mask (ascending = parents first), then a plain loop that asks for the record eight
         * steps ahead and, once that has arrived, for the entity four steps ahead */
        uint32_t R = 0;
        for (uint32_t w = 0; w < words; w++) {
            uint64_t m = scat ? scat[w] : 0;
            while (m) {
                const uint32_t slot = w * 64 + (uint32_t)__builtin_ctzll(m);
                m &= m - 1;
                if (res.slot_user[slot] && push_u32(&gs->slots, &R, &gs->cap_slots, slot)) return _CERR_NOMEM;
            }
        }
        for (uint32_t k = 0; k < R; k++) {
            if (k + 8 < R) {
                const uint32_t sl = gs->slots[k + 8];
                __builtin_prefetch(&gs->rec[(uintptr_t)res.slot_user[sl] - 1], 0, 1);
                __builtin_prefetch(res.mx + 16 * (size_t)sl, 0, 0);
                __builtin_prefetch(res.inverse_mx + 16 * (size_t)sl, 0, 0);
            }
            if (k + 4 < R)
                prefetch_entity(gs->rec[(uintptr_t)res.slot_user[gs->slots[k + 4]] - 1].e);
            const uint32_t slot = gs->slots[k];
            struct gs_rec *rr = &gs->rec[(uintptr_t)res.slot_user[slot] - 1];
            if (rr->cls != 1) continue;                          /* class 4: after the pose, from the second launch */
            scatter_one(gs, rr, &res, slot, true);
            st->written_back++;
        }
    }
    const double ts2 = timing ? now_ms() : 0;
    gs_consume_fetched(gs);                                         /* came into view (or contain the camera) after frames of being left out */
    const double t3 = now_ms();
    uint32_t n_cand = 0;
    CK(hooks_and_picks(gs, mq, &res, &n_cand));
    st->batched = gs->n_batched; st->host = gs->n_host + gs->n_deferred;
    if (timing) fprintf(stderr, "fast_frame: mirror %.3f device %.3f scatter %.3f = lag+pend %.3f count %.3f rows %.3f fetched %.3f (rebuilt %llu) hooks+bv %.3f (cand %u host %u)\n", t1 - t0, t2 - t1, t3 - t2, ts0 - t2, ts1 - ts0, ts2 - ts1, t3 - ts2, (unsigned long long)n_rebuilt, now_ms() - t3, n_cand, gs->n_host);
    st->ms_walk = t1 - t0; st->ms_device = t2 - t1; st->ms_scatter = now_ms() - t2;
    return 0;
}

