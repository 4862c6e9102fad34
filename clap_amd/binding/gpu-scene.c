/*
 * gpu-scene.c -- CLAP-side binding of libclapgpu (see gpu-scene.h).  C23 like the engine,
 * compiled with the engine's flags against the engine's headers.
 *
 * What one gpu_mq_update() has to achieve (the steps of a WALKED frame; most frames skip most of them, below):
 *   1. walk mq->txmodels -> txm->entities in list order (what mq_for_each_matching does,
 *      model.c:1911-1922); look every ALIVE entity up in a pointer -> record table;
 *   2. decide which entities are batched: hook == default_update, no skeleton animation
 *      (animated_update, model.c:1715-1716), no physics body (phys_body_update /
 *      phys_body_rotate_xform, model.c:1659-1687 -- ODE is an absent submodule of the reference, so nothing that
 *      reads a dBody can be built into the checker), no joint attachment (it rides the palette of the SAME frame,
 *      which gpu-anim.inc.c computes after this update), and a batched (or no) parent that comes EARLIER in the
 *      list.  An entity that carries a light IS batched: step 5 hands its position on (light_set_pos,
 *      model.c:1689-1694);
 *   3. mirror creations, deletions, e->parent, e->flags and -- where xform.updated is set --
 *      position / rotation / scale into libclapgpu_scene, clearing xform.updated as
 *      default_update does (model.c:1615, 1668);
 *   4. clapgpu_scene_mq_update(): ONE kernel launch (update + cull of the frame's views), results in mapped memory;
 *   5. a batched entity that the reference would have rebuilt this frame (root: xform.updated; child: xform.updated or
 *      parent_seq != parent->seq, model.c:1609-1616) takes mx / inverse_mx / aabb / aabb_center from the results and has
 *      seq / parent_seq advanced the same way; the camera bounding-volume pick (model.c:1697-1713) is replayed for the
 *      entities whose box holds a query point; every other entity runs its own hook, in list order, so host entities
 *      see their device parents' fresh matrices and the order of side effects is the reference's.
 *
 * Where to find what.  This file: records and the pointer table; gpu_scene_init / _done; notifications (gpu_scene_touch*,
 * _entity_created / _deleting: entities placed into / taken out of the standing layout, gs_take_created); mq_update_frame,
 * which picks the kind of frame, and gpu_mq_update.  Beside it, behind gpu-scene-internal.h (the structs and the helpers
 * the files share, mirror_one -- step 3 for one entity -- and scatter_fetched among them):
 *   gpu-scene-walk.c     the walked frame as named parts -- walk_begin, walk_queue (the list chase on this thread,
 *                        criteria / classes / pushes on the workers), walk_settle, walk_device, walk_tail --, the class rule
 *                        and the chain resolver, gs_queue_unchanged (frames WITHOUT notifications go by the records),
 *                        by_host_fields (after a re-tile the mask comes from the host fields);
 *   gpu-scene-results.c  scatter_one (step 5 for one entity), the second launch, the GPU_SCATTER_DRAWN fetches, the mirror
 *                        passes, gs_fast_frame (a NOTIFIED frame: O(touched + rebuilt)) and gs_frame_results (the second half of
 *                        every frame: write-back by mask on the workers, hooks and bounding-volume candidates merged in
 *                        list order);
 *   gpu-scene-draw.c     views, verdicts, LOD pick, draw lists, snapshot;
 *   gpu-scene-pool.c     the worker pool and gpu_scene_par_for.
 *
 * A child that precedes its parent in list order lags one frame in the reference (model.c:1911-1922
 * walks creation order).  The device computes converged, parents-first results, so such a child -- and
 * its subtree -- is left on the host, where the lag is reproduced exactly: every entity, batched or not,
 * ends the frame with the reference's bits.
 */
#include "gpu-scene-internal.h"

static struct gpu_scene *g_bound;     /* the scene the engine-named entry points (gpu-exports.inc.c) serve */

int gs_rehash(struct gpu_scene *gs, uint32_t n_bucket)
{
    uint32_t *nb = malloc((size_t)n_bucket * sizeof(*nb));
    if (!nb) return _CERR_NOMEM;
    memset(nb, 0xff, (size_t)n_bucket * sizeof(*nb));
    for (uint32_t i = 0; i < gs->n_rec; i++) {
        struct gs_rec *r = &gs->rec[i];
        if (!r->e) continue;
        uint32_t *b = &nb[ptr_hash(r->e) & (n_bucket - 1)];
        r->next = *b;
        *b = i;
    }
    free(gs->bucket);
    gs->bucket = nb; gs->n_bucket = n_bucket;
    return 0;
}

int gs_model_handle(struct gpu_scene *gs, model3d *m, uint32_t *out)
{
    for (uint32_t i = 0; i < gs->n_models; i++)
        if (gs->models[i].model == m) { *out = gs->models[i].handle; return 0; }
    if (gs->n_models == gs->cap_models) {
        gs->cap_models = gs->cap_models ? 2 * gs->cap_models : 16;
        gs->models = realloc(gs->models, gs->cap_models * sizeof(*gs->models));
        if (!gs->models) return _CERR_NOMEM;
    }
    const float aabb[6] = { m->aabb[0][0], m->aabb[0][1], m->aabb[0][2], m->aabb[1][0], m->aabb[1][1], m->aabb[1][2] };
    int rc = clapgpu_scene_model_new(gs->scene, aabb, m->skip_aabb, out);
    if (rc) return rc;
    rc = clapgpu_scene_model_lods(gs->scene, *out, m->lod_min, m->lod_max);
    if (rc) return rc;
    gs->models[gs->n_models++] = (struct gs_model){ m, *out, m->lod_min, m->lod_max };
    return 0;
}

int gpu_scene_init(struct gpu_scene **out, int device, int (*default_hook)(entity3d *, void *))
{
    if (!out || !default_hook) return _CERR_INVALID_ARGUMENTS;
    struct gpu_scene *gs = calloc(1, sizeof(*gs));
    if (!gs) return _CERR_NOMEM;
    int rc = clapgpu_scene_create(&gs->scene, device);
    if (rc) { free(gs); return rc; }
    gs->default_hook = default_hook;
    clapgpu_scene_set_lod_sync(gs->scene, 1);                    /* gpu_scene_select_lod reports the LODs a pick changed itself */
    gs->free_rec = NO_REC;
    gs->verify = getenv("GPU_SCENE_VERIFY") != NULL;
    const char *sp = getenv("GPU_SCENE_SCATTER");
    gs->scatter_drawn = sp && !strcmp(sp, "drawn");
    const char *ip = getenv("GPU_SCENE_INCREMENTAL");
    gs->incremental = !(ip && !strcmp(ip, "0"));
    const char *rp = getenv("GPU_SCENE_REPLAY");
    gs->replay = !(rp && !strcmp(rp, "0"));
    gpu_scene_pool_ref();
    clapgpu_scene_set_parallel_for(gs->scene, gpu_scene_par_for, gs_par_threads());   /* the mirror's re-tile borrows the pool */
    *out = gs;
    return 0;
}

void gpu_scene_done(struct gpu_scene *gs)
{
    if (!gs) return;
    gpu_scene_pool_unref();
    clapgpu_scene_destroy(gs->scene);
    free(gs->rec); free(gs->bucket); free(gs->order); free(gs->prev_order); free(gs->models);
    free(gs->char_list);
    free(gs->lag_parent); free(gs->lag_keep); free(gs->att_list); free(gs->att_handles); free(gs->att_jt); free(gs->att_bind);
    free(gs->draw); free(gs->draw_lod); free(gs->draw_g); free(gs->draw_g_lod); free(gs->groups); free(gs->pend); free(gs->shown); free(gs->xptr); free(gs->ftab);
    free(gs->claim); free(gs->created); free(gs->dead_recs); free(gs->wtxm); free(gs->cands); free(gs->hf); free(gs->hf_mask); free(gs->keep_changes); free(gs->wq);
    free(gs->walk_fetch); free(gs->draw_txm); free(gs->slot_ent); free(gs->slot_txm); free(gs->slot_lod); free(gs->txms);
    free(gs->touched); free(gs->host_list); free(gs->deferred); free(gs->posmap); free(gs->slots); free(gs->vq_e); free(gs->vq_slot); free(gs->vq_ok);
    if (g_bound == gs) g_bound = NULL;
    free(gs);
}

static unsigned g_device_errors;

const struct gpu_scene_stats *gpu_scene_last_stats(const struct gpu_scene *gs)
{
    ((struct gpu_scene *)gs)->stats.device_errors = g_device_errors;
    return &gs->stats;
}

void gpu_scene_device_error(const char *what, int rc)
{
    static const char *seen[8];
    g_device_errors++;
    for (unsigned k = 0; k < 8; k++) {
        if (seen[k] == what) return;                                 /* this call site has been reported */
        if (!seen[k]) { seen[k] = what; break; }
    }
    fprintf(stderr, "clap gpu binding: %s failed (%d): %s -- served by the engine's host path; further failures of this call are "
                    "only counted (gpu_scene_device_errors())\n", what, rc, clapgpu_last_error());
}

unsigned gpu_scene_device_errors(void) { return g_device_errors; }

void gpu_scene_animation_elsewhere(struct gpu_scene *gs, bool elsewhere) { gs->anim_elsewhere = elsewhere; }

void gpu_scene_characters(struct gpu_scene *gs, bool (*is_plain)(entity3d *, int (*)(entity3d *, void *)),
                          int (*host_half)(entity3d *, void *))
{
    if (!gs) return;
    gs->char_plain = is_plain; gs->char_half = host_half;
    gs->topology_pending = true;
}

/* advances with every walk of the queue: between two equal values no entity changed its class */
uint32_t gpu_scene_walk_generation(const struct gpu_scene *gs) { return gs ? gs->gen : 0; }

bool gpu_scene_entity_is_batched(struct gpu_scene *gs, entity3d *e)
{
    const uint32_t i = rec_find(gs, e);
    return i != NO_REC && gs->rec[i].gen == gs->gen && (gs->rec[i].cls == 1 || gs->rec[i].cls == 4);
}

bool gpu_scene_last_was_fast(const struct gpu_scene *gs) { return gs->last_fast; }

void gpu_scene_set_notify(struct gpu_scene *gs, bool on)
{
    gs->notify = on; gs->topology_pending = true;
    if (!on) { gs->roomy = false; clapgpu_scene_set_incremental(gs->scene, 0); }
}

/* The first entity that comes or goes between two frames says what kind of queue this is: that frame is walked and
 * re-tiled as it always was, and from that re-tile on the mirror leaves room for such edits (an eighth of every row's lanes,
 * a spare row per tile of a hierarchy).  A queue whose make-up never changes stays packed tight and pays nothing (1 M
 * entities, all moving: the room costs ~10 % of a frame). */
static void want_room(struct gpu_scene *gs)
{
    if (gs->roomy) return;
    gs->roomy = true;
    clapgpu_scene_set_incremental(gs->scene, 1);
    gs->topology_pending = true;
}

void gpu_scene_set_incremental(struct gpu_scene *gs, bool on)
{
    if (!gs) return;
    gs->incremental = on;
    if (!on && (gs->n_created || gs->n_dead_recs)) gs->topology_pending = true;
    if (!on) { gs->roomy = false; clapgpu_scene_set_incremental(gs->scene, 0); }
}
void gpu_scene_set_verify(struct gpu_scene *gs, bool on) { if (gs) gs->verify = on; }

/* verification mode: batched entities whose transform was written past the mutators; they join the touched list */
static unsigned int verify_untouched(struct gpu_scene *gs)
{
    unsigned int found = 0;
    for (uint32_t k = 0; k < gs->n_order; k++) {
        struct gs_rec *r = &gs->rec[gs->order[k]];
        if ((r->cls != 1 && r->cls != 4) || !r->e || r->pending || !transform_is_updated(&r->e->xform)) continue;
        if (found++ < 4)
            fprintf(stderr, "gpu_scene: entity %p (queue position %u) has xform.updated set but was not reported: a transform_* "
                            "write without gpu_scene_touch()\n", (void *)r->e, k);
        gpu_scene_touch(gs, r->e);
    }
    return found;
}

void gpu_scene_bind(struct gpu_scene *gs, struct mq *mq, struct view *view)
{
    g_bound = gs;
    if (!gs) return;
    if (gs->bound_mq && mq != gs->bound_mq) {
        /* the object serves another queue from now on: what GPU_SCATTER_DRAWN left on the device for the old one's entities
         * comes over first (the new queue's walk meets none of them), and the next update walks.  With a topology report
         * pending a record may name freed memory: then the rows go to the entities the OLD queue's lists still hold, as a
         * walk would hand them out (found by `clap_dropin fuzz 305`: topology report, then another queue's frame) */
        if (gs->any_pend && gpu_scene_fetch_all(gs) == _CERR_NOT_SUPPORTED) gs_fetch_met_in_queue(gs, gs->bound_mq);
        gs->topology_pending = true;
    }
    gs->bound_mq = mq; gs->bound_view = view;
}

struct gpu_scene *gpu_scene_bound(void) { return g_bound; }
struct mq *gpu_scene_bound_mq(void) { return g_bound ? g_bound->bound_mq : NULL; }
struct view *gpu_scene_bound_view(void) { return g_bound ? g_bound->bound_view : NULL; }

/* an engine mutator (entity3d_position / _move / _rotate / _scale / _visible, model.c:1810-1842) changed e */
void gpu_scene_touch(struct gpu_scene *gs, entity3d *e)
{
    if (!gs || !gs->notify) return;
    const uint32_t i = rec_find(gs, e);
    if (i == NO_REC) return;                                         /* not ours (another queue), or new: its creator reports it */
    struct gs_rec *r = &gs->rec[i];
    if (r->pending) return;
    r->pending = 1;
    if (r->order_pos < gs->n_order && gs->vq_ok) gs->vq_ok[r->order_pos] = 0;      /* until the next update has mirrored it */
    if (push_u32(&gs->touched, &gs->n_touched, &gs->cap_touched, i)) gs->topology_pending = true;
}

/* entity3d_position / _move / _rotate / _scale changed e's transform and nothing else (transform_set_updated is set,
 * model.c:1810-1842): remembered by address.  Whoever changes e->flags, e->parent or e->update says so through
 * gpu_scene_touch() / gpu_scene_topology() as before -- this path does not look for it (the verification aid does: with
 * it on, every notification takes the checked path). */
void gpu_scene_touch_xform(struct gpu_scene *gs, entity3d *e)
{
    if (!gs || !gs->notify || gs->topology_pending) return;      /* a pending walk re-reads every transform anyway */
    if (gs->verify || !gs->ftab) { gpu_scene_touch(gs, e); return; }
    if (gs->n_xptr == gs->cap_xptr) {
        /* an entity may be written several times a frame; a list four times the queue says the game re-writes everything
         * all the time: the walk is the cheaper frame then */
        const uint64_t limit = 4ull * gs->n_order + 65536;
        if (gs->cap_xptr >= limit) { gs->topology_pending = true; return; }
        uint64_t cap = gs->cap_xptr ? 2ull * gs->cap_xptr : 4096;
        if (cap > limit) cap = limit;
        entity3d **q = realloc(gs->xptr, cap * sizeof(*q));
        if (!q) { gs->topology_pending = true; return; }
        gs->xptr = q; gs->cap_xptr = (uint32_t)cap;
    }
    gs->xptr[gs->n_xptr++] = e;
}

/* an entity taken in (or out: handle CLAPGPU_NO_ENTITY -- the key stays, the probe chains run through it) without a walk */
static int ftab_set(struct gpu_scene *gs, const entity3d *e, uint32_t handle, uint32_t slot)
{
    if (!gs->ftab) return 0;
    uint32_t h = ftab_home(gs, e);
    while (gs->ftab[h].key && gs->ftab[h].key != (uint64_t)(uintptr_t)e) h = (h + 1) & gs->ftab_mask;
    if (!gs->ftab[h].key) {
        if (handle == CLAPGPU_NO_ENTITY) return 0;
        if (10ull * (gs->ftab_count + 1) > 7ull * gs->ftab_cap) return gs_ftab_build(gs);   /* (order[] holds the new record already) */
        gs->ftab_count++;
    }
    gs->ftab[h] = (struct gs_fast){ (uint64_t)(uintptr_t)e, handle, slot };
    return 0;
}

/* entity3d_update(e, data) / entity3d_reset(e) is about to run e's update on the host: under GPU_SCATTER_DRAWN the
 * reference's body reads e->parent->mx / ->seq and advances e's own counters (model.c:1609-1616), so both entities are
 * shown what the device has first; e->seq is noted so that gpu_scene_host_updated() knows how far the host moved it */
void gpu_scene_host_update_begin(struct gpu_scene *gs, entity3d *e)
{
    if (!gs || !e) return;
    if (e->parent) gpu_scene_fetch(gs, e->parent);
    gpu_scene_fetch(gs, e);
}

/* entity3d_update(e, data) / entity3d_reset(e) (model.c:1793, 1726; callers outside the frame loop: instantiate_entity
 * model.c:1872, terrain.c:551) ran e's update on the host just now: mx, inverse_mx, aabb, seq, xform.updated are final, as
 * the reference leaves them.  The device's copy of a batched entity is not: it gets the transform with the next update and
 * rebuilds the entity there (its children follow its seq counter), and the write-back skips the fields the host owns. */
void gpu_scene_host_updated(struct gpu_scene *gs, entity3d *e)
{
    if (!gs) return;
    const uint32_t i = rec_find(gs, e);
    if (i == NO_REC) return;
    struct gs_rec *r = &gs->rec[i];
    if (r->cls != 1 && r->cls != 4) return;                      /* host-class: nothing is mirrored */
    r->host_done = 1;
    /* GPU_SCATTER_DRAWN: the host counted this rebuild itself; the device's must come back to be reconciled with it */
    if (gs->scatter_drawn && !r->keep && r->handle != CLAPGPU_NO_ENTITY && !clapgpu_scene_entity_keep(gs->scene, r->handle, 1)) r->keep = 1;
    if (!gs->notify || r->pending) return;
    r->pending = 1;
    if (r->order_pos < gs->n_order && gs->vq_ok) gs->vq_ok[r->order_pos] = 0;
    if (push_u32(&gs->touched, &gs->n_touched, &gs->cap_touched, i)) gs->topology_pending = true;
}

/* entity3d_make / entity3d_delete, e->parent = ..., e->update = ..., a body / light / joint attached: the next
 * gpu_mq_update() walks the queue once */
void gpu_scene_topology(struct gpu_scene *gs) { if (gs) gs->topology_pending = true; }

/* ---- creation / deletion without a walk (gpu-scene.h) ------------------------------------------------------------------ */
void gpu_scene_entity_created(struct gpu_scene *gs, entity3d *e)
{
    if (!gs || !e) return;
    if (gs->notify && gs->incremental && gs->walked) want_room(gs);
    if (!gs->notify || !gs->incremental || !gs->walked || gs->topology_pending) { gs->topology_pending = true; return; }
    if (gs->n_created == gs->cap_created) {
        const uint32_t cap = gs->cap_created ? 2 * gs->cap_created : 64;
        entity3d **q = cap > (1u << 20) ? NULL : realloc(gs->created, (size_t)cap * sizeof(*q));   /* a level load: the walk is the cheaper frame */
        if (!q) { gs->topology_pending = true; return; }
        gs->created = q; gs->cap_created = cap;
    }
    gs->created[gs->n_created++] = e;
}

void gpu_scene_entity_deleting(struct gpu_scene *gs, entity3d *e)
{
    if (!gs || !e) return;
    if (gs->notify && gs->incremental && gs->walked) want_room(gs);
    if (!gs->notify || !gs->incremental || !gs->walked || gs->topology_pending || gs->in_frame) {
        /* the next update walks the queue.  If the allocator hands this entity3d's memory to a new entity before then, the walk
         * meets a familiar address: the record says that it is not the entity it knew (same model, xform.updated cleared by an
         * instantiate_entity-style default_update: nothing else would tell, and the device would keep the old transform) */
        const uint32_t g = rec_find(gs, e);
        if (g != NO_REC) gs->rec[g].gone = 1;
        gs->topology_pending = true;
        return;
    }
    for (uint32_t k = gs->n_created; k-- > 0;)                   /* made and gone between two frames: never seen */
        if (gs->created[k] == e) {
            memmove(gs->created + k, gs->created + k + 1, (size_t)(gs->n_created - k - 1) * sizeof(*gs->created));
            gs->n_created--;
            return;
        }
    const uint32_t i = rec_find(gs, e);
    if (i == NO_REC) return;                                     /* another queue's entity */
    struct gs_rec *r = &gs->rec[i];
    const struct scene *scene = gs->hook_data;
    if (r->cls == 2 && !r->lag && e != gs->last_control && !(scene && e == scene->control)) {
        /* a host-class entity (its own hook, or below such a one): nothing of it is on the device; it leaves the list of
         * hooks a fast frame runs -- unless another host-class entity hangs below it (the walk sorts that out) */
        uint32_t at = NO_REC;
        for (uint32_t k = 0; k < gs->n_host; k++) {
            const struct gs_rec *h = &gs->rec[gs->host_list[k]];
            if (gs->host_list[k] == i) at = k;
            else if (h->e && h->parent_e == e) { r->gone = 1; gs->topology_pending = true; return; }
        }
        if (at == NO_REC || push_u32(&gs->dead_recs, &gs->n_dead_recs, &gs->cap_dead_recs, i)) { r->gone = 1; gs->topology_pending = true; return; }
        memmove(gs->host_list + at, gs->host_list + at + 1, (size_t)(gs->n_host - at - 1) * sizeof(*gs->host_list));
        gs->n_host--;
        if (gs->vq_e && r->order_pos < gs->cap_vq) { gs->vq_e[r->order_pos] = NULL; gs->vq_ok[r->order_pos] = 0; }
        uint32_t *hl = &gs->bucket[ptr_hash(e) & (gs->n_bucket - 1)];
        while (*hl != i) hl = &gs->rec[*hl].next;
        *hl = r->next;
        r->e = NULL; r->cls = 0; r->self_ok = 0;
        r->parent_e = NULL; r->parent_rec = NO_REC;
        gs->n_live--;
        gs->inc_removed++;
        return;
    }
    /* in place: a batched leaf nobody depends on -- no batched child (the mirror knows), no host-class child reading its
     * matrix, not the control entity, no hook half of its own, no joint */
    if (r->cls != 1 || r->host_child || r->att || r->handle == CLAPGPU_NO_ENTITY || e->update != gs->default_hook ||
        e == gs->last_control || (scene && e == scene->control) ||
        push_u32(&gs->dead_recs, &gs->n_dead_recs, &gs->cap_dead_recs, i)) {
        r->gone = 1;
        gs->topology_pending = true;
        return;
    }
    if (clapgpu_scene_entity_delete_placed(gs->scene, r->handle)) {
        gs->n_dead_recs--;
        r->gone = 1;
        gs->topology_pending = true;
        return;
    }
    const uint32_t slot = r->slot;
    if (gs->pend && slot < gs->cap_pend) { gs->pend[slot] = 0; if (gs->shown) gs->shown[slot] = 0; }
    if (slot < gs->cap_slot_arrays) gs->slot_ent[slot] = NULL;
    if (gs->vq_e && r->order_pos < gs->cap_vq) { gs->vq_e[r->order_pos] = NULL; gs->vq_ok[r->order_pos] = 0; }
    ftab_set(gs, e, CLAPGPU_NO_ENTITY, 0);
    /* the record stays where order[] names it, as a tombstone, until the next walk: out of the hash, no entity, no class */
    uint32_t *link = &gs->bucket[ptr_hash(e) & (gs->n_bucket - 1)];
    while (*link != i) link = &gs->rec[*link].next;
    *link = r->next;
    r->e = NULL; r->cls = 0; r->self_ok = 0; r->keep = r->user_keep = 0;
    r->handle = r->parent_handle = CLAPGPU_NO_ENTITY;
    r->parent_e = NULL; r->parent_rec = NO_REC;
    gs->n_live--;
    if (gs->n_batched) gs->n_batched--;
    gs->inc_removed++;
}

static int ensure_order(struct gpu_scene *gs, uint32_t n)
{
    if (n > gs->cap_order) {
        uint32_t cap = gs->cap_order ? gs->cap_order : 4096;
        while (cap < n) cap *= 2;
        uint32_t *o = realloc(gs->order, (size_t)cap * sizeof(*o));
        if (o) gs->order = o;
        uint32_t *po = realloc(gs->prev_order, (size_t)cap * sizeof(*po));
        if (po) gs->prev_order = po;
        if (!o || !po) return _CERR_NOMEM;
        gs->cap_order = cap;
    }
    if (gs->cap_order > gs->cap_vq) {
        const uint32_t cap = gs->cap_order;
        entity3d **ve = realloc(gs->vq_e, (size_t)cap * sizeof(*ve));
        if (ve) gs->vq_e = ve;
        uint32_t *vs = realloc(gs->vq_slot, (size_t)cap * 4);
        if (vs) gs->vq_slot = vs;
        uint8_t *vo = realloc(gs->vq_ok, cap);
        if (vo) gs->vq_ok = vo;
        if (!ve || !vs || !vo) return _CERR_NOMEM;
        gs->cap_vq = cap;
    }
    return 0;
}

/* the per-slot state of a fast frame, for a layout that grew at its end (a growth tile) */
static int ensure_slot_state(struct gpu_scene *gs, uint32_t n_slots)
{
    if (gs->pend && gs->shown && n_slots > gs->cap_pend) {
        uint16_t *pn = realloc(gs->pend, (size_t)n_slots * sizeof(*pn));
        if (pn) gs->pend = pn;
        uint16_t *sn = realloc(gs->shown, (size_t)n_slots * sizeof(*sn));
        if (sn) gs->shown = sn;
        if (!pn || !sn) return _CERR_NOMEM;
        memset(gs->pend + gs->cap_pend, 0, (size_t)(n_slots - gs->cap_pend) * sizeof(*pn));
        memset(gs->shown + gs->cap_pend, 0, (size_t)(n_slots - gs->cap_pend) * sizeof(*sn));
        gs->cap_pend = n_slots;
    }
    if (gs->cap_slot_arrays && n_slots > gs->cap_slot_arrays) {
        const uint32_t old = gs->cap_slot_arrays;
        entity3d **a = realloc(gs->slot_ent, (size_t)n_slots * sizeof(*a));
        if (a) gs->slot_ent = a;
        uint16_t *b = realloc(gs->slot_txm, (size_t)n_slots * sizeof(*b));
        if (b) gs->slot_txm = b;
        int8_t *c = realloc(gs->slot_lod, n_slots);
        if (c) gs->slot_lod = c;
        if (!a || !b || !c) { gs->cap_slot_arrays = 0; return 0; }   /* the draw list goes through the records then */
        memset(gs->slot_ent + old, 0, (size_t)(n_slots - old) * sizeof(*a));
        gs->cap_slot_arrays = n_slots;
    }
    return 0;
}

/*
 * The entities reported by gpu_scene_entity_created() since the last update, in creation order (= list order inside a
 * txmodel: entity3d_make appends, model.c:1759): each gets a record, a place in the standing device layout and a seat at
 * the end of order[]; its transform and flags travel with this frame's touched entities.  Returns 1 when one of them has
 * to be met by a walk instead (then the frame is a walk: records made so far are found by it like any other).
 */
int gs_take_created(struct gpu_scene *gs, struct mq *mq)
{
    const struct scene *scene = mq->priv;
    for (uint32_t k = 0; k < gs->n_created; k++) {
        entity3d *e = gs->created[k];
        if (!entity3d_matches(e, ENTITY3D_ALIVE)) continue;      /* the walk would not meet it either */
        uint32_t rank = 0xffffffffu;
        for (uint32_t t = gs->n_wtxm; t-- > 0;)
            if (gs->wtxm[t].txm == e->txmodel) { rank = t; break; }
        if (rank == 0xffffffffu) {
            model3dtx *txm;
            bool ours = false;
            list_for_each_entry(txm, &mq->txmodels, entry) if (txm == e->txmodel) { ours = true; break; }
            if (ours) return 1;                                  /* a txmodel the last walk has not seen */
            continue;                                            /* another queue's entity */
        }
        if ((e->parent && e->parent_joint != JOINT_TYPE_MAX) || rec_find(gs, e) != NO_REC) return 1;
        /* plain: what the device can hold without anything else being set up.  Batchable in another way (a body-less
         * character, an animated entity whose pose runs elsewhere): the walk registers those.  Everything else is
         * host-class -- its own hook runs it, at its place in the list */
        const bool selfb = self_batchable(gs, e);
        const bool plain = selfb && e->update == gs->default_hook && !entity_animated(e);
        if (selfb && !plain) return 1;
        const uint64_t key = ((uint64_t)rank << 32) | gs->wtxm[rank].next;
        uint32_t pi = NO_REC;
        if (e->parent) {
            /* below a parent the last walk met, listed earlier (one listed later is read a frame late: the walk's lag
             * machinery), batched or host-class (not one of the frame's second launch) */
            pi = rec_find(gs, e->parent);
            if (pi == NO_REC || (gs->rec[pi].cls != 1 && gs->rec[pi].cls != 2) || gs->rec[pi].order_key > key ||
                (gs->rec[pi].cls == 1 && gs->rec[pi].handle == CLAPGPU_NO_ENTITY))
                return 1;
        }
        if (!plain || (pi != NO_REC && gs->rec[pi].cls == 2)) {
            /* host-class: a record, a seat in order[] and, by its place in the queue, in the list of hooks */
            CK(ensure_order(gs, gs->n_order + 1));
            if (gs->n_host == gs->cap_host) {
                if (push_u32(&gs->host_list, &gs->n_host, &gs->cap_host, 0)) return _CERR_NOMEM;
                gs->n_host--;
            }
            const uint32_t i = rec_add(gs, e);
            if (i == NO_REC) return _CERR_NOMEM;
            struct gs_rec *r = &gs->rec[i];
            gs->wtxm[rank].next++;
            r->model = e->txmodel->model;
            r->parent_e = e->parent; r->parent_rec = pi;
            r->gen = gs->gen;
            r->cls = 2; r->self_ok = selfb; r->animated = entity_animated(e);
            r->order_key = key;
            r->order_pos = gs->n_order;
            gs->order[gs->n_order++] = i;
            gs->appended = true;
            gs->vq_e[r->order_pos] = e; gs->vq_slot[r->order_pos] = CLAPGPU_NO_ENTITY; gs->vq_ok[r->order_pos] = 0;
            uint32_t at = gs->n_host;
            while (at && gs->rec[gs->host_list[at - 1]].order_key > key) at--;
            memmove(gs->host_list + at + 1, gs->host_list + at, (size_t)(gs->n_host - at) * sizeof(*gs->host_list));
            gs->host_list[at] = i;
            gs->n_host++;
            if (pi != NO_REC && gs->rec[pi].cls == 1) {          /* its hook reads that parent's mx / seq every frame: a standing reader */
                struct gs_rec *pr = &gs->rec[pi];
                pr->host_child = 1;
                if (gs->scatter_drawn && !pr->keep && !clapgpu_scene_entity_keep(gs->scene, pr->handle, 1)) {
                    pr->keep = 1;
                    gpu_scene_fetch(gs, pr->e);
                }
            }
            gs->inc_placed++;
            continue;
        }
        uint32_t mh;
        CK(gs_model_handle(gs, e->txmodel->model, &mh));
        CK(ensure_order(gs, gs->n_order + 1));
        const uint32_t i = rec_add(gs, e);
        if (i == NO_REC) return _CERR_NOMEM;
        struct gs_rec *r = &gs->rec[i];
        uint32_t handle, slot;
        const int rc = clapgpu_scene_entity_new_placed(gs->scene, mh, (void *)(uintptr_t)(i + 1u),
                                                       pi == NO_REC ? CLAPGPU_NO_ENTITY : gs->rec[pi].handle, &handle, &slot);
        if (rc) {
            rec_del(gs, i);
            if (rc == CLAPGPU_ERR_NOT_SUPPORTED) return 1;       /* no room where it would have to go: the walk re-tiles */
            return rc;
        }
        gs->wtxm[rank].next++;
        r->model = e->txmodel->model;
        r->handle = handle; r->slot = slot;
        r->parent_e = e->parent; r->parent_rec = pi;
        r->parent_handle = pi == NO_REC ? CLAPGPU_NO_ENTITY : gs->rec[pi].handle;
        r->flags = ENTITY3D_ALIVE | ENTITY3D_VISIBLE;            /* what the mirror's entity starts with; the touched pass brings e->flags */
        r->lod_force = -1; r->lod_cur = 0;
        if (e->force_lod != -1 || e->cur_lod != 0) {
            CK(clapgpu_scene_entity_lod(gs->scene, handle, e->force_lod, e->cur_lod));
            r->lod_force = e->force_lod; r->lod_cur = e->cur_lod;
        }
        r->gen = gs->gen;
        r->cls = 1; r->self_ok = 1;
        r->order_key = key;
        r->order_pos = gs->n_order;
        gs->order[gs->n_order++] = i;
        gs->appended = true;
        CK(ensure_slot_state(gs, clapgpu_scene_slot_count(gs->scene)));
        if (gs->pend && slot < gs->cap_pend) { gs->pend[slot] = 0; gs->shown[slot] = e->seq; }
        if (slot < gs->cap_slot_arrays) {
            const uint32_t g = txm_index(gs, e->txmodel);
            if (g == 0xffffffffu || e->cur_lod < -128 || e->cur_lod > 127) gs->cap_slot_arrays = 0;
            else { gs->slot_ent[slot] = e; gs->slot_txm[slot] = (uint16_t)g; gs->slot_lod[slot] = (int8_t)e->cur_lod; }
        }
        gs->vq_e[r->order_pos] = e; gs->vq_slot[r->order_pos] = slot; gs->vq_ok[r->order_pos] = 0;   /* until the touched pass has its flags */
        CK(ftab_set(gs, e, handle, slot));
        if (gs->scatter_drawn && (e->light_idx >= 0 || (scene && e == scene->control)) &&
            !clapgpu_scene_entity_keep(gs->scene, handle, 1))
            r->keep = 1;
        if (!transform_is_updated(&e->xform)) {
            /* never positioned, or updated on the spot already (entity3d_update / _reset before its first frame): the host
             * fields are final as they are; the device builds its copy, the write-back leaves the entity3d alone unless its
             * parent moved on (gpu_scene_host_updated) */
            r->host_done = 1;
            if (gs->scatter_drawn && !r->keep && !clapgpu_scene_entity_keep(gs->scene, handle, 1)) r->keep = 1;
        }
        r->pending = 1;
        if (push_u32(&gs->touched, &gs->n_touched, &gs->cap_touched, i)) return _CERR_NOMEM;
        gs->n_batched++;
        gs->inc_placed++;
    }
    gs->n_created = 0;
    return 0;
}

static int mq_update_frame(struct gpu_scene *gs, struct mq *mq, struct view *view)
{
    struct gpu_scene_stats *st = &gs->stats;
    gs->hook_data = mq->priv;
    memset(st, 0, sizeof(*st));
    gs->gen++;
    if (gs->notify && gs->walked && !gs->topology_pending) {
        gs->gen--;                                                /* nothing entered or left the queue: the records' generation stands */
        const unsigned int untouched = gs->verify ? verify_untouched(gs) : 0;
        const int rc = gs_fast_frame(gs, mq, view);
        st->untouched_writes = untouched;
        gs->last_fast = rc == 0;
        if (rc <= 0) return rc;
        gs->gen++;
        memset(st, 0, sizeof(*st));                               /* a touched entity changed class: walk */
    } else if (!gs->notify && gs->replay && gs->walked && !gs->topology_pending && gs->n_order >= GS_REPLAY_MIN &&
               gs_par_threads() > 1 && !gs->n_touched && gs_queue_unchanged(gs, mq)) {
        /* no notifications, and the queue is the one the last walk met: the frame by the records (see gs_queue_unchanged) */
        if (gs->n_order > gs->cap_touched) {
            uint32_t *q = realloc(gs->touched, (size_t)gs->cap_order * sizeof(*q));
            if (!q) return _CERR_NOMEM;
            gs->touched = q; gs->cap_touched = gs->cap_order;
        }
        memcpy(gs->touched, gs->order, (size_t)gs->n_order * sizeof(*gs->touched));
        gs->n_touched = gs->n_order;
        gs->gen--;
        gs->replaying = true;
        const int rc = gs_fast_frame(gs, mq, view);
        gs->replaying = false;
        gs->last_fast = false;                                    /* (the word is kept for frames that looked at what was reported only) */
        if (rc <= 0) { st->replayed = rc == 0; return rc; }
        gs->gen++;
        memset(st, 0, sizeof(*st));                               /* an entity would be classified differently now: walk */
    }
    return gs_walked_frame(gs, mq, view);
}

int gpu_mq_update(struct gpu_scene *gs, struct mq *mq, struct view *view)
{
    if (!gs || !mq) return _CERR_INVALID_ARGUMENTS;
    /* a hook that runs inside the frame may delete entities (the reference's list walk takes that in its stride): nothing is
     * taken out of the lists the frame is iterating -- gpu_scene_entity_deleting() marks the record, the rest of the frame
     * skips it, the next frame walks */
    gs->in_frame = true;
    const int rc = mq_update_frame(gs, mq, view);
    gs->in_frame = false;
    return rc;
}
