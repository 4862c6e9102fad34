/*
 * gpu-scene-walk.c -- the WALKED frame of the entity binding (gpu-scene.c; shared declarations in gpu-scene-internal.h):
 * steps 1-5 when the queue's make-up may have changed.  In file order: link_parent / unbatch (what a class asks of the
 * mirror besides mirror_one); the tables a walk leaves behind (slot arrays, the address table); gs_queue_unchanged (a frame
 * without notifications whose queue stood goes by the records instead); the chain resolver and by_host_fields (after a
 * re-tile the write-back mask comes from the host fields); walk_tail's passes; the walk's parts -- walk_begin, the class
 * rule, walk_classify / walk_act (the serial walk), the workers' walk, walk_queue, walk_settle, walk_device, walk_tail --
 * and gs_walked_frame, which runs them in order.
 */
#include "gpu-scene-internal.h"

static int link_parent(struct gpu_scene *gs, struct gs_rec *r)
{
    const uint32_t ph = r->e->parent ? gs->rec[parent_rec(gs, r)].handle : CLAPGPU_NO_ENTITY;
    if (ph != r->parent_handle) {
        CK(clapgpu_scene_entity_set_parent(gs->scene, r->handle, ph));
        r->parent_handle = ph;
    }
    return 0;
}

static int unbatch(struct gpu_scene *gs, struct gs_rec *r)        /* left the batch (gained a body, a hook, ...) */
{
    if (r->handle != CLAPGPU_NO_ENTITY) {
        CK(clapgpu_scene_entity_delete(gs->scene, r->handle));
        r->handle = r->parent_handle = CLAPGPU_NO_ENTITY;
        gs->stats.deleted++;
    }
    return 0;
}

/* the tables a walk leaves behind are filled from the records on the workers (1 M entities: ~40 ms of a walked frame on one) */
#define GS_TABLES_PAR_MIN 16384u
struct walk_tables_ctx { struct gpu_scene *gs; uint32_t n_slots; int bad; uint32_t count; };
static void slot_arrays_range(void *ctx, uint32_t lo, uint32_t hi)
{
    struct walk_tables_ctx *wc = ctx;
    struct gpu_scene *gs = wc->gs;
    for (uint32_t k = lo; k < hi; k++) {
        const struct gs_rec *r = &gs->rec[gs->order[k]];
        if ((r->cls != 1 && r->cls != 4) || r->slot >= wc->n_slots) continue;
        if (r->lod_cur < -128 || r->lod_cur > 127) { __atomic_store_n(&wc->bad, 1, __ATOMIC_RELAXED); return; }
        gs->slot_ent[r->slot] = r->e;                            /* (a slot has one record) */
        gs->slot_txm[r->slot] = (uint16_t)(r->order_key >> 32);
        gs->slot_lod[r->slot] = (int8_t)r->lod_cur;
    }
}

static int slot_arrays_build(struct gpu_scene *gs)
{
    const uint32_t n = clapgpu_scene_slot_count(gs->scene);
    if (n > gs->cap_slot_arrays) {
        entity3d **a = realloc(gs->slot_ent, (size_t)n * sizeof(*a));
        if (a) gs->slot_ent = a;
        uint16_t *b = realloc(gs->slot_txm, (size_t)n * sizeof(*b));
        if (b) gs->slot_txm = b;
        int8_t *c = realloc(gs->slot_lod, n);
        if (c) gs->slot_lod = c;
        if (!a || !b || !c) { gs->cap_slot_arrays = 0; return _CERR_NOMEM; }
        gs->cap_slot_arrays = n;
    }
    if (n) memset(gs->slot_ent, 0, (size_t)n * sizeof(*gs->slot_ent));
    /* from the records alone (an entity3d is 448 bytes somewhere else): the txmodel is the walk's rank of it (order_key), the
     * LOD what mirror_one() last saw in e->cur_lod */
    gs->n_txms = 0;
    if (gs->n_wtxm > 65535) { gs->cap_slot_arrays = 0; return _CERR_NOMEM; }
    for (uint32_t t = 0; t < gs->n_wtxm; t++) {
        gs->n_txms = t;                                          /* (txm_index appends at n_txms) */
        if (gs->n_txms == gs->cap_txms) {
            const uint32_t cap = gs->cap_txms ? 2 * gs->cap_txms : 32;
            const model3dtx **q = realloc(gs->txms, (size_t)cap * sizeof(*q));
            if (!q) { gs->cap_slot_arrays = 0; return _CERR_NOMEM; }
            gs->txms = q; gs->cap_txms = cap;
        }
        gs->txms[t] = gs->wtxm[t].txm;
    }
    gs->n_txms = gs->n_wtxm;
    struct walk_tables_ctx wc = { gs, n, 0, 0 };
    gpu_scene_par_for(slot_arrays_range, &wc, gs->n_order, gs->n_order >= GS_TABLES_PAR_MIN ? gs_par_threads() : 1);
    if (wc.bad) { gs->cap_slot_arrays = 0; return _CERR_NOMEM; }   /* a LOD outside int8: the record path then */
    return 0;
}

/* (every key is distinct and nobody looks anything up before the join: a home is claimed by its key, the rest follows) */
static void ftab_range(void *ctx, uint32_t lo, uint32_t hi)
{
    struct walk_tables_ctx *wc = ctx;
    struct gpu_scene *gs = wc->gs;
    uint32_t count = 0;
    for (uint32_t k = lo; k < hi; k++) {
        const struct gs_rec *r = &gs->rec[gs->order[k]];
        if (!r->e) continue;                                      /* taken out in place since the walk */
        count++;
        uint32_t h = ftab_home(gs, r->e);
        for (;;) {
            uint64_t none = 0;
            if (__atomic_compare_exchange_n(&gs->ftab[h].key, &none, (uint64_t)(uintptr_t)r->e, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) break;
            h = (h + 1) & gs->ftab_mask;
        }
        gs->ftab[h].handle = (r->cls == 1 || r->cls == 4) ? r->handle : CLAPGPU_NO_ENTITY;
        gs->ftab[h].slot = r->slot;
    }
    __atomic_fetch_add(&wc->count, count, __ATOMIC_RELAXED);
}

int gs_ftab_build(struct gpu_scene *gs)
{
    uint32_t cap = 1024;
    while (cap < 2 * gs->n_order) cap *= 2;
    if (cap != gs->ftab_cap) {
        struct gs_fast *t = realloc(gs->ftab, (size_t)cap * sizeof(*t));
        if (!t) { free(gs->ftab); gs->ftab = NULL; gs->ftab_cap = 0; return _CERR_NOMEM; }
        gs->ftab = t; gs->ftab_cap = cap;
    }
    gs->ftab_mask = cap - 1;
    memset(gs->ftab, 0, (size_t)cap * sizeof(*gs->ftab));
    struct walk_tables_ctx wc = { gs, 0, 0, 0 };
    gpu_scene_par_for(ftab_range, &wc, gs->n_order, gs->n_order >= GS_TABLES_PAR_MIN ? gs_par_threads() : 1);
    gs->ftab_count = wc.count;
    return 0;
}

/*
 * Frames WITHOUT notifications.  Nothing tells the binding what changed, so the reference's way is to look at every entity --
 * but not necessarily by chasing the lists on one core: if the queue is still the one the last walk met (every entity's list
 * successor is the next record's entity, every txmodel's list starts and ends where it did: checked on the workers, one
 * list node per entity) the frame goes by the records -- every record "touched", the mirror pass on the workers re-reading
 * what a walk would read (flags, xform.updated, the inputs of the entity's class, its LODs) -- and falls back to the walk
 * the moment anything a walk would have classified differently shows up.  1 M entities: 72 ms of list walk -> a few ms.
 */
struct quc_ctx { struct gpu_scene *gs; int changed; };
static void queue_unchanged_range(void *ctx, uint32_t lo, uint32_t hi)
{
    struct quc_ctx *qc = ctx;
    struct gpu_scene *gs = qc->gs;
    for (uint32_t k = lo; k < hi; k++) {
        const struct gs_rec *r = &gs->rec[gs->order[k]];
        if (k + 8 < hi) __builtin_prefetch(&gs->rec[gs->order[k + 8]].e->entry, 0, 1);
        const uint32_t rank = (uint32_t)(r->order_key >> 32);
        const struct list *head = &gs->wtxm[rank].txm->entities;
        const struct list *n = r->e->entry.next;                 /* the next ALIVE entity behind it in its txmodel's list */
        while (n != head && !entity3d_matches(list_entry((struct list *)n, entity3d, entry), ENTITY3D_ALIVE)) n = n->next;
        const entity3d *want = (k + 1 < gs->n_order && (uint32_t)(gs->rec[gs->order[k + 1]].order_key >> 32) == rank)
                               ? gs->rec[gs->order[k + 1]].e : NULL;
        const entity3d *got = n == head ? NULL : list_entry((struct list *)n, entity3d, entry);
        if (got != want) { __atomic_store_n(&qc->changed, 1, __ATOMIC_RELAXED); return; }
    }
}

bool gs_queue_unchanged(struct gpu_scene *gs, struct mq *mq)
{
    uint32_t t = 0;
    model3dtx *txm;
    list_for_each_entry(txm, &mq->txmodels, entry) {             /* the txmodels, and where each one's list starts */
        if (t >= gs->n_wtxm || gs->wtxm[t].txm != txm) return false;
        const struct list *head = &txm->entities, *n = head->next;
        while (n != head && !entity3d_matches(list_entry((struct list *)n, entity3d, entry), ENTITY3D_ALIVE)) n = n->next;
        const entity3d *first = n == head ? NULL : list_entry((struct list *)n, entity3d, entry);
        const entity3d *want = gs->wtxm[t].next ? gs->rec[gs->order[gs->wtxm[t].first]].e : NULL;
        if (first != want) return false;
        t++;
    }
    if (t != gs->n_wtxm) return false;
    struct quc_ctx qc = { gs, 0 };
    const double q0 = getenv("GPU_SCENE_TIMING") ? now_ms() : 0;
    gpu_scene_par_for(queue_unchanged_range, &qc, gs->n_order, gs_par_threads());   /* (only from GS_REPLAY_MIN entities up) */
    if (q0 != 0) fprintf(stderr, "queue_unchanged: %u entities in %.3f ms (%s)\n", gs->n_order, now_ms() - q0, qc.changed ? "changed" : "the same");
    return !qc.changed;
}

/*
 * A walked frame that RE-TILED.  The device has rebuilt every row of the new layout, so its mask cannot say what the reference
 * would have rebuilt -- the host fields do (model.c:1609-1616, 1667): an entity is rebuilt if its transform was written, or if
 * its parent_seq is not its parent's seq AS THE PARENT LEAVES THIS FRAME (the parent comes earlier in the list).  That is a
 * recurrence up the ancestor chain -- rebuilt(e) = dirty(e) || parent_seq(e) != seq(parent) + rebuilt(parent) --, which one
 * thread used to evaluate in list order over every entity3d (1 M entities: 45-50 ms).  Here: pass A copies the four values it
 * needs out of every batched entity (on the workers), pass B walks each entity's chain over that compact array until it
 * meets a decided ancestor (states are written once with the same value by whoever gets there first), and the result is a
 * mask by slot of the NEW layout -- which gs_frame_results() takes in place of the device's, write-back on the workers, hooks
 * and bounding-volume pick merged in list order, exactly as after a frame whose layout stood.
 */
#define HF_NONE 0xffffffffu

/*
 * The chain resolver of the workers' passes over order[] (by_host_fields, the walk's classes): entries of `stride` bytes at
 * `base`, each beginning with a uint32_t `ppos` (its parent's entry, which comes earlier) and holding a uint8_t state at
 * `state_at`, 0 while undecided.  Entry k's state: walk up ppos to the first decided ancestor, then write the states back down,
 * each from its parent's by step(ctx, entry, parent's state).  Every state is written once, with the same value by whoever gets
 * there first, so the workers may meet on a chain.  Iterative on a fixed buffer: a chain with more than GS_CHAIN_SEG undecided
 * entries is decided from its top, GS_CHAIN_SEG entries a round, each round walking up from k again.
 */
#define GS_CHAIN_SEG 64u
static inline uint8_t chain_resolve(char *base, size_t stride, size_t state_at, uint32_t k,
                                    uint8_t (*step)(const void *, uint32_t, uint8_t), const void *ctx)
{
    for (;;) {
        uint32_t seg[GS_CHAIN_SEG], n = 0, cur = k;              /* the last GS_CHAIN_SEG undecided entries met on the way up */
        uint8_t s;
        while (!(s = __atomic_load_n((uint8_t *)(base + (size_t)cur * stride + state_at), __ATOMIC_RELAXED))) {
            seg[n++ % GS_CHAIN_SEG] = cur;
            cur = *(const uint32_t *)(base + (size_t)cur * stride);
        }
        const uint32_t top = n > GS_CHAIN_SEG ? n - GS_CHAIN_SEG : 0;
        for (uint32_t i = n; i-- > top;) {
            const uint32_t c = seg[i % GS_CHAIN_SEG];
            s = step(ctx, c, s);
            __atomic_store_n((uint8_t *)(base + (size_t)c * stride + state_at), s, __ATOMIC_RELAXED);
        }
        if (!top) return s;
    }
}

struct hf_ctx { struct gpu_scene *gs; uint32_t n_slots; };
static void hf_collect_range(void *ctx, uint32_t lo, uint32_t hi)
{
    struct hf_ctx *hc = ctx;
    struct gpu_scene *gs = hc->gs;
    for (uint32_t k = lo; k < hi; k++) {
        struct gs_rec *r = &gs->rec[gs->order[k]];
        struct gs_hf *h = &gs->hf[k];
        if (k + 24 < hi) __builtin_prefetch(&gs->rec[gs->order[k + 24]], 0, 1);
        if (k + 8 < hi) prefetch_entity(gs->rec[gs->order[k + 8]].e);
        h->state = 1; h->dirty = 0; h->ppos = HF_NONE; h->seq0 = h->pseq = 0;
        if (r->gone || (r->cls != 1 && r->cls != 4)) continue;
        const entity3d *e = r->e;
        r->slot = clapgpu_scene_entity_slot(gs->scene, r->handle);
        if (r->slot != CLAPGPU_NO_ENTITY) seq_shown(gs, r->slot, e->seq);    /* (rebuilt ones are shown their new seq by the write-back) */
        if (r->cls == 4) continue;                               /* after the pose, from the second launch: gpu_scene_run_deferred() */
        r->host_done = 0;                                        /* the host fields decide here: a host-updated entity is simply not dirty */
        h->seq0 = e->seq; h->pseq = e->parent_seq; h->dirty = r->xform_dirty;
        h->state = 0;
        if (r->slot == CLAPGPU_NO_ENTITY || r->slot >= hc->n_slots) { h->state = 1; continue; }   /* (cannot be: the mirror holds every batched entity) */
        if (h->dirty) h->state = 2;
        else if (!e->parent) h->state = 1;
        else if (r->parent_rec != NO_REC && gs->rec[r->parent_rec].e == e->parent && gs->rec[r->parent_rec].gen == gs->gen)
            h->ppos = gs->rec[r->parent_rec].order_pos;          /* a batched entity's parent is batched and comes earlier (the class rules) */
        else
            h->state = e->parent_seq != e->parent->seq ? 2 : 1;  /* (cannot be either; by the parent as it stands) */
    }
}

/* the resolver's step: rebuilt (2) or not (1), from whether the parent was */
static uint8_t hf_step(const void *ctx, uint32_t c, uint8_t ps)
{
    const struct gs_hf *hf = ctx;
    return hf[c].pseq != (uint16_t)(hf[hf[c].ppos].seq0 + (ps == 2)) ? 2 : 1;
}

static void hf_decide_range(void *ctx, uint32_t lo, uint32_t hi)
{
    struct hf_ctx *hc = ctx;
    struct gpu_scene *gs = hc->gs;
    for (uint32_t k = lo; k < hi; k++) {
        if (chain_resolve((char *)gs->hf, sizeof(*gs->hf), offsetof(struct gs_hf, state), k, hf_step, gs->hf) != 2) continue;
        const uint32_t slot = gs->rec[gs->order[k]].slot;
        __atomic_fetch_or(&gs->hf_mask[slot >> 6], 1ull << (slot & 63), __ATOMIC_RELAXED);
    }
}

static int by_host_fields(struct gpu_scene *gs, clapgpu_scene_arrays *res)
{
    if (gs->n_order > gs->cap_hf) {
        struct gs_hf *q = realloc(gs->hf, (size_t)gs->cap_order * sizeof(*q));
        if (!q) return _CERR_NOMEM;
        gs->hf = q; gs->cap_hf = gs->cap_order;
    }
    const uint32_t words = res->n_slots / 64;
    if (words > gs->cap_hf_mask) {
        uint64_t *q = realloc(gs->hf_mask, (size_t)words * 8);
        if (!q) return _CERR_NOMEM;
        gs->hf_mask = q; gs->cap_hf_mask = words;
    }
    if (words) memset(gs->hf_mask, 0, (size_t)words * 8);       /* (nothing batched: no slots, no mask) */
    struct hf_ctx hc = { gs, res->n_slots };
    const int nt = gs->n_order >= 8192 ? gs_par_threads() : 1;
    gpu_scene_par_for(hf_collect_range, &hc, gs->n_order, nt);
    gpu_scene_par_for(hf_decide_range, &hc, gs->n_order, nt);
    res->rebuilt_mask = gs->hf_mask;
    res->exported_mask = NULL;                                   /* (a walked frame exports everything) */
    return 0;
}

/* What a walk leaves behind for the frames that are not walked, from the records, on the workers: the verdict table in list
 * order, which batched parents a host-class child reads, which entities are standing readers under GPU_SCATTER_DRAWN. */
struct walk_tail_ctx { struct gpu_scene *gs; struct scene *scene; uint32_t n_changes; };
static void tail_verdicts_range(void *ctx, uint32_t lo, uint32_t hi)
{
    struct gpu_scene *gs = ((struct walk_tail_ctx *)ctx)->gs;
    for (uint32_t k = lo; k < hi; k++) {
        struct gs_rec *r = &gs->rec[gs->order[k]];
        gs->vq_e[k] = r->e; gs->vq_slot[k] = r->slot; gs->vq_ok[k] = verdict_ok(r) && r->slot != CLAPGPU_NO_ENTITY;
        r->host_child = 0;
    }
}

static void tail_host_child_range(void *ctx, uint32_t lo, uint32_t hi)
{
    struct gpu_scene *gs = ((struct walk_tail_ctx *)ctx)->gs;
    for (uint32_t k = lo; k < hi; k++) {
        const struct gs_rec *r = &gs->rec[gs->order[k]];
        if ((r->cls != 2 && r->cls != 3) || !r->e->parent) continue;
        const uint32_t pr = rec_find(gs, r->e->parent);
        if (pr != NO_REC) __atomic_store_n(&gs->rec[pr].host_child, 1, __ATOMIC_RELAXED);   /* (several children, one value) */
    }
}

static void tail_keep_range(void *ctx, uint32_t lo, uint32_t hi)
{
    struct walk_tail_ctx *tc = ctx;
    struct gpu_scene *gs = tc->gs;
    for (uint32_t k = lo; k < hi; k++) {
        const struct gs_rec *r = &gs->rec[gs->order[k]];
        if ((r->cls != 1 && r->cls != 4) || r->handle == CLAPGPU_NO_ENTITY) continue;
        const uint8_t keep = r->user_keep || r->host_child || r->keep_auto || (tc->scene && r->e == tc->scene->control);   /* (the records alone: keep_auto was taken while the entity was at hand) */
        if (keep != r->keep) gs->keep_changes[__atomic_fetch_add(&tc->n_changes, 1, __ATOMIC_RELAXED)] = gs->order[k];
    }
}

/* ---- a WALKED frame, in the order gs_walked_frame() runs its parts -------------------------------------------------- */

/* A walked frame writes everything back, and it may re-tile: whatever GPU_SCATTER_DRAWN left on the device comes over
 * first, so that the host fields the walk decides by (xform.updated, seq / parent_seq) are the reference's.  The rows
 * only: an entity3d is written when the walk MEETS it -- what was deleted since the last frame (the reason for many a
 * walk) is freed memory, and nothing but the queue's own lists says which entities those are.  Then the frame's lists and
 * counters start empty. */
static int walk_begin(struct gpu_scene *gs, struct mq *mq)
{
    struct gpu_scene_stats *st = &gs->stats;
    struct scene *scene = mq->priv;
    gs->walk_fetch_on = false;
    if (gs->any_pend) {
        uint32_t n_rows = 0;
        CK(clapgpu_scene_fetch(gs->scene, NULL, &n_rows));
        clapgpu_scene_arrays fr;
        if (n_rows && !clapgpu_scene_results(gs->scene, &fr)) {
            const uint32_t words = fr.n_slots / 64;
            if (words > gs->cap_walk_fetch) {
                uint64_t *q = realloc(gs->walk_fetch, (size_t)words * 8);
                if (!q) return _CERR_NOMEM;
                gs->walk_fetch = q; gs->cap_walk_fetch = words;
            }
            memcpy(gs->walk_fetch, fr.fetched_mask, (size_t)words * 8);
            gs->res = fr;
            gs->fetch_seen = fr.fetch_serial;
            gs->walk_fetch_on = true;
        }
    }
    clapgpu_scene_set_export(gs->scene, CLAPGPU_SCENE_EXPORT_ALL);
    gs->drawn_now = false;
    for (uint32_t k = 0; k < gs->n_touched; k++) gs->rec[gs->touched[k]].pending = 0;
    gs->n_touched = 0;
    gs->n_xptr = 0;                                              /* the walk reads every transform itself */
    gs->n_created = 0;                                           /* ... and meets every entity made since the last one */
    gs->appended = false;
    gs->n_wtxm = 0;
    st->placed = gs->inc_placed; st->removed = gs->inc_removed;  /* (taken in / out in place before something else asked for the walk) */
    st->registered += gs->inc_placed; st->deleted += gs->inc_removed;
    gs->inc_placed = gs->inc_removed = 0;
    gs->topology_pending = false;
    gs->last_fast = false;
    gs->n_host = 0; gs->n_batched = 0; gs->n_deferred = 0; gs->n_att = 0; gs->n_char = 0;
    if (scene && scene->camera)                                  /* the device's containment mask: what the second half goes by when the layout stands */
        clapgpu_scene_set_bv_points(gs->scene, transform_pos(&scene->camera->xform, NULL),
                                    scene->control ? transform_pos(&scene->control->xform, NULL) : NULL, CLAPGPU_NO_ENTITY);
    else
        clapgpu_scene_set_bv_points(gs->scene, NULL, NULL, CLAPGPU_NO_ENTITY);

    return 0;
}

/* steps 2 and 3 for ONE entity the walk has met and given its place in order[]: its class (from its own criteria and its
 * parent's class, which is settled: the parent comes earlier or does not count), then what the class asks of the mirror */
static int walk_act(struct gpu_scene *gs, struct mq *mq, uint32_t i);

/*
 * The class rule (step 2, struct gs_rec.cls): an entity's class from its own criteria and from `pc`, its parent's class when
 * that parent was met EARLIER in this walk -- GS_PC_NONE without a parent, GS_PC_UNMET for a parent the walk has not met (it
 * comes later in the list, or is not in the queue).  The serial walk and the workers' chain resolver both decide by it.
 */
#define GS_PC_NONE  0
#define GS_PC_UNMET 0xff
static inline uint8_t class_of(const struct gpu_scene *gs, bool self_ok, bool rides, bool animated, uint8_t pc)
{
    /* A child that precedes its parent in list order sees the parent's matrix of the previous frame in the reference
     * (model.c:1911-1922 walks creation order): it stays on the host, where that lag is reproduced exactly, and so does
     * everything below it.  Such a child of a joint is read one frame late too, joint transforms included, which running
     * its hook at its place in the list reproduces. */
    if (pc == GS_PC_UNMET) return 2;
    /* With the pose computed after this update (gpu_anim_update), an entity riding a parent's joint (model.c:1626-1641)
     * must wait for it: the reference gives it the joint transforms of THIS frame, written by the parent's animated_update
     * earlier in the list.  It -- and everything below it -- is run by gpu_scene_run_deferred(), which gpu_anim_update calls
     * when the palettes are back. */
    if (!self_ok) return gs->anim_elsewhere && (rides || pc == 3 || pc == 4) ? 3 : 2;
    if (pc == GS_PC_NONE) return 1;
    if (!rides) return pc == 4 && animated ? 3 : pc;  /* 1, 4 (below a joint rider), or the parent's host class; an animated one
                                                         below a rider: its own pose would need its matrix before the second launch */
    /* rides a joint of a character whose palette the device computes this frame: the frame's second entity launch, behind
     * the pose (gpu_scene_run_deferred) */
    if (gs->anim_elsewhere && pc == 1 && !animated) return 4;
    /* the parent's hook runs on the host (its palette is fresh when it returns), or the rider is nested below another rider /
     * animated itself: its own hook, deferred behind the pose when that runs elsewhere */
    return gs->anim_elsewhere ? 3 : 2;
}

static int walk_classify(struct gpu_scene *gs, struct mq *mq, uint32_t i)
{
    struct gs_rec *r = &gs->rec[i];
    entity3d *e = r->e;
    r->self_ok = self_batchable(gs, e);
    r->rides = e->parent && e->parent_joint != JOINT_TYPE_MAX; r->animated = entity_animated(e);
    uint8_t pc = GS_PC_NONE;
    if (!r->self_ok || !e->parent) {
        r->parent_e = e->parent; r->parent_rec = NO_REC;  /* (a detached child: else every later touch reads as "re-parented") */
        if (e->parent) {
            /* a host-class entity's parent matters only behind the pose */
            const uint32_t p = gs->anim_elsewhere ? rec_find(gs, e->parent) : NO_REC;
            pc = p != NO_REC && gs->rec[p].gen == gs->gen ? gs->rec[p].cls : GS_PC_UNMET;
        }
    } else {
        const uint32_t p = parent_rec(gs, r);            /* NO_REC unless already met in THIS walk */
        pc = p != NO_REC ? gs->rec[p].cls : GS_PC_UNMET;
    }
    r->cls = class_of(gs, r->self_ok, r->rides, r->animated, pc);
    return walk_act(gs, mq, i);
}

static int walk_act(struct gpu_scene *gs, struct mq *mq, uint32_t i)
{
    struct gs_rec *r = &gs->rec[i];
    entity3d *e = r->e;
    if (r->cls == 1 || r->cls == 4) {
        r->keep_auto = r->cls == 4 || e->light_idx >= 0 || e->update != gs->default_hook || entity_animated(e);
        if (e->update != gs->default_hook) {             /* a body-less character: its hook's host half, at its place in the list */
            gs->char_half(e, mq->priv);
            if (push_u32(&gs->char_list, &gs->n_char, &gs->cap_char, i)) return _CERR_NOMEM;
            r = &gs->rec[i];
        }
        CK(mirror_one(gs, r));
        CK(link_parent(gs, r));
    } else {
        CK(unbatch(gs, r));
    }
    return 0;
}

/*
 * The same two steps for a big queue, on the workers.  The list chase is serial by nature; what the walk does per entity
 * besides it is not, and at a million entities that was most of its 70 ms (four or five cache lines of every 448-byte
 * entity3d, its record, the mirror's record, three rows of the upload image).  So the chase only matches records and fills
 * order[], and then, over order[]:
 *   A  every entity's own criteria and its parent's place in the list (own record only; the parents' records are read),
 *   B  the classes: an entity's class is a function of its criteria and of its parent's class when that parent comes EARLIER
 *      in the list -- a recurrence up the ancestor chain, walked per entity until it meets a decided ancestor (states are
 *      written once, the same value by whoever gets there first),
 *   C  what the class asks of the mirror, where that is a push of flags and transform (clapgpu_scene_entity_transform_mt:
 *      nothing shared is touched); anything that changes the mirror's make-up -- a new handle, another model, another parent,
 *      a joint attachment, a LOD, an entity that leaves the batch, a character's host half -- is noted and
 *   D  done afterwards on this thread in list order by walk_act(), the serial walk's own code; so is the parent link of the
 *      children of such entities.
 */
#define WQ_NONE 0xffffffffu
struct gs_wq { uint32_t ppos; uint8_t state, todo; };             /* todo: 1 = walk_act on this thread, 2 = its parent link only */
struct wq_ctx { struct gpu_scene *gs; int rc; uint32_t pushed; };

static void wq_inputs_range(void *ctx, uint32_t lo, uint32_t hi)
{
    struct gpu_scene *gs = ((struct wq_ctx *)ctx)->gs;
    for (uint32_t k = lo; k < hi; k++) {
        struct gs_rec *r = &gs->rec[gs->order[k]];
        struct gs_wq *w = &gs->wq[k];
        if (k + 24 < hi) __builtin_prefetch(&gs->rec[gs->order[k + 24]], 0, 1);
        if (k + 8 < hi) prefetch_entity(gs->rec[gs->order[k + 8]].e);
        entity3d *e = r->e, *p = e->parent;
        w->ppos = WQ_NONE; w->todo = 0;
        r->self_ok = self_batchable(gs, e);
        r->rides = p && e->parent_joint != JOINT_TYPE_MAX;
        r->animated = entity_animated(e);
        uint32_t pi = NO_REC;
        if (!r->self_ok) {
            r->parent_e = p; r->parent_rec = NO_REC;
            if (p && gs->anim_elsewhere) pi = rec_find(gs, p);
        } else if (!p) {
            r->parent_e = NULL; r->parent_rec = NO_REC;
        } else {
            if (r->parent_e != p || r->parent_rec == NO_REC || gs->rec[r->parent_rec].e != p) {   /* (parent_rec()) */
                r->parent_e = p;
                r->parent_rec = rec_find(gs, p);
            }
            pi = r->parent_rec;
        }
        if (pi != NO_REC && gs->rec[pi].gen == gs->gen && gs->rec[pi].order_pos < k) w->ppos = gs->rec[pi].order_pos;   /* met EARLIER in this walk */
        /* decided here unless it takes the parent's class (0: the chain resolver) */
        w->state = !p ? class_of(gs, r->self_ok, r->rides, r->animated, GS_PC_NONE)
                 : w->ppos == WQ_NONE ? class_of(gs, r->self_ok, r->rides, r->animated, GS_PC_UNMET) : 0;
    }
}

/* the resolver's step: entry c's class from its parent's, which comes earlier in the list */
static uint8_t wq_step(const void *ctx, uint32_t c, uint8_t pc)
{
    const struct gpu_scene *gs = ctx;
    const struct gs_rec *r = &gs->rec[gs->order[c]];
    return class_of(gs, r->self_ok, r->rides, r->animated, pc);
}

static void wq_class_range(void *ctx, uint32_t lo, uint32_t hi)
{
    const struct gpu_scene *gs = ((struct wq_ctx *)ctx)->gs;
    for (uint32_t k = lo; k < hi; k++)
        chain_resolve((char *)gs->wq, sizeof(*gs->wq), offsetof(struct gs_wq, state), k, wq_step, gs);
}

static void wq_act_range(void *ctx, uint32_t lo, uint32_t hi)
{
    struct wq_ctx *wc = ctx;
    struct gpu_scene *gs = wc->gs;
    uint32_t pushed = 0;
    for (uint32_t k = lo; k < hi; k++) {
        struct gs_rec *r = &gs->rec[gs->order[k]];
        struct gs_wq *w = &gs->wq[k];
        entity3d *e = r->e;
        r->cls = w->state;
        if (r->cls != 1 && r->cls != 4) { w->todo = r->handle != CLAPGPU_NO_ENTITY; continue; }   /* leaves the batch: unbatch() */
        r->keep_auto = r->cls == 4 || e->light_idx >= 0 || e->update != gs->default_hook || r->animated;
        const uint8_t att = r->cls == 4 && e->parent_joint != JOINT_TYPE_MAX;
        const uint32_t ph = e->parent ? gs->rec[r->parent_rec].handle : CLAPGPU_NO_ENTITY;
        if (e->update != gs->default_hook || r->handle == CLAPGPU_NO_ENTITY || r->model != e->txmodel->model ||
            e->force_lod != r->lod_force || e->cur_lod != r->lod_cur || att != r->att || ph != r->parent_handle ||
            (e->parent && ph == CLAPGPU_NO_ENTITY)) {
            w->todo = 1;
            continue;
        }
        /* mirror_one(), the part that changes nothing but this entity's own inputs */
        const uint32_t flags = e->flags & (ENTITY3D_ALIVE | 0xffffu);
        const bool same_flags = flags == r->flags;
        r->flags = flags;
        r->xform_dirty = transform_is_updated(&e->xform);
        if (r->host_done && r->xform_dirty) r->host_done = 2;
        if (!r->xform_dirty && !r->host_done && same_flags) continue;
        const int rc = clapgpu_scene_entity_transform_mt(gs->scene, r->handle, transform_pos(&e->xform, NULL),
                                                         transform_rotation_quat(&e->xform), e->scale, flags, r->xform_dirty || r->host_done);
        if (rc) __atomic_store_n(&wc->rc, rc, __ATOMIC_RELAXED);
        if (r->xform_dirty || r->host_done) pushed++;
    }
    __atomic_fetch_add(&wc->pushed, pushed, __ATOMIC_RELAXED);
}

/* children of entities whose handle is about to change (a new handle, another model): their parent link follows it */
static void wq_links_range(void *ctx, uint32_t lo, uint32_t hi)
{
    struct gpu_scene *gs = ((struct wq_ctx *)ctx)->gs;
    for (uint32_t k = lo; k < hi; k++) {
        const struct gs_rec *r = &gs->rec[gs->order[k]];
        struct gs_wq *w = &gs->wq[k];
        if (__atomic_load_n(&w->todo, __ATOMIC_RELAXED) || (r->cls != 1 && r->cls != 4) || !r->e->parent) continue;
        const struct gs_rec *pr = &gs->rec[r->parent_rec];
        if (pr->order_pos < gs->n_order && __atomic_load_n(&gs->wq[pr->order_pos].todo, __ATOMIC_RELAXED) == 1)
            __atomic_store_n(&w->todo, 2, __ATOMIC_RELAXED);     /* (a neighbour may be reading this one as ITS parent's: 0 or 2, never 1) */
    }
}

static uint32_t walk_par_min(void)
{
    static uint32_t v;
    if (!v) { const char *e = getenv("GPU_SCENE_WALK_PAR_MIN"); v = e && atoi(e) > 0 ? (uint32_t)atoi(e) : 16384u; }   /* tuning knob; the tests set 1 */
    return v;
}

static int walk_queue(struct gpu_scene *gs, struct mq *mq)
{
    struct gpu_scene_stats *st = &gs->stats;
    /*
     * 1-3 in ONE walk of the queue (the entity structs are far larger than the caches, so every
     * extra pass over them costs as much as the reference's whole update).  prev_order[] is last
     * frame's walk: an unchanged queue is matched without hashing, and its entities are prefetched
     * ahead of the list chase.  A big queue's steps 2 and 3 follow on the workers (above).
     */
    { uint32_t *t = gs->prev_order; gs->prev_order = gs->order; gs->order = t; }
    gs->n_prev = gs->n_order;
    gs->n_order = 0;
    const bool later = gs->n_prev >= walk_par_min() && gs_par_threads() > 1;   /* (by last walk's size: a first walk goes one by one) */
    const double t_chase = now_ms();
    /* the entity's list node GS_CHASE_AHEAD steps ahead, through a record asked for GS_CHASE_REC_AHEAD ahead: 15.4-16.9 ->
     * 11.6-12.8 ms at 1 M entities (8 / none before; 16 / 40 and 32 / none: slower) */
    enum { GS_CHASE_AHEAD = 12, GS_CHASE_REC_AHEAD = 32 };
    uint32_t cursor = 0;
    model3dtx *txm;
    entity3d *e, *it;
    list_for_each_entry(txm, &mq->txmodels, entry) {
        if (gs->n_wtxm == gs->cap_wtxm) {
            const uint32_t cap = gs->cap_wtxm ? 2 * gs->cap_wtxm : 32;
            struct gs_wtxm *q = realloc(gs->wtxm, (size_t)cap * sizeof(*q));
            if (!q) return _CERR_NOMEM;
            gs->wtxm = q; gs->cap_wtxm = cap;
        }
        const uint32_t rank = gs->n_wtxm++;
        gs->wtxm[rank] = (struct gs_wtxm){ txm, 0, gs->n_order };
        list_for_each_entry_iter(e, it, &txm->entities, entry) {
            if (!entity3d_matches(e, ENTITY3D_ALIVE)) continue;
            uint32_t i;
            if (cursor < gs->n_prev && gs->rec[gs->prev_order[cursor]].e == e) {
                i = gs->prev_order[cursor++];
                if (cursor + GS_CHASE_REC_AHEAD < gs->n_prev) __builtin_prefetch(&gs->rec[gs->prev_order[cursor + GS_CHASE_REC_AHEAD]], 0, 1);
                if (cursor + GS_CHASE_AHEAD < gs->n_prev) {
                    const entity3d *ahead = gs->rec[gs->prev_order[cursor + GS_CHASE_AHEAD]].e;   /* (NULL: a tombstone of order[]) */
                    if (!later) prefetch_entity(ahead);
                    else if (ahead) __builtin_prefetch(&ahead->entry, 0, 1);   /* the chase reads the list node and the flags */
                }
            } else {
                i = rec_find(gs, e);
                if (i == NO_REC) {
                    i = rec_add(gs, e);
                    if (i == NO_REC) return _CERR_NOMEM;
                } else if (gs->rec[i].gen + 1 == gs->gen) {
                    cursor = gs->rec[i].order_pos + 1;            /* resynchronise after a deletion */
                }
            }
            if (gs->n_order == gs->cap_order) {
                const uint32_t cap = gs->cap_order ? 2 * gs->cap_order : 4096;
                uint32_t *o = realloc(gs->order, (size_t)cap * sizeof(*o));
                if (o) gs->order = o;
                uint32_t *po = realloc(gs->prev_order, (size_t)cap * sizeof(*po));
                if (po) gs->prev_order = po;
                if (!o || !po) return _CERR_NOMEM;
                gs->cap_order = cap;
            }
            struct gs_rec *r = &gs->rec[i];
            if (r->gone) {                                       /* the entity this record knew was deleted: e is a new one at its address */
                CK(unbatch(gs, r));
                *r = (struct gs_rec){ .e = e, .next = r->next, .parent_rec = NO_REC, .handle = CLAPGPU_NO_ENTITY, .slot = CLAPGPU_NO_ENTITY,
                                      .parent_handle = CLAPGPU_NO_ENTITY };
            }
            if (gs->walk_fetch_on && (r->cls == 1 || r->cls == 4) && r->slot < gs->res.n_slots &&
                ((gs->walk_fetch[r->slot >> 6] >> (r->slot & 63)) & 1)) {
                scatter_fetched(gs, r, &gs->res, r->slot);       /* (its class and slot are still last walk's) */
                st->fetched++;
            }
            r->gen = gs->gen;
            r->order_pos = gs->n_order;
            r->order_key = ((uint64_t)rank << 32) | gs->wtxm[rank].next++;
            gs->order[gs->n_order++] = i;
            if (!later) CK(walk_classify(gs, mq, i));
        }
    }
    if (later && gs->n_order) {
        if (gs->n_order > gs->cap_wq) {
            struct gs_wq *q = realloc(gs->wq, (size_t)gs->cap_order * sizeof(*q));
            if (!q) return _CERR_NOMEM;
            gs->wq = q; gs->cap_wq = gs->cap_order;
        }
        struct wq_ctx wc = { gs, 0, 0 };
        const bool timing = getenv("GPU_SCENE_TIMING") != NULL;
        double tw[6] = { 0 };
        if (timing) tw[0] = now_ms();
        gpu_scene_par_for(wq_inputs_range, &wc, gs->n_order, gs_par_threads());
        if (timing) tw[1] = now_ms();
        gpu_scene_par_for(wq_class_range, &wc, gs->n_order, gs_par_threads());
        if (timing) tw[2] = now_ms();
        gpu_scene_par_for(wq_act_range, &wc, gs->n_order, gs_par_threads());
        if (timing) tw[3] = now_ms();
        gpu_scene_par_for(wq_links_range, &wc, gs->n_order, gs_par_threads());
        if (timing) tw[4] = now_ms();
        if (wc.rc) return wc.rc;
        st->uploaded += wc.pushed;
        clapgpu_scene_mark_all_dirty(gs->scene);
        uint32_t n_todo = 0;
        for (uint32_t k = 0; k < gs->n_order; k++) {             /* D: what changes the mirror's make-up, in list order */
            const uint8_t todo = gs->wq[k].todo;
            if (todo == 1) CK(walk_act(gs, mq, gs->order[k]));
            else if (todo == 2) CK(link_parent(gs, &gs->rec[gs->order[k]]));
            n_todo += todo != 0;
        }
        if (timing)
            fprintf(stderr, "walk: chase %.3f ms, criteria %.3f, classes %.3f, pushes %.3f, links %.3f, %u entities one by one %.3f\n",
                    tw[0] - t_chase, tw[1] - tw[0], tw[2] - tw[1], tw[3] - tw[2], tw[4] - tw[3], n_todo, now_ms() - tw[4]);
    }
    if (gs->any_pend) {                                          /* what the walk did not meet is gone, and its counters with it */
        if (gs->pend) memset(gs->pend, 0, (size_t)gs->cap_pend * sizeof(*gs->pend));
        gs->any_pend = false;
        gs->walk_fetch_on = false;
    }
    return 0;
}

/* records of entities that left the queue since the last walk; the lists the second half of the frame goes by */
static int walk_settle(struct gpu_scene *gs)
{
    struct gpu_scene_stats *st = &gs->stats;
    for (uint32_t k = 0; k < gs->n_dead_recs; k++) {             /* taken out in place since the last walk: order[] no longer names them */
        struct gs_rec *r = &gs->rec[gs->dead_recs[k]];
        if (r->e) continue;                                      /* (cannot be: nothing hands a tombstone out before this) */
        r->next = gs->free_rec;
        gs->free_rec = gs->dead_recs[k];
    }
    gs->n_dead_recs = 0;
    /* entities that left the queue (entity3d_delete, model.c:1787): met last frame, not this one */
    if (gs->n_live != gs->n_order) {
        for (uint32_t k = 0; k < gs->n_prev; k++) {
            const uint32_t i = gs->prev_order[k];
            struct gs_rec *r = &gs->rec[i];
            if (!r->e || r->gen == gs->gen) continue;
            if (r->handle != CLAPGPU_NO_ENTITY) {
                CK(clapgpu_scene_entity_delete(gs->scene, r->handle));
                st->deleted++;
            }
            rec_del(gs, i);
        }
    }

    /* the lists the second half of the frame goes by, in list order -- from the records: the classes are settled */
    for (uint32_t k = 0; k < gs->n_order; k++) {
        const struct gs_rec *r = &gs->rec[gs->order[k]];
        if (r->cls == 1) { gs->n_batched++; continue; }
        if (r->cls == 4) { gs->n_batched++; if (push_u32(&gs->att_list, &gs->n_att, &gs->cap_att, gs->order[k])) return _CERR_NOMEM; }
        else if (r->cls == 3) { if (push_u32(&gs->deferred, &gs->n_deferred, &gs->cap_deferred, gs->order[k])) return _CERR_NOMEM; }
        else if (push_u32(&gs->host_list, &gs->n_host, &gs->cap_host, gs->order[k])) return _CERR_NOMEM;
    }
    /* host-class children that precede their BATCHED parent in the list (see lag_parent above) */
    gs->n_lag = 0;
    for (uint32_t k = 0; k < gs->n_host; k++) {
        struct gs_rec *r = &gs->rec[gs->host_list[k]];
        r->lag = 0;
        if (!r->e->parent) continue;
        const uint32_t pr = rec_find(gs, r->e->parent);
        if (pr == NO_REC || gs->rec[pr].gen != gs->gen || gs->rec[pr].cls != 1 || gs->rec[pr].order_pos < r->order_pos) continue;
        if (push_u32(&gs->lag_parent, &gs->n_lag, &gs->cap_lag, pr)) return _CERR_NOMEM;
        r->lag = gs->n_lag;
    }
    if (gs->n_lag) {
        struct lag_keep *lk = realloc(gs->lag_keep, (size_t)gs->cap_lag * sizeof(*lk));
        if (!lk) return _CERR_NOMEM;
        gs->lag_keep = lk;
    }

    return 0;
}

/* 4: the device -- and, under GPU_SCATTER_DRAWN, the per-slot counters laid out for the layout it left */
static int walk_device(struct gpu_scene *gs, struct view *view, clapgpu_scene_arrays *out, bool *shown_stands_out)
{
    struct gpu_scene_stats *st = &gs->stats;
    const uint32_t layout_before = clapgpu_scene_layout_generation(gs->scene);
    clapgpu_frustum fr;
    if (view) frustum_of(view, &fr);
    CK(gs_views_before_update(gs, view));
    CK(clapgpu_scene_mq_update(gs->scene, view ? &fr : NULL));
    st->retiled = layout_before != clapgpu_scene_layout_generation(gs->scene);
    gs->culled_view = view;
    gs->vis_cursor = 0;
    if (view) memcpy(gs->culled_planes, view->main.frustum_planes, sizeof(gs->culled_planes));
    gs->cull_checked = false;
    clapgpu_scene_arrays res = { 0 };
    if (clapgpu_scene_results(gs->scene, &res))                  /* an empty batch has none */
        memset(&res, 0, sizeof(res));
    gs->res = res;

    bool shown_stands = true;                                    /* shown[] of the last frames still describes this layout's slots */
    if (gs->scatter_drawn && gs->notify && res.n_slots) {        /* the counters GPU_SCATTER_DRAWN keeps per slot, for this layout */
        shown_stands = !st->retiled && gs->shown && gs->cap_pend >= res.n_slots && !gs->shown_stale;
        gs->shown_stale = false;
        if (res.n_slots > gs->cap_pend) {
            uint16_t *pn = realloc(gs->pend, (size_t)res.n_slots * sizeof(*pn));
            if (pn) gs->pend = pn;
            uint16_t *sn = realloc(gs->shown, (size_t)res.n_slots * sizeof(*sn));
            if (sn) gs->shown = sn;
            if (!pn || !sn) return _CERR_NOMEM;
            gs->cap_pend = res.n_slots;
        } else if (!gs->shown) {
            gs->shown = malloc((size_t)gs->cap_pend * sizeof(*gs->shown));
            if (!gs->shown) return _CERR_NOMEM;
        }
        memset(gs->pend, 0, (size_t)gs->cap_pend * sizeof(*gs->pend));   /* (every counter was consumed with the walk's fetch) */
        if (!shown_stands) memset(gs->shown, 0, (size_t)gs->cap_pend * sizeof(*gs->shown));
    }
    gs->shown_live = gs->scatter_drawn && gs->notify && res.n_slots && gs->shown;
    *out = res;
    *shown_stands_out = shown_stands;
    return 0;
}

/* what a walk leaves behind for the frames that are not walked: verdict table, address table, slot arrays, standing readers */
static int walk_tail(struct gpu_scene *gs, struct scene *scene)
{
    if (gs->n_order > gs->cap_vq) {
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
    struct walk_tail_ctx tc = { gs, scene, 0 };
    const int tail_threads = gs->n_order >= GS_TABLES_PAR_MIN ? gs_par_threads() : 1;
    gpu_scene_par_for(tail_verdicts_range, &tc, gs->n_order, tail_threads);
    if (gs->notify && gs_ftab_build(gs)) gs->n_xptr = 0;            /* without the table gpu_scene_touch_xform takes the checked path */
    slot_arrays_build(gs);                                       /* on failure the draw list goes through the records */
    /* GPU_SCATTER_DRAWN: the standing host readers (gpu-scene.h).  A host-class entity's hook reads its parent's mx / seq
     * (parent_transform_apply, model.c:1609-1641) -- also when that parent comes later in the list (lag_parent) */
    if (gs->notify)                                              /* (also: such a parent cannot be taken out of the layout in place) */
        gpu_scene_par_for(tail_host_child_range, &tc, gs->n_order, tail_threads);
    if (gs->scatter_drawn && gs->notify) {
        gs->last_control = scene ? scene->control : NULL;
        if (gs->n_order > gs->cap_keep_changes) {
            uint32_t *q = realloc(gs->keep_changes, (size_t)gs->cap_order * sizeof(*q));
            if (!q) return _CERR_NOMEM;
            gs->keep_changes = q; gs->cap_keep_changes = gs->cap_order;
        }
        gpu_scene_par_for(tail_keep_range, &tc, gs->n_order, tail_threads);
        for (uint32_t c = 0; c < tc.n_changes; c++) {            /* the mirror's own bookkeeping: on this thread */
            struct gs_rec *r = &gs->rec[gs->keep_changes[c]];
            const uint8_t keep = !r->keep;
            if (!clapgpu_scene_entity_keep(gs->scene, r->handle, keep)) r->keep = keep;
        }
    }
    return 0;
}

/* A walked frame: its parts in order, and what it leaves behind for the frames that are not walked */
int gs_walked_frame(struct gpu_scene *gs, struct mq *mq, struct view *view)
{
    struct gpu_scene_stats *st = &gs->stats;
    CK(walk_begin(gs, mq));
    const double t0 = now_ms();
    CK(walk_queue(gs, mq));                                      /* 1-3: the one serial pass over the lists */
    const double t1 = now_ms();
    CK(walk_settle(gs));
    const double t2 = now_ms();
    clapgpu_scene_arrays res = { 0 };
    bool shown_stands = true;
    CK(walk_device(gs, view, &res, &shown_stands));
    const double t3 = now_ms();
    if (!st->retiled && gs->walked && shown_stands && res.n_slots) {
        /* 5, the layout stood: the device's masks say what was rebuilt and which boxes hold the camera -- the second half of
         * a notified frame (gs_frame_results), on the workers where there is much to write back */
        const int rc = gs_frame_results(gs, mq, &res, t0, t2, t3);
        if (rc) return rc;
        st->ms_walk = t1 - t0; st->ms_mirror = t2 - t1;
    } else {
        /* 5, after a re-tile (the device rebuilt EVERYTHING; the host fields say what the reference would have), a first walk,
         * or a queue with nothing batched: the same second half, over a mask made from the host fields on the workers */
        clapgpu_scene_arrays hres = res;
        CK(by_host_fields(gs, &hres));
        const int rc = gs_frame_results(gs, mq, &hres, t0, t2, t3);
        if (rc) return rc;
        st->ms_walk = t1 - t0; st->ms_mirror = t2 - t1;
    }
    CK(walk_tail(gs, mq->priv));
    gs->walked = true;
    return 0;
}
