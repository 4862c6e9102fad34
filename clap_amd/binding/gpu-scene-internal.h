/*
 * gpu-scene-internal.h -- what the translation units of the entity binding share: struct gs_rec, struct gpu_scene, the
 * thresholds, the prototypes of the gs_ functions one file defines for another, and the helpers that passes in other files
 * call per entity (static inline here, so that the host passes keep them inlined).  Not part of the engine's interface:
 * that is gpu-scene.h.  Which file holds what: gpu-scene.c's header comment.
 */
#ifndef GPU_SCENE_INTERNAL_H
#define GPU_SCENE_INTERNAL_H

#ifndef _GNU_SOURCE
#define _GNU_SOURCE                 /* qsort_r */
#endif
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <time.h>
#include <pthread.h>
#include <unistd.h>
#include <stdio.h>

#include "gpu-scene.h"
#include "scene.h"

#ifdef CONFIG_GPU_SCENE
/* the engine's view_entity_in_frustum IS the binding then (gpu-exports.inc.c): fall back to the reference's body */
bool ref_view_entity_in_frustum(struct view *view, entity3d *e);
#define view_entity_in_frustum ref_view_entity_in_frustum
/* and so is entity3d_update: the hooks the binding runs itself are the reference's dispatch, not a notification */
void ref_entity3d_update(entity3d *e, void *data);
#define entity3d_update ref_entity3d_update
/* and entity3d_set_lod: the pick the binding makes for a host-class entity is the reference's own, not a notification */
void ref_entity3d_set_lod(entity3d *e, int lod, bool force);
#define entity3d_set_lod ref_entity3d_set_lod
#endif
#include "clapgpu_scene.h"
#include "clapgpu_snapshot.h"

#define NO_REC 0xffffffffu
#define CK(x) do { int rc__ = (x); if (rc__) return rc__; } while (0)

struct gs_rec {
    entity3d    *e;             /* key; NULL = free record */
    model3d     *model;
    entity3d    *parent_e;      /* e->parent when parent_rec was resolved */
    uint32_t    parent_rec;
    uint32_t    next;           /* hash chain / free list */
    uint32_t    handle;         /* libclapgpu_scene handle, CLAPGPU_NO_ENTITY while on the host */
    uint32_t    slot;           /* its row in the result arrays; refreshed when the layout is rebuilt */
    uint32_t    parent_handle;
    uint32_t    flags;
    uint32_t    gen;            /* last frame this entity was met in the queue */
    uint32_t    order_pos;      /* its position in that frame's walk */
    uint8_t     cls;            /* 0 unknown, 1 batched, 2 host, 3 host but deferred behind the frame's pose, 4 batched in the frame's
                                   SECOND entity launch, behind the pose: subtrees riding a batched character's joint */
    uint8_t     att;            /* the mirror has this entity marked as joint-attached */
    uint8_t     self_ok;
    uint8_t     xform_dirty;    /* xform.updated as seen in step 3 (cleared in step 5, like default_update) */
    uint8_t     pending;        /* on the touched list (notification mode) */
    uint8_t     host_done;      /* entity3d_update() / entity3d_reset() ran this entity's update on the host between frames: the device
                                   still has to rebuild it (its children follow its seq), the host fields are already final */
    uint8_t     gone;           /* gpu_scene_entity_deleting() named this entity and it was not taken out in place: whatever the next walk
                                   meets at this address is ANOTHER entity (malloc hands a freed entity3d's memory to the next one) */
    uint8_t     rides, animated; /* e->parent_joint names a joint / entity_animated(e), as the last walk saw them (inputs of its class) */
    uint8_t     keep_auto;      /* a standing host reader the walk can see on the entity itself (light carrier, hook half of its own, animated, joint rider) */
    uint8_t     keep, user_keep, host_child;   /* GPU_SCATTER_DRAWN: written back whenever rebuilt (as the mirror holds it) / asked for by
                                   gpu_scene_keep() / a host-class child reads this entity's mx and seq (last walk) */
    uint32_t    lag;            /* host-class entity listed BEFORE its batched parent: index + 1 into gs->lag_*[], else 0 */
    uint64_t    order_key;      /* its place in the queue: txmodel's rank << 32 | position in that txmodel's list (order_pos is the
                                   place in order[], where entities taken in without a walk stand at the end) */
    int32_t     lod_force, lod_cur; /* e->force_lod / e->cur_lod as the mirror holds them (gpu_scene_select_lod) */
};

struct gs_model { model3d *model; uint32_t handle; unsigned int lod_min, lod_max; };

struct gs_wq;
struct gpu_scene {
    clapgpu_scene   *scene;
    int             (*default_hook)(entity3d *, void *);
    /* records: dense array + chained pointer hash.  A steady queue never hashes: the k-th entity of
     * this walk is checked against the k-th record of the previous walk first. */
    struct gs_rec   *rec;   uint32_t n_rec, cap_rec, free_rec, n_live;
    uint32_t        *bucket; uint32_t n_bucket;
    uint32_t        *order, *prev_order; uint32_t n_order, n_prev, cap_order;
    clapgpu_scene_arrays res;
    struct gs_model *models; uint32_t n_models, cap_models;
    uint32_t        gen, vis_cursor;
    bool            anim_elsewhere;
    /* body-less characters (gpu-character.inc.c): is this entity's hook character_update over default_update, and the
     * host half of that hook, run before the entity is mirrored */
    bool            (*char_plain)(entity3d *, int (*)(entity3d *, void *));
    int             (*char_half)(entity3d *, void *);
    uint32_t        *char_list; uint32_t n_char, cap_char;         /* batched characters in list order (last walk) */
    /* notification mode: the engine's mutators report what they touch (gpu_scene_touch / gpu_scene_topology) and
     * a frame costs O(touched + rebuilt + host-class entities) instead of two walks over every entity3d */
    bool            notify, topology_pending, walked, last_fast, verify;
    /* verdict table by queue position: entity, slot, 'the mask bit is the answer' -- 13 bytes per entity read in order
     * by _models_render's loop instead of a 64-byte record and the 448-byte entity */
    entity3d        **vq_e; uint32_t *vq_slot; uint8_t *vq_ok; uint32_t cap_vq;
    bool            cull_checked, cull_ok;                         /* the culled view's planes were compared since they last changed */
    uint32_t        *touched; uint32_t n_touched, cap_touched;
    /* transform-only notifications (gpu_scene_touch_xform): the entity's address is all a mutator leaves behind -- no
     * look-up, no cache miss beside the entity it has just written; the frame's mirror pass resolves the addresses
     * through a flat table (address -> record, mirror handle) rebuilt by every walk, on all worker threads */
    entity3d        **xptr; uint32_t n_xptr, cap_xptr;
    uint64_t        *claim; uint32_t cap_claim;                    /* one bit per slot: taken by a worker of this frame's address-list pass */
    struct gs_fast { uint64_t key; uint32_t handle, slot; } *ftab; uint32_t ftab_mask, ftab_cap;
    uint32_t        *host_list; uint32_t n_host, cap_host;         /* host-class records in list order (last walk) */
    uint32_t        *deferred; uint32_t n_deferred, cap_deferred;  /* class 3 records in list order (last walk) */
    uint32_t        *att_list; uint32_t n_att, cap_att;            /* class 4 records in list order (last walk) */
    uint32_t        *att_handles; float *att_jt, *att_bind; uint32_t cap_att_roots;   /* scratch of the second launch */
    /* host-class entities whose BATCHED parent comes later in the list (last walk): the reference runs such a child
     * before its parent, i.e. against the parent's mx / seq of the PREVIOUS frame (model.c:1911-1922); a fast frame
     * writes all batched results back first, so it keeps each such parent's old mx / seq aside for the child's hook */
    uint32_t        *lag_parent; uint32_t n_lag, cap_lag;
    struct lag_keep { mat4x4 mx; uint16_t seq; } *lag_keep;
    uint64_t        *posmap; uint32_t cap_posmap;                  /* scratch: bounding-volume candidates by queue position */
    uint32_t        *slots; uint32_t cap_slots;                    /* scratch: rebuilt slots of the frame */
    uint32_t        n_batched;
    struct mq       *bound_mq; struct view *bound_view;
    void            *hook_data;                                    /* mq->priv of the running gpu_mq_update(): what the hooks get as `data` */
    struct view     *culled_view;
    vec4            culled_planes[6];
    /* the frame's other views (gpu_scene_add_view): xview[k] registered; xslot[k] = its plane among the mirror's extra views
     * in the last update (-1: it was the main view, or no view was culled), the planes that were culled, and whether a
     * verdict has compared them since */
    struct view     *xview[GPU_SCENE_EXTRA_VIEWS]; uint32_t n_xview;
    int             xslot[GPU_SCENE_EXTRA_VIEWS];
    vec4            xplanes[GPU_SCENE_EXTRA_VIEWS][6];
    bool            xchecked[GPU_SCENE_EXTRA_VIEWS], xok[GPU_SCENE_EXTRA_VIEWS];
    entity3d        **draw; int32_t *draw_lod; uint32_t n_draw, cap_draw;   /* gpu_scene_select_lod's draw list */
    uint16_t        *draw_txm;                                     /* ... and each entry's txmodel, as an index into txms[] */
    /* by device slot, laid out by every walk: the entity, its txmodel's index and the cur_lod its entity3d holds -- a pass's
     * draw list is built from these three streams without touching an entity3d (or a record) unless its LOD changed */
    entity3d        **slot_ent; uint16_t *slot_txm; int8_t *slot_lod; uint32_t cap_slot_arrays;
    const model3dtx **txms; uint32_t n_txms, cap_txms;
    /* the same list grouped by txmodel, in the order the txmodels first appear on it (gpu_scene_visible_of) */
    entity3d        **draw_g; int32_t *draw_g_lod; uint32_t cap_draw_g;
    struct gs_draw_group { const model3dtx *txm; uint32_t start, n; } *groups; uint32_t n_groups, cap_groups;
    bool            groups_valid;
    /* GPU_SCATTER_DRAWN: rebuilds of a slot the host has not been shown yet (e->seq lags by this much, uint16 like seq) */
    bool            scatter_drawn, drawn_now;                      /* the policy; it is in force for the frame being run (a fast frame) */
    bool            shown_stale;                                   /* the policy was switched on: the next walk lays shown[] out anew */
    bool            shown_live;                                    /* shown[] describes the CURRENT slots: laid out by the last walk (a walk under
                                                                      GPU_SCATTER_ALL re-tiles without it) and kept by every write-back since */
    uint16_t        *pend; uint32_t cap_pend; bool any_pend;
    /* ... and the seq each batched entity's entity3d was last GIVEN by a frame (walk, write-back or fetch; a host update in
     * between -- entity3d_update / _reset -- does not count: the device catches up with one rebuild in the next frame and
     * the children follow only then).  shown[p] + pend[p] is what a child of p copied into parent_seq when it was last
     * rebuilt on the device (model.c:1613), whatever has happened to e->parent or to p's entity3d on the host since */
    uint16_t        *shown;
    entity3d        *last_control;
    uint32_t        fetch_seen;                                    /* clapgpu_scene_arrays.fetch_serial already copied out */
    uint64_t        *walk_fetch; uint32_t cap_walk_fetch; bool walk_fetch_on;   /* rows fetched for a walk, applied as the walk meets each entity */
    /* creation / deletion without a walk (gpu_scene_entity_created / _deleting) */
    entity3d        **created; uint32_t n_created, cap_created;    /* reported since the last update, in creation order */
    uint32_t        *dead_recs; uint32_t n_dead_recs, cap_dead_recs;   /* records of entities taken out in place: tombstones in order[] until the next walk */
    struct gs_wtxm { const model3dtx *txm; uint32_t next, first; } *wtxm; uint32_t n_wtxm, cap_wtxm;   /* the queue's txmodels in list order (last walk); the next list position in each */
    bool            in_frame;                                      /* gpu_mq_update() is running (its hooks may call back into the notifications) */
    bool            replay, replaying;                             /* frames without notifications may go by the records (gs_queue_unchanged); this frame does */
    bool            incremental, roomy;                            /* allowed; the mirror's re-tiles leave room (from the first entity that came or went between frames) */
    bool            appended;                                      /* order[] is no longer in list order: entities were taken in since the last walk */
    uint32_t        ftab_count;
    struct gs_cand { uint64_t key; uint32_t rec; } *cands; uint32_t cap_cands;
    uint32_t        inc_placed, inc_removed;
    /* a walked frame that re-tiled: what the REFERENCE would have rebuilt, decided from the host fields on the workers (by_host_fields) */
    struct gs_hf { uint32_t ppos; uint16_t seq0, pseq; uint8_t dirty, state; } *hf; uint32_t cap_hf;
    uint64_t        *hf_mask; uint32_t cap_hf_mask;
    uint32_t        *keep_changes; uint32_t cap_keep_changes;      /* scratch of a walk's last pass */
    struct gs_wq    *wq; uint32_t cap_wq;                          /* a big queue's walk: per queue position, its steps 2 and 3 on the workers */
    struct gpu_scene_stats stats;
};

/*
 * Frames that touch or rebuild hundreds of thousands of entities: the two passes over the 448-byte entity3d structs
 * are memory latency on one core, so they are split over a few worker threads (the engine's frame is single-threaded;
 * the binding may use workers as long as every call is synchronous, SURVEY 8b "Threading").
 */
#define GS_PAR_MIN 65536u
/* A frame without notifications goes by the records only where that is done on the workers: on one thread the two passes it
 * takes (queue check, mirror pass, both through records in list order over entities that lie in creation order) LOSE to
 * the plain list walk -- 20 k entities 0.95 vs 0.78 ms, 64 k 6.1 vs 3.9 --, split over the workers they win from ~16 k
 * entities on (two wake-ups of the pool, ~0.1 ms, against a walk of 0.35 ms and up). */
#define GS_REPLAY_MIN 16384u
/* rebuilt rows from which the write-back is split over the workers (a row is ~60 ns on one thread -- a 448-byte entity3d
 * and its 164 bytes of results, both cold --, a wake-up of the pool ~0.05 ms): 70 k entities, 13 k rebuilt: 0.87 ms serial */
#define GS_SCATTER_PAR_MIN 12288u
#define GS_SCATTER_SPARSE 8              /* ... off the mask words when GS_SCATTER_SPARSE * rebuilt <= entities in the queue, else in list order */
/* touched entities (reported one by one, or by address) from which the mirror pass is split over the workers */
#define GS_MIRROR_PAR_MIN 16384u

struct par_job {
    struct gpu_scene *gs;
    const clapgpu_scene_arrays *res;
    const uint64_t *scat;       /* which slots' rows came back this frame */
    uint32_t lo, hi;            /* range of touched[] or order[] */
    int phase;
    uint32_t count;             /* out: uploaded / written back */
    int need_walk, rc;
    uint32_t *deferred; uint32_t n_deferred, cap_deferred;       /* children whose parent lies in an earlier chunk */
    uint32_t *whole; uint32_t n_whole, cap_whole;                /* entities updated on the host since the last frame (host_done): left out */
    void (*range_fn)(void *, uint32_t, uint32_t); void *ctx;     /* gpu_scene_par_for */
    uint32_t *cursor; uint32_t total, grain;                     /* ... its ranges handed out piece by piece (see there) */
};

#define GS_MAX_THREADS 32
#define GS_PAR_PIECES 8u                 /* pieces a thread of gpu_scene_par_for takes its ranges in (see there) */

/* defined in one file of the binding, called from another (gs_: the engine links these objects beside its own) */
int gs_rehash(struct gpu_scene *gs, uint32_t n_bucket);                                     /* gpu-scene.c */
int gs_model_handle(struct gpu_scene *gs, model3d *m, uint32_t *out);
int gs_take_created(struct gpu_scene *gs, struct mq *mq);
int gs_ftab_build(struct gpu_scene *gs);                                                     /* gpu-scene-walk.c */
bool gs_queue_unchanged(struct gpu_scene *gs, struct mq *mq);
int gs_walked_frame(struct gpu_scene *gs, struct mq *mq, struct view *view);
void gs_consume_fetched(struct gpu_scene *gs);                                               /* gpu-scene-results.c */
void gs_fetch_met_in_queue(struct gpu_scene *gs, struct mq *mq);
int gs_fast_frame(struct gpu_scene *gs, struct mq *mq, struct view *view);
int gs_frame_results(struct gpu_scene *gs, struct mq *mq, const clapgpu_scene_arrays *resp, double t0, double t1, double t2);
int gs_views_before_update(struct gpu_scene *gs, struct view *view);                        /* gpu-scene-draw.c */
int gs_par_threads(void);                                                                    /* gpu-scene-pool.c */
void gs_par_run(void *(*fn)(void *), struct par_job *jobs, int nt);

static inline uint32_t ptr_hash(const void *p)
{
    uint64_t x = (uint64_t)(uintptr_t)p;
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33;
    return (uint32_t)x;
}

static inline uint32_t rec_find(const struct gpu_scene *gs, const entity3d *e)
{
    if (!gs->n_bucket) return NO_REC;
    for (uint32_t i = gs->bucket[ptr_hash(e) & (gs->n_bucket - 1)]; i != NO_REC; i = gs->rec[i].next)
        if (gs->rec[i].e == e) return i;
    return NO_REC;
}

static inline uint32_t rec_add(struct gpu_scene *gs, entity3d *e)
{
    uint32_t i;
    if (gs->free_rec != NO_REC) {
        i = gs->free_rec;
        gs->free_rec = gs->rec[i].next;
    } else {
        if (gs->n_rec == gs->cap_rec) {
            const uint32_t cap = gs->cap_rec ? 2 * gs->cap_rec : 4096;
            struct gs_rec *nr = realloc(gs->rec, (size_t)cap * sizeof(*nr));
            if (!nr) return NO_REC;
            gs->rec = nr; gs->cap_rec = cap;
        }
        i = gs->n_rec++;
    }
    if (gs->n_live + 1 > gs->n_bucket) {
        gs->rec[i].e = NULL;                                  /* not yet hashable */
        if (gs_rehash(gs, gs->n_bucket ? 2 * gs->n_bucket : 8192)) return NO_REC;
    }
    gs->rec[i] = (struct gs_rec){ .e = e, .parent_rec = NO_REC, .handle = CLAPGPU_NO_ENTITY, .slot = CLAPGPU_NO_ENTITY,
                                  .parent_handle = CLAPGPU_NO_ENTITY };
    uint32_t *b = &gs->bucket[ptr_hash(e) & (gs->n_bucket - 1)];
    gs->rec[i].next = *b;
    *b = i;
    gs->n_live++;
    return i;
}

static inline void rec_del(struct gpu_scene *gs, uint32_t i)
{
    uint32_t *link = &gs->bucket[ptr_hash(gs->rec[i].e) & (gs->n_bucket - 1)];
    while (*link != i) link = &gs->rec[*link].next;
    *link = gs->rec[i].next;
    gs->rec[i].e = NULL;
    gs->rec[i].next = gs->free_rec;
    gs->free_rec = i;
    gs->n_live--;
}

static inline void prefetch_entity(const entity3d *e)
{
    /* sizeof(entity3d) is seven cache lines and both passes touch most of them; the record array
     * tells us which entity comes eight steps later without chasing the list */
    const char *p = (const char *)e;
    if (!p) return;                                              /* a tombstone of order[] (gpu_scene_entity_deleting) */
    for (unsigned o = 0; o < sizeof(entity3d); o += 64)
        __builtin_prefetch(p + o, 1, 1);
}

static inline double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

static inline int frustum_of(const struct view *view, clapgpu_frustum *fr)
{
    memcpy(fr->planes, view->main.frustum_planes, sizeof(fr->planes));      /* view.h:16 */
    memcpy(fr->corners, view->main.frustum_corners, sizeof(fr->corners));   /* view.h:17 */
    return 0;
}

/* Criteria an entity meets on its own (step 2); the parent's class is folded in during the walk. */
static inline bool self_batchable(const struct gpu_scene *gs, entity3d *e)
{
    /* light carriers are batched: scatter_one() hands the position on.  An entity riding a joint (e->parent_joint) is
     * batchable too -- in the frame's second launch, if its parent's palette is computed on the device this frame: the walk
     * decides (class 4), since that depends on the parent */
    const bool plain_char = gs->char_plain && gs->hook_data && (e->flags & ENTITY3D_IS_CHARACTER) && gs->char_plain(e, gs->default_hook);
    return (e->update == gs->default_hook || plain_char) &&
           (gs->anim_elsewhere || !entity_animated(e)) &&
           !(e->flags & (ENTITY3D_HAS_PHYSICS | (plain_char ? 0 : ENTITY3D_IS_CHARACTER) | ENTITY3D_IS_UI | ENTITY3D_IS_PARTICLE));
}

/* The record of r's parent, or NO_REC if the parent is not an ALIVE member of this queue. */
static inline uint32_t parent_rec(struct gpu_scene *gs, struct gs_rec *r)
{
    entity3d *p = r->e->parent;
    if (r->parent_e != p || r->parent_rec == NO_REC || gs->rec[r->parent_rec].e != p) {   /* a miss is retried: the parent may be met later in the walk */
        r->parent_e = p;
        r->parent_rec = rec_find(gs, p);
    }
    return (r->parent_rec != NO_REC && gs->rec[r->parent_rec].gen == gs->gen) ? r->parent_rec : NO_REC;
}

static inline uint8_t verdict_ok(const struct gs_rec *r)
{
    return (r->cls == 1 || r->cls == 4) &&
           (r->flags & (ENTITY3D_ALIVE | ENTITY3D_VISIBLE | ENTITY3D_SKIP_CULLING)) == (ENTITY3D_ALIVE | ENTITY3D_VISIBLE);
}

static inline int push_u32(uint32_t **arr, uint32_t *n, uint32_t *cap, uint32_t v)
{
    if (*n == *cap) {
        const uint32_t c = *cap ? 2 * *cap : 1024;
        uint32_t *p = realloc(*arr, (size_t)c * sizeof(*p));
        if (!p) return _CERR_NOMEM;
        *arr = p; *cap = c;
    }
    (*arr)[(*n)++] = v;
    return 0;
}

/* a scene has tens of txmodels: the last hit first, then a scan */
static inline uint32_t txm_index(struct gpu_scene *gs, const model3dtx *txm)
{
    static uint32_t last;
    if (last < gs->n_txms && gs->txms[last] == txm) return last;
    for (uint32_t g = 0; g < gs->n_txms; g++)
        if (gs->txms[g] == txm) return last = g;
    if (gs->n_txms == gs->cap_txms) {
        const uint32_t cap = gs->cap_txms ? 2 * gs->cap_txms : 32;
        const model3dtx **q = realloc(gs->txms, (size_t)cap * sizeof(*q));
        if (!q || cap > 65535) return 0xffffffffu;
        gs->txms = q; gs->cap_txms = cap;
    }
    gs->txms[gs->n_txms] = txm;
    return last = gs->n_txms++;
}

static inline uint32_t ftab_home(const struct gpu_scene *gs, const void *e) { return ptr_hash(e) & gs->ftab_mask; }

/* GPU_SCATTER_DRAWN: rebuilds of `slot` the entity3d has not been shown (0 under GPU_SCATTER_ALL) */
static inline uint16_t pend_of(const struct gpu_scene *gs, uint32_t slot)
{
    return (gs->any_pend && slot < gs->cap_pend) ? gs->pend[slot] : 0;
}

/* what r's parent's seq counter read when the DEVICE last rebuilt r's entity (model.c:1613 copies it into parent_seq): by
 * the parent's record as the last walk linked it -- not by e->parent, which the game may have cleared or the engine freed
 * since -- and without the steps a host update took since the last frame.  GPU_SCATTER_ALL: the parent's own counter. */
static inline uint16_t parent_seq_now(const struct gpu_scene *gs, const struct gs_rec *r, const entity3d *parent)
{
    /* (only while shown[] is kept: a walk under GPU_SCATTER_ALL does not lay it out, and a re-tile moves the slots under it --
     * `clap_dropin fuzz 77`: drawn, back to all, a re-tile, then a child rebuilt in a frame that is not walked.  The policy
     * alone does not say: rows left stale before a switch to GPU_SCATTER_ALL are still owed their counters -- fuzz 5016) */
    if (gs->shown_live && gs->shown && r->parent_rec != NO_REC) {
        const struct gs_rec *pr = &gs->rec[r->parent_rec];
        if ((pr->cls == 1 || pr->cls == 4) && pr->slot < gs->cap_pend)
            return (uint16_t)(gs->shown[pr->slot] + gs->pend[pr->slot]);
    }
    return parent ? parent->seq : 0;
}

static inline void seq_shown(struct gpu_scene *gs, size_t slot, uint16_t seq)
{
    if (gs->shown && slot < gs->cap_pend) gs->shown[slot] = seq;
}

static inline void copy_rows(struct gs_rec *r, const clapgpu_scene_arrays *res, size_t slot)
{
    entity3d *e = r->e;
    memcpy(e->mx, res->mx + 16 * slot, sizeof(mat4x4));
    memcpy(e->inverse_mx, res->inverse_mx + 16 * slot, sizeof(mat4x4));
    if (!r->model->skip_aabb) {                                  /* entity3d_aabb_update, model.c:1204-1205 */
        memcpy(e->aabb, res->aabb + 6 * slot, sizeof(e->aabb));
        memcpy(e->aabb_center, res->aabb_center + 3 * slot, sizeof(vec3));
    }
}

/* GPU_SCATTER_DRAWN: an entity the device rebuilt in earlier frames without telling the host, fetched now (it came into
 * view, or somebody asked): the rows, and the counters as the reference would have left them -- seq advanced once per
 * rebuild, parent_seq equal to the parent's (model.c:1613-1616: a child is rebuilt whenever its parent was). */
static inline void scatter_fetched(struct gpu_scene *gs, struct gs_rec *r, const clapgpu_scene_arrays *res, size_t slot)
{
    entity3d *e = r->e, *parent = e->parent;
    const uint16_t k = pend_of(gs, (uint32_t)slot);
    if (k) {
        e->seq = (uint16_t)(e->seq + k);
        gs->pend[slot] = 0;
        if (r->parent_e) e->parent_seq = parent_seq_now(gs, r, parent);   /* the parent it had when those rebuilds ran */
    }
    seq_shown(gs, slot, e->seq);
    copy_rows(r, res, slot);
}

/* Step 3 for one batched entity: creation, flags, transform.  The parent link follows in link_parent(). */
static inline int mirror_one(struct gpu_scene *gs, struct gs_rec *r)
{
    struct gpu_scene_stats *st = &gs->stats;
    entity3d *e = r->e;
    model3d *model = e->txmodel->model;

    if (r->handle != CLAPGPU_NO_ENTITY && r->model != model) {   /* same address, another entity */
        CK(clapgpu_scene_entity_delete(gs->scene, r->handle));
        r->handle = r->parent_handle = CLAPGPU_NO_ENTITY;
        st->deleted++;
    }
    const bool fresh = r->handle == CLAPGPU_NO_ENTITY;
    if (fresh) {
        uint32_t mh;
        CK(gs_model_handle(gs, model, &mh));
        CK(clapgpu_scene_entity_new(gs->scene, mh, (void *)(uintptr_t)((uint32_t)(r - gs->rec) + 1u), &r->handle));
        r->model = model;
        r->flags = ENTITY3D_ALIVE | ENTITY3D_VISIBLE;            /* what entity_new starts with */
        r->lod_force = -1; r->lod_cur = 0;                        /* likewise (entity3d_make, model.c:1741) */
        r->keep = 0;
        st->registered++;
    }
    if (e->force_lod != r->lod_force || e->cur_lod != r->lod_cur) {   /* entity3d_set_lod since (model.c:593-609) */
        CK(clapgpu_scene_entity_lod(gs->scene, r->handle, e->force_lod, e->cur_lod));
        r->lod_force = e->force_lod; r->lod_cur = e->cur_lod;
    }
    const uint32_t flags = e->flags & (ENTITY3D_ALIVE | 0xffffu);
    if (flags != r->flags) {
        CK(clapgpu_scene_entity_flags(gs->scene, r->handle, flags & ~r->flags, r->flags & ~flags));
        r->flags = flags;
    }
    r->xform_dirty = transform_is_updated(&e->xform);
    if (r->host_done && r->xform_dirty) r->host_done = 2;        /* written again since the host updated it */
    if (gs->drawn_now && r->xform_dirty) transform_clear_updated(&e->xform);   /* its write-back may not come: default_update's clear (model.c:1615, 1668) here */
    if (r->xform_dirty || fresh || r->host_done) {       /* host_done: the flag is already cleared, the device copy is not yet current */
        CK(clapgpu_scene_entity_transform(gs->scene, r->handle, transform_pos(&e->xform, NULL),
                                          transform_rotation_quat(&e->xform), e->scale));
        st->uploaded++;
    }
    const uint8_t att = r->cls == 4 && e->parent_joint != JOINT_TYPE_MAX;
    if (fresh) r->att = 0;
    if (att != r->att) {
        CK(clapgpu_scene_entity_set_attach(gs->scene, r->handle, att));
        r->att = att;
    }
    return 0;
}

#endif
