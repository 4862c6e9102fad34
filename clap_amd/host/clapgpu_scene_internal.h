/*
 * clapgpu_scene_internal.h -- what the files of the host mirror share (clapgpu_scene.c: lifecycle, handles, entity verbs,
 * results; clapgpu_scene_layout.c: slabs, re-tile, in-place edits; clapgpu_scene_frame.c: the frame's launches;
 * clapgpu_scene_lod.c: LOD pick and draw list).  Nothing here is part of the library's interface.
 *
 * Reference structures mirrored: struct mq / model3dtx / entity3d lists (model.h:334,222,377),
 * transform_t (transform.h:8-12), entity3d.parent / seq / parent_seq (model.h:402-405),
 * entity3d_flags (model.h:293-312).
 */
#ifndef CLAPGPU_SCENE_INTERNAL_H
#define CLAPGPU_SCENE_INTERNAL_H
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <stdio.h>
#include <time.h>
#include "clapgpu_scene.h"

#define WAVE 64u
#define MIRROR_LOCAL __attribute__((visibility("hidden")))     /* shared by the mirror's files, not exported */
#define CK(x) do { int rc__ = (x); if (rc__) return rc__; } while (0)

struct ent {
    float    pos_scale[4];
    float    rot[4];
    uint32_t flags;          /* entity3d_flags bits, no DIRTY */
    uint32_t parent;         /* handle or CLAPGPU_NO_ENTITY */
    uint32_t model;
    uint32_t slot;
    void    *user;
    uint8_t  live, dirty, attached;   /* attached: rides a joint of its parent (e->parent_joint, model.c:1626-1641) */
    uint8_t  keep;                    /* clapgpu_scene_entity_keep: a standing host reader, exported whenever rebuilt */
    uint32_t n_children;              /* live entities whose parent this is (an entity with children cannot be deleted in place) */
    int32_t  force_lod, cur_lod;      /* entity3d.force_lod / .cur_lod (model.h:415-416; entity3d_set_lod, model.c:593-609) */
};

/* ---- the two slabs, stated once ------------------------------------------------------------------------------------------
 * The arrays that cross PCIe every frame are carved out of two page-locked slabs that mirror two device slabs, each array
 * `cap` slots long (cap a multiple of 64: every array starts 16-B aligned):
 *   in:  pos_scale | rot | flags | touched                                  (one copy up)
 *   out: mx | inv_mx | aabb | center | vis | rebuilt | inside | exported    (one copy down)
 * The enum gives each array's byte offset per slot of capacity; a slot mask is mask_stride(cap) words long. */
enum { IN_ROT = 16, IN_FLAGS = 32, IN_TOUCHED = 36, OUT_INV = 64, OUT_AABB = 128, OUT_CENTER = 152, OUT_MASKS = 164 };
struct in_slab  { float *pos_scale, *rot; uint32_t *flags; uint64_t *touched; };
struct out_slab { float *mx, *inv, *aabb, *center; uint64_t *vis, *rebuilt, *inside, *exported; };

static inline size_t mask_stride(size_t cap) { return cap / 64 + 2; }
static inline size_t in_slab_bytes(size_t cap) { return cap * IN_TOUCHED + mask_stride(cap) * 8; }
static inline size_t out_slab_bytes(size_t cap) { return cap * OUT_MASKS + 4 * mask_stride(cap) * 8; }
/* vis | rebuilt | inside as one copy, up to the last word a layout of n slots uses */
static inline size_t masks_span_bytes(size_t cap, size_t n) { return (2 * mask_stride(cap) + n / 64) * 8; }

static inline struct in_slab in_slab_at(void *base, size_t cap)
{
    char *b = base;
    return (struct in_slab){ (float *)b, (float *)(b + cap * IN_ROT), (uint32_t *)(b + cap * IN_FLAGS), (uint64_t *)(b + cap * IN_TOUCHED) };
}

static inline struct out_slab out_slab_at(void *base, size_t cap)
{
    char *b = base;
    uint64_t *m = (uint64_t *)(b + cap * OUT_MASKS);
    const size_t ms = mask_stride(cap);
    return (struct out_slab){ (float *)b, (float *)(b + cap * OUT_INV), (float *)(b + cap * OUT_AABB), (float *)(b + cap * OUT_CENTER),
                              m, m + ms, m + 2 * ms, m + 3 * ms };
}

struct clapgpu_scene {
    struct ent *e;  uint32_t n_handles, cap_handles;
    uint32_t   *free_list;  uint32_t n_free, cap_free;
    uint32_t   *dead_list;  uint32_t n_dead, cap_dead;           /* deleted since the last re-tile: handles not reusable yet */
    uint32_t   *dirty_list; uint32_t n_dirty, cap_dirty;
    float      *models;     uint32_t n_models, cap_models;       /* [m][8] model_table rows */
    int         topology_dirty, models_dirty, tiled, bulk_dirty;
    int         timing;                                          /* CLAPGPU_SCENE_TIMING was set at create: the re-tile's and the small frame's times to stderr */

    /* layout */
    uint32_t    n_slots, n_rows, n_tiles, n_levels;
    uint32_t   *slot_handle;                                     /* slot -> handle or NO_ENTITY */
    uint32_t   *tile_row_start_host, *level_start_host;

    /* host staging (slot order) */
    float      *h_pos_scale, *h_rot, *h_mx, *h_inv, *h_aabb, *h_center;
    int32_t    *h_parent, *h_model;
    uint32_t   *h_flags;
    uint64_t   *h_mask, *h_rebuilt, *h_inside;
    void      **slot_user;                                       /* slot -> the entity's user pointer (NULL: padding) */
    uint32_t    cap_slots;
    uint32_t    up_lo, up_hi, n_staged;                           /* slots whose upload image was written since the last frame */
    /* camera bounding-volume points (default_update's pick, model.c:1703-1713) */
    int         bv_on, bv_has_ctl; float bv_cam[3], bv_ctl[3]; uint32_t bv_ctl_handle;
    clapgpu_bv_query bvq; uint64_t *d_bv_result;

    /* the two slabs (in_slab_at / out_slab_at), host and device */
    void       *h_in, *h_out, *d_in, *d_out;
    size_t      in_bytes, out_bytes;
    /* small scenes (zero_copy): no copy calls and no blocking wait in a frame, and with the tile layout ONE launch:
     * the upload image and the result slab are device-mapped, the frame's touched slots are flagged in h_touched, and
     * clapgpu_entities_update_tiles_hostio reads the flagged inputs from the image, writes what it rebuilds (and the
     * masks) into h_out as well and raises *h_done, which mq_update polls.  With the level layout (a tree wider than a
     * wavefront) the touched records travel as a mapped list scattered by clapgpu_entities_apply_inputs and the results
     * come back through clapgpu_entities_export_rebuilt.  At a testbed-sized scene (10 k entities) the three copies'
     * fixed latencies and the blocking wait were 0.13 of a 0.15 ms device step around a 15-30 us kernel. */
    int         zero_copy;
    uint32_t    zero_copy_max_slots;
    clapgpu_entity_input *h_list; void *d_list; uint32_t cap_list;    /* mapped: host pointer / device alias */
    void       *d_out_host;                                            /* device alias of h_out */
    void       *d_in_host;                                             /* device alias of h_in (zero_copy: the image is mapped) */
    uint64_t   *h_touched;                                             /* behind the image: one bit per slot written since the last frame */
    uint32_t   *h_done, *d_done, *d_counter, frame_id;
    /* joint attachments (clapgpu_scene_attached_update): table + the two matrix pools + the kernel's work space */
    void       *h_att, *d_att; size_t att_bytes; uint32_t cap_att; int att_mapped;
    float      *d_att_local;
    clapgpu_frustum last_frustum; int have_frustum;
    /* export policy (clapgpu_scene_set_export): with EXPORT_DRAWN a one-launch frame writes back only the rebuilt rows
     * somebody reads (drawn, containing a bounding-volume point, kept); the others go stale in h_out -- the device arrays
     * hold them -- and are fetched when they come into view or when asked for (clapgpu_scene_fetch) */
    int         export_drawn;
    uint64_t   *h_keep, *d_keep; int keep_dirty;                       /* slot order; the device copy follows before a launch */
    uint64_t   *h_exported;                                            /* mapped, behind the three masks of h_out */
    uint64_t   *h_stale, *h_fetched; uint32_t n_stale_words, n_fetched, fetch_serial; /* plain host memory, mask_stride(cap_slots) words */
    uint64_t   *h_select; void *d_select;                              /* mapped: the rows a fetch asks for */
    int         fetch_accumulate;                                      /* fetch_rows adds to the rows this mq_update's launch already brought over */
    uint64_t   *d_stale;                                               /* device twin of h_stale, kept by the launches themselves (clapgpu_entities_hostio.stale_mask) */
    /* the layout edited in place (clapgpu_scene_entity_new_placed / _delete_placed): a queue whose make-up changes by a few
     * entities a frame keeps its tiles; a re-tile is the fall-back */
    uint32_t    max_depth;                                             /* rows of the deepest tree at the last re-tile */
    uint32_t    grow_tile;                                             /* the tile new roots go into (NO_ENTITY: none yet) */
    uint32_t    cap_tiles;                                             /* entries tile_row_start_host can hold, minus one */
    int         incremental;                                           /* clapgpu_scene_set_incremental: re-tiles leave room for edits */
    uint32_t   *free_roots; uint32_t n_free_roots, cap_free_roots;     /* first-row slots freed by deletions */
    uint32_t   *raw_words; uint32_t n_raw, cap_raw, raw_lo, raw_hi;    /* words of h_touched set outside the dirty list (tombstones); their slot range */
    uint32_t   *edits; uint32_t n_edits, cap_edits, edit_lo, edit_hi;  /* slots whose parent / model the device has not been given yet */
    clapgpu_entity_place *h_place; void *d_place; uint32_t cap_place;  /* ... as the mapped list clapgpu_entities_place takes */
    uint32_t    grown_from, tiles_from;                                /* first slot / tile appended since the device last saw the layout (NO_ENTITY: none) */
    uint32_t   *limbo; uint32_t n_limbo, cap_limbo;                    /* handles deleted in place: reusable once the frame's dirty list is spent */

    /* device */
    clapgpu_entities d;
    uint32_t   *d_tile_row_start;
    float      *d_models; uint32_t d_models_cap;
    int         have_results;
    uint32_t    layout_gen;

    /* the render passes' LOD pick and draw list (clapgpu_scene_select_lod): force_lod / cur_lod in slot order on both
     * sides (the host copy follows every pick, so a range of it can be pushed at any time), the ordered visible list
     * and the LOD each entry is drawn with */
    int32_t    *h_force_lod, *h_cur_lod;  int32_t *d_force_lod, *d_cur_lod;
    uint32_t   *d_visible, *d_visible_count; int32_t *d_draw_lod; void *d_vis_scratch;
    uint32_t   *h_draw_slot; int32_t *h_draw_lod; uint32_t *h_visible_count;     /* page-locked */
    uint32_t    lod_cap, lod_lo, lod_hi, n_draw;                                  /* [lod_lo, lod_hi): host values not on the device yet */
    uint32_t    lod_layout_gen;
    int         lod_sync_by_caller;                                               /* clapgpu_scene_set_lod_sync */
    /* a small scene's draw list lands in device-mapped host memory: the two launches write it (and its length) where the host
     * reads it, one wait -- no length copy, wait, list copies, wait (two round trips of ~35 us around two ~8 us launches) */
    int         lod_mapped; void *a_draw_slot, *a_draw_lod, *a_visible_count;

    /* the frame's other views (clapgpu_scene_set_views): frusta + device planes in xv (what clapgpu_entities.views points at),
     * the host copies of the masks (device-mapped when the scene is zero-copy: the one-launch frame writes them itself) and
     * the union of every view's mask for the export policy's fetches */
    clapgpu_views xv; uint32_t xv_want, xv_cap_slots; int xv_mapped;
    uint64_t   *h_xv_mask[CLAPGPU_EXTRA_VIEWS_MAX]; void *a_xv_mask[CLAPGPU_EXTRA_VIEWS_MAX];
    uint64_t   *h_xv_union;

    /* a caller's thread pool for the re-tile's passes over every handle / slot (clapgpu_scene_set_parallel_for) */
    clapgpu_scene_parallel_for par_for; int par_threads;
};

/* clapgpu_scene.c */
MIRROR_LOCAL int  mirror_grow_list(uint32_t **arr, uint32_t *cap, uint32_t need, uint32_t first);
MIRROR_LOCAL int  mirror_release_handles(clapgpu_scene *s, const uint32_t *list, uint32_t *n);
MIRROR_LOCAL int  mirror_new_handle(clapgpu_scene *s, uint32_t model, void *user, uint32_t *handle);
MIRROR_LOCAL void mirror_free_device(clapgpu_scene *s);
/* clapgpu_scene_layout.c */
MIRROR_LOCAL int  mirror_retile(clapgpu_scene *s);
MIRROR_LOCAL int  mirror_apply_edits(clapgpu_scene *s);
/* clapgpu_scene_frame.c */
MIRROR_LOCAL int  mirror_fetch_rows(clapgpu_scene *s, const uint64_t *w0, const uint64_t *w1, const uint64_t *w2);
MIRROR_LOCAL void mirror_free_views(clapgpu_scene *s);
/* clapgpu_scene_lod.c */
MIRROR_LOCAL void mirror_free_lod(clapgpu_scene *s);

static inline double scene_now_us(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}

/* ---- on the per-entity verb path: inline in every file that uses them --------------------------------------------------- */
static inline struct ent *get(const clapgpu_scene *s, uint32_t h)
{
    return (s && h < s->n_handles && s->e[h].live) ? &s->e[h] : NULL;
}

/* the flags word of the upload image: the entity3d bits + what only the device knows */
static inline uint32_t img_flags(const struct ent *e, int xform_updated)
{
    return e->flags | (e->attached ? CLAPGPU_E_JOINT_ATTACHED : 0) | (xform_updated ? CLAPGPU_E_DIRTY : 0);
}

/* dirty bit 0: queued for upload; bit 1: xform.updated (transform_set_updated, transform.c:21-24) */
static inline void mark_dirty(clapgpu_scene *s, uint32_t h, int xform_updated)
{
    if (!s->e[h].dirty) {
        if (s->n_dirty == s->cap_dirty && mirror_grow_list(&s->dirty_list, &s->cap_dirty, s->n_dirty + 1, 1024)) {
            s->e[h].dirty |= xform_updated ? 3 : 1;              /* out of memory: the next frame uploads everything instead */
            s->topology_dirty = 1;
            return;
        }
        s->dirty_list[s->n_dirty++] = h;
    }
    s->e[h].dirty |= xform_updated ? 3 : 1;
    /* the layout stands: write the upload image now, while the caller's data is hot, instead of in a second pass */
    if (!s->topology_dirty && s->h_in && s->e[h].slot < s->n_slots) {
        const struct ent *e = &s->e[h];
        const uint32_t slot = e->slot;
        memcpy(s->h_pos_scale + 4 * (size_t)slot, e->pos_scale, 16);
        memcpy(s->h_rot + 4 * (size_t)slot, e->rot, 16);
        s->h_flags[slot] = img_flags(e, e->dirty & 2);
        if (slot < s->up_lo) s->up_lo = slot;
        if (slot >= s->up_hi) s->up_hi = slot + 1;
    }
}
#endif
