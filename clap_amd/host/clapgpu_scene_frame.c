/*
 * clapgpu_scene_frame.c -- the host mirror's frame (see clapgpu_scene_internal.h): clapgpu_scene_mq_update and
 * clapgpu_scene_attached_update over one launch-and-collect path with three transports (one fused hostio launch; mapped
 * memory with an export launch; staged copies), the stale / fetched rows of the export policy, the extra views and the
 * cull entry points.
 */
#include "clapgpu_scene_internal.h"

/* the mapped side of a one-launch small frame: the image (and its touched bits) in, the result slab and the word out */
static void scene_hostio(clapgpu_scene *s, clapgpu_entities_hostio *io, int with_inputs, int filtered)
{
    const struct in_slab in = in_slab_at(s->d_in_host, s->cap_slots);
    const struct out_slab o = out_slab_at(s->d_out_host, s->cap_slots);
    memset(io, 0, sizeof(*io));
    io->pos_scale = in.pos_scale; io->rot = in.rot; io->flags = in.flags;
    io->touched = with_inputs ? in.touched : NULL;
    io->mx = o.mx; io->inv_mx = o.inv; io->aabb = o.aabb; io->center = o.center;
    io->vis_mask = o.vis; io->rebuilt_mask = o.rebuilt; io->inside_mask = s->bv_on ? o.inside : NULL; io->exported_mask = o.exported;
    io->keep_mask = filtered ? s->d_keep : NULL;
    io->stale_mask = s->d_stale;
    io->counter = s->d_counter; io->done = s->d_done; io->done_value = ++s->frame_id;
}

/* After a one-launch frame: rows the launch rebuilt but did not write back are stale in h_out, rows it wrote are fresh. */
static void stale_after_launch(clapgpu_scene *s)
{
    const size_t words = s->n_slots / 64;
    uint32_t nz = 0, late_rows = 0;
    /* fetched_mask names the rows of THIS call only (fetch_rows): here the ones the launch itself brought over although it
     * did not rebuild them -- stale rows that have a reader now (exported, not rebuilt); exported_mask goes back to "rebuilt
     * and written", which is what a caller scatters as this frame's rebuilds */
    if (s->n_fetched) { memset(s->h_fetched, 0, words * 8); s->n_fetched = 0; }
    for (size_t w = 0; w < words; w++) {
        const uint64_t ex = s->h_exported[w], rb = s->h_rebuilt[w], late = ex & ~rb;
        const uint64_t st = (s->h_stale[w] | rb) & ~ex;
        s->h_stale[w] = st;
        nz += st != 0;
        if (late) {
            s->h_fetched[w] = late;
            s->h_exported[w] = ex & rb;
            late_rows += (uint32_t)__builtin_popcountll(late);
        }
    }
    s->n_stale_words = nz;
    if (late_rows) { s->n_fetched = late_rows; s->fetch_serial++; }
}

/* an export launch's destination: the mapped result slab (with_masks: and its masks), the next completion word */
static clapgpu_entities_export export_to_host(clapgpu_scene *s, int with_masks)
{
    const struct out_slab o = out_slab_at(s->d_out_host, s->cap_slots);
    clapgpu_entities_export x = { .mx = o.mx, .inv_mx = o.inv, .aabb = o.aabb, .center = o.center };
    if (with_masks) { x.vis_mask = o.vis; x.rebuilt_mask = o.rebuilt; x.inside_mask = s->bv_on ? o.inside : NULL; }
    x.counter = s->d_counter; x.done = s->d_done; x.done_value = ++s->frame_id;
    return x;
}

/* rows = stale & want (NULL: every stale row): over from the device arrays into h_out, named in h_fetched */
int mirror_fetch_rows(clapgpu_scene *s, const uint64_t *w0, const uint64_t *w1, const uint64_t *w2)
{
    const size_t words = s->n_slots / 64;
    /* fetched_mask names the rows of THIS call only: a caller copies them out once (fetch_serial says whether there is
     * anything new); rows of an earlier call may since have been superseded on the host */
    if (s->n_fetched && !s->fetch_accumulate) { memset(s->h_fetched, 0, words * 8); s->n_fetched = 0; }
    if (!s->n_stale_words || !s->h_select) return CLAPGPU_OK;
    uint32_t cnt = 0;
    for (size_t w = 0; w < words; w++) {
        uint64_t sel = s->h_stale[w];
        if (sel && (w0 || w1 || w2)) sel &= (w0 ? w0[w] : 0) | (w1 ? w1[w] : 0) | (w2 ? w2[w] : 0);
        s->h_select[w] = sel;
        cnt += (uint32_t)__builtin_popcountll(sel);
    }
    if (!cnt) return CLAPGPU_OK;
    CK(mirror_apply_edits(s));
    clapgpu_entities_export x = export_to_host(s, 0);
    x.stale_mask = s->d_stale;
    CK(clapgpu_entities_export_rows(NULL, &s->d, &x, s->d_select));
    CK(clapgpu_wait_word(s->h_done, s->frame_id, NULL));
    uint32_t nz = 0;
    for (size_t w = 0; w < words; w++) {
        s->h_fetched[w] = s->fetch_accumulate ? (s->h_fetched[w] | s->h_select[w]) : s->h_select[w];
        s->h_stale[w] &= ~s->h_select[w];
        nz += s->h_stale[w] != 0;
    }
    s->n_stale_words = nz;
    s->n_fetched = s->fetch_accumulate ? s->n_fetched + cnt : cnt;
    s->fetch_serial++;
    return CLAPGPU_OK;
}

void mirror_free_views(clapgpu_scene *s)
{
    for (int v = 0; v < CLAPGPU_EXTRA_VIEWS_MAX; v++) {
        if (s->xv.vis_mask[v]) clapgpu_free(s->xv.vis_mask[v]);
        if (s->xv.vis_row_pop[v]) clapgpu_free(s->xv.vis_row_pop[v]);
        if (s->h_xv_mask[v]) clapgpu_host_free(s->h_xv_mask[v]);
        s->xv.vis_mask[v] = NULL; s->xv.vis_row_pop[v] = NULL; s->xv.host_vis_mask[v] = NULL;
        s->h_xv_mask[v] = NULL; s->a_xv_mask[v] = NULL;
    }
    free(s->h_xv_union); s->h_xv_union = NULL;
    s->xv_cap_slots = 0;
}

/* the planes of the extra views, for the current capacity */
static int ensure_views(clapgpu_scene *s)
{
    if (!s->xv_want) { s->xv.n = 0; return CLAPGPU_OK; }
    if (s->xv_cap_slots != s->cap_slots || s->xv_mapped != s->zero_copy) {
        mirror_free_views(s);
        const size_t mw = mask_stride(s->cap_slots);
        s->xv_mapped = s->zero_copy;
        for (uint32_t v = 0; v < CLAPGPU_EXTRA_VIEWS_MAX; v++) {
            CK(clapgpu_malloc((void **)&s->xv.vis_mask[v], mw * 8));
            CK(clapgpu_malloc((void **)&s->xv.vis_row_pop[v], ((size_t)s->cap_slots / 64 + 16) / 16 * 16));
            CK(clapgpu_memset(s->xv.vis_mask[v], 0, mw * 8, NULL));
            if (s->xv_mapped) CK(clapgpu_host_malloc_mapped((void **)&s->h_xv_mask[v], &s->a_xv_mask[v], mw * 8));
            else CK(clapgpu_host_malloc((void **)&s->h_xv_mask[v], mw * 8));
            memset(s->h_xv_mask[v], 0, mw * 8);
        }
        s->h_xv_union = calloc(mw, 8);
        if (!s->h_xv_union) return CLAPGPU_ERR_NOMEM;
        s->xv_cap_slots = s->cap_slots;
    }
    s->xv.n = s->xv_want;
    return CLAPGPU_OK;
}

/* what ANY view of the last launch draws: the main mask alone without extra views */
static const uint64_t *views_union(clapgpu_scene *s)
{
    if (!s->xv.n || !s->h_xv_union) return s->h_mask;
    const size_t words = s->n_slots / 64;
    for (size_t w = 0; w < words; w++) {
        uint64_t m = s->h_mask[w];
        for (uint32_t v = 0; v < s->xv.n; v++) m |= s->h_xv_mask[v][w];
        s->h_xv_union[w] = m;
    }
    return s->h_xv_union;
}

/* the extra views' masks of a launch that did not write them to the host itself */
static int download_views(clapgpu_scene *s)
{
    for (uint32_t v = 0; v < s->xv.n; v++)
        CK(clapgpu_memcpy_d2h(s->h_xv_mask[v], s->xv.vis_mask[v], ((size_t)s->n_slots / 64) * 8, NULL));
    return CLAPGPU_OK;
}

int clapgpu_scene_set_views(clapgpu_scene *s, uint32_t n_extra, const clapgpu_frustum *extra)
{
    if (!s || n_extra > CLAPGPU_EXTRA_VIEWS_MAX || (n_extra && !extra)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    s->xv_want = n_extra;
    for (uint32_t v = 0; v < n_extra; v++) s->xv.frustum[v] = extra[v];
    if (!n_extra) s->xv.n = 0;
    return CLAPGPU_OK;
}

/* ---- launch and collect: the tail clapgpu_scene_mq_update and clapgpu_scene_attached_update share ------------------------
 * Where the two differ the difference is a parameter here or stays with the caller, and is meant:
 *   fused   mq_update: inputs by the touched bits, the export policy's filter (after h_keep went up), stale rows that are read
 *           come over in the same launch, the views' masks are written home; afterwards the stale / fetched bookkeeping runs
 *           whenever the policy filters.  attached_update: no inputs, no filter, no option; bookkeeping only if rows are stale.
 *   staged  mq_update copies the whole result slab when anything may have been rebuilt, else the masks; attached_update the
 *           masks, then the 64-row span its launch rebuilt.
 *   d.n_attach  zero for mq_update's launch; set for attached_update's and zeroed after it, also when the launch fails. */

/* the frame's launch: update + export (+ the touched inputs) in one with a hostio block, else the tiles or the levels alone */
static int launch_entities(clapgpu_scene *s, const clapgpu_frustum *fr, const clapgpu_entities_hostio *io)
{
    if (io) return clapgpu_entities_update_tiles_hostio(NULL, &s->d, s->d_tile_row_start, s->n_tiles, 0, fr, io);
    if (s->tiled) return clapgpu_entities_update_tiles(NULL, &s->d, s->d_tile_row_start, s->n_tiles, 0, fr);
    return clapgpu_entities_update(NULL, &s->d, s->level_start_host, s->n_levels, 0, fr);
}

/* zero-copy without the fused launch: what the update rebuilt, and the masks, straight into the mapped result slab; then the
 * completion word, and the extra views' masks by copy (t_launched: when the export was queued, for the timing line) */
static int export_rebuilt_mapped(clapgpu_scene *s, int views, double *t_launched)
{
    clapgpu_entities_export x = export_to_host(s, 1);
    CK(clapgpu_entities_export_rebuilt(NULL, &s->d, &x));
    if (t_launched) *t_launched = scene_now_us();
    CK(clapgpu_wait_word(s->h_done, s->frame_id, NULL));
    if (views) { CK(download_views(s)); CK(clapgpu_stream_sync(NULL)); }
    return CLAPGPU_OK;
}

/* staged: the result slab in one copy (whole; the three masks included: cap <= 9/8 n + 4096) or its masks alone, the views'
 * masks, a wait; rebuilt_rows: then only the span of rows the masks say this launch rebuilt */
static int collect_staged(clapgpu_scene *s, int whole, int views, int rebuilt_rows)
{
    const size_t n = s->n_slots, cap = s->cap_slots, words = n / 64;
    if (whole) CK(clapgpu_memcpy_d2h(s->h_out, s->d_out, cap * OUT_MASKS + masks_span_bytes(cap, n), NULL));
    else CK(clapgpu_memcpy_d2h(s->h_mask, s->d.vis_mask, masks_span_bytes(cap, n), NULL));
    if (views) CK(download_views(s));
    CK(clapgpu_stream_sync(NULL));
    size_t lo = words, hi = 0;
    for (size_t w = 0; rebuilt_rows && w < words; w++)
        if (s->h_rebuilt[w]) { if (w < lo) lo = w; hi = w + 1; }
    if (hi > lo) {
        const size_t a = lo * 64, cnt = (hi - lo) * 64;
        CK(clapgpu_memcpy_d2h(s->h_mx + 16 * a, s->d.mx + 16 * a, cnt * 64, NULL));
        CK(clapgpu_memcpy_d2h(s->h_inv + 16 * a, s->d.inv_mx + 16 * a, cnt * 64, NULL));
        CK(clapgpu_memcpy_d2h(s->h_aabb + 6 * a, s->d.aabb + 6 * a, cnt * 24, NULL));
        CK(clapgpu_memcpy_d2h(s->h_center + 3 * a, s->d.center + 3 * a, cnt * 12, NULL));
        CK(clapgpu_stream_sync(NULL));
    }
    return CLAPGPU_OK;
}

/* a launch without a camera leaves no verdicts, one without bounding-volume points no containment */
static void finish_masks(clapgpu_scene *s, const clapgpu_frustum *fr)
{
    if (!fr) memset(s->h_mask, 0, (s->n_slots / 64) * 8);   /* (and no extra view has a mask: xv.n is 0 for such a frame) */
    if (!s->bv_on) memset(s->h_inside, 0, (s->n_slots / 64) * 8);
}

/* ---- clapgpu_scene_mq_update, stage by stage; what one stage decides for the next travels in the plan -------------------- */
struct frame_plan {
    int      upload, full;             /* there are inputs to ship; everything is (a re-tile, a new model table) */
    int      bulk_any, bulk;           /* clapgpu_scene_mark_all_dirty since the last frame; ... and no re-tile took the image up */
    uint32_t lo, hi;                   /* the slot range of the image written since the last frame */
    uint32_t n_touched, n_bits;        /* slots now in dirty_list (reused for them); how many of them are flagged in h_touched */
    int      fused, by_bits, by_list;  /* update + export (+ the touched inputs) as one launch; how the inputs travel */
};

/* 1: the layout, then the lists -- dirty list to touched slots / the mapped record list, limbo to the free list, raw words, bulk */
static int settle_lists(clapgpu_scene *s, struct frame_plan *p)
{
    if (s->topology_dirty) {
        CK(mirror_retile(s));
        p->upload = p->full = 1;
    } else
        CK(mirror_apply_edits(s));
    if (!p->full && s->n_dirty) {
        /* the upload image was written as the verbs came in (mark_dirty); here only the bookkeeping */
        const int bits = s->zero_copy && s->tiled;       /* one launch: the kernel reads the flagged slots from the image */
        if (s->zero_copy && !bits && s->n_dirty > s->cap_list) {  /* the mapped record list grows with the busiest frame seen */
            uint32_t cap = s->cap_list ? s->cap_list : 1024;
            while (cap < s->n_dirty) cap *= 2;
            if (s->h_list) clapgpu_host_free(s->h_list);
            s->h_list = NULL; s->cap_list = 0;
            CK(clapgpu_host_malloc_mapped((void **)&s->h_list, &s->d_list, (size_t)cap * sizeof(*s->h_list)));
            s->cap_list = cap;
        }
        for (uint32_t k = 0; k < s->n_dirty; k++) {
            struct ent *e = &s->e[s->dirty_list[k]];
            const uint8_t was = e->dirty;
            e->dirty = 0;
            if (!e->live) continue;
            if (bits) {
                s->h_touched[e->slot >> 6] |= 1ull << (e->slot & 63);
            } else if (s->zero_copy) {
                clapgpu_entity_input *r = &s->h_list[p->n_touched];
                r->slot = e->slot;
                r->flags = img_flags(e, was & 2);
                memcpy(r->pos_scale, e->pos_scale, 16);
                memcpy(r->rot, e->rot, 16);
            }
            s->dirty_list[p->n_touched++] = e->slot;     /* the list is reused for the slots touched */
        }
        p->lo = s->up_lo; p->hi = s->up_hi;
        s->n_dirty = 0;
        p->upload = p->n_touched != 0 && p->hi > p->lo;
        if (bits) p->n_bits = p->n_touched;
    }
    if (s->n_limbo) CK(mirror_release_handles(s, s->limbo, &s->n_limbo));   /* deleted in place: nothing lists these handles any more */
    if (!p->full && s->n_raw) {                          /* tombstones: flags words flagged outside the dirty list */
        if (!p->upload || s->raw_lo < p->lo) p->lo = s->raw_lo;
        if (!p->upload || s->raw_hi > p->hi) p->hi = s->raw_hi;
        p->upload = 1;
    }
    p->bulk_any = s->bulk_dirty;
    p->bulk = s->bulk_dirty && !p->full;
    if (p->bulk) {                                       /* clapgpu_scene_entity_transform_mt wrote the image directly */
        p->upload = 1; p->lo = 0; p->hi = s->n_slots; p->n_touched = s->n_slots;   /* whole image up, flags cleared linearly */
    }
    s->bulk_dirty = 0;
    s->up_lo = 0xffffffffu; s->up_hi = 0;
    return CLAPGPU_OK;
}

/* 2: a changed model table goes up whole, and every entity is rebuilt against it */
static int upload_models(clapgpu_scene *s, struct frame_plan *p)
{
    if (!s->models_dirty) return CLAPGPU_OK;
    if (s->n_models > s->d_models_cap) {
        if (s->d_models) clapgpu_free(s->d_models);
        s->d_models_cap = s->n_models * 2;
        CK(clapgpu_malloc((void **)&s->d_models, (size_t)s->d_models_cap * 32));
    }
    CK(clapgpu_memcpy_h2d(s->d_models, s->models, (size_t)s->n_models * 32, NULL));
    s->d.model_table = s->d_models;
    s->d.n_models = s->n_models;
    s->models_dirty = 0;
    p->full = 1;
    return CLAPGPU_OK;
}

/* 3: the inputs -- by the touched bits (nothing to issue: h_touched says which slots of the mapped image the launch takes),
 * as the mapped record list (same bytes as the image, no copy call), or by copy */
static int ship_inputs(clapgpu_scene *s, struct frame_plan *p)
{
    const size_t n = s->n_slots;
    p->fused = s->zero_copy && s->tiled;
    p->by_bits = p->fused && p->upload && !p->full;      /* bulk: clapgpu_scene_entity_transform_mt flagged its slots itself */
    p->by_list = s->zero_copy && !p->fused && p->upload && !p->full && !p->bulk && p->n_touched <= s->cap_list;
    if (p->by_list) return clapgpu_entities_apply_inputs(NULL, &s->d, (const clapgpu_entity_input *)s->d_list, p->n_touched);
    if (p->by_bits || !p->upload) return CLAPGPU_OK;
    /* one copy of the whole input slab after a re-tile or when most of it changed; else the slot range */
    const size_t a = p->full ? 0 : p->lo, cnt = p->full ? n : (size_t)p->hi - p->lo;
    if (p->full || 2 * cnt > n) return clapgpu_memcpy_h2d(s->d_in, s->h_in, (size_t)s->cap_slots * IN_FLAGS + n * 4, NULL);
    CK(clapgpu_memcpy_h2d((float *)s->d.pos_scale + 4 * a, s->h_pos_scale + 4 * a, cnt * 16, NULL));
    CK(clapgpu_memcpy_h2d((float *)s->d.rot + 4 * a, s->h_rot + 4 * a, cnt * 16, NULL));
    return clapgpu_memcpy_h2d(s->d.flags + a, s->h_flags + a, cnt * 4, NULL);
}

/* 4: what rides the launch -- the bounding-volume query and the frame's other views */
static int set_query_and_views(clapgpu_scene *s, const clapgpu_frustum *frustum)
{
    if (s->bv_on) {
        memcpy(s->bvq.cam_pos, s->bv_cam, 12); memcpy(s->bvq.ctl_pos, s->bv_ctl, 12);
        const struct ent *ce = s->bv_has_ctl ? get(s, s->bv_ctl_handle) : NULL;
        s->bvq.has_ctl = s->bv_has_ctl; s->bvq.ctl_entity = ce ? ce->slot : 0xffffffffu;
        s->bvq.result = NULL;                            /* the containment mask is what the callers replay: no result word, no fill launch */
        s->d.bv = &s->bvq;
    } else {
        s->d.bv = NULL;
    }
    s->have_frustum = frustum != NULL;
    if (frustum) s->last_frustum = *frustum;
    if (frustum) CK(ensure_views(s)); else s->xv.n = 0;  /* the frame's other views ride the main one's launch */
    s->d.views = s->xv.n ? &s->xv : NULL;
    s->d.n_attach = 0;                                   /* joint attachments ride the palettes of THIS frame: clapgpu_scene_attached_update */
    return CLAPGPU_OK;
}

/* 5: the launch and its results into h_out, by the transport the scene has */
static int launch_and_collect(clapgpu_scene *s, const clapgpu_frustum *frustum, const struct frame_plan *p)
{
    const char *how = p->by_bits ? "touched bits" : p->by_list ? "list" : p->upload ? "copy" : "none";
    const double t0 = scene_now_us();
    double t1 = t0;
    if (p->fused) {
        clapgpu_entities_hostio io;
        if (s->keep_dirty && s->export_drawn) {
            CK(clapgpu_memcpy_h2d(s->d_keep, s->h_keep, (s->n_slots / 64) * 8, NULL));
            CK(clapgpu_stream_sync(NULL));                 /* h_keep is pageable and may change right after this call */
            s->keep_dirty = 0;
        }
        scene_hostio(s, &io, p->by_bits, s->export_drawn);
        io.options |= CLAPGPU_HOSTIO_EXPORT_STALE_READ;    /* what an earlier frame left stale and this one reads comes over in the same launch */
        for (uint32_t v = 0; v < s->xv.n; v++) s->xv.host_vis_mask[v] = s->a_xv_mask[v];   /* the launch writes the views' masks home itself */
        CK(launch_entities(s, frustum, &io));
        t1 = scene_now_us();
        CK(clapgpu_wait_word(s->h_done, s->frame_id, NULL));
        if (s->export_drawn || s->n_stale_words) stale_after_launch(s);
        else if (s->n_fetched) { memset(s->h_fetched, 0, (s->n_slots / 64) * 8); s->n_fetched = 0; }
        if (s->timing)
            fprintf(stderr, "scene small frame: %u inputs by %s, one launch %.1f us, wait %.1f us\n", p->n_touched, how, t1 - t0, scene_now_us() - t1);
        return CLAPGPU_OK;
    }
    CK(launch_entities(s, frustum, NULL));
    /* staged: unless something may have been rebuilt the last download stands, and the masks alone come down */
    if (!s->zero_copy) return collect_staged(s, p->upload || p->full || !s->have_results, 1, 0);
    CK(export_rebuilt_mapped(s, s->xv.n != 0, &t1));
    if (s->timing)
        fprintf(stderr, "scene small frame: %u inputs by %s, launches %.1f us, wait %.1f us\n", p->n_touched, how, t1 - t0, scene_now_us() - t1);
    return CLAPGPU_OK;
}

/* 6: the touched bits were taken by this frame's launch or by its copy */
static void clear_touched(clapgpu_scene *s, const struct frame_plan *p)
{
    for (uint32_t k = 0; k < p->n_bits; k++) s->h_touched[s->dirty_list[k] >> 6] = 0;
    for (uint32_t k = 0; k < s->n_raw; k++) s->h_touched[s->raw_words[k]] = 0;
    s->n_raw = 0;
    if (p->bulk_any && s->zero_copy) memset(s->h_touched, 0, mask_stride(s->cap_slots) * 8);   /* what clapgpu_scene_entity_transform_mt flagged */
}

/* 7: EXPORT_DRAWN -- whoever is read this frame and was left stale by an earlier one (an entity that came into view, a box
 * that now contains the camera, a reader registered since) comes over now.  The launch has brought over what it found stale
 * and read (stale_after_launch); this catches what it could not know: nothing, unless a caller's masks changed behind it */
static int fetch_what_is_read(clapgpu_scene *s, const clapgpu_frustum *frustum)
{
    s->fetch_accumulate = 1;
    const int rc = frustum ? mirror_fetch_rows(s, views_union(s), s->bv_on ? s->h_inside : NULL, s->h_keep)
                           : mirror_fetch_rows(s, NULL, NULL, NULL);    /* a pass without a camera draws everything (model.c:969) */
    s->fetch_accumulate = 0;
    return rc;
}

/* 8: the image's DIRTY flags: the kernel cleared its copy too */
static void clear_dirty_flags(clapgpu_scene *s, const struct frame_plan *p)
{
    if (p->full || 4 * (size_t)p->n_touched > s->n_slots)
        for (size_t i = 0; i < s->n_slots; i++) s->h_flags[i] &= ~CLAPGPU_E_DIRTY;
    else
        for (uint32_t k = 0; k < p->n_touched; k++) s->h_flags[s->dirty_list[k]] &= ~CLAPGPU_E_DIRTY;
}

int clapgpu_scene_mq_update(clapgpu_scene *s, const clapgpu_frustum *frustum)
{
    if (!s) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    struct frame_plan p = { .lo = 0xffffffffu };
    CK(settle_lists(s, &p));
    CK(upload_models(s, &p));
    if (s->n_models == 0) {                              /* nothing to launch */
        for (uint32_t k = 0; k < p.n_bits; k++) s->h_touched[s->dirty_list[k] >> 6] = 0;
        return CLAPGPU_OK;
    }
    CK(ship_inputs(s, &p));
    CK(set_query_and_views(s, frustum));
    CK(launch_and_collect(s, frustum, &p));
    clear_touched(s, &p);
    finish_masks(s, frustum);
    if (p.fused) CK(fetch_what_is_read(s, frustum));
    clear_dirty_flags(s, &p);
    s->have_results = 1;
    return CLAPGPU_OK;
}

struct att_key { uint32_t slot, k; };
static int att_cmp(const void *a, const void *b)
{
    const struct att_key *x = a, *y = b;
    return x->slot < y->slot ? -1 : x->slot > y->slot;
}

/*
 * The second launch of a frame with joint attachments (model.c:1626-1641): entity handles[k] rides
 * parent.mx * ((jt[k] * bind[k]) * local), jt[k] = its parent's joint_transforms[parent_joint] of THIS frame -- which
 * exist only after the pose that followed clapgpu_scene_mq_update() -- and bind[k] that joint's bind matrix.  Such
 * entities are rebuilt every frame, everything below them follows through the seq counters; nothing else is touched.
 * On return the result arrays hold the rebuilt rows and rebuilt_mask says which they are.
 */
int clapgpu_scene_attached_update(clapgpu_scene *s, uint32_t n, const uint32_t *handles, const float *jt, const float *bind)
{
    if (!s || (n && (!handles || !jt || !bind))) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!n) return CLAPGPU_OK;
    if (s->topology_dirty || !s->have_results || !s->n_models) return CLAPGPU_ERR_NOT_SUPPORTED;   /* mq_update first */
    CK(mirror_apply_edits(s));
    const size_t need = (size_t)n * (sizeof(clapgpu_attach) + 128);
    if (n > s->cap_att || s->att_mapped != s->zero_copy) {
        uint32_t cap = s->cap_att ? s->cap_att : 64;
        while (cap < n) cap *= 2;
        if (s->h_att) clapgpu_host_free(s->h_att);
        if (s->d_att && !s->att_mapped) clapgpu_free(s->d_att);
        if (s->d_att_local) clapgpu_free(s->d_att_local);
        s->h_att = s->d_att = NULL; s->d_att_local = NULL; s->cap_att = 0;
        const size_t bytes = (size_t)cap * (sizeof(clapgpu_attach) + 128);
        s->att_mapped = s->zero_copy;
        if (s->att_mapped) CK(clapgpu_host_malloc_mapped(&s->h_att, &s->d_att, bytes));
        else { CK(clapgpu_host_malloc(&s->h_att, bytes)); CK(clapgpu_malloc(&s->d_att, bytes)); }
        CK(clapgpu_malloc((void **)&s->d_att_local, (size_t)cap * 64));
        s->cap_att = cap;
    }
    struct att_key *key = malloc((size_t)n * sizeof(*key));
    if (!key) return CLAPGPU_ERR_NOMEM;
    for (uint32_t k = 0; k < n; k++) {
        const struct ent *e = get(s, handles[k]);
        if (!e || !e->attached || e->parent == CLAPGPU_NO_ENTITY || e->slot >= s->n_slots) { free(key); return CLAPGPU_ERR_INVALID_ARGUMENTS; }
        key[k].slot = e->slot; key[k].k = k;
    }
    qsort(key, n, sizeof(*key), att_cmp);                /* the kernel looks an entity up by binary search */
    clapgpu_attach *tab = s->h_att;
    float *pj = (float *)((char *)s->h_att + (size_t)n * sizeof(clapgpu_attach)), *pb = pj + 16 * (size_t)n;
    for (uint32_t i = 0; i < n; i++) {
        if (i && key[i].slot == key[i - 1].slot) { free(key); return CLAPGPU_ERR_INVALID_ARGUMENTS; }
        tab[i] = (clapgpu_attach){ .entity = key[i].slot, .jt = i, .bind = i };
        memcpy(pj + 16 * (size_t)i, jt + 16 * (size_t)key[i].k, 64);
        memcpy(pb + 16 * (size_t)i, bind + 16 * (size_t)key[i].k, 64);
    }
    free(key);
    if (!s->att_mapped) CK(clapgpu_memcpy_h2d(s->d_att, s->h_att, need, NULL));
    s->d.n_attach = n;
    s->d.attach = s->d_att;
    s->d.jt_pool = (const float *)((const char *)s->d_att + (size_t)n * sizeof(clapgpu_attach));
    s->d.bind_pool = s->d.jt_pool + 16 * (size_t)n;
    s->d.attach_local = s->d_att_local;
    const clapgpu_frustum *fr = s->have_frustum ? &s->last_frustum : NULL;
    const int fused = s->zero_copy && s->tiled;
    clapgpu_entities_hostio io;
    if (fused) scene_hostio(s, &io, 0, 0);               /* the few attached subtrees: every rebuilt row comes back */
    const int rc = launch_entities(s, fr, fused ? &io : NULL);
    s->d.n_attach = 0;
    if (rc) return rc;
    if (fused) {
        CK(clapgpu_wait_word(s->h_done, s->frame_id, NULL));
        if (s->n_stale_words) stale_after_launch(s);
    } else if (s->zero_copy)
        CK(export_rebuilt_mapped(s, fr && s->xv.n, NULL));
    else
        CK(collect_staged(s, 0, fr != NULL, 1));         /* the masks first, then only the span of rows this launch rebuilt */
    finish_masks(s, fr);
    return CLAPGPU_OK;
}

/* view_entity_in_frustum for a frustum other than the one of the last mq_update (the engine recomputes its frusta in
 * scene_cameras_calc, AFTER mq_update: clap.c:614-616): re-tests every entity's stored box, refreshes vis_mask */
int clapgpu_scene_cull(clapgpu_scene *s, const clapgpu_frustum *frustum)
{
    if (!s || !frustum) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!s->have_results || s->topology_dirty) return CLAPGPU_ERR_NOT_SUPPORTED;   /* nothing on the device yet */
    CK(mirror_apply_edits(s));
    CK(ensure_views(s));
    s->d.views = s->xv.n ? &s->xv : NULL;
    for (uint32_t v = 0; v < s->xv.n; v++) s->xv.host_vis_mask[v] = NULL;
    CK(clapgpu_entities_cull(NULL, &s->d, frustum));   /* every view of the frame from one read of the boxes */
    CK(clapgpu_memcpy_d2h(s->h_mask, s->d.vis_mask, ((size_t)s->n_slots / 64) * 8, NULL));
    CK(download_views(s));
    CK(clapgpu_stream_sync(NULL));
    s->have_frustum = 1; s->last_frustum = *frustum;
    CK(mirror_fetch_rows(s, views_union(s), NULL, NULL));     /* EXPORT_DRAWN: what the views draw and an earlier frame left stale */
    return CLAPGPU_OK;
}

/* one extra view alone: its planes moved since the launch that culled it (light_update runs after mq_update, scene.c:1166-1171) */
int clapgpu_scene_cull_view(clapgpu_scene *s, uint32_t view, const clapgpu_frustum *frustum)
{
    if (!s || !frustum || view >= s->xv_want) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!s->have_results || s->topology_dirty) return CLAPGPU_ERR_NOT_SUPPORTED;
    CK(mirror_apply_edits(s));
    CK(ensure_views(s));
    s->xv.frustum[view] = *frustum;
    clapgpu_entities one = s->d;
    one.vis_mask = s->xv.vis_mask[view]; one.vis_row_pop = s->xv.vis_row_pop[view]; one.views = NULL;
    CK(clapgpu_entities_cull(NULL, &one, frustum));
    CK(clapgpu_memcpy_d2h(s->h_xv_mask[view], s->xv.vis_mask[view], ((size_t)s->n_slots / 64) * 8, NULL));
    CK(clapgpu_stream_sync(NULL));
    CK(mirror_fetch_rows(s, s->h_xv_mask[view], NULL, NULL));
    return CLAPGPU_OK;
}
