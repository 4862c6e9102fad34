/*
 * clapgpu_scene_lod.c -- the host mirror's LOD pick and draw list for the render passes (see clapgpu_scene_internal.h).
 */
#include "clapgpu_scene_internal.h"

/* ---- the render passes' LOD pick and draw list (model.c:959-992) ------------------------------------------------------ */
int clapgpu_scene_entity_lod(clapgpu_scene *s, uint32_t handle, int force_lod, int cur_lod)
{
    struct ent *e = get(s, handle);
    if (!e) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    e->force_lod = force_lod;
    e->cur_lod = cur_lod;
    if (s->lod_cap && s->lod_layout_gen == s->layout_gen && !s->topology_dirty && e->slot < s->n_slots) {
        s->h_force_lod[e->slot] = force_lod;
        s->h_cur_lod[e->slot] = cur_lod;
        if (e->slot < s->lod_lo) s->lod_lo = e->slot;
        if (e->slot + 1 > s->lod_hi) s->lod_hi = e->slot + 1;
    }
    return CLAPGPU_OK;
}

int clapgpu_scene_entity_cur_lod(const clapgpu_scene *s, uint32_t handle)
{
    const struct ent *e = get(s, handle);
    return e ? e->cur_lod : -1;
}

void mirror_free_lod(clapgpu_scene *s)
{
    void *dev[] = { s->d_force_lod, s->d_cur_lod, s->d_visible, s->d_visible_count, s->d_draw_lod, s->d_vis_scratch };
    for (unsigned i = 0; i < sizeof(dev) / sizeof(dev[0]); i++)
        if (dev[i]) clapgpu_free(dev[i]);
    void *host[] = { s->h_draw_slot, s->h_draw_lod, s->h_visible_count };
    for (unsigned i = 0; i < sizeof(host) / sizeof(host[0]); i++)
        if (host[i]) clapgpu_host_free(host[i]);
    free(s->h_force_lod); free(s->h_cur_lod);
    s->d_force_lod = s->d_cur_lod = s->d_draw_lod = NULL; s->d_visible = s->d_visible_count = NULL; s->d_vis_scratch = NULL;
    s->h_draw_slot = NULL; s->h_draw_lod = NULL; s->h_visible_count = NULL; s->h_force_lod = s->h_cur_lod = NULL;
    s->lod_cap = 0; s->n_draw = 0;
}

static int ensure_lod(clapgpu_scene *s)
{
    if (s->lod_cap < s->cap_slots) {
        mirror_free_lod(s);
        const size_t n = s->cap_slots;
        s->h_force_lod = malloc(n * 4); s->h_cur_lod = malloc(n * 4);
        if (!s->h_force_lod || !s->h_cur_lod) return CLAPGPU_ERR_NOMEM;
        CK(clapgpu_malloc((void **)&s->d_force_lod, n * 4)); CK(clapgpu_malloc((void **)&s->d_cur_lod, n * 4));
        CK(clapgpu_malloc((void **)&s->d_visible, n * 4));   CK(clapgpu_malloc((void **)&s->d_draw_lod, n * 4));
        CK(clapgpu_malloc((void **)&s->d_visible_count, 16));
        CK(clapgpu_malloc(&s->d_vis_scratch, clapgpu_visible_scratch_bytes((uint32_t)n)));
        s->lod_mapped = s->zero_copy && n <= CLAPGPU_SCENE_LOD_MAPPED_SLOTS;
        if (s->lod_mapped) {
            CK(clapgpu_host_malloc_mapped((void **)&s->h_draw_slot, &s->a_draw_slot, n * 4));
            CK(clapgpu_host_malloc_mapped((void **)&s->h_draw_lod, &s->a_draw_lod, n * 4));
            CK(clapgpu_host_malloc_mapped((void **)&s->h_visible_count, &s->a_visible_count, 16));
        } else {
            CK(clapgpu_host_malloc((void **)&s->h_draw_slot, n * 4)); CK(clapgpu_host_malloc((void **)&s->h_draw_lod, n * 4));
            CK(clapgpu_host_malloc((void **)&s->h_visible_count, 16));
        }
        s->lod_cap = s->cap_slots;
        s->lod_layout_gen = s->layout_gen - 1;                       /* force the fill below */
    }
    if (s->lod_layout_gen != s->layout_gen) {                        /* a re-tile moved the entities: slot order anew */
        for (uint32_t i = 0; i < s->n_slots; i++) {
            const uint32_t h = s->slot_handle[i];
            s->h_force_lod[i] = h == CLAPGPU_NO_ENTITY ? -1 : s->e[h].force_lod;
            s->h_cur_lod[i] = h == CLAPGPU_NO_ENTITY ? 0 : s->e[h].cur_lod;
        }
        s->lod_lo = 0; s->lod_hi = s->n_slots;
        s->lod_layout_gen = s->layout_gen;
    }
    if (s->lod_lo < s->lod_hi) {
        const size_t off = s->lod_lo, cnt = s->lod_hi - s->lod_lo;
        CK(clapgpu_memcpy_h2d(s->d_force_lod + off, s->h_force_lod + off, cnt * 4, NULL));
        CK(clapgpu_memcpy_h2d(s->d_cur_lod + off, s->h_cur_lod + off, cnt * 4, NULL));
    }
    s->lod_lo = 0xffffffffu; s->lod_hi = 0;
    return CLAPGPU_OK;
}

int clapgpu_scene_select_lod(clapgpu_scene *s, const float cam_pos[3], uint32_t *n_draw)
{
    return clapgpu_scene_select_lod_view(s, CLAPGPU_SCENE_MAIN_VIEW, cam_pos, n_draw);
}

int clapgpu_scene_select_lod_view(clapgpu_scene *s, uint32_t view, const float cam_pos[3], uint32_t *n_draw)
{
    if (!s || !n_draw || (view != CLAPGPU_SCENE_MAIN_VIEW && view >= s->xv.n)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    *n_draw = 0;
    if (!s->have_results || s->topology_dirty) return CLAPGPU_ERR_NOT_SUPPORTED;   /* nothing on the device yet */
    if (s->n_slots == 0) { s->n_draw = 0; return CLAPGPU_OK; }
    CK(mirror_apply_edits(s));
    CK(ensure_lod(s));
    /* the ordered visible list from the mask the last update / cull left on the device, then -- with a camera -- the LOD
     * pick over it (one launch each); without one the pass keeps every cur_lod (model.c:974: `if (camera)`) */
    uint32_t *out_slot = s->lod_mapped ? s->a_draw_slot : s->d_visible, *out_count = s->lod_mapped ? s->a_visible_count : s->d_visible_count;
    int32_t *out_lod = s->lod_mapped ? s->a_draw_lod : s->d_draw_lod;
    clapgpu_entities of_view = s->d;                     /* the plane the list is made from */
    if (view != CLAPGPU_SCENE_MAIN_VIEW) { of_view.vis_mask = s->xv.vis_mask[view]; of_view.vis_row_pop = s->xv.vis_row_pop[view]; }
    if (cam_pos)
        CK(clapgpu_visible_compact_lod(NULL, &of_view, 0, cam_pos, s->d_force_lod, s->d_cur_lod, out_slot, out_count, out_lod, s->d_vis_scratch));
    else
        CK(clapgpu_visible_compact(NULL, of_view.vis_mask, of_view.vis_row_pop, s->n_slots, 0, out_slot, out_count, s->d_vis_scratch));
    if (!s->lod_mapped) CK(clapgpu_memcpy_d2h(s->h_visible_count, s->d_visible_count, 4, NULL));
    CK(clapgpu_stream_sync(NULL));
    const uint32_t n = *s->h_visible_count;
    if (n > s->n_slots) return CLAPGPU_ERR_UNKNOWN;
    if (n && !s->lod_mapped) {
        CK(clapgpu_memcpy_d2h(s->h_draw_slot, s->d_visible, (size_t)n * 4, NULL));
        if (cam_pos) CK(clapgpu_memcpy_d2h(s->h_draw_lod, s->d_draw_lod, (size_t)n * 4, NULL));
        CK(clapgpu_stream_sync(NULL));
    }
    for (uint32_t k = 0; k < n && !(cam_pos && s->lod_sync_by_caller); k++) {   /* the host copies follow the pick: where it changed something */
        const uint32_t slot = s->h_draw_slot[k];
        if (!cam_pos) { s->h_draw_lod[k] = s->h_cur_lod[slot]; continue; }
        if (s->h_cur_lod[slot] == s->h_draw_lod[k]) continue;
        s->h_cur_lod[slot] = s->h_draw_lod[k];
        const uint32_t h = s->slot_handle[slot];
        if (h != CLAPGPU_NO_ENTITY) s->e[h].cur_lod = s->h_draw_lod[k];
    }
    s->n_draw = n;
    *n_draw = n;
    return CLAPGPU_OK;
}

/* A caller that walks the draw list anyway (and knows every entity's last LOD) tells the mirror where the pick changed one,
 * instead of the mirror comparing every entry itself: clapgpu_scene_set_lod_sync(s, 1), then clapgpu_scene_lod_picked() for
 * each changed entry of every list picked with a camera -- distinct slots may be reported from several threads at once. */
void clapgpu_scene_set_lod_sync(clapgpu_scene *s, int by_caller) { if (s) s->lod_sync_by_caller = by_caller != 0; }

void clapgpu_scene_lod_picked(clapgpu_scene *s, uint32_t slot, int lod)
{
    if (!s || !s->lod_cap || slot >= s->n_slots) return;
    s->h_cur_lod[slot] = lod;
    const uint32_t h = s->slot_handle[slot];
    if (h != CLAPGPU_NO_ENTITY) s->e[h].cur_lod = lod;
}

uint32_t clapgpu_scene_draw_list(const clapgpu_scene *s, const uint32_t **slots, const int32_t **lods)
{
    if (!s || !s->lod_cap) return 0;
    if (slots) *slots = s->h_draw_slot;
    if (lods) *lods = s->h_draw_lod;
    return s->n_draw;
}
