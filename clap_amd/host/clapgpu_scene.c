/*
 * clapgpu_scene.c -- C host mirror of a CLAP model queue over libclapgpu (see include/clapgpu_scene.h).  Plain C11; this
 * file owns the lifecycle, the model table, the handle table, the entity verbs and the result accessors.  The tile layout
 * (C counterpart of clap_amd/tiler.py) is in clapgpu_scene_layout.c, the frame's launches in clapgpu_scene_frame.c, the LOD
 * pick in clapgpu_scene_lod.c; clapgpu_scene_internal.h holds what they share.
 */
#include <math.h>
#include "clapgpu_scene_internal.h"

/* room for `need` entries in a plain list of handles / slots / words, doubling from `first` */
int mirror_grow_list(uint32_t **arr, uint32_t *cap, uint32_t need, uint32_t first)
{
    if (need <= *cap) return CLAPGPU_OK;
    uint32_t c = *cap ? *cap : first;
    while (c < need) c *= 2;
    uint32_t *q = realloc(*arr, (size_t)c * sizeof(uint32_t));
    if (!q) return CLAPGPU_ERR_NOMEM;
    *arr = q; *cap = c;
    return CLAPGPU_OK;
}

/* handles nothing lists any more go back to the free list */
int mirror_release_handles(clapgpu_scene *s, const uint32_t *list, uint32_t *n)
{
    CK(mirror_grow_list(&s->free_list, &s->cap_free, s->n_free + *n, 256));
    memcpy(s->free_list + s->n_free, list, (size_t)*n * sizeof(uint32_t));
    s->n_free += *n;
    *n = 0;
    return CLAPGPU_OK;
}

int clapgpu_scene_create(clapgpu_scene **out, int device)
{
    if (!out) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    CK(clapgpu_init(device));
    clapgpu_scene *s = calloc(1, sizeof(*s));
    if (!s) return CLAPGPU_ERR_NOMEM;
    s->topology_dirty = 1;
    s->grow_tile = s->grown_from = s->tiles_from = CLAPGPU_NO_ENTITY;
    s->zero_copy_max_slots = CLAPGPU_SCENE_ZERO_COPY_SLOTS;
    const char *zc = getenv("CLAPGPU_SCENE_ZERO_COPY_SLOTS");   /* tuning knob: 0 = always copy */
    if (zc) s->zero_copy_max_slots = (uint32_t)strtoul(zc, NULL, 0);
    s->timing = getenv("CLAPGPU_SCENE_TIMING") != NULL;
    *out = s;
    return CLAPGPU_OK;
}

void clapgpu_scene_set_zero_copy_slots(clapgpu_scene *s, uint32_t max_slots)
{
    if (!s || s->zero_copy_max_slots == max_slots) return;
    s->zero_copy_max_slots = max_slots;
    s->cap_slots = 0;                                   /* the slabs are re-made in the new mode by the next re-tile */
    s->topology_dirty = 1;
}

int clapgpu_scene_is_zero_copy(const clapgpu_scene *s) { return s ? s->zero_copy : 0; }

void mirror_free_device(clapgpu_scene *s)
{
    mirror_free_lod(s);
    void *p[] = { s->d_in, s->d_out, (void *)s->d.parent, (void *)s->d.model, s->d.seqs, s->d.vis_row_pop,
                  s->d_tile_row_start };
    for (unsigned i = 0; i < sizeof(p) / sizeof(p[0]); i++)
        if (p[i]) clapgpu_free(p[i]);
    memset(&s->d, 0, sizeof(s->d));
    s->d_in = s->d_out = NULL;
    s->d_tile_row_start = NULL;
}

void clapgpu_scene_destroy(clapgpu_scene *s)
{
    if (s) mirror_free_views(s);
    if (!s) return;
    mirror_free_device(s);
    if (s->d_models) clapgpu_free(s->d_models);
    free(s->e); free(s->free_list); free(s->dead_list); free(s->dirty_list); free(s->models); free(s->slot_handle);
    free(s->tile_row_start_host); free(s->level_start_host);
    if (s->h_in) clapgpu_host_free(s->h_in);
    if (s->h_out) clapgpu_host_free(s->h_out);
    if (s->h_parent) clapgpu_host_free(s->h_parent);
    if (s->h_model) clapgpu_host_free(s->h_model);
    free(s->slot_user);
    if (s->d_bv_result) clapgpu_free(s->d_bv_result);
    if (s->h_list) clapgpu_host_free(s->h_list);
    if (s->h_done) clapgpu_host_free(s->h_done);
    if (s->d_counter) clapgpu_free(s->d_counter);
    if (s->h_att) clapgpu_host_free(s->h_att);
    if (s->d_att && !s->att_mapped) clapgpu_free(s->d_att);
    if (s->d_att_local) clapgpu_free(s->d_att_local);
    if (s->d_keep) clapgpu_free(s->d_keep);
    if (s->h_select) clapgpu_host_free(s->h_select);
    free(s->h_keep); free(s->h_stale); free(s->h_fetched); free(s->free_roots); free(s->raw_words); free(s->edits); free(s->limbo);
    if (s->h_place) clapgpu_host_free(s->h_place);
    if (s->d_stale) clapgpu_free(s->d_stale);
    free(s);
}

int clapgpu_scene_model_new(clapgpu_scene *s, const float aabb[6], int skip_aabb, uint32_t *model)
{
    if (!s || !aabb || !model) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (s->n_models == s->cap_models) {
        const uint32_t cap = s->cap_models ? 2 * s->cap_models : 16;
        float *q = realloc(s->models, (size_t)cap * 8 * sizeof(float));
        if (!q) return CLAPGPU_ERR_NOMEM;
        s->models = q; s->cap_models = cap;
    }
    float *row = s->models + 8 * (size_t)s->n_models;
    uint32_t skip = skip_aabb ? 1u : 0u;
    row[0] = aabb[0]; row[1] = aabb[1]; row[2] = aabb[2];
    memcpy(&row[3], &skip, 4);
    row[4] = aabb[3]; row[5] = aabb[4]; row[6] = aabb[5]; row[7] = 0.f;     /* lod_min = lod_max = 0 until clapgpu_scene_model_lods */
    *model = s->n_models++;
    s->models_dirty = 1;
    return CLAPGPU_OK;
}

int clapgpu_scene_model_lods(clapgpu_scene *s, uint32_t model, unsigned int lod_min, unsigned int lod_max)
{
    if (!s || model >= s->n_models || lod_min > 255 || lod_max > 255) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    const uint32_t bits = lod_min | (lod_max << 8);
    memcpy(&s->models[8 * (size_t)model + 7], &bits, 4);
    s->models_dirty = 1;
    return CLAPGPU_OK;
}

int mirror_new_handle(clapgpu_scene *s, uint32_t model, void *user, uint32_t *handle)
{
    uint32_t h;
    if (s->n_free) {
        h = s->free_list[--s->n_free];
    } else {
        if (s->n_handles == s->cap_handles) {
            const uint32_t cap = s->cap_handles ? 2 * s->cap_handles : 1024;
            struct ent *q = realloc(s->e, (size_t)cap * sizeof(struct ent));
            if (!q) return CLAPGPU_ERR_NOMEM;
            s->e = q; s->cap_handles = cap;
        }
        h = s->n_handles++;
    }
    struct ent *e = &s->e[h];
    memset(e, 0, sizeof(*e));
    e->pos_scale[3] = 1.f;                              /* model.c:1738 scale = 1 */
    e->rot[3] = 1.f;                                    /* transform_init: identity quat */
    e->flags = CLAPGPU_E_ALIVE | CLAPGPU_E_VISIBLE;
    e->parent = CLAPGPU_NO_ENTITY;
    e->model = model;
    e->user = user;
    e->live = 1;
    e->force_lod = -1;                                  /* entity3d_make, model.c:1741; cur_lod 0 */
    *handle = h;
    return CLAPGPU_OK;
}

int clapgpu_scene_entity_new(clapgpu_scene *s, uint32_t model, void *user, uint32_t *handle)
{
    if (!s || !handle || model >= s->n_models) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    CK(mirror_new_handle(s, model, user, handle));
    s->topology_dirty = 1;
    return CLAPGPU_OK;
}

int clapgpu_scene_entity_delete(clapgpu_scene *s, uint32_t handle)
{
    struct ent *e = get(s, handle);
    if (!e) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    /* Its children become roots (like a NULL e->parent) -- found by ONE pass for all of a frame's deletions when the layout
     * is rebuilt (release_dead), not by a pass over every entity per deletion; until then the handle is not handed out again,
     * so a child's parent field cannot come to name a stranger. */
    CK(mirror_grow_list(&s->dead_list, &s->cap_dead, s->n_dead + 1, 256));
    e->live = 0;
    if (e->parent != CLAPGPU_NO_ENTITY && e->parent < s->n_handles && s->e[e->parent].live && s->e[e->parent].n_children)
        s->e[e->parent].n_children--;
    s->dead_list[s->n_dead++] = handle;
    s->topology_dirty = 1;
    return CLAPGPU_OK;
}

int clapgpu_scene_entity_set_parent(clapgpu_scene *s, uint32_t handle, uint32_t parent)
{
    struct ent *e = get(s, handle);
    if (!e || (parent != CLAPGPU_NO_ENTITY && (!get(s, parent) || parent == handle)))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (e->parent != parent) {
        if (e->parent != CLAPGPU_NO_ENTITY && e->parent < s->n_handles && s->e[e->parent].live && s->e[e->parent].n_children)
            s->e[e->parent].n_children--;
        if (parent != CLAPGPU_NO_ENTITY) s->e[parent].n_children++;
        e->parent = parent;
        s->topology_dirty = 1;
    }
    return CLAPGPU_OK;
}

int clapgpu_scene_entity_position(clapgpu_scene *s, uint32_t handle, const float pos[3])
{
    struct ent *e = get(s, handle);
    if (!e || !pos) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    memcpy(e->pos_scale, pos, 12);
    mark_dirty(s, handle, 1);
    return CLAPGPU_OK;
}

int clapgpu_scene_entity_transform(clapgpu_scene *s, uint32_t handle, const float pos[3], const float q[4], float scale)
{
    struct ent *e = get(s, handle);
    if (!e || !pos || !q) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    memcpy(e->pos_scale, pos, 12);
    e->pos_scale[3] = scale;
    memcpy(e->rot, q, 16);
    mark_dirty(s, handle, 1);
    return CLAPGPU_OK;
}

/* entity_transform + entity_flags for callers that update many DIFFERENT handles from several threads at once (no
 * topology verb may run meanwhile): nothing shared is touched, so the caller has to finish with
 * clapgpu_scene_mark_all_dirty(), which makes the next mq_update upload the whole image. */
int clapgpu_scene_entity_transform_mt(clapgpu_scene *s, uint32_t handle, const float pos[3], const float q[4], float scale,
                                      uint32_t flags, int xform_updated)
{
    struct ent *e = get(s, handle);
    if (!e || !pos || !q) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    memcpy(e->pos_scale, pos, 12);
    e->pos_scale[3] = scale;
    memcpy(e->rot, q, 16);
    e->flags = flags & ~CLAPGPU_E_DIRTY;
    if (!s->topology_dirty && s->h_in && e->slot < s->n_slots) {
        memcpy(s->h_pos_scale + 4 * (size_t)e->slot, e->pos_scale, 16);
        memcpy(s->h_rot + 4 * (size_t)e->slot, e->rot, 16);
        s->h_flags[e->slot] = img_flags(e, xform_updated);
        if (s->zero_copy && s->tiled)                    /* one-launch frames read the flagged slots from the image: no bulk copy */
            __atomic_fetch_or(&s->h_touched[e->slot >> 6], 1ull << (e->slot & 63), __ATOMIC_RELAXED);
    } else {
        e->dirty |= xform_updated ? 3 : 1;               /* picked up by the re-tile's full image */
    }
    return CLAPGPU_OK;
}

/* The transform alone (entity3d_position / _move / _rotate / _scale leave the flags as they are), same threading rules;
 * xform_updated is OR-ed in, so pushing an entity twice in a frame -- the second time with its flag already taken -- is
 * harmless.  Finish with clapgpu_scene_mark_all_dirty(). */
int clapgpu_scene_entity_xform_mt(clapgpu_scene *s, uint32_t handle, const float pos[3], const float q[4], float scale, int xform_updated)
{
    struct ent *e = get(s, handle);
    if (!e || !pos || !q) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    memcpy(e->pos_scale, pos, 12);
    e->pos_scale[3] = scale;
    memcpy(e->rot, q, 16);
    if (!s->topology_dirty && s->h_in && e->slot < s->n_slots) {
        memcpy(s->h_pos_scale + 4 * (size_t)e->slot, e->pos_scale, 16);
        memcpy(s->h_rot + 4 * (size_t)e->slot, e->rot, 16);
        if (xform_updated) s->h_flags[e->slot] |= CLAPGPU_E_DIRTY;
        if (s->zero_copy && s->tiled)
            __atomic_fetch_or(&s->h_touched[e->slot >> 6], 1ull << (e->slot & 63), __ATOMIC_RELAXED);
    } else if (xform_updated) {
        e->dirty |= 3;                                   /* picked up by the re-tile's full image */
    }
    return CLAPGPU_OK;
}

/* what the call above will touch for (handle, slot), asked for ahead of time: the mirror's own record and the three rows of
 * the upload image -- four cache lines nothing else would bring in before the call stalls on each in turn */
void clapgpu_scene_entity_xform_prefetch(const clapgpu_scene *s, uint32_t handle, uint32_t slot)
{
    if (!s || handle >= s->n_handles) return;
    __builtin_prefetch(&s->e[handle], 1, 1);
    if (s->topology_dirty || !s->h_in || slot >= s->n_slots) return;
    __builtin_prefetch(s->h_pos_scale + 4 * (size_t)slot, 1, 1);
    __builtin_prefetch(s->h_rot + 4 * (size_t)slot, 1, 1);
    __builtin_prefetch(s->h_flags + slot, 1, 1);
}

void clapgpu_scene_mark_all_dirty(clapgpu_scene *s) { if (s) s->bulk_dirty = 1; }

int clapgpu_scene_entity_rotation(clapgpu_scene *s, uint32_t handle, const float q[4])
{
    struct ent *e = get(s, handle);
    if (!e || !q) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    memcpy(e->rot, q, 16);
    mark_dirty(s, handle, 1);
    return CLAPGPU_OK;
}

int clapgpu_scene_entity_move(clapgpu_scene *s, uint32_t handle, const float off[3])
{
    struct ent *e = get(s, handle);
    if (!e || !off) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    for (int i = 0; i < 3; i++)                             /* transform_move: vec3_add(pos, pos, off) */
        e->pos_scale[i] = e->pos_scale[i] + off[i];
    mark_dirty(s, handle, 1);
    return CLAPGPU_OK;
}

/* transform_set_angles (transform.c:62-73): clamp_radians / clamp_degrees + to_radians (util.h:77-95),
 * then quat_from_euler_xyz (linmath.h:857-870) with the host's sinf / cosf, like the reference */
void clapgpu_quat_from_angles(const float angles[3], int degrees, float q[4])
{
    float r[3];
    for (int i = 0; i < 3; i++) {
        float a = angles[i];
        if (degrees) {
            a = fabsf(a) <= 180.0 ? a : (a - copysignf(360.0, a));
            a = a * M_PI / 180.0;
        } else {
            a = fabsf(a) <= M_PI ? a : (a - copysignf(M_PI * 2.0, a));
        }
        r[i] = a;
    }
    float cx = cosf(r[0] * 0.5f), sx = sinf(r[0] * 0.5f);
    float cy = cosf(r[1] * 0.5f), sy = sinf(r[1] * 0.5f);
    float cz = cosf(r[2] * 0.5f), sz = sinf(r[2] * 0.5f);
    q[0] = sx * cy * cz - cx * sy * sz;
    q[1] = cx * sy * cz + sx * cy * sz;
    q[2] = cx * cy * sz - sx * sy * cz;
    q[3] = cx * cy * cz + sx * sy * sz;
}

int clapgpu_scene_entity_rotate(clapgpu_scene *s, uint32_t handle, float rx, float ry, float rz)
{
    struct ent *e = get(s, handle);
    if (!e) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    const float angles[3] = { rx, ry, rz };
    clapgpu_quat_from_angles(angles, 0, e->rot);            /* entity3d_rotate: radians (model.c:1818-1821) */
    mark_dirty(s, handle, 1);
    return CLAPGPU_OK;
}

int clapgpu_scene_entity_visible(clapgpu_scene *s, uint32_t handle, unsigned int visible)
{
    return clapgpu_scene_entity_flags(s, handle, visible ? CLAPGPU_E_VISIBLE : 0, visible ? 0 : CLAPGPU_E_VISIBLE);
}

int clapgpu_scene_entity_scale(clapgpu_scene *s, uint32_t handle, float scale)
{
    struct ent *e = get(s, handle);
    if (!e) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    e->pos_scale[3] = scale;
    mark_dirty(s, handle, 1);
    return CLAPGPU_OK;
}

int clapgpu_scene_entity_flags(clapgpu_scene *s, uint32_t handle, uint32_t set, uint32_t clear)
{
    struct ent *e = get(s, handle);
    if (!e) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    e->flags = ((e->flags | set) & ~clear) & ~CLAPGPU_E_DIRTY;
    mark_dirty(s, handle, 0);                           /* flags upload only: entity3d_visible() does not touch xform */
    return CLAPGPU_OK;
}

int clapgpu_scene_entity_set_attach(clapgpu_scene *s, uint32_t handle, int attached)
{
    struct ent *e = get(s, handle);
    if (!e) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (e->attached != (attached ? 1 : 0)) {
        e->attached = attached ? 1 : 0;
        s->topology_dirty = 1;                           /* the flag travels with the upload image */
    }
    return CLAPGPU_OK;
}

/* ---------------------------------------------------------------- results */
/* under EXPORT_DRAWN a row nobody has read since it was rebuilt is fetched by the first accessor that asks for it */
#define RESULT(field, stride)                                                        \
    const struct ent *e = get(s, handle);                                            \
    if (e && s->n_stale_words && clapgpu_scene_fetch_entity((clapgpu_scene *)s, handle)) return NULL; \
    return (e && s->have_results && e->slot < s->n_slots) ? s->field + (stride) * (size_t)e->slot : NULL

const float *clapgpu_scene_entity_mx(const clapgpu_scene *s, uint32_t handle)          { RESULT(h_mx, 16); }
const float *clapgpu_scene_entity_inverse_mx(const clapgpu_scene *s, uint32_t handle)  { RESULT(h_inv, 16); }
const float *clapgpu_scene_entity_aabb(const clapgpu_scene *s, uint32_t handle)        { RESULT(h_aabb, 6); }
const float *clapgpu_scene_entity_aabb_center(const clapgpu_scene *s, uint32_t handle) { RESULT(h_center, 3); }

int clapgpu_scene_entity_in_frustum(const clapgpu_scene *s, uint32_t handle)
{
    const struct ent *e = get(s, handle);
    if (!e || !s->have_results || e->slot >= s->n_slots) return 0;
    return (int)((s->h_mask[e->slot >> 6] >> (e->slot & 63)) & 1);
}

void *clapgpu_scene_entity_user(const clapgpu_scene *s, uint32_t handle)
{
    const struct ent *e = get(s, handle);
    return e ? e->user : NULL;
}

uint32_t clapgpu_scene_visible(const clapgpu_scene *s, uint32_t *handles, uint32_t capacity)
{
    uint32_t cnt = 0;
    if (!s || !s->have_results) return 0;
    for (uint32_t w = 0; w < s->n_slots / 64; w++) {
        uint64_t m = s->h_mask[w];
        while (m) {
            const uint32_t bit = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            if (handles && cnt < capacity) handles[cnt] = s->slot_handle[w * 64 + bit];
            cnt++;
        }
    }
    return cnt;
}

uint32_t clapgpu_scene_entity_slot(const clapgpu_scene *s, uint32_t handle)
{
    const struct ent *e = get(s, handle);
    return (e && e->slot < s->n_slots) ? e->slot : CLAPGPU_NO_ENTITY;
}

int clapgpu_scene_results(const clapgpu_scene *s, clapgpu_scene_arrays *out)
{
    if (!s || !out || !s->have_results) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    out->n_slots = s->n_slots;
    out->mx = s->h_mx; out->inverse_mx = s->h_inv; out->aabb = s->h_aabb; out->aabb_center = s->h_center;
    out->vis_mask = s->h_mask; out->rebuilt_mask = s->h_rebuilt; out->inside_mask = s->h_inside;
    out->slot_user = (void *const *)s->slot_user;
    out->exported_mask = (s->zero_copy && s->tiled) ? s->h_exported : s->h_rebuilt;
    out->stale_mask = s->h_stale; out->fetched_mask = s->h_fetched;
    out->n_stale_words = s->n_stale_words; out->n_fetched = s->n_fetched; out->fetch_serial = s->fetch_serial;
    out->n_views = s->xv.n;
    for (uint32_t v = 0; v < CLAPGPU_EXTRA_VIEWS_MAX; v++) out->view_mask[v] = v < s->xv.n ? s->h_xv_mask[v] : NULL;
    return CLAPGPU_OK;
}

void clapgpu_scene_set_export(clapgpu_scene *s, int policy)
{
    if (s) s->export_drawn = policy == CLAPGPU_SCENE_EXPORT_DRAWN;
}

int clapgpu_scene_export_is_drawn(const clapgpu_scene *s) { return s && s->export_drawn && s->zero_copy && s->tiled; }

int clapgpu_scene_entity_keep(clapgpu_scene *s, uint32_t handle, int keep)
{
    struct ent *e = get(s, handle);
    if (!e) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (e->keep == (keep ? 1 : 0)) return CLAPGPU_OK;
    e->keep = keep ? 1 : 0;
    if (!s->topology_dirty && s->h_keep && e->slot < s->n_slots) {   /* else the re-tile lays the bits out */
        if (keep) s->h_keep[e->slot >> 6] |= 1ull << (e->slot & 63);
        else s->h_keep[e->slot >> 6] &= ~(1ull << (e->slot & 63));
        s->keep_dirty = 1;
    }
    return CLAPGPU_OK;
}

int clapgpu_scene_fetch(clapgpu_scene *s, const uint64_t *want, uint32_t *n_rows)
{
    if (!s) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (n_rows) *n_rows = 0;
    if (!s->have_results || s->topology_dirty) return s->n_stale_words ? CLAPGPU_ERR_NOT_SUPPORTED : CLAPGPU_OK;
    CK(mirror_fetch_rows(s, want, NULL, NULL));
    if (n_rows) *n_rows = s->n_fetched;
    return CLAPGPU_OK;
}

int clapgpu_scene_fetch_entity(clapgpu_scene *s, uint32_t handle)
{
    const struct ent *e = get(s, handle);
    if (!e) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!s->n_stale_words || e->slot >= s->n_slots || !((s->h_stale[e->slot >> 6] >> (e->slot & 63)) & 1)) return CLAPGPU_OK;
    if (!s->have_results || s->topology_dirty) return CLAPGPU_ERR_NOT_SUPPORTED;
    /* one row: a one-bit `want` (n / 64 words, zeroed) beside a device round trip */
    const size_t words = s->n_slots / 64;
    uint64_t *want = calloc(words ? words : 1, 8);
    if (!want) return CLAPGPU_ERR_NOMEM;
    want[e->slot >> 6] = 1ull << (e->slot & 63);
    const int rc = mirror_fetch_rows(s, want, NULL, NULL);
    free(want);
    return rc;
}

void clapgpu_scene_set_bv_points(clapgpu_scene *s, const float cam_pos[3], const float *ctl_pos, uint32_t ctl_handle)
{
    if (!s) return;
    s->bv_on = cam_pos != NULL;
    if (cam_pos) memcpy(s->bv_cam, cam_pos, 12);
    s->bv_has_ctl = ctl_pos != NULL;
    if (ctl_pos) memcpy(s->bv_ctl, ctl_pos, 12);
    s->bv_ctl_handle = ctl_handle;
}
