/*
 * clapgpu_scene_layout.c -- the host mirror's slot layout (see clapgpu_scene_internal.h): the slabs' capacity, the re-tile
 * (depths, widths, packing, slots, upload image: C counterpart of clap_amd/tiler.py) and the edits that change a standing
 * layout in place.
 */
#include "clapgpu_scene_internal.h"

void clapgpu_scene_set_parallel_for(clapgpu_scene *s, clapgpu_scene_parallel_for fn, int threads)
{
    if (!s) return;
    s->par_for = threads > 1 ? fn : NULL;
    s->par_threads = threads;
}

/* a pass over [0, n) on the caller's pool, or right here */
static void run_ranges(const clapgpu_scene *s, void (*fn)(void *, uint32_t, uint32_t), void *ctx, uint32_t n)
{
    static uint32_t par_min;
    if (!par_min) {
        const char *v = getenv("CLAPGPU_SCENE_PAR_MIN");         /* tuning knob; the tests set 1 */
        par_min = v && atoi(v) > 0 ? (uint32_t)atoi(v) : 16384u;
    }
    if (s->par_for && n >= par_min) s->par_for(fn, ctx, n, s->par_threads);
    else fn(ctx, 0, n);
}

void clapgpu_scene_set_incremental(clapgpu_scene *s, int on)
{
    if (s) s->incremental = on != 0;                     /* from the next re-tile on */
}

int clapgpu_scene_layout_is_tiled(const clapgpu_scene *s) { return s ? s->tiled : 0; }
uint32_t clapgpu_scene_slot_count(const clapgpu_scene *s) { return s ? s->n_slots : 0; }
uint32_t clapgpu_scene_layout_generation(const clapgpu_scene *s) { return s ? s->layout_gen : 0; }

/* before a re-tile: orphans of the entities deleted since the last one become roots, their handles reusable */
static int release_dead(clapgpu_scene *s)
{
    if (!s->n_dead) return CLAPGPU_OK;
    for (uint32_t h = 0; h < s->n_handles; h++) {
        struct ent *c = &s->e[h];
        if (c->live && c->parent != CLAPGPU_NO_ENTITY && !(c->parent < s->n_handles && s->e[c->parent].live))
            c->parent = CLAPGPU_NO_ENTITY;
    }
    return mirror_release_handles(s, s->dead_list, &s->n_dead);
}

static int ensure_slots(clapgpu_scene *s, uint32_t n_slots)
{
    if (n_slots <= s->cap_slots) return CLAPGPU_OK;
    /* an eighth of head room, in 4096-slot steps: the slabs cross PCIe whole, so capacity is traffic */
    uint32_t cap = (n_slots + n_slots / 8 + 4095u) & ~4095u;
    size_t n = cap;                                     /* a multiple of 64: every sub-array below starts 16-B aligned */
#define RE(p, bytes) do { void *q__ = realloc(p, bytes); if (!q__) return CLAPGPU_ERR_NOMEM; p = q__; } while (0)
    RE(s->slot_handle, n * 4); RE(s->slot_user, n * sizeof(void *));
#undef RE
    /* mirror_retile() rewrites the upload image in full and downloads are overwritten by the next frame, so
     * nothing has to survive the growth */
    mirror_free_device(s);
    if (s->h_in) clapgpu_host_free(s->h_in);
    if (s->h_out) clapgpu_host_free(s->h_out);
    s->h_in = s->h_out = NULL;
    /* page-locked: the small copies that carry an in-place edit's parent / model index are then queued, not staged and waited for */
    if (s->h_parent) clapgpu_host_free(s->h_parent);
    if (s->h_model) clapgpu_host_free(s->h_model);
    s->h_parent = s->h_model = NULL;
    CK(clapgpu_host_malloc((void **)&s->h_parent, n * 4));
    CK(clapgpu_host_malloc((void **)&s->h_model, n * 4));
    s->models_dirty = 1;                                /* mirror_free_device() dropped d.model_table */
    s->have_results = 0;
    s->in_bytes = in_slab_bytes(n);
    s->out_bytes = out_slab_bytes(n);
    s->zero_copy = cap <= s->zero_copy_max_slots;
    if (s->zero_copy) CK(clapgpu_host_malloc_mapped(&s->h_in, &s->d_in_host, s->in_bytes));
    else CK(clapgpu_host_malloc(&s->h_in, s->in_bytes));
    if (s->zero_copy) {
        CK(clapgpu_host_malloc_mapped(&s->h_out, &s->d_out_host, s->out_bytes));
        memset(s->h_out, 0, s->out_bytes);
        if (!s->h_done) {
            void *dd = NULL;
            CK(clapgpu_host_malloc_mapped((void **)&s->h_done, &dd, 64));
            s->d_done = dd;
            *s->h_done = 0;
            CK(clapgpu_malloc((void **)&s->d_counter, 4));
            CK(clapgpu_memset(s->d_counter, 0, 4, NULL));
        }
    } else {
        CK(clapgpu_host_malloc(&s->h_out, s->out_bytes));
    }
    CK(clapgpu_malloc(&s->d_in, s->in_bytes));
    CK(clapgpu_malloc(&s->d_out, s->out_bytes));
    const struct in_slab hi = in_slab_at(s->h_in, n), di = in_slab_at(s->d_in, n);
    const struct out_slab ho = out_slab_at(s->h_out, n), dq = out_slab_at(s->d_out, n);
    s->h_pos_scale = hi.pos_scale; s->h_rot = hi.rot; s->h_flags = hi.flags; s->h_touched = hi.touched;
    s->d.pos_scale = di.pos_scale; s->d.rot = di.rot; s->d.flags = di.flags;
    s->h_mx = ho.mx; s->h_inv = ho.inv; s->h_aabb = ho.aabb; s->h_center = ho.center;
    s->h_mask = ho.vis; s->h_rebuilt = ho.rebuilt; s->h_inside = ho.inside; s->h_exported = ho.exported;
    s->d.mx = dq.mx; s->d.inv_mx = dq.inv; s->d.aabb = dq.aabb; s->d.center = dq.center;
    s->d.vis_mask = dq.vis; s->d.rebuilt_mask = dq.rebuilt; s->bvq.inside_mask = dq.inside;
    const size_t mw = mask_stride(n), rows = n / WAVE;
    memset(s->h_touched, 0, mw * 8);
    if (s->d_keep) clapgpu_free(s->d_keep);
    if (s->h_select) clapgpu_host_free(s->h_select);
    s->d_keep = NULL; s->h_select = NULL; s->d_select = NULL;
    free(s->h_keep); free(s->h_stale); free(s->h_fetched);
    s->h_keep = calloc(mw, 8); s->h_stale = calloc(mw, 8); s->h_fetched = calloc(mw, 8);
    if (!s->h_keep || !s->h_stale || !s->h_fetched) return CLAPGPU_ERR_NOMEM;
    CK(clapgpu_malloc((void **)&s->d_keep, mw * 8));
    if (s->d_stale) clapgpu_free(s->d_stale);
    s->d_stale = NULL;
    CK(clapgpu_malloc((void **)&s->d_stale, mw * 8));
    CK(clapgpu_memset(s->d_stale, 0, mw * 8, NULL));
    if (s->zero_copy) CK(clapgpu_host_malloc_mapped((void **)&s->h_select, &s->d_select, mw * 8));
    s->n_stale_words = 0; s->n_fetched = 0; s->keep_dirty = 1;
    void **dp[] = { (void **)&s->d.parent, (void **)&s->d.model, (void **)&s->d.seqs, (void **)&s->d.vis_row_pop,
                    (void **)&s->d_tile_row_start };
    size_t sz[] = { n * 4, n * 4, n * 4, (rows + 16) / 16 * 16, (rows + 2) * 4 };     /* (at most a tile per row, and the end) */
    for (unsigned i = 0; i < sizeof(dp) / sizeof(dp[0]); i++)
        CK(clapgpu_malloc(dp[i], sz[i]));
    s->cap_slots = cap;
    return CLAPGPU_OK;
}

/* depth of every live entity under its root; returns max depth + 1, or 0 on a parent cycle.  Each range walks up from its
 * handles to the first ancestor whose depth is known and assigns the chain; ranges that meet on a chain write the same values
 * (root before depth, depth with release: whoever reads a depth finds its root). */
#define DEPTH_UNK 0xffffffffu
struct depth_ctx { clapgpu_scene *s; uint32_t *depth, *root; uint32_t maxd; int cycle; };
static void depths_range(void *ctx, uint32_t lo, uint32_t hi)
{
    struct depth_ctx *dc = ctx;
    clapgpu_scene *s = dc->s;
    uint32_t *depth = dc->depth, *root = dc->root, maxd = 0;
    for (uint32_t h = lo; h < hi; h++) {
        if (!s->e[h].live || __atomic_load_n(&depth[h], __ATOMIC_ACQUIRE) != DEPTH_UNK) continue;
        uint32_t cur = h, len = 0;                       /* walk up to a known ancestor (or the root) */
        while (s->e[cur].parent != CLAPGPU_NO_ENTITY && __atomic_load_n(&depth[s->e[cur].parent], __ATOMIC_ACQUIRE) == DEPTH_UNK) {
            cur = s->e[cur].parent;
            if (++len > s->n_handles) { __atomic_store_n(&dc->cycle, 1, __ATOMIC_RELAXED); return; }
        }
        uint32_t base_d, base_r;
        if (s->e[cur].parent == CLAPGPU_NO_ENTITY) { base_d = 0; base_r = cur; }
        else { base_d = __atomic_load_n(&depth[s->e[cur].parent], __ATOMIC_ACQUIRE) + 1; base_r = __atomic_load_n(&root[s->e[cur].parent], __ATOMIC_RELAXED); }
        uint32_t x = h;
        for (uint32_t k = 0; k <= len; k++) {
            const uint32_t d = base_d + (len - k);
            __atomic_store_n(&root[x], base_r, __ATOMIC_RELAXED);
            __atomic_store_n(&depth[x], d, __ATOMIC_RELEASE);
            if (d + 1 > maxd) maxd = d + 1;
            x = s->e[x].parent;
        }
    }
    uint32_t seen = __atomic_load_n(&dc->maxd, __ATOMIC_RELAXED);
    while (maxd > seen && !__atomic_compare_exchange_n(&dc->maxd, &seen, maxd, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) { }
}

static uint32_t compute_depths(clapgpu_scene *s, uint32_t *depth, uint32_t *root)
{
    memset(depth, 0xff, (size_t)s->n_handles * 4);
    struct depth_ctx dc = { s, depth, root, 0, 0 };
    run_ranges(s, depths_range, &dc, s->n_handles);
    if (dc.cycle) return 0;
    return dc.maxd ? dc.maxd : 1;
}

/* the re-tile's other passes over every handle / slot */
struct retile_ctx {
    clapgpu_scene *s; const uint32_t *depth, *root, *tree_of; uint32_t *width; uint32_t maxd; int wide;
};
static void widths_range(void *ctx, uint32_t lo, uint32_t hi)
{
    struct retile_ctx *rc = ctx;
    const clapgpu_scene *s = rc->s;
    for (uint32_t h = lo; h < hi; h++)
        if (s->e[h].live) {
            const uint32_t t = rc->tree_of[rc->root[h]];
            if (__atomic_add_fetch(&rc->width[(size_t)t * rc->maxd + rc->depth[h]], 1, __ATOMIC_RELAXED) > WAVE)
                __atomic_store_n(&rc->wide, 1, __ATOMIC_RELAXED);
        }
}

static void image_range(void *ctx, uint32_t lo, uint32_t hi)      /* in units of 64 slots: a range owns its words of h_keep */
{
    struct retile_ctx *rc = ctx;
    clapgpu_scene *s = rc->s;
    for (uint32_t i = lo * WAVE; i < hi * WAVE; i++) {
        const uint32_t h = s->slot_handle[i];
        s->slot_user[i] = h == CLAPGPU_NO_ENTITY ? NULL : s->e[h].user;
        if (h != CLAPGPU_NO_ENTITY && s->e[h].keep) s->h_keep[i >> 6] |= 1ull << (i & 63);
        if (h == CLAPGPU_NO_ENTITY) {
            const float id[4] = { 0, 0, 0, 1 };
            memcpy(s->h_pos_scale + 4 * (size_t)i, id, 16);
            memcpy(s->h_rot + 4 * (size_t)i, id, 16);
            s->h_parent[i] = -1; s->h_model[i] = 0; s->h_flags[i] = 0;
            continue;
        }
        const struct ent *e = &s->e[h];
        memcpy(s->h_pos_scale + 4 * (size_t)i, e->pos_scale, 16);
        memcpy(s->h_rot + 4 * (size_t)i, e->rot, 16);
        s->h_parent[i] = e->parent == CLAPGPU_NO_ENTITY ? -1 : (int32_t)s->e[e->parent].slot;
        s->h_model[i] = (int32_t)e->model;
        s->h_flags[i] = img_flags(e, 1);                             /* everything is rebuilt after a re-tile */
    }
}

/* Slots in HANDLE order inside each row, as one thread would give them, from passes that have no order in them: the handles
 * are cut into chunks; every chunk counts its entities per row (or per level), a pass over the rows turns the counts into
 * each chunk's first lane, and every chunk then hands out its lanes in handle order. */
static uint32_t rt_chunk(void)                                    /* handles per chunk (CLAPGPU_SCENE_RT_CHUNK: the tests set a few hundred) */
{
    static uint32_t v;
    if (!v) { const char *e = getenv("CLAPGPU_SCENE_RT_CHUNK"); v = e && atoi(e) > 0 ? (uint32_t)atoi(e) : 16384u; }
    return v;
}
struct slots_ctx {
    clapgpu_scene *s; const uint32_t *depth, *root, *tree_of, *row_of_tree; uint32_t *cnt; uint32_t n_cells, n_chunks, H, chunk; int tiled;
};
static inline uint32_t slots_cell(const struct slots_ctx *sc, uint32_t h)
{
    return sc->tiled ? sc->row_of_tree[sc->tree_of[sc->root[h]]] + sc->depth[h] : sc->s->level_start_host[sc->depth[h]] / WAVE;
}

static void slots_count_range(void *ctx, uint32_t lo, uint32_t hi)      /* in chunks */
{
    struct slots_ctx *sc = ctx;
    for (uint32_t c = lo; c < hi; c++) {
        uint32_t *cnt = sc->cnt + (size_t)c * sc->n_cells;
        const uint32_t h1 = (c + 1) * sc->chunk < sc->H ? (c + 1) * sc->chunk : sc->H;
        for (uint32_t h = c * sc->chunk; h < h1; h++)
            if (sc->s->e[h].live) cnt[slots_cell(sc, h)]++;
    }
}

static void slots_first_range(void *ctx, uint32_t lo, uint32_t hi)      /* in cells */
{
    struct slots_ctx *sc = ctx;
    for (uint32_t cell = lo; cell < hi; cell++) {
        uint32_t run = 0;
        for (uint32_t c = 0; c < sc->n_chunks; c++) {
            uint32_t *p = sc->cnt + (size_t)c * sc->n_cells + cell;
            const uint32_t t = *p;
            *p = run; run += t;
        }
    }
}

static void slots_assign_range(void *ctx, uint32_t lo, uint32_t hi)     /* in chunks */
{
    struct slots_ctx *sc = ctx;
    clapgpu_scene *s = sc->s;
    for (uint32_t c = lo; c < hi; c++) {
        uint32_t *cnt = sc->cnt + (size_t)c * sc->n_cells;
        const uint32_t h1 = (c + 1) * sc->chunk < sc->H ? (c + 1) * sc->chunk : sc->H;
        for (uint32_t h = c * sc->chunk; h < h1; h++) {
            if (!s->e[h].live) continue;
            const uint32_t cell = slots_cell(sc, h);
            const uint32_t k = cnt[cell]++;
            s->e[h].slot = (sc->tiled ? cell * WAVE : s->level_start_host[sc->depth[h]]) + k;
            s->slot_handle[s->e[h].slot] = h;
        }
    }
}

static void undirty_range(void *ctx, uint32_t lo, uint32_t hi)
{
    clapgpu_scene *s = ctx;
    for (uint32_t h = lo; h < hi; h++) s->e[h].dirty = 0;
}

int mirror_retile(clapgpu_scene *s)
{
    const int timing = s->timing;
    double tp[8] = { 0 };
    tp[0] = timing ? scene_now_us() : 0;
    CK(release_dead(s));
    if (s->h_in)                                         /* tombstones of in-place deletions: the whole image follows anyway */
        for (uint32_t k = 0; k < s->n_raw; k++) s->h_touched[s->raw_words[k]] = 0;
    const uint32_t H = s->n_handles;
    uint32_t *depth = malloc(((size_t)H + 1) * 4), *root = malloc(((size_t)H + 1) * 4);
    uint32_t *tree_of = malloc(((size_t)H + 1) * 4);
    if (!depth || !root || !tree_of) return CLAPGPU_ERR_NOMEM;
    uint32_t maxd = compute_depths(s, depth, root);
    if (!maxd) { free(depth); free(root); free(tree_of); return CLAPGPU_ERR_INVALID_ARGUMENTS; }
    if (timing) tp[1] = scene_now_us();

    uint32_t n_trees = 0, n_live = 0;
    for (uint32_t h = 0; h < H; h++)
        if (s->e[h].live) { n_live++; if (s->e[h].parent == CLAPGPU_NO_ENTITY) tree_of[h] = n_trees++; }
    uint32_t *width = calloc((size_t)(n_trees ? n_trees : 1) * maxd, 4);
    if (!width) return CLAPGPU_ERR_NOMEM;
    struct retile_ctx rtc = { s, depth, root, tree_of, width, maxd, 0 };
    run_ranges(s, widths_range, &rtc, H);
    int tiled = !rtc.wide;

    uint32_t n_rows = 0;
    uint32_t *row_of_tree = malloc(((size_t)n_trees + 1) * 4);       /* first row of the tree's tile */
    uint32_t *row_fill = NULL;
    free(s->tile_row_start_host);
    free(s->level_start_host);
    s->tile_row_start_host = malloc(((size_t)n_trees + 2) * 4);      /* at most one tile per tree */
    s->cap_tiles = n_trees + 1;
    s->max_depth = maxd; s->grow_tile = CLAPGPU_NO_ENTITY; s->n_free_roots = 0;
    s->n_raw = 0; s->n_edits = 0; s->grown_from = s->tiles_from = CLAPGPU_NO_ENTITY;
    /* a mirror that is edited in place (clapgpu_scene_set_incremental) leaves every row an eighth of its lanes and every tile
     * of a hierarchy one row: room for the children that come before the next re-tile */
    const uint32_t row_limit = s->incremental ? WAVE - WAVE / 8 : WAVE;
    const uint32_t spare_rows = (s->incremental && maxd > 1) ? 1 : 0;
    s->level_start_host = malloc(((size_t)maxd + 2) * 4);
    if (!row_of_tree || !s->tile_row_start_host || !s->level_start_host) return CLAPGPU_ERR_NOMEM;
    if (tiled) {
        /* next-fit packing of whole trees: every level of a tile holds <= 64 entities */
        uint32_t *fill = calloc(maxd, 4);
        uint32_t tile_first_row = 0, tile_rows = 0;
        s->n_tiles = 0;
        for (uint32_t t = 0; t < n_trees; t++) {
            const uint32_t *w = width + (size_t)t * maxd;
            int fits = 1;
            uint32_t rows = 0;
            for (uint32_t d = 0; d < maxd; d++) { if (fill[d] && fill[d] + w[d] > row_limit) fits = 0; if (w[d]) rows = d + 1; }
            if (!fits) {                                            /* close the tile */
                s->tile_row_start_host[s->n_tiles++] = tile_first_row;
                tile_first_row += tile_rows + spare_rows;
                tile_rows = 0;
                memset(fill, 0, maxd * 4);
            }
            for (uint32_t d = 0; d < maxd; d++) fill[d] += w[d];
            if (rows > tile_rows) tile_rows = rows;
            row_of_tree[t] = tile_first_row;
        }
        if (n_trees) { s->tile_row_start_host[s->n_tiles++] = tile_first_row; tile_first_row += tile_rows + spare_rows; }
        s->tile_row_start_host[s->n_tiles] = tile_first_row;
        n_rows = tile_first_row;
        free(fill);
    } else {
        /* level-major: level d = rows [level_row[d], level_row[d+1]) */
        uint32_t *cnt = calloc(maxd, 4);
        for (uint32_t h = 0; h < H; h++) if (s->e[h].live) cnt[depth[h]]++;
        s->n_levels = maxd;
        uint32_t r = 0;
        for (uint32_t d = 0; d < maxd; d++) { s->level_start_host[d] = r * WAVE; r += (cnt[d] + WAVE - 1) / WAVE; }
        s->level_start_host[maxd] = r * WAVE;
        n_rows = r;
        free(cnt);
    }
    if (n_rows == 0) n_rows = 1;
    if (timing) tp[2] = scene_now_us();
    int rc = ensure_slots(s, n_rows * WAVE);
    if (rc) return rc;
    s->n_rows = n_rows;
    s->n_slots = n_rows * WAVE;
    s->tiled = tiled;
    if (!tiled) s->level_start_host[s->n_levels] = s->n_slots;      /* the kernel wants the last start == n */

    /* slots: handle order inside each row */
    if (timing) tp[3] = scene_now_us();
    memset(s->slot_handle, 0xff, (size_t)s->n_slots * 4);          /* CLAPGPU_NO_ENTITY */
    const uint32_t chunk = rt_chunk(), n_chunks = (H + chunk - 1) / chunk;
    uint32_t *chunk_cnt = (s->par_for && n_chunks > 1 && (uint64_t)n_chunks * n_rows <= (64u << 20)) ? calloc((size_t)n_chunks * n_rows, 4) : NULL;
    if (chunk_cnt) {
        struct slots_ctx sc = { s, depth, root, tree_of, row_of_tree, chunk_cnt, n_rows, n_chunks, H, chunk, tiled };
        s->par_for(slots_count_range, &sc, n_chunks, s->par_threads);
        run_ranges(s, slots_first_range, &sc, n_rows);
        s->par_for(slots_assign_range, &sc, n_chunks, s->par_threads);
        free(chunk_cnt);
    } else {
    row_fill = calloc(n_rows, 4);
    for (uint32_t h = 0; h < H; h++) {
        if (!s->e[h].live) continue;
        uint32_t row;
        if (tiled) {
            row = row_of_tree[tree_of[root[h]]] + depth[h];
            s->e[h].slot = row * WAVE + row_fill[row]++;
        } else {
            uint32_t base = s->level_start_host[depth[h]] / WAVE;
            uint32_t k = row_fill[base]++;                           /* counter kept in the level's first row */
            s->e[h].slot = s->level_start_host[depth[h]] + k;
        }
        s->slot_handle[s->e[h].slot] = h;
    }
    }
    /* the slots moved: what was stale under the old layout is rebuilt (and exported or marked stale again) by the launch
     * that follows; the standing readers' bits are laid out anew */
    if (timing) tp[4] = scene_now_us();
    const size_t mask_bytes = mask_stride(s->cap_slots) * 8;
    memset(s->h_stale, 0, mask_bytes);
    CK(clapgpu_memset(s->d_stale, 0, mask_bytes, NULL));
    memset(s->h_fetched, 0, mask_bytes);
    memset(s->h_keep, 0, mask_bytes);
    s->n_stale_words = 0; s->n_fetched = 0; s->keep_dirty = 1;
    /* full staging image */
    run_ranges(s, image_range, &rtc, s->n_slots / WAVE);
    free(depth); free(root); free(tree_of); free(width); free(row_of_tree); free(row_fill);
    if (timing) tp[5] = scene_now_us();

    s->d.n = s->n_slots;
    const size_t n = s->n_slots;
    CK(clapgpu_memcpy_h2d((void *)s->d.parent, s->h_parent, n * 4, NULL));
    CK(clapgpu_memcpy_h2d((void *)s->d.model, s->h_model, n * 4, NULL));
    CK(clapgpu_memset(s->d.seqs, 0, n * 4, NULL));
    CK(clapgpu_memset(s->d_out, 0, s->out_bytes, NULL));
    /* the host's result slab is NOT cleared here (at a million entities that alone was 15 ms of a re-tile): the launch that
     * follows rebuilds and exports every live row and writes every mask word of the layout; padding rows are never read
     * (no slot_user), and a box-less model's rows are never copied out.  It is zeroed once, where it is allocated. */
    if (tiled)
        CK(clapgpu_memcpy_h2d(s->d_tile_row_start, s->tile_row_start_host, ((size_t)s->n_tiles + 1) * 4, NULL));
    /* every live handle, not only the listed ones: an entity marked dirty while the list could not grow (mark_dirty's
     * out-of-memory path) would otherwise stay "queued" for ever and never be listed again */
    run_ranges(s, undirty_range, s, H);
    s->n_dirty = 0;
    s->topology_dirty = 0;
    s->up_lo = 0xffffffffu; s->up_hi = 0;
    s->layout_gen++;
    if (timing) {
        const double t_end = scene_now_us();
        uint64_t fnv = 1469598103934665603ull;                   /* the layout, for comparing runs (serial / on a pool) */
        for (uint32_t i = 0; i < s->n_slots; i++) fnv = (fnv ^ s->slot_handle[i]) * 1099511628211ull;
        fprintf(stderr, "retile: %u handles -> %u slots: depths %.0f us, trees + packing %.0f, slabs %.0f, slots %.0f, image %.0f, uploads %.0f; layout %016llx\n",
                H, s->n_slots, tp[1] - tp[0], tp[2] - tp[1], tp[3] - tp[2], tp[4] - tp[3], tp[5] - tp[4], t_end - tp[5], (unsigned long long)fnv);
    }
    return CLAPGPU_OK;
}

/* ---- the standing layout edited in place ---------------------------------------------------------------------------------
 * A queue that gains and loses a few entities a frame (pickups, projectiles, effects) would pay for a re-tile -- every
 * entity's depth, a new packing, the whole upload image, every slot moved under the caller -- each time.  These two verbs
 * edit the tile layout where it stands instead: a new root takes a free first-row lane (one a deleted root left, or one of
 * a growth tile appended behind the others), a new child a free lane of the row below its parent in the parent's own tile
 * (the kernel hands a parent's matrix to the next row through registers: that is the only place a child can be), a deleted
 * leaf becomes a lane that is not ALIVE.  No other entity moves: slots, masks and the caller's per-slot state stand.
 * Either verb returns CLAPGPU_ERR_NOT_SUPPORTED, having changed nothing, when the edit does not fit (no free lane, no row
 * below, out of capacity, a layout that is not the one-launch tile form): the caller then uses the plain verbs and the next
 * mq_update re-tiles.  The device is told with the next mq_update (the new lanes' inputs through the touched bits like any
 * moved entity's, parent / model indices by a small copy): until then results for such an entity are not defined. */
static int push_list(uint32_t **arr, uint32_t *n, uint32_t *cap, uint32_t v)
{
    CK(mirror_grow_list(arr, cap, *n + 1, 64));
    (*arr)[(*n)++] = v;
    return CLAPGPU_OK;
}

static int layout_editable(const clapgpu_scene *s)
{
    return !s->topology_dirty && s->tiled && s->zero_copy && s->have_results && s->h_in && s->n_tiles && s->n_models;
}

static uint32_t tile_of_row(const clapgpu_scene *s, uint32_t row)
{
    uint32_t lo = 0, hi = s->n_tiles;                    /* tile_row_start_host[lo] <= row < tile_row_start_host[hi] */
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s->tile_row_start_host[mid] <= row) lo = mid; else hi = mid;
    }
    return lo;
}

static int free_lane(const clapgpu_scene *s, uint32_t row)
{
    const uint32_t *sh = s->slot_handle + (size_t)row * WAVE;
    for (int l = 0; l < (int)WAVE; l++)
        if (sh[l] == CLAPGPU_NO_ENTITY) return l;
    return -1;
}

static void touch_raw(clapgpu_scene *s, uint32_t slot)
{
    s->h_touched[slot >> 6] |= 1ull << (slot & 63);
    if (!s->n_raw || slot < s->raw_lo) s->raw_lo = slot;
    if (!s->n_raw || slot + 1 > s->raw_hi) s->raw_hi = slot + 1;
    if (push_list(&s->raw_words, &s->n_raw, &s->cap_raw, slot >> 6))
        s->bulk_dirty = 1;                               /* cannot remember the word: the next frame clears them all */
}

/* a tile of max_depth (+ spare) empty rows behind the others; the device hears of it in mirror_apply_edits() */
static int append_tile(clapgpu_scene *s)
{
    const uint32_t rows = s->max_depth + ((s->incremental && s->max_depth > 1) ? 1 : 0);
    if (!rows || (uint64_t)(s->n_rows + rows) * WAVE > s->cap_slots) return CLAPGPU_ERR_NOT_SUPPORTED;
    if (s->n_tiles + 1 > s->cap_tiles) {
        const uint32_t cap = 2 * s->cap_tiles + 16;
        uint32_t *q = realloc(s->tile_row_start_host, ((size_t)cap + 1) * 4);
        if (!q) return CLAPGPU_ERR_NOMEM;
        s->tile_row_start_host = q; s->cap_tiles = cap;
    }
    const uint32_t first = s->n_slots, end = first + rows * WAVE;
    static const float id[4] = { 0, 0, 0, 1 };
    for (uint32_t i = first; i < end; i++) {
        s->slot_handle[i] = CLAPGPU_NO_ENTITY; s->slot_user[i] = NULL;
        memcpy(s->h_pos_scale + 4 * (size_t)i, id, 16);
        memcpy(s->h_rot + 4 * (size_t)i, id, 16);
        s->h_parent[i] = -1; s->h_model[i] = 0; s->h_flags[i] = 0;
    }
    if (s->lod_cap >= end && s->lod_layout_gen == s->layout_gen) {
        for (uint32_t i = first; i < end; i++) { s->h_force_lod[i] = -1; s->h_cur_lod[i] = 0; }
        if (first < s->lod_lo) s->lod_lo = first;
        if (end > s->lod_hi) s->lod_hi = end;
    }
    if (s->grown_from == CLAPGPU_NO_ENTITY) { s->grown_from = first; s->tiles_from = s->n_tiles; }
    s->grow_tile = s->n_tiles;
    s->tile_row_start_host[s->n_tiles] = s->n_rows;      /* (it was the end of the last tile already) */
    s->n_tiles++;
    s->n_rows += rows;
    s->tile_row_start_host[s->n_tiles] = s->n_rows;
    s->n_slots = s->n_rows * WAVE;
    return CLAPGPU_OK;
}

/* parent / model indices of the edited slots, and appended tiles, to the device: before anything is launched on the layout */
int mirror_apply_edits(clapgpu_scene *s)
{
    if (s->grown_from == CLAPGPU_NO_ENTITY && !s->n_edits) return CLAPGPU_OK;
    if (s->grown_from != CLAPGPU_NO_ENTITY) {
        const size_t a = s->grown_from, cnt = s->n_slots - a;
        CK(clapgpu_memcpy_h2d((int32_t *)s->d.parent + a, s->h_parent + a, cnt * 4, NULL));
        CK(clapgpu_memcpy_h2d((int32_t *)s->d.model + a, s->h_model + a, cnt * 4, NULL));
        CK(clapgpu_memset(s->d.flags + a, 0, cnt * 4, NULL));           /* nothing ALIVE there until the image says so */
        CK(clapgpu_memset(s->d.seqs + a, 0, cnt * 4, NULL));
        CK(clapgpu_memcpy_h2d(s->d_tile_row_start + s->tiles_from, s->tile_row_start_host + s->tiles_from,
                              ((size_t)s->n_tiles + 1 - s->tiles_from) * 4, NULL));
        s->d.n = s->n_slots;
        s->grown_from = s->tiles_from = CLAPGPU_NO_ENTITY;
    }
    if (s->n_edits) {
        /* the frame's edited lanes as one mapped list, one small launch (two copies and two fills each, queued one behind
         * the other in front of the update, cost a 10 k-entity frame 35 us).  zero_box: a model without a box (skip_aabb)
         * never writes one, so the lane's last tenant's must not stay (a fresh entity3d's is all zeros, and so is every
         * row after a re-tile) */
        if (s->n_edits > s->cap_place) {
            uint32_t cap = s->cap_place ? s->cap_place : 64;
            while (cap < s->n_edits) cap *= 2;
            if (s->h_place) clapgpu_host_free(s->h_place);
            s->h_place = NULL; s->cap_place = 0;
            CK(clapgpu_host_malloc_mapped((void **)&s->h_place, &s->d_place, (size_t)cap * sizeof(*s->h_place)));
            s->cap_place = cap;
        }
        for (uint32_t k = 0; k < s->n_edits; k++) {
            const uint32_t i = s->edits[k] & 0x3fffffffu;
            s->h_place[k] = (clapgpu_entity_place){ .slot = i, .parent = s->h_parent[i], .model = s->h_model[i],
                                                    .flags = ((s->edits[k] >> 31) ? CLAPGPU_PLACE_ZERO_BOX : 0) |
                                                             ((s->edits[k] & 0x40000000u) ? CLAPGPU_PLACE_CLEAR_STALE : 0) };
        }
        CK(clapgpu_entities_place(NULL, &s->d, (const clapgpu_entity_place *)s->d_place, s->n_edits, s->d_stale));
        s->n_edits = 0;
    }
    return CLAPGPU_OK;
}

int clapgpu_scene_entity_new_placed(clapgpu_scene *s, uint32_t model, void *user, uint32_t parent, uint32_t *handle, uint32_t *slot_out)
{
    if (!s || !handle || model >= s->n_models || (parent != CLAPGPU_NO_ENTITY && !get(s, parent))) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!layout_editable(s)) return CLAPGPU_ERR_NOT_SUPPORTED;
    uint32_t slot = CLAPGPU_NO_ENTITY;
    if (parent == CLAPGPU_NO_ENTITY) {
        while (s->n_free_roots && slot == CLAPGPU_NO_ENTITY) {
            const uint32_t c = s->free_roots[--s->n_free_roots];
            if (c < s->n_slots && s->slot_handle[c] == CLAPGPU_NO_ENTITY) slot = c;
        }
        if (slot == CLAPGPU_NO_ENTITY && s->grow_tile != CLAPGPU_NO_ENTITY) {
            const uint32_t row = s->tile_row_start_host[s->grow_tile];
            const int l = free_lane(s, row);
            if (l >= 0) slot = row * WAVE + (uint32_t)l;
        }
        if (slot == CLAPGPU_NO_ENTITY) {
            CK(append_tile(s));
            slot = s->tile_row_start_host[s->grow_tile] * WAVE;
        }
    } else {
        const struct ent *pe = &s->e[parent];
        if (pe->slot >= s->n_slots || pe->attached) return CLAPGPU_ERR_NOT_SUPPORTED;
        const uint32_t row = pe->slot / WAVE + 1, t = tile_of_row(s, row - 1);
        if (row >= s->tile_row_start_host[t + 1]) return CLAPGPU_ERR_NOT_SUPPORTED;     /* the parent sits in its tile's last row */
        const int l = free_lane(s, row);
        if (l < 0) return CLAPGPU_ERR_NOT_SUPPORTED;
        slot = row * WAVE + (uint32_t)l;
    }
    CK(mirror_grow_list(&s->edits, &s->cap_edits, s->n_edits + 1, 64));   /* before anything is changed: the list must be able to take the slot */
    const int32_t parent_slot = parent == CLAPGPU_NO_ENTITY ? -1 : (int32_t)s->e[parent].slot;
    CK(mirror_new_handle(s, model, user, handle));              /* (may move s->e) */
    struct ent *e = &s->e[*handle];
    e->slot = slot;
    e->parent = parent;
    if (parent != CLAPGPU_NO_ENTITY) s->e[parent].n_children++;
    s->slot_handle[slot] = *handle;
    s->slot_user[slot] = user;
    s->h_parent[slot] = parent_slot;
    s->h_model[slot] = (int32_t)model;
    if (!s->n_edits || slot < s->edit_lo) s->edit_lo = slot;
    if (!s->n_edits || slot + 1 > s->edit_hi) s->edit_hi = slot + 1;
    uint32_t skip_bits;
    memcpy(&skip_bits, &s->models[8 * (size_t)model + 3], 4);
    const uint64_t bit = 1ull << (slot & 63);
    int was_stale = 0;
    if (s->h_stale[slot >> 6] & bit) {
        s->h_stale[slot >> 6] &= ~bit;
        if (!s->h_stale[slot >> 6] && s->n_stale_words) s->n_stale_words--;
        was_stale = 1;                                   /* the device's twin follows with the frame's place list */
    }
    s->edits[s->n_edits++] = slot | (skip_bits ? 0x80000000u : 0) | (was_stale ? 0x40000000u : 0);
    if (s->h_keep[slot >> 6] & bit) { s->h_keep[slot >> 6] &= ~bit; s->keep_dirty = 1; }
    s->h_fetched[slot >> 6] &= ~bit;
    if (s->lod_cap > slot && s->lod_layout_gen == s->layout_gen) {
        s->h_force_lod[slot] = -1; s->h_cur_lod[slot] = 0;
        if (slot < s->lod_lo) s->lod_lo = slot;
        if (slot + 1 > s->lod_hi) s->lod_hi = slot + 1;
    }
    mark_dirty(s, *handle, 1);                           /* its inputs into the image; the launch takes them by the touched bit */
    if (slot_out) *slot_out = slot;
    return CLAPGPU_OK;
}

int clapgpu_scene_entity_delete_placed(clapgpu_scene *s, uint32_t handle)
{
    struct ent *e = get(s, handle);
    if (!e) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!layout_editable(s) || e->n_children || e->attached || e->slot >= s->n_slots) return CLAPGPU_ERR_NOT_SUPPORTED;
    CK(mirror_grow_list(&s->limbo, &s->cap_limbo, s->n_limbo + 1, 64));
    const uint32_t slot = e->slot;
    s->h_flags[slot] = 0;                                /* not ALIVE: never rebuilt, drawn or picked again */
    touch_raw(s, slot);
    s->slot_handle[slot] = CLAPGPU_NO_ENTITY;
    s->slot_user[slot] = NULL;
    const uint64_t bit = 1ull << (slot & 63);
    if (s->h_stale[slot >> 6] & bit) {
        s->h_stale[slot >> 6] &= ~bit;
        if (!s->h_stale[slot >> 6] && s->n_stale_words) s->n_stale_words--;
        /* the device's twin follows with the frame's place list (parent / model as they are) */
        if (push_list(&s->edits, &s->n_edits, &s->cap_edits, slot | 0x40000000u)) s->topology_dirty = 1;   /* (a re-tile clears both) */
    }
    if (s->h_keep[slot >> 6] & bit) { s->h_keep[slot >> 6] &= ~bit; s->keep_dirty = 1; }
    s->h_fetched[slot >> 6] &= ~bit;
    if (e->parent != CLAPGPU_NO_ENTITY && e->parent < s->n_handles && s->e[e->parent].live && s->e[e->parent].n_children)
        s->e[e->parent].n_children--;
    const uint32_t row = slot / WAVE;
    if (s->tile_row_start_host[tile_of_row(s, row)] == row)
        push_list(&s->free_roots, &s->n_free_roots, &s->cap_free_roots, slot);   /* (a failure only loses the lane until the next re-tile) */
    e->live = 0;
    s->limbo[s->n_limbo++] = handle;
    return CLAPGPU_OK;
}
