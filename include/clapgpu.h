/*
 * clapgpu.h -- C ABI of libclapgpu.so: the MI355X (gfx950) batch replacement for
 * the per-frame scene-update hot path of virtuoso/clap.
 *
 * Plain C, plain pointers and sizes.  All `dev` pointers are HIP device pointers
 * (from clapgpu_malloc, hipMalloc, or any allocator sharing the HIP context, e.g.
 * a torch tensor's data_ptr()); `stream` is a hipStream_t passed as void* (NULL =
 * the default stream).  Every function returns a cerr_enum-compatible int
 * (reference core/error.h:12-49): 0 = OK, negative = error; launches are
 * asynchronous on `stream` unless stated otherwise.
 *
 * Each entry point names the reference interface it replaces (file:line relative
 * to the reference tree).  INTEGRATION.md shows the binding a CLAP maintainer adds.
 *
 * Conventions (identical to oracle/clap_oracle.h):
 *   mat4  = float[16], column-major, (col c,row r) at [4c+r]  (linmath.h `mat4x4 M`, M[c][r])
 *   quat  = (x,y,z,w)                                          (linmath.h:835-840)
 */
#ifndef CLAPGPU_H
#define CLAPGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes: the subset of cerr_enum (error.h:12-49) this library returns ---- */
#define CLAPGPU_OK                      0
#define CLAPGPU_ERR_NOMEM              -1   /* _CERR_NOMEM */
#define CLAPGPU_ERR_INVALID_ARGUMENTS  -2   /* _CERR_INVALID_ARGUMENTS */
#define CLAPGPU_ERR_NOT_SUPPORTED      -3   /* _CERR_NOT_SUPPORTED */
#define CLAPGPU_ERR_TOO_LARGE         -11   /* _CERR_TOO_LARGE */
#define CLAPGPU_ERR_INIT_FAILED       -14   /* _CERR_INITIALIZATION_FAILED */
#define CLAPGPU_ERR_OUT_OF_BOUNDS     -26   /* _CERR_OUT_OF_BOUNDS */
#define CLAPGPU_ERR_UNKNOWN           -32   /* _CERR_UNKNOWN_ERROR (a HIP runtime error; see clapgpu_last_error) */

/* ---- entity3d_flags bits the path reads (model.h:293-312) + the dirty mirror ---- */
#define CLAPGPU_E_VISIBLE       (1u << 0)    /* ENTITY3D_VISIBLE */
#define CLAPGPU_E_SKIP_CULLING  (1u << 14)   /* ENTITY3D_SKIP_CULLING */
#define CLAPGPU_E_DIRTY         (1u << 16)   /* mirror of transform_t.updated (transform.h:11) */
#define CLAPGPU_E_JOINT_ATTACHED (1u << 17) /* e->parent_joint != JOINT_TYPE_MAX (model.h:386-403); see clapgpu_attach */
#define CLAPGPU_E_ALIVE         (1u << 31)   /* ENTITY3D_ALIVE */

/* ---- runtime ---- */
/* Number of HIP devices visible; <0 on error.  Does not create a context. */
int clapgpu_device_count(void);
/* Bind the calling thread to `device` (hipSetDevice) and verify it is a gfx950 part. */
int clapgpu_init(int device);
/* Text of the last HIP error seen by this library on the calling thread ("" if none). */
const char *clapgpu_last_error(void);
/* For the CALLERS' failure-path tests (oracle/ref/dropin.c `fail`, tests/test_dropin.py): after `launches` more kernel
 * launches have been checked, every later launch of this process reports a launch failure (the kernel itself runs;
 * the entry point returns CLAPGPU_ERR_UNKNOWN with clapgpu_last_error() set).  < 0 turns it off (the default).  Armed only
 * in a process started with CLAPGPU_TEST_HOOKS in its environment: anywhere else the call does nothing. */
void clapgpu_test_fail_after(int launches);
/* ABI version: bumped whenever a signature or struct below changes.  CLAPGPU_ABI_VERSION is the version this header
 * describes; a caller compares clapgpu_abi_version() of the library it loaded with it before any other call and refuses
 * anything else (an experiment build reports its version with the top bit set, so it is refused too). */
#define CLAPGPU_ABI_VERSION 53u
uint32_t clapgpu_abi_version(void);

int clapgpu_malloc(void **dev, size_t bytes);
int clapgpu_free(void *dev);
/* Page-locked host memory for the staging arrays of a binding: copies to and from it run at the
 * link rate and truly asynchronously (pageable memory is bounced through a driver buffer). */
int clapgpu_host_malloc(void **host, size_t bytes);
/* Page-locked host memory that kernels address directly (zero-copy over PCIe): *dev_alias is what goes into the
 * device-pointer fields of the structs below; free with clapgpu_host_free(*host).  Coherent: a kernel's stores are
 * visible to the host once the kernel has completed (or, inside a kernel, after __threadfence_system()).  For batches
 * small enough that the copies' fixed latencies (one each way + a blocking wait) exceed the transfer itself:
 * libclapgpu_scene uses it below ~128 k entities (clapgpu_entities_apply_inputs / _export_rebuilt). */
int clapgpu_host_malloc_mapped(void **host, void **dev_alias, size_t bytes);
int clapgpu_host_free(void *host);
int clapgpu_memcpy_h2d(void *dev, const void *host, size_t bytes, void *stream);
int clapgpu_memcpy_d2h(void *host, const void *dev, size_t bytes, void *stream);
int clapgpu_memset(void *dev, int value, size_t bytes, void *stream);
int clapgpu_stream_sync(void *stream);

/* ======================================================================== */
/* Entities: transform hierarchy -> inverse -> world AABB -> frustum cull    */
/* ======================================================================== */

/*
 * View frustum of the main subview: view.h:16-17 (`frustum_planes[6]`,
 * `frustum_corners[8]`), produced on the host by clapgpu_frustum_calc().
 */
typedef struct clapgpu_frustum {
    float planes[6][4];
    float corners[8][4];
} clapgpu_frustum;

/* transform.c:132-138 transform_view_mat4x4 (host, O(1) per frame) */
void clapgpu_view_matrix(const float pos[3], const float quat[4], float view_mx[16]);
/* linmath.h:611-651 mat4x4_invert, 959-987 mat4x4_from_quat (host; the arithmetic the kernels use) */
void clapgpu_mat4_invert(const float m[16], float out[16]);
void clapgpu_mat4_from_quat(const float quat_xyzw[4], float out[16]);
/* linmath.h:709-776 mat4x4_perspective_ndc_z_{2,1} via render-common.c:77-82 (host) */
void clapgpu_perspective(float fov, float aspect, float near_plane, float far_plane,
                         int ndc_z_zero_one, float proj_mx[16]);
/* view.c:248-289 subview_calc_frustum (host) */
void clapgpu_frustum_calc(const float view_mx[16], const float proj_mx[16],
                          int ndc_z_zero_one, clapgpu_frustum *out);

/*
 * SoA mirror of the entity3d fields on the path (model.h:372-429), all device
 * pointers, `n` entities.  Entities are stored so that parent[i] < i; a
 * "level" is a maximal index range whose parents all lie in earlier levels.
 * Level starts must be multiples of 64 (pad with flags == 0 entities) so that
 * each 64-entity wavefront owns exactly one vis_mask word.
 *
 *   inputs   pos_scale[n][4]  (pos.xyz, scale)       transform_t.pos, entity3d.scale
 *            rot[n][4]        quat xyzw              transform_t.rotation
 *            parent[n]        index or -1            entity3d.parent (jointless attach)
 *            model[n]         index into model_table entity3d.txmodel->model
 *            model_table[m][8]  (min.xyz, skip_aabb as uint32 bits, max.xyz,
 *                                lod_min | lod_max << 8 as uint32 bits)
 *                                                    model3d.aabb, .skip_aabb, .lod_min, .lod_max
 *   in/out   flags[n]         CLAPGPU_E_* bits       entity3d.flags + xform.updated
 *            seqs[n]          seq | parent_seq<<16   entity3d.seq / .parent_seq (uint16 wrap)
 *   outputs  mx[n][16], inv_mx[n][16]                entity3d.mx, .inverse_mx
 *            aabb[n][6]  (min.xyz, max.xyz)          entity3d.aabb
 *            center[n][3]                            entity3d.aabb_center
 *            vis_mask[ceil(n/64)]  bit i%64 of word i/64 = entity i passes the
 *                                  draw predicate of _models_render (model.c:959-973)
 *            vis_row_pop[ceil(n/64)] popcount of each vis_mask word (uint8); allocate the
 *                                  array rounded up to a multiple of 16 bytes, 16-B aligned
 */
/*
 * Joint attachment (parent_transform_apply's second flavour, model.c:1626-1641): entity `entity`
 * (flag CLAPGPU_E_JOINT_ATTACHED) rides mx = parent.mx * ((jt_pool[jt] * bind_pool[bind]) * local)
 * where jt_pool[jt] is the parent's joint_transforms[parent_joint] of THIS frame and
 * bind_pool[bind] that joint's bind matrix; it is rebuilt every frame (never skipped).  Launch
 * order is the caller's: parents' entity update -> clapgpu_pose_update -> the update of the
 * tiles holding attached subtrees.  The table is sorted by `entity`.  (In the reference a
 * resolved joint index equal to JOINT_TYPE_MAX (6) is indistinguishable from "no joint",
 * model.c:1609,1624: do not flag such an entity.)
 */
typedef struct clapgpu_attach {
    uint32_t entity, jt, bind, pad;
} clapgpu_attach;

/*
 * default_update's camera bounding-volume pick (model.c:1703-1713, consumed by
 * scene_camera_calc, scene.c:1018-1038): among ALIVE entities whose world AABB contains the
 * camera position or the control entity's position (except the control entity itself) the one of
 * largest volume (|model dx| scale)(|model dy| scale)(|model dz| scale).
 * *result (device uint64, zeroed by the update call) = float bits of the volume << 32 |
 * (0xFFFFFFFF - entity index), 0 if none: the largest key is the first entity of largest volume.
 * result may be NULL when inside_mask is given (no maximum is formed then, and the update call queues no fill for it).
 * inside_mask (device, n / 64 words, may be NULL): bit i = entity i passed the containment test.  A caller whose
 * entity order differs from the device's index order (the reference breaks volume ties by LIST order) replays
 * the pick over those few entities itself.
 */
typedef struct clapgpu_bv_query {
    float     cam_pos[3];
    uint32_t  has_ctl;
    float     ctl_pos[3];
    uint32_t  ctl_entity;
    uint64_t *result;
    uint64_t *inside_mask;
} clapgpu_bv_query;

/*
 * Extra views culled by the SAME launch as the main frustum: the frame's other render passes.  pipeline_render() runs one
 * shadow pass per cascade with view = &light->view[0] and no camera (pipeline-builder.c:34-46, 246-272; model.c:752-760)
 * before the model pass with the camera's view, and every pass asks view_entity_in_frustum(view, e) for every entity
 * (model.c:966-973; the test reads view->main only, view.c:296-337): two frusta a frame, more with more shadowed lights.
 * The rows' boxes are in registers when the main view is tested: a further view costs ~150 flops and 1/64 word per entity.
 * Every view v gets its own vis_mask / vis_row_pop plane (same shapes as clapgpu_entities'), written exactly as the main
 * plane is: bit i = entity i passes _models_render's draw predicate for that view, ALIVE && VISIBLE && (SKIP_CULLING || its
 * box is in that view's frustum).  CLAPGPU_E_SKIP_CULLING means the same in every plane: no view's planes are consulted for
 * such an entity, its bit is ALIVE && VISIBLE in the main plane and in every further one.  In every plane the bits at or
 * past n are zero, vis_row_pop[w] is the popcount of word w, and no vis_row_pop byte past ceil(n/64) is written.  Only read
 * when the call has a main frustum.  host_vis_mask: clapgpu_entities_update_tiles_hostio only -- device aliases of mapped host words the launch
 * writes as well (NULL: not wanted); such a view's drawn entities count as read for the export policy (keep_mask).
 */
#define CLAPGPU_EXTRA_VIEWS_MAX 4                          /* CASCADES_MAX, shader_constants.h:9 */
typedef struct clapgpu_views {
    uint32_t        n, pad;                                /* extra views: 0 .. CLAPGPU_EXTRA_VIEWS_MAX */
    clapgpu_frustum frustum[CLAPGPU_EXTRA_VIEWS_MAX];
    uint64_t       *vis_mask[CLAPGPU_EXTRA_VIEWS_MAX];     /* device */
    uint8_t        *vis_row_pop[CLAPGPU_EXTRA_VIEWS_MAX];  /* device, 16-byte aligned */
    uint64_t       *host_vis_mask[CLAPGPU_EXTRA_VIEWS_MAX];
} clapgpu_views;

typedef struct clapgpu_entities {
    uint32_t        n;
    uint32_t        n_models;
    const float    *pos_scale;
    const float    *rot;
    const int32_t  *parent;
    const int32_t  *model;
    const float    *model_table;
    uint32_t       *flags;
    uint32_t       *seqs;
    float          *mx;
    float          *inv_mx;
    float          *aabb;
    float          *center;
    uint64_t       *vis_mask;
    uint8_t        *vis_row_pop;
    /* optional (zero / NULL when unused) */
    uint32_t        n_attach;
    uint32_t        pad;
    const clapgpu_attach *attach;        /* device, sorted by entity */
    const float    *jt_pool;             /* device mat4[]: joint_transforms of the characters */
    const float    *bind_pool;           /* device mat4[]: model_joint.bind */
    float          *attach_local;        /* device work space, n_attach mat4 */
    const clapgpu_bv_query *bv;          /* HOST pointer */
    uint64_t       *rebuilt_mask;        /* device, n / 64 words, may be NULL: bit i = this update rebuilt entity i
                                            (mx / inverse_mx / aabb / seq changed): what a host mirror has to copy back */
    const clapgpu_views *views;          /* HOST pointer or NULL: the frame's other frusta, culled by the same launch */
} clapgpu_entities;

/* mode bits for clapgpu_entities_update */
#define CLAPGPU_UPDATE_ALL_DIRTY  (1u << 0)   /* treat every ALIVE entity as xform.updated; flags[] is not written */

/*
 * Replaces mq_update() over default_update entities (model.c:1953 -> 1649-1695,
 * parent_transform_apply 1594-1647, mat4x4_invert, entity3d_aabb_update 1200-1234)
 * and, when `frustum` is non-NULL, the per-entity view_entity_in_frustum() test of
 * _models_render (view.c:296-337, model.c:959-973) fused into the same pass.
 *
 * level_start is a HOST array of n_levels+1 ascending offsets (level_start[0] == 0,
 * level_start[n_levels] == e->n, every start a multiple of 64).  One launch per level.
 * With frustum == NULL vis_mask is left untouched.
 */
int clapgpu_entities_update(void *stream, const clapgpu_entities *e,
                            const uint32_t *level_start, uint32_t n_levels,
                            uint32_t mode, const clapgpu_frustum *frustum);

/*
 * One hierarchy level of the above: entities [first, first+count), whose parents
 * were all updated by earlier calls on the same stream.  `first` must be a multiple
 * of 64.  (Used by callers that interleave their own work or timing between levels.)
 */
int clapgpu_entities_update_level(void *stream, const clapgpu_entities *e,
                                  uint32_t first, uint32_t count,
                                  uint32_t mode, const clapgpu_frustum *frustum);

/*
 * Single-launch form of clapgpu_entities_update for forests laid out in TILES.
 * A tile is a run of consecutive 64-entity rows; row r = entities [64r, 64r+64).
 * Tile t = rows [tile_row_start[t], tile_row_start[t+1]) and holds whole subtrees,
 * one hierarchy level per row: a child in row r has its parent in row r-1 of the
 * same tile (taken from registers, never re-read from HBM).  Unused lanes of a row
 * are padding entities (flags == 0).  A parent outside the tile's previous row is
 * legal only if it is not rebuilt by this call (it is read from mx[] / seqs[]).
 * tile_row_start is a DEVICE array of n_tiles+1 ascending row indices.
 * One wavefront walks one tile; tiles are independent, so one launch covers every level.
 */
int clapgpu_entities_update_tiles(void *stream, const clapgpu_entities *e,
                                  const uint32_t *tile_row_start, uint32_t n_tiles,
                                  uint32_t mode, const clapgpu_frustum *frustum);

/*
 * Cull only: view_entity_in_frustum() over all entities from the stored aabb[]
 * (one call per render pass in the reference, model.c:969-970).  Writes vis_mask, and the planes of e->views with it.
 */
int clapgpu_entities_cull(void *stream, const clapgpu_entities *e, const clapgpu_frustum *frustum);

/*
 * Frames of a HOST mirror without copy calls (what libclapgpu_scene does for the level layout): the frame's touched
 * entities travel as one list of 40-byte records in device-mapped host memory (clapgpu_host_malloc_mapped) and are
 * scattered into pos_scale / rot / flags by clapgpu_entities_apply_inputs(); after the update,
 * clapgpu_entities_export_rebuilt() copies the rows of mx / inv_mx / aabb / center the update rebuilt (e->rebuilt_mask)
 * and the three bit masks into the mirror's mapped result arrays and then stores done_value into *done, which the host
 * polls (clapgpu_wait_word) -- no copy calls, no blocking wait.  counter: one zeroed device uint32 of scratch.
 */
typedef struct clapgpu_entity_input {
    uint32_t slot, flags;               /* flags as in clapgpu_entities.flags (CLAPGPU_E_DIRTY where xform.updated) */
    float    pos_scale[4], rot[4];
} clapgpu_entity_input;
typedef struct clapgpu_entities_export {
    float    *mx, *inv_mx, *aabb, *center;                 /* device-mapped host arrays, same shapes as clapgpu_entities' */
    uint64_t *vis_mask, *rebuilt_mask, *inside_mask;       /* inside_mask may be NULL */
    uint32_t *counter;                                     /* device scratch */
    uint32_t *done;                                        /* device-mapped host word */
    uint32_t  done_value, pad;
    uint64_t *stale_mask;                                  /* clapgpu_entities_export_rows: clapgpu_entities_hostio.stale_mask, or NULL */
} clapgpu_entities_export;
int clapgpu_entities_apply_inputs(void *stream, const clapgpu_entities *e, const clapgpu_entity_input *list, uint32_t n_list);
int clapgpu_entities_export_rebuilt(void *stream, const clapgpu_entities *e, const clapgpu_entities_export *x);
/*
 * A standing layout edited in place (entity3d_make / entity3d_delete between two frames, model.c:1730-1791; libclapgpu_scene's
 * clapgpu_scene_entity_new_placed): the lanes that got a new tenant, as one list in device-mapped host memory -- parent[slot]
 * and model[slot] are set; CLAPGPU_PLACE_ZERO_BOX also clears the lane's aabb / center rows (a model with skip_aabb never writes
 * them, and a fresh entity3d's are zeros, not the last tenant's).  One small launch instead of two copies and two fills per edit.
 */
typedef struct clapgpu_entity_place { uint32_t slot; int32_t parent, model; uint32_t flags; } clapgpu_entity_place;
#define CLAPGPU_PLACE_ZERO_BOX    1u    /* clear the lane's aabb / center rows */
#define CLAPGPU_PLACE_CLEAR_STALE 2u    /* clear the lane's bit in stale_mask (clapgpu_entities_hostio.stale_mask; the lane's last tenant's) */
int clapgpu_entities_place(void *stream, const clapgpu_entities *e, const clapgpu_entity_place *list, uint32_t n_list,
                           uint64_t *stale_mask);
/*
 * The rows a mirror asks for after the fact (a mirror that takes back only what is drawn, clapgpu_entities_hostio.keep_mask,
 * fetches the rest on demand: an entity that comes into view, entity3d_update() on a hidden one, ...): copies the rows of
 * mx / inv_mx / aabb / center flagged in select_mask (e->n / 64 words, device-readable: device memory or a mapped host
 * alias) into x's mapped arrays and raises *x->done = x->done_value.  x's three mask pointers are not used.
 */
int clapgpu_entities_export_rows(void *stream, const clapgpu_entities *e, const clapgpu_entities_export *x,
                                 const uint64_t *select_mask);

/*
 * The same small frame as ONE launch, for the tile layout: clapgpu_entities_update_tiles() that takes the inputs of the
 * slots flagged in `touched` (one bit per slot, set by the host for this frame) from the mirror's device-mapped upload
 * image (pos_scale / rot / flags in slot order, the bytes a copy would have carried) and stores them into the device
 * arrays as it goes, writes every row it rebuilds into the mapped result arrays as well, the three masks with them, and
 * raises *done = done_value when the last workgroup has finished (clapgpu_wait_word).  touched == NULL: no inputs this
 * launch (a second launch behind a pose: clapgpu_scene_attached_update).  Three dependent launches of a few microseconds
 * each cost a 10 k-entity frame 50 of its 68 us in launch-to-launch latency; this is one.
 */
#define CLAPGPU_HOSTIO_EXPORT_STALE_READ 1u
typedef struct clapgpu_entities_hostio {
    const float    *pos_scale, *rot;                       /* device aliases of the mapped upload image */
    const uint32_t *flags;
    const uint64_t *touched;                               /* device alias of the mapped touched-slot bits, or NULL */
    float    *mx, *inv_mx, *aabb, *center;                 /* device aliases of the mapped result arrays */
    uint64_t *vis_mask, *rebuilt_mask, *inside_mask;       /* vis_mask needed with a frustum; inside_mask may be NULL */
    uint32_t *counter;                                     /* device scratch: one zeroed uint32 */
    uint32_t *done;                                        /* device-mapped host word */
    uint32_t  done_value, options;                         /* CLAPGPU_HOSTIO_* bits */
    /* Export policy.  keep_mask == NULL: every rebuilt row is written to the mapped result arrays (what _models_render and
     * every other reader of e->mx / e->inverse_mx / e->aabb finds in the reference after mq_update, model.c:1022-1028,
     * 975-998).  keep_mask != NULL (device-readable, e->n / 64 words): only the rebuilt rows a reader exists for THIS
     * frame -- entities that pass the draw predicate (vis_mask; all of them without a frustum), entities whose box contains
     * a bounding-volume point (inside_mask), entities flagged in keep_mask (the mirror's standing readers: parents of
     * host-updated children, light carriers, the control entity ...).  The device arrays hold every row either way;
     * clapgpu_entities_export_rows() brings any of them over later.  exported_mask (mapped, may be NULL): bit i = row i was
     * written by this launch. */
    const uint64_t *keep_mask;
    uint64_t       *exported_mask;
    /* stale_mask (DEVICE memory, e->n / 64 words, zeroed by the caller once; may be NULL): bit i = the mirror's copy of row i is
     * older than the device's.  The launch keeps it -- a row it rebuilds without exporting becomes stale, one it exports stops
     * being so -- and, with CLAPGPU_HOSTIO_EXPORT_STALE_READ in `options`, also writes every stale row that has a reader NOW
     * (drawn by this launch's frustum, holding a bounding-volume point, flagged in keep_mask; every one without keep_mask)
     * although it did not rebuild it: what came into view is current when the launch is, without a second launch asking for
     * it.  Such rows are flagged in exported_mask and NOT in rebuilt_mask.  clapgpu_entities_export_rows() clears the bits
     * of what it hands over. */
    uint64_t       *stale_mask;
} clapgpu_entities_hostio;
int clapgpu_entities_update_tiles_hostio(void *stream, const clapgpu_entities *e, const uint32_t *tile_row_start,
                                         uint32_t n_tiles, uint32_t mode, const clapgpu_frustum *frustum,
                                         const clapgpu_entities_hostio *io);
/* Busy-wait until *word == value (a word a kernel stores into mapped host memory).  Checks `stream` every so often: if
 * it has drained and the word still differs, the signalling launch failed -> CLAPGPU_ERR_UNKNOWN instead of a hang. */
int clapgpu_wait_word(const volatile uint32_t *word, uint32_t value, void *stream);

/*
 * Ordered compaction of vis_mask into the ascending entity-index list the draw
 * loop iterates: visible[0..*count) = index_base + i for every set bit i.
 * `visible` needs room for n entries, `count` is one device uint32; index_base is the
 * global id of this shard's entity 0 (0 on a single GPU).  With vis_row_pop (as left by
 * the update / cull kernels) and n <= 4M the list is built in ONE launch; otherwise
 * (vis_row_pop == NULL or larger n) in two, using `scratch` =
 * clapgpu_visible_scratch_bytes(n) bytes of device memory.  (Build-defined: the
 * reference walks its entity list and tests each entity in place, model.c:958-973.)
 */
size_t clapgpu_visible_scratch_bytes(uint32_t n);
int clapgpu_visible_compact(void *stream, const uint64_t *vis_mask, const uint8_t *vis_row_pop,
                            uint32_t n, uint32_t index_base, uint32_t *visible, uint32_t *count,
                            void *scratch);

/*
 * Per-pass LOD pick of _models_render for the entities on the visible list (model.c:975-992,
 * SURVEY 8f rank 1): a forced LOD wins; otherwise, unless the camera is inside the entity's box,
 * lod = clamp((int)(| |aabb_center - cam|^2 - avg_edge^2 | / 3600), lod_min, lod_max) with
 * avg_edge = cbrtf(X Y Z) (entity3d_aabb_avg_edge, model.c:1261-1264).  visible / count as
 * produced by clapgpu_visible_compact (ids minus index_base index this shard's arrays);
 * force_lod[n] may be NULL (= -1 everywhere); cur_lod[n] is entity3d.cur_lod (in/out);
 * draw_lod[k] is the LOD visible[k] is drawn with: (visible, draw_lod) is the draw list.
 */
int clapgpu_entities_lod(void *stream, const clapgpu_entities *e, const uint32_t *visible,
                         const uint32_t *count, uint32_t index_base, const float cam_pos[3],
                         const int32_t *force_lod, int32_t *cur_lod, int32_t *draw_lod);
/* clapgpu_visible_compact + clapgpu_entities_lod over this batch's own vis_mask by one call: the ordered visible list of a
 * render pass and the LOD each entry is drawn with.  (Two launches: the single-kernel form was measured slower.) */
int clapgpu_visible_compact_lod(void *stream, const clapgpu_entities *e, uint32_t index_base, const float cam_pos[3],
                                const int32_t *force_lod, int32_t *cur_lod, uint32_t *visible, uint32_t *count,
                                int32_t *draw_lod, void *scratch);

/* ======================================================================== */
/* Multi-GPU: range sharding + the one exchange                  */
/* ======================================================================== */

/*
 * The path shards by entity range with whole subtrees on one rank: contiguous TILE ranges of (nearly) equal row
 * count.  tile_row_start: HOST array of n_tiles + 1 row offsets (clapgpu_entities_update_tiles).  Rank r of `world`
 * owns tiles [*first_tile, *end_tile).  Pure function: every rank computes the same cuts.
 */
int clapgpu_shard_tile_range(const uint32_t *tile_row_start, uint32_t n_tiles, uint32_t rank, uint32_t world,
                             uint32_t *first_tile, uint32_t *end_tile);

/*
 * The only exchange of a frame: the RCCL allgather (over xGMI) of every rank's compacted visible set, sent as its
 * 1-bit-per-entity mask -- one fixed-size collective, no counts, no padding, no host sync -- and its local expansion
 * into the identical ascending GLOBAL id list on every rank (shards are equal padded ranges: rank r's entity i has
 * global id r * n_pad + i).  RCCL is opened at run time (clapgpu_exchange_set_library: a path, e.g. the copy the
 * process already has; default: librccl.so of the process / the system); CLAPGPU_ERR_NOT_SUPPORTED without one.
 * Bootstrap: rank 0 calls clapgpu_exchange_unique_id(), the launcher carries the 128 bytes to every rank.
 *   vis_mask       this rank's mask, device, n_pad / 64 words
 *   gathered_mask  device, world * n_pad / 64 words (out)
 *   visible, visible_count, scratch   as clapgpu_visible_compact over world * n_pad entities; visible NULL = mask only
 * Issued on `stream`: put it on a side stream to overlap the next frame's update (two mask buffers).
 */
#define CLAPGPU_EXCHANGE_ID_BYTES 128
typedef struct clapgpu_exchange clapgpu_exchange;
void clapgpu_exchange_set_library(const char *path);
/* 1 if RCCL can be opened in this process (no communicator is made).  clapgpu_exchange_create() is COLLECTIVE -- it
 * returns when every rank has called it -- so ranks agree on this answer first (MIN over ranks) and only create the
 * exchange when all of them can; otherwise all take the launcher's fallback together. */
int  clapgpu_exchange_available(void);
int  clapgpu_exchange_unique_id(uint8_t id[CLAPGPU_EXCHANGE_ID_BYTES]);
int  clapgpu_exchange_create(clapgpu_exchange **out, const uint8_t id[CLAPGPU_EXCHANGE_ID_BYTES], int rank, int world);
/* ncclCommCount / ncclCommUserRank of the communicator and the PCI bus id of the device this rank drives
 * ("0000:c1:00.0"): gathered over all ranks they prove that N ranks on N DISTINCT GPUs took part (bench.py refuses to
 * print a line otherwise). */
int  clapgpu_exchange_info(const clapgpu_exchange *x, int *comm_ranks, int *comm_rank, char pci_bus_id[32]);
void clapgpu_exchange_destroy(clapgpu_exchange *x);
int  clapgpu_exchange_visible(void *stream, clapgpu_exchange *x, const uint64_t *vis_mask, uint32_t n_pad,
                              uint64_t *gathered_mask, uint32_t *visible, uint32_t *visible_count, void *scratch);
/* ... for shards of DIFFERENT sizes (the ranges clapgpu_shard_tile_range cuts from one scene are only nearly equal; a rank
 * may even be empty): every rank sends cap_pad / 64 words -- its own mask, zero beyond its n_pad[rank] -- and rank r's slot i
 * gets the scene-global id base[r] + i.  base / n_pad: HOST arrays of `world` entries, identical on every rank, ascending and
 * disjoint (clapgpu_shard_bases makes them); gathered_mask: world * cap_pad / 64 words; visible / scratch sized for
 * world * cap_pad entities (clapgpu_visible_scratch_bytes).  clapgpu_visible_compact_ranges is the expansion alone (the
 * exchange's second half: testable on one GPU), clapgpu_visible_expand_ranges_host the same on the host. */
int  clapgpu_exchange_visible_ranges(void *stream, clapgpu_exchange *x, const uint64_t *vis_mask, uint32_t cap_pad,
                                     const uint32_t *base, const uint32_t *n_pad, uint64_t *gathered_mask,
                                     uint32_t *visible, uint32_t *visible_count, void *scratch);
int  clapgpu_visible_compact_ranges(void *stream, const uint64_t *gathered_mask, uint32_t n_ranges, uint32_t cap_pad,
                                    const uint32_t *base, const uint32_t *n_pad, uint32_t *visible, uint32_t *count, void *scratch);
uint32_t clapgpu_visible_expand_ranges_host(const uint64_t *gathered_mask, uint32_t n_ranges, uint32_t cap_pad,
                                            const uint32_t *base, const uint32_t *n_pad, uint32_t *visible, uint32_t capacity);
/* first global id, padded size of every rank's shard and the largest of them, for clapgpu_shard_tile_range's cut (host) */
int  clapgpu_shard_bases(const uint32_t *tile_row_start, uint32_t n_tiles, uint32_t world, uint32_t *base, uint32_t *n_pad,
                         uint32_t *cap_pad);

/* ======================================================================== */
/* Particle systems: advect / respawn / billboard (core/particle.c)          */
/* ======================================================================== */

#define CLAPGPU_PART_DIST_LIN     0   /* particle_dist, particle.h:13-18 */
#define CLAPGPU_PART_DIST_SQRT    1
#define CLAPGPU_PART_DIST_CBRT    2
#define CLAPGPU_PART_DIST_POW075  3

/* struct particle_system's simulation fields (particle.c:17-29), 64 bytes */
typedef struct clapgpu_particle_system {
    float    center[3];          /* transform_pos(&ps->e->xform) */
    uint32_t dist;               /* ps->dist */
    double   radius, min_radius, radius_squared, velocity;
    uint32_t first, count;       /* particles [first, first+count); first is a multiple of 64 */
    uint32_t pad[2];
} clapgpu_particle_system;

/*
 * All particle systems of a model queue, particles stored system after system, every
 * system starting at a multiple of 64 (row_sys[r] = system of particles [64r, 64r+64)).
 *   pos[n][3]   particle.pos; after the call it IS ps->pos_array (particle.c:116,124):
 *               system s uploads pos + 3*first, count vec3s
 *   vel[n][3]   particle.velocity
 *   rng_state[2] the libc drand48 state as 48-bit integers: [1] = position of the stream
 *               before this call (input) and after it (output); [0] is internal.
 *               Initialise both to the same value (glibc default 0x1234ABCD330E).
 *   billboard_mx[n_sys][16]  entity3d.mx of each system's entity (particle.c:93-100), or NULL
 *   respawn_mask[n/64], respawn_row_pop[n/64 rounded up to 16], respawn_list[n],
 *   respawn_count[1], scratch (clapgpu_visible_scratch_bytes(n)): work space
 *   respawn_groups[CLAPGPU_RESPAWN_GROUP_WORDS]: persistent work space, ZEROED ONCE by the caller
 *               when the batch is created and then left alone (per-frame respawn counts of groups
 *               of rows, double-banked by frame); may be NULL, which costs ~10 us per call at 4 M
 *               particles (the respawn ranks then come from a scan of every row's count)
 */
#define CLAPGPU_RESPAWN_GROUP_WORDS 132
typedef struct clapgpu_particles {
    uint32_t  n;
    uint32_t  n_sys;
    const clapgpu_particle_system *sys;
    const uint32_t *row_sys;
    float    *pos;
    float    *vel;
    uint64_t *rng_state;
    float    *billboard_mx;
    uint64_t *respawn_mask;
    uint8_t  *respawn_row_pop;
    uint32_t *respawn_list;
    uint32_t *respawn_count;
    void     *scratch;
    uint32_t *respawn_groups;
} clapgpu_particles;

/*
 * Replaces particles_update() (particle.c:89-120) for every system, in system order, with
 * the reference's single drand48 stream reproduced exactly (7 draws per respawn, in particle
 * order).  view_mx = scene camera's view.main.view_mx (HOST pointer, 16 floats).
 */
int clapgpu_particles_update(void *stream, const clapgpu_particles *p, const float view_mx[16]);

/* ======================================================================== */
/* Skeletal pose blend + joint palette (core/model.c:1266-1404, interp.h)    */
/* ======================================================================== */

/*
 * Skinning constants of one model3d (model.h:104-110,59; set once by model3d_add_skinning,
 * model.c:524-538, and gltf_instantiate_one), device pointers.
 *   parent[j]   parent joint or -1 (child of root_pose)        model_joint.children, inverted
 *   depth[j]    level of joint j under joint 0, or -1 if j is NOT reachable from joint 0:
 *               the reference starts its recursion at joint 0 (model.c:1583) and never
 *               touches the others
 *   n_levels    1 + max depth
 *   invmx[j], bind[j] = invert(invmx[j])                       model_joint.invmx, .bind
 */
typedef struct clapgpu_skeleton {
    uint32_t        nr_joints;          /* <= 256 (JOINTS_MAX = 200, shader_constants.h:6) */
    uint32_t        n_levels;
    const int32_t  *parent;
    const int32_t  *depth;
    const float    *root_pose;          /* mat4 */
    const float    *invmx;              /* [nr_joints] mat4 */
    const float    *bind;               /* [nr_joints] mat4 */
} clapgpu_skeleton;

/*
 * Every animation of the model (struct animation / struct channel, model.h:133-142,
 * model.c:678-685), keyframe times strictly increasing per channel (glTF).
 *   chan_table[a][j][path] = (time_off, data_off, nr, 0) uint32x4: the channel of animation a
 *       that drives (joint j, path) -- key times at times[time_off .. +nr), key values at
 *       data[data_off ..] (floats, 3 per key for T/S, 4 for R); nr == 0: no such channel.
 *       path 0 translation, 1 rotation, 2 scale (enum chan_path); when the reference lists
 *       several channels for one (joint, path) the last one wins (model.c:1348-1349).
 *       16-byte aligned.
 */
typedef struct clapgpu_animations {
    uint32_t        n_anims;
    uint32_t        n_times;        /* floats in times[] (0: unknown) */
    const uint32_t *chan_table;
    const float    *times;
    const float    *data;
    /* the key-major copy of the pools made by clapgpu_animations_pack() for this model, the max_keys it was made with and
     * the layout word pack() returned (lanes, animation count, whether some (joint, path) has no channel).  REQUIRED by
     * clapgpu_pose_update(): besides the re-layout the copy holds, per rotation key pair, what quat_slerp (interp.h:91-118)
     * derives from the pair alone -- acos of the inner product and its sine -- evaluated by the host's libm, the very calls
     * the reference makes; the kernel has no other source for them.  Skeletons whose animations' key rows fit in LDS (one
     * animation of <= 31 keys per channel, two of <= 15, ...) search them there; one wavefront per character up to
     * 64 joints, two to four above. */
    const void     *packed;
    uint32_t        packed_keys, packed_layout;
    uint32_t        n_data, pad;    /* floats in data[] (0: unknown): with it clapgpu_animations_pack() refuses a channel that reads past the pool */
} clapgpu_animations;

/* Key-major pools, once per model: a HOST-side re-layout of chan_table / times / data (three synchronous copies on
 * `stream`) plus the rotation intervals' constants.  Checks what the kernel's exactness rests on: every channel's key times
 * strictly increasing (glTF requires it; the kernel's branch-free bracket equals channel_time_to_idx, model.c:1266-1288, only
 * then -- a channel with equal or descending times returns CLAPGPU_ERR_INVALID_ARGUMENTS and the caller keeps such a model on
 * the host path), no channel longer than max_keys or reaching past n_times / n_data.  max_keys = the largest nr of any channel; packed:
 * clapgpu_animations_packed_bytes() of device memory, 16-byte aligned; *packed_layout goes into
 * clapgpu_animations.packed_layout (clapgpu_pose_update rejects pools made for another skeleton class or animation count). */
size_t clapgpu_animations_packed_bytes(uint32_t n_anims, uint32_t max_keys, uint32_t nr_joints);
int    clapgpu_animations_pack(void *stream, const clapgpu_animations *an, uint32_t nr_joints, uint32_t max_keys, void *packed,
                               uint32_t *packed_layout);

/*
 * The animated entities of that model.
 *   anim[c]        queued_animation.animation of the current queue entry (model.c:1572-1576)
 *   frame_time[c]  (float)((now - ani_time) * speed), model.c:1578-1582
 *   entity[c]      index of the character's entity in entity_mx (NULL: c)
 *   entity_mx      the entity world matrices (clapgpu_entities.mx)
 *   trs[c][j][10]  joint translation(3) rotation(4) scale(3): struct joint (model.h:363-366),
 *                  in/out -- a path no channel drives keeps its value
 *   joint_transforms[c][j][16]  entity3d.joint_transforms, the UNIFORM_JOINT_TRANSFORMS payload
 *                  (model.c:1020-1022); joints not reachable from joint 0 are not written
 *   joint_pos[c][j][4]          struct joint.pos (camera.c:195-196); NULL = not computed
 *   skip           CLAPGPU_POSE_SKIP_*: outputs nothing reads this frame.  struct joint's translation / rotation / scale
 *                  and pos are host-visible state whose only per-frame reader is one_joint_transform itself
 *                  (model.c:1352-1404) and camera_target (camera.c:191-205); the draw path consumes joint_transforms
 *                  alone (model.c:1020-1022).  With SKIP_TRS the blended T/R/S stay in registers; that is 40 of the 120
 *                  bytes a joint writes, joint_pos another 16.  SKIP_TRS is refused (CLAPGPU_ERR_INVALID_ARGUMENTS) for a
 *                  model some of whose (joint, path) pairs have no channel in some animation: such a path keeps the
 *                  joint's LAST interpolated value (model.c:1301), which lives in trs[].
 */
#define CLAPGPU_POSE_SKIP_TRS        (1u << 0)
#define CLAPGPU_POSE_SKIP_JOINT_POS  (1u << 1)
/* joint_pos[] receives the MODEL-space position (model.c:1392-1397: column 3 of joint_transforms * bind) instead of
 * e->mx times it, and entity_mx is not read: the pose no longer waits for the frame's entity update.
 * clapgpu_joint_pos_world() finishes model.c:1400 afterwards -- the same mat4x4_mul_vec4_post, the same bits. */
#define CLAPGPU_POSE_JOINT_POS_MODEL (1u << 2)
typedef struct clapgpu_pose_batch {
    uint32_t        n_chars;
    uint32_t        skip;
    const uint32_t *anim;
    const float    *frame_time;
    const uint32_t *entity;
    const float    *entity_mx;
    float          *trs;
    float          *joint_transforms;
    float          *joint_pos;
} clapgpu_pose_batch;

/*
 * The time base of animated_update() (model.c:1563-1592) for the batch, on the device: per character
 *   frame_time[c] = (float)((now - ani_time[c]) * speed[c])        (double arithmetic, model.c:1578-1582)
 *   ended[c]      = (now - ani_time[c]) * speed[c] >= time_end[anim[c]]      (model.c:1590)
 * and for a character whose current queue entry repeats (restart[c] != 0) the animation_next() ->
 * animation_start() that follows: ani_time[c] = now (model.c:1406-1424, 1455-1483).  Entries that do
 * not repeat are left to the host, which reads ended[] to run its queue logic and callbacks
 * (animation_end, frame_cb, ani_cleared).  Run before clapgpu_pose_update with the same frame_time
 * array.  time_end[a] = animation.time_end of the model's animation a; now = clap_get_current_time().
 * (The whole queue logic on the device, callbacks included: clapgpu_animation_queue_time, ABI 46.)
 */
typedef struct clapgpu_anim_clock {
    uint32_t        n_chars;
    uint32_t        n_anims;
    const uint32_t *anim;
    const float    *time_end;
    double         *ani_time;
    const float    *speed;
    const uint8_t  *restart;
    float          *frame_time;
    uint8_t        *ended;
} clapgpu_anim_clock;
int clapgpu_animation_time(void *stream, const clapgpu_anim_clock *clk, double now);
/* The same with `now` read from device memory (one double): the launch then carries no per-frame value
 * and can sit in a captured HIP graph; the caller writes *now_dev before replaying it. */
int clapgpu_animation_time_dev(void *stream, const clapgpu_anim_clock *clk, const double *now_dev);

/* Replaces channels_transform() + one_joint_transform(e, 0, -1) of animated_update()
 * (model.c:1582-1583) for every character of the batch. */
int clapgpu_pose_update(void *stream, const clapgpu_skeleton *sk, const clapgpu_animations *an,
                        const clapgpu_pose_batch *pb);
/* model.c:1400 for a batch posed with CLAPGPU_POSE_JOINT_POS_MODEL: joint_pos[c][j] = entity_mx[entity[c]] * joint_pos[c][j]
 * (mat4x4_mul_vec4_post), in place, for every joint under joint 0 (the others are never written, as in the fused form). */
int clapgpu_joint_pos_world(void *stream, const clapgpu_skeleton *sk, const clapgpu_pose_batch *pb);

/* ======================================================================== */
/* Vertex skinning (shaders/model.vert:32-48)                                */
/* ======================================================================== */

/*
 * Character c skins mesh vertices [vert_first[c], vert_first[c] + vert_count[c]) of the
 * vertex pool with its palette joint_transforms[c][nr_joints] and writes them at
 * out_first[c].  Vertex attributes in the reference's formats (mesh.h:125-131, gltf.c:387-388):
 * position f32x3, normal f32x3, joints u8x4, weights f32x4 (16-B aligned).  Instances of one
 * model share vert_first.  Outputs: position f32x3 + normal f32x3 in the joint-space-blended
 * model space the shader would feed to `trs` (model.vert:44-45).
 *
 * The w component.  The shader multiplies proj * view * trs by the vec4 total_local_pos (model.vert:32-45), whose
 * w = sum_i weights[i] * (row 3 of joint_transforms[joints[i]] . (position, 1)) -- for affine palettes the SUM OF THE
 * WEIGHTS, which the reference never renormalises.  A draw that feeds vec4(out_position, 1) therefore equals the
 * shader only for vertices whose weights sum to 1.  Two ways to stay exact:
 *   - out_w != NULL: the kernel also writes that w (f32 per vertex, 28 B / vertex out instead of 24) and the draw
 *     feeds vec4(out_position, out_w);
 *   - out_w == NULL: the caller vouches that |sum(weights) - 1| is negligible for every vertex of the pool;
 *     clapgpu_load_gltf() reports the worst deviation per mesh (clapgpu_load.h: weight_sum_max_dev) so that a
 *     caller can decide.
 */
typedef struct clapgpu_skin_batch {
    uint32_t        n_chars;
    uint32_t        nr_joints;
    const uint32_t *vert_first;
    const uint32_t *vert_count;
    const uint32_t *out_first;
    const float    *position;
    const float    *normal;
    const uint8_t  *joints;
    const float    *weights;
    const float    *joint_transforms;
    float          *out_position;
    float          *out_normal;
    float          *out_w;              /* optional: total_local_pos.w per output vertex (see above) */
} clapgpu_skin_batch;

int clapgpu_skin(void *stream, const clapgpu_skin_batch *b);

/*
 * Skinning that follows the cull and the LOD (ABI 48).  The reference skins in its vertex shader, so only entities that
 * pass _models_render's draw predicate in some pass (model.c:959-973) are skinned, and only the vertices the bound index
 * buffer model->index[e->cur_lod] references (model.c:993-997, 1042; LOD_MAX = 4 index buffers over one vertex buffer,
 * model.h:42).  clapgpu_skin_drawn(b, sel) skins that subset of what clapgpu_skin(b) skins.  THE RULE:
 *
 * Character c of the batch has entity slot s = entity[c] (entity == NULL: s = c).
 *   Drawn.  c is drawn when bit s (bit s % 64 of word s / 64) is set in at least one of the n_planes mask planes; n_planes
 *     is 1 .. 1 + CLAPGPU_EXTRA_VIEWS_MAX and a plane has the shape of clapgpu_entities.vis_mask for n_entities entities.
 *     s >= n_entities: c is not drawn and CLAPGPU_SKINSEL_ENTITY_RANGE is set; nothing is read outside the planes.
 *   Its LOD (of a drawn character; nothing is asked of the others).  l = cur_lod[s] (cur_lod == NULL: 0).  l < 0 or
 *     l >= n_lods: LOD 0 is used and CLAPGPU_SKINSEL_LOD_RANGE is set.  n_lods <= CLAPGPU_SKIN_LODS; without rows
 *     n_lods == 0 stands for CLAPGPU_SKIN_LODS.
 *   Its vertices.  Row r = row[c] (row == NULL: 0) of the tables lod_first[n_rows][n_lods] and lod_count[n_rows][n_lods]
 *     names list[lod_first[r][l] .. lod_first[r][l] + lod_count[r][l]): ascending, distinct LOCAL vertex indices (vertex v
 *     of the character is vertex vert_first[c] + v of the pool).  lod_first == CLAPGPU_SKIN_LOD_ALL: the whole range
 *     [0, vert_count[c]) with no list read (lod_count is not read).  n_rows == 0: no tables at all, every drawn character
 *     is skinned whole.  A listed index >= vert_count[c] is skipped and sets CLAPGPU_SKINSEL_LIST_RANGE; so does the part
 *     of a range that lies past list[n_list) (skipped: nothing is read outside the list) and a row[c] >= n_rows (that
 *     character is skinned whole).
 *   What is written.  For every drawn c and every vertex v it names, out_position, out_normal (and out_w when given) at
 *     out_first[c] + v get exactly the bits clapgpu_skin writes there.  Every other byte of the three arrays keeps its value.
 *   What is reported, by every call (n_chars != 0): skinned[c] = the LOD used, CLAPGPU_SKIN_NOT_DRAWN for a character that
 *     is not drawn; chars[0 .. *count) = the drawn characters in ascending order, *count one device word.  *status is
 *     sticky: the call ORs bits into it and never clears it (the caller zeroes it once).
 *
 * All pointers are device pointers except the struct itself.  scratch: clapgpu_skin_select_scratch_bytes(n_chars) bytes,
 * 256-byte aligned, not shared with a call that may run at the same time.  No allocation and no host synchronisation: a
 * captured graph can hold the call.  n_chars == 0: CLAPGPU_OK, nothing is launched.  CLAPGPU_ERR_INVALID_ARGUMENTS before
 * any HIP call for a NULL batch, select or required array (the batch's as for clapgpu_skin; skinned, chars, count,
 * status; lod_first and lod_count with rows; list with n_list != 0), n_planes outside its range or a NULL plane, n_lods
 * outside 1 .. CLAPGPU_SKIN_LODS with rows (above it without), a scratch that is NULL or not 256-byte aligned; nr_joints
 * as for clapgpu_skin (CLAPGPU_ERR_TOO_LARGE).
 */
#define CLAPGPU_SKIN_LODS              4u            /* LOD_MAX, model.h:42 */
#define CLAPGPU_SKIN_LOD_ALL           0xffffffffu   /* lod_first: every vertex of the character, no list */
#define CLAPGPU_SKIN_NOT_DRAWN         0xffu         /* skinned[c] of a character that is not drawn */
#define CLAPGPU_SKINSEL_ENTITY_RANGE   (1u << 0)
#define CLAPGPU_SKINSEL_LOD_RANGE      (1u << 1)
#define CLAPGPU_SKINSEL_LIST_RANGE     (1u << 2)
typedef struct clapgpu_skin_select {
    uint32_t        n_planes;            /* 1 .. 1 + CLAPGPU_EXTRA_VIEWS_MAX (0 in a clapgpu_frame: the frame's own planes) */
    uint32_t        n_entities;          /* entities a plane covers */
    const uint64_t *planes[1 + CLAPGPU_EXTRA_VIEWS_MAX];
    const uint32_t *entity;              /* [n_chars] or NULL */
    const int32_t  *cur_lod;             /* [n_entities] or NULL */
    uint32_t        n_rows;              /* rows of the LOD tables; 0: none */
    uint32_t        n_lods;
    const uint32_t *row;                 /* [n_chars] or NULL */
    const uint32_t *lod_first;           /* [n_rows][n_lods] */
    const uint32_t *lod_count;           /* [n_rows][n_lods] */
    const uint32_t *list;                /* [n_list] */
    uint32_t        n_list;
    uint32_t        pad;
    uint8_t        *skinned;             /* [n_chars] out */
    uint32_t       *chars;               /* [n_chars] out */
    uint32_t       *count;               /* [1] out */
    uint32_t       *status;              /* [1] CLAPGPU_SKINSEL_*, sticky */
    void           *scratch;
} clapgpu_skin_select;

size_t clapgpu_skin_select_scratch_bytes(uint32_t n_chars);
int clapgpu_skin_drawn(void *stream, const clapgpu_skin_batch *b, const clapgpu_skin_select *sel);

/* ======================================================================== */
/* Rigid bodies: phys_step schedule, integrate, read-back, AABB broadphase   */
/* (core/physics.c over ODE).  ODE is an absent submodule of the reference:  */
/* the arithmetic is restated from ODE's published quickstep -- see          */
/* oracle/physics.c and DESIGN.md; parity for this block is UNPINNED.        */
/* ======================================================================== */

#define CLAPGPU_BODY_DISABLED      (1u << 0)   /* dxBodyDisabled */
#define CLAPGPU_BODY_AUTO_DISABLE  (1u << 1)   /* dBodySetAutoDisableFlag(body, 1), physics.c:1039 */
#define CLAPGPU_BODY_NO_GRAVITY    (1u << 2)   /* dBodySetGravityMode(body, 0) */

/* world parameters phys_init() / phys_body_new() set (physics.c:1125-1129, 1039-1042) */
typedef struct clapgpu_world {
    double  gravity[3];
    double  linear_damping;
    double  linear_damping_threshold_sq;
    double  adis_linear_threshold_sq;
    double  adis_angular_threshold_sq;
    double  adis_time;
    int32_t adis_steps;
    int32_t pad;
} clapgpu_world;

#define CLAPGPU_BODY_GYROSCOPIC    (1u << 3)   /* dxBodyGyroscopic: dBodyCreate sets it, dBodySetGyroscopicMode(b, 0) clears it */
#define CLAPGPU_BODY_HAS_JOINT     (1u << 4)   /* the body holds a (contact) joint this step: ODE never auto-disables a jointless
                                                  body; set by clapgpu_contacts_geoms, cleared by clapgpu_bodies_step (or, ahead
                                                  of it, by clapgpu_bodies_islands) */
#define CLAPGPU_BODY_KINEMATIC     (1u << 5)   /* dBodySetKinematic (physics.c:1031): ODE stores invMass = 0 and a zero invI.  Read by
                                                  the step's force path only (clapgpu_bodies.facc given, see clapgpu_bodies_step) */
#define CLAPGPU_GEOM_SPHERE  0
#define CLAPGPU_GEOM_CAPSULE 1
#define CLAPGPU_GEOM_BOX     2                 /* an axis-aligned box given by its AABB (stand-in for any static geom) */
#define CLAPGPU_GEOM_OTHER   3                 /* trimesh etc.: broadphase only, no narrowphase here (with a mesh set:
                                                  clapgpu_contacts_meshes / clapgpu_sweep_capsules) */

/*
 * Bodies of the character_space, fp64 like the reference's dDOUBLE ODE (physics.h:5-9): capsules
 * (phys_geom_capsule_new -> dCreateCapsule + dMassSetCapsuleTotal, physics.c:814-873) and, when the
 * capsule's length comes out 0, spheres (dCreateSphere + dMassSetSphereTotal, physics.c:866-873).
 *   pos[n][3], quat[n][4] (w,x,y,z = ODE order), lvel[n][3], avel[n][3]  in/out
 *   mass[n], radius[n]                                                     dMass.mass, geom radius
 *   yoffset[n]      phys_body.yoffset (physics.c:797-799)
 *   bflags[n]       CLAPGPU_BODY_* ; adis_steps_left / adis_time_left: ODE's auto-disable counters
 *   body_entity[n]  index of the entity3d the geom's data points at, or -1
 *   length[n]       capsule cylinder length, 0 = sphere; NULL = all spheres
 *   inertia[n][3]   diagonal of dMass.I in the body frame (clapgpu_mass_capsule_total / _sphere_total);
 *                   NULL = no rotational dynamics beyond the free spin (as if dBodySetGyroscopicMode(b, 0))
 *   geom_offset_R   dGeomSetOffsetRotation of the capsule geoms (physics.c:974-978), ODE dMatrix3
 *                   (3 rows of 4); clapgpu_geom_offset_rotation() fills it
 *   aabb[n][6]      out: the geom's AABB (minx,maxx,miny,maxy,minz,maxz), ODE's dReal aabb[6]; written by
 *                   clapgpu_bodies_aabb and by clapgpu_bodies_step for the bodies it moves; may be NULL
 *   axis[n][3]      out: the capsule's axis in world space (column 2 of body R * offset R); may be NULL
 *   adis_average_samples  dBodySetAutoDisableAverageSamplesCount (ODE's default: 1 = the instantaneous
 *                   velocity); > 1 needs adis_samples[n][samples][6] (lvel, avel ring) and adis_counter[n]
 *   facc[n][3]      in/out: the force accumulator (dxBody::facc): clapgpu_bodies_push adds to it, clapgpu_bodies_step
 *                   consumes it and leaves 0.  NULL = no accumulated forces: the step integrates gravity alone
 */
typedef struct clapgpu_bodies {
    uint32_t        n;
    uint32_t        adis_average_samples;
    double         *pos;
    double         *quat;
    double         *lvel;
    double         *avel;
    const double   *mass;
    const double   *radius;
    const double   *yoffset;
    uint32_t       *bflags;
    int32_t        *adis_steps_left;
    double         *adis_time_left;
    const int32_t  *body_entity;
    const double   *length;
    const double   *inertia;
    double          geom_offset_R[12];
    double         *aabb;
    double         *axis;
    double         *adis_samples;
    uint32_t       *adis_counter;
    /* optional (NULL: none): [n][8] doubles -- position, capsule axis, radius, length of every body's geom in ONE
     * 64-byte record, rewritten by clapgpu_bodies_step / clapgpu_bodies_aabb beside pos / axis whenever they move a geom.
     * Hand the same pointer to the narrowphase as clapgpu_geoms.records: a candidate pair's PARTNER is then one 64-byte
     * sector instead of four scattered ones (position, axis, radius, length) -- near_callback's gathers were 158 of the
     * contact kernel's 231 MB at configs[3].  16-byte aligned. */
    double         *geom_records;
    double         *facc;           /* last, so that positional initialisers and zeroed structs keep their meaning */
} clapgpu_bodies;

/* host helpers for the set-up the reference does once per body (no device work) */
void clapgpu_geom_offset_rotation(double R[12]);                        /* dRFromAxisAndAngle(1,1,1,-2pi/3), physics.c:974-978 */
void clapgpu_mass_sphere_total(double total_mass, double radius, double I[3]);                 /* dMassSetSphereTotal */
void clapgpu_mass_capsule_total(double total_mass, int direction, double radius, double length, double I[3]);
/* phys_geom_capsule_new (physics.c:814-873): entity AABB extents -> capsule radius, length, yoffset, direction, ray_off */
void clapgpu_capsule_geom(float X, float Y, float Z, double geom_radius, double geom_offset,
                          float *radius, float *length, float *yoffset, int *direction, float *ray_off);
/* axis + AABB of every body geom from the current pose (dxCapsule::computeAABB / dxSphere::computeAABB) */
int clapgpu_bodies_aabb(void *stream, const clapgpu_bodies *b);

/* physics.c:773-787: adds dt to *time_acc and returns how many 1/120 s substeps to run (0..5) */
int  clapgpu_phys_step_schedule(double *time_acc, double dt);
void clapgpu_world_defaults(clapgpu_world *w);

/*
 * dWorldQuickStep(world, h) for bodies without constraint rows (physics.c:769): auto-disable bookkeeping
 * (bodies holding a joint only, averaged over adis_average_samples), gravity, the implicit gyroscopic torque
 * of CLAPGPU_BODY_GYROSCOPIC bodies with an inertia tensor, velocity and pose update, linear damping, then
 * the moved geom's axis and AABB.
 * With b->facc (ODE 0.16 quickstep for a body without constraint rows, restated; PARITY UNPINNED like this block), for
 * every enabled body:
 *   f[j] = facc[j] + (NO_GRAVITY ? 0.0 : m * g[j])            ODE's facc += m * g, in that order
 *   lvel[j] += (h * invMass) * f[j]                            invMass = 1.0 / m, or 0.0 for a CLAPGPU_BODY_KINEMATIC body
 *   a KINEMATIC body's world inverse inertia is all zeros: its avel takes nothing from the gyroscopic torque (the
 *   product with the zero tensor is still formed and added, as ODE does)
 *   the rest as without forces; then facc[i] = 0 for every body the step stepped.
 * The accumulator of a DISABLED body -- one that came in disabled, or that this step's auto-disable put to sleep -- is
 * left untouched: this library's rule (ODE does not step such a body either); clapgpu_bodies_push wakes what it pushes.
 * Without b->facc the launch is the gravity-only kernel, bit for bit what it was before the accumulator existed, and
 * CLAPGPU_BODY_KINEMATIC is not looked at: give kinematic bodies an accumulator.
 * clapgpu_bodies_step_prebin and clapgpu_frame_issue take the same descriptor and behave alike: forces added before a
 * frame are consumed by its first substep, and survive a frame of 0 substeps.
 * Waking by contact (ODE's island pass enabling a sleeping body joined to an awake one) is clapgpu_bodies_islands, run in
 * front of this call; without it a sleeping body wakes through clapgpu_bodies_push or through the host clearing
 * CLAPGPU_BODY_DISABLED.
 */
int clapgpu_bodies_step(void *stream, const clapgpu_bodies *b, const clapgpu_world *w, double h);
/* The same step, which ALSO does the first launch of the next clapgpu_bp_collide(bp, b->n, b->aabb) -- the bin pass reads
 * nothing but the box the step has just computed: one launch and one pass over the boxes less per substep.  The collide
 * call recognises the pre-binned array by (pointer, count) and skips its bin launch; if b->aabb is changed by anything
 * else in between (clapgpu_bodies_aabb, an upload) call clapgpu_bp_invalidate(bp) first.  Results are the same pairs
 * (the list is canonical whatever order the bin atomics took).  b->aabb is required. */
struct clapgpu_bp;
int clapgpu_bodies_step_prebin(void *stream, const clapgpu_bodies *b, const clapgpu_world *w, double h, struct clapgpu_bp *bp);
int clapgpu_bp_invalidate(void *stream, struct clapgpu_bp *bp);

/*
 * phys_body_update() for every body (physics.c:789-812, 96-109): writes entity pos
 * (y - yoffset, double -> float) and rotation (wxyz -> xyzw) into the entity SoA
 * (clapgpu_entities.pos_scale / .rot, n_entities slots: a body_entity outside them writes nothing),
 * sets CLAPGPU_E_DIRTY, and moving[i] = |lvel| > 1e-3 (may be NULL).
 */
int clapgpu_phys_body_update(void *stream, const clapgpu_bodies *b, uint32_t n_entities, float *pos_scale,
                             float *rot, uint32_t *entity_flags, uint8_t *moving);

/*
 * default_update's push of the entity rotation to the physics body of characters and static
 * colliders (model.c:1680-1687 -> phys_body_rotate_xform, physics.c:136-145): link k = (body
 * link_body[k], entity link_entity[k]).  For a linked entity without a parent whose CLAPGPU_E_DIRTY
 * is set (or any, under CLAPGPU_UPDATE_ALL_DIRTY) the body quaternion becomes the entity's
 * (x,y,z,w) -> (w,x,y,z) in double, normalised as dBodySetQuaternion does.  Call BEFORE
 * clapgpu_entities_update, which clears the dirty flags.
 */
int clapgpu_bodies_rotate_from_entities(void *stream, const clapgpu_bodies *b, const clapgpu_entities *e,
                                        uint32_t mode, uint32_t n_links, const uint32_t *link_body,
                                        const uint32_t *link_entity);

/*
 * near_callback() for the sphere bodies (physics.c:399-449): dCollide on every
 * candidate pair of clapgpu_bp_collide, plus the surface parameters phys_contact_surface
 * (physics.c:291-330) gives each contact.  One record per pair, in pair order (the reference
 * creates its contact joints in callback order; here the canonical pair order): nc = dCollide's
 * return value (0 or 1 for spheres).  ODE's dContactGeom / dSurfaceParameters fields, doubles.
 * material[b] = (bounce, bounce_vel, mu, soft_erp, soft_cfm) of body b's phys_body
 * (physics.c:77-81), or NULL for bodies without parameters.  *contact_total (device, may be NULL)
 * receives the number of touching pairs.  n_pairs is read from the device counter pair_total,
 * clamped to capacity.  Contact joints and the LCP solve stay in ODE.
 */
#define CLAPGPU_CONTACT_BOUNCE   0x004   /* dContactBounce  (ode/contact.h) */
#define CLAPGPU_CONTACT_SOFT_ERP 0x008   /* dContactSoftERP */
#define CLAPGPU_CONTACT_SOFT_CFM 0x010   /* dContactSoftCFM */
typedef struct clapgpu_contact {
    double   pos[3], normal[3], depth;
    double   mu, bounce, bounce_vel, soft_erp, soft_cfm;
    uint32_t mode;
    uint32_t nc;
} clapgpu_contact;
int clapgpu_contacts_spheres(void *stream, const clapgpu_bodies *b, const uint32_t *pairs,
                             const uint32_t *pair_total, uint32_t capacity, const double *material,
                             clapgpu_contact *contacts, uint32_t *contact_total);
/*
 * The same for the (body, static geom) candidate pairs of clapgpu_bp_collide: dCollide of a
 * sphere (g1) against an axis-aligned box (g2) -- ODE's dCollideSphereBox with the box given as static_aabb[s]
 * (position = centre, side = max - min, no rotation): the sphere centre clamped to the box, contact at the
 * clamped point with the normal from the box to the sphere, or, for a centre inside the box, at the
 * centre with the normal through the closest face and depth = distance to that face + radius.
 * static_material[s] = the static collider's phys_body parameters (same 5 doubles); surface defaults
 * unless both material arrays are given (phys_contact_surface needs both phys bodies, physics.c:296).
 */
int clapgpu_contacts_sphere_box(void *stream, const clapgpu_bodies *b, uint32_t n_static,
                                const double *static_aabb, const uint32_t *pairs, const uint32_t *pair_total,
                                uint32_t capacity, const double *material, const double *static_material,
                                clapgpu_contact *contacts, uint32_t *contact_total);

/*
 * Broadphase over explicit fp64 AABBs (round 2): both calls of __phys_step (physics.c:751-753) in one pass of
 * four launches.  Bodies are binned by their AABB centre into a hash grid of 4x4x4-cell blocks (cell >= the
 * largest body AABB edge); one wavefront per block tests the block's own bodies against the block + its halo
 * staged in LDS, and against the static geoms registered for that block.
 *   clapgpu_bp_create   n_max bodies; statics: n_static AABBs in HOST memory (copied and binned on the host; a static
 *                       that moves is registered again by clapgpu_bp_statics_update; those spanning more than 64
 *                       blocks are kept in a list every block tests)
 *   clapgpu_bp_collide  aabb: device [n][6] (clapgpu_bodies.aabb).  pairs / static_pairs are ascending (i, j), i < j resp. (body, static);
 *                       *_total = number found (device uint32), at most `capacity` written (when a total
 *                       exceeds its capacity the written part is incomplete).  static outputs may be NULL.
 *   clapgpu_bp_status   host sync; bit 0: a body AABB edge exceeded `cell` (pairs may be missing)
 *
 * Bodies of mixed sizes (ABI 41): clapgpu_bp_create_levels makes a multi-level grid, as ODE's hash space is one.  Level l
 * (0 .. levels - 1) has the cell size cell * 2^l; a body lives on the lowest level whose cell is not smaller than its
 * largest AABB edge (an edge equal to cell * 2^l is level l; a NaN edge fits level 0) and is tested against its own and
 * every coarser level.  An edge above the top level's cell sets status bit 0 with the meaning above.  Every call that
 * takes a clapgpu_bp takes either kind, and the outputs of clapgpu_bp_collide keep their contract word for word.
 * levels == 1 is the object of clapgpu_bp_create (which stays the call it is); levels == 0 or above
 * CLAPGPU_BP_LEVELS_MAX, or levels > 1 with n_max > 2^28: CLAPGPU_ERR_INVALID_ARGUMENTS.  A leveled object is never
 * pre-binned (clapgpu_bodies_step_prebin runs the plain step) and holds no index unless it is asked to
 * (clapgpu_bp_leveled_index, ABI 44): see clapgpu_bp_index.
 *   clapgpu_bp_levels     the levels of the object (0 for NULL)
 *   clapgpu_bp_cell_slot  host only, no device work: the cell slot of cell (cx, cy, cz) of `level` in this object (for
 *                         tests and tools); 0xffffffff for a level the object does not have
 */
#define CLAPGPU_BP_LEVELS_MAX 16
typedef struct clapgpu_bp clapgpu_bp;
typedef struct clapgpu_trimesh clapgpu_trimesh;                        /* a set of static triangle meshes: clapgpu_trimesh_create */
int  clapgpu_bp_create(clapgpu_bp **out, uint32_t n_max, double cell, uint32_t n_static, const double *static_aabb_host);
int      clapgpu_bp_create_levels(clapgpu_bp **out, uint32_t n_max, double cell, uint32_t levels,
                                  uint32_t n_static, const double *static_aabb_host);
uint32_t clapgpu_bp_levels(const clapgpu_bp *bp);
uint32_t clapgpu_bp_cell_slot(const clapgpu_bp *bp, uint32_t level, int32_t cx, int32_t cy, int32_t cz);
void clapgpu_bp_destroy(clapgpu_bp *bp);
int  clapgpu_bp_collide(void *stream, clapgpu_bp *bp, uint32_t n, const double *aabb,
                        uint32_t *pairs, uint32_t capacity, uint32_t *pair_total,
                        uint32_t *static_pairs, uint32_t static_capacity, uint32_t *static_pair_total);
int  clapgpu_bp_status(void *stream, clapgpu_bp *bp, uint32_t *status);
const double *clapgpu_bp_static_aabb(const clapgpu_bp *bp);            /* the device copy of the static AABBs */

/*
 * Moving statics (ABI 45): dGeomSetPosition on a geom without a body (phys_body_set_position / phys_body_move /
 * phys_body_rotate_xform, physics.c:208-240) -- ODE's hash space bins every geom again at every dSpaceCollide; here the
 * caller says which boxes are the new ones.
 *
 * clapgpu_bp_statics_update re-registers the static boxes of `bp` on the device: static_aabb is DEVICE memory,
 * [n_static][6] as at create, n_static the count the object was created with (another count, a NULL bp or a NULL array:
 * CLAPGPU_ERR_INVALID_ARGUMENTS; 0 statics: CLAPGPU_OK, nothing done).  After the call the object is, for every caller,
 * the object clapgpu_bp_create[_levels] would have made from the same (n_max, cell, levels) and the new boxes: the same
 * registrations per block bucket and level, the same large lists, the same bounds.  clapgpu_bp_static_aabb(bp) holds the
 * new boxes AT THE SAME ADDRESS, so every clapgpu_geoms.aabb built on it stays valid.  static_aabb may be that very
 * pointer (boxes rewritten in place by a kernel of the caller's, in stream order before the call); otherwise it must not
 * overlap it.
 *
 * The call SYNCHRONISES the stream, twice (as clapgpu_characters_move_ordered does): once for the counts that size the new
 * image, once at its end.  Work of other streams that reads the object must have finished.  The images stand in a second
 * device allocation of the object, made by the first update, grown geometrically when an update needs more and freed by
 * clapgpu_bp_destroy; the image of clapgpu_bp_create is then no longer used.  An object that is never updated is the
 * object it was before ABI 45.
 *
 * Transactional: the object changes only after every launch and copy of the update has been issued without error and
 * waited for, the copy into clapgpu_bp_static_aabb(bp) being the last of them; an error in between is returned and the
 * object goes on answering with the old statics (from an in-place update its box array, the caller's, is the new one).
 *
 * What the call drops: the index (clapgpu_bp_index; its view describes the old statics: a query through the grid is
 * refused until the next clapgpu_bp_index, as after clapgpu_bp_invalidate) and a recorded prebin
 * (clapgpu_bodies_step_prebin; undone as clapgpu_bp_invalidate undoes it).  What stays: the sticky status bits, the bin
 * epoch, the leveled-index switch, the contact ticket word.  A HIP graph captured from calls that use the object holds
 * the old image's addresses and counts BY VALUE: capture it again after an update (this is not detected).
 * A static that owns a mesh: update its box first, then clapgpu_trimesh_pose, then clapgpu_bp_index.  Where few of the
 * meshes move, a set of clapgpu_trimesh_create_parts takes clapgpu_trimesh_pose_meshes in its place: the moved meshes alone.
 *
 * For tests and tools, in the spirit of clapgpu_bp_cell_slot:
 *   clapgpu_bp_statics_sizes  host state only (any output may be NULL): the block buckets, the registrations of all
 *                             levels, the large statics of all levels, where each level's part of the large list
 *                             starts (levels + 1 values used; all zero for a one-level object), the bounds of the
 *                             registered boxes (min xyz, max xyz; min > max: none)
 *   clapgpu_bp_statics_read   host sync; the image into HOST arrays (any may be NULL): start [levels * (buckets + 1)],
 *                             entries [n_entries], large [n_large], entry_boxes [n_entries][6], large_boxes
 *                             [n_large][6].  CLAPGPU_ERR_UNKNOWN when a record does not carry its entry's index or its
 *                             cell words are not zero.
 */
int clapgpu_bp_statics_update(void *stream, clapgpu_bp *bp, uint32_t n_static, const double *static_aabb);
int clapgpu_bp_statics_sizes(const clapgpu_bp *bp, uint32_t *buckets, uint32_t *n_entries, uint32_t *n_large,
                             uint32_t large_start[CLAPGPU_BP_LEVELS_MAX + 1], double bounds[6]);
int clapgpu_bp_statics_read(void *stream, const clapgpu_bp *bp, uint32_t *start, uint32_t *entries, uint32_t *large,
                            double *entry_boxes, double *large_boxes);

/*
 * near_callback (physics.c:399-449) on candidate pairs (ia in A, ib in B; g1 = A's geom): dCollide for spheres,
 * capsules and axis-aligned boxes (dCollideSpheres, dCollideCapsuleSphere, dCollideCapsuleCapsule with its
 * two-contact parallel case, dCollideSphereBox, dCollideCapsuleBox; reversed like dCollide when only the
 * swapped collider exists) + phys_contact_surface (physics.c:291-330).  One 160-byte record per pair; the record
 * arrays must be 16-byte aligned (CLAPGPU_ERR_INVALID_ARGUMENTS otherwise: they are written as 16-byte pieces).
 * A capsule whose axis touches a box is where ODE switches to dBoxBox: flagged CLAPGPU_CONTACT_DEEP, nc bits 0.
 * body_flags_a / _b (may be NULL): bflags of the body sets behind A / B; touching pairs set CLAPGPU_BODY_HAS_JOINT.
 */
typedef struct clapgpu_geoms {
    uint32_t        n, pad;
    const double   *pos;            /* [n][3] geom position (boxes: the centre of aabb is used) */
    const double   *axis;           /* [n][3] capsule axis (clapgpu_bodies.axis) */
    const double   *radius, *length;/* [n]; length NULL = no capsules */
    const uint8_t  *kind;           /* [n] CLAPGPU_GEOM_*; NULL = sphere when length is 0, else capsule */
    const double   *aabb;           /* [n][6] boxes */
    const double   *material;       /* [n][5] bounce, bounce_vel, mu, soft_erp, soft_cfm (physics.c:77-81); may be NULL */
    const double   *records;        /* optional: [n][8] = (pos, axis, radius, length) per geom, the SAME values as the arrays
                                       above in one 64-byte record (clapgpu_bodies.geom_records); only read for geom sets
                                       without kind / aabb (spheres and capsules: what bodies are).  16-byte aligned */
} clapgpu_geoms;
#define CLAPGPU_CONTACT_DEEP 0x80000000u
typedef struct clapgpu_contact2 {
    double   pos[3], normal[3], depth;
    double   mu, bounce, bounce_vel, soft_erp, soft_cfm;
    uint32_t mode;
    uint32_t nc;                    /* 0, 1, 2, or CLAPGPU_CONTACT_DEEP */
    double   pos2[3], normal2[3], depth2;
} clapgpu_contact2;
int clapgpu_contacts_geoms(void *stream, const clapgpu_geoms *A, const clapgpu_geoms *B, const uint32_t *pairs,
                           const uint32_t *pair_total, uint32_t capacity, clapgpu_contact2 *contacts,
                           uint32_t *contact_total, uint32_t *body_flags_a, uint32_t *body_flags_b);
/*
 * near_callback over BOTH candidate lists of a step -- bodies x bodies and bodies x statics (physics.c:751-753) -- in ONE
 * launch, with no counter fill in front of it: the same records and totals as clapgpu_contacts_geoms(bodies, bodies, ...)
 * followed by clapgpu_contacts_geoms(bodies, statics, ...), body_flags as body_flags_a of both.  `bp` lends eight bytes of
 * scratch (a ticket-and-counts word the kernel leaves at zero); capacities below 2^24 pairs each, else
 * CLAPGPU_ERR_TOO_LARGE (use the two calls).  Two launches and two fills were 62 us of a frame for 47 us of work.
 */
int clapgpu_contacts_geoms_both(void *stream, clapgpu_bp *bp, const clapgpu_geoms *bodies, const clapgpu_geoms *statics,
                                const uint32_t *pairs, const uint32_t *pair_total, uint32_t capacity,
                                clapgpu_contact2 *contacts, uint32_t *contact_total,
                                const uint32_t *static_pairs, const uint32_t *static_pair_total, uint32_t static_capacity,
                                clapgpu_contact2 *static_contacts, uint32_t *static_contact_total, uint32_t *body_flags);

/*
 * phys_body_sweep_capsule (physics.c:559-670) for a batch of sweeps: sweep k marches a probe copy of body
 * sweep_body[k] (a geom of A) along delta[k] in max(2, ceil(|delta| / (radius / 2))) steps and collides it at
 * every step with its candidate geoms cand[cand_first[k] .. cand_first[k + 1]): an index into B (statics) or,
 * with bit 31 set, into A (other bodies; the body itself is skipped).  Out per sweep: frac (best_frac),
 * normal[3], hit (body index, -2 - static index, or -1).  Contacts are taken in candidate order, 16 per
 * step at most (MAX_CONTACTS).  One wavefront per sweep.
 * meshes (may be NULL: no mesh set; else created with n_statics == B->n): a candidate static that owns a mesh of the
 * set is collided through that mesh's triangles alone, by the triangle rule stated at clapgpu_contacts_meshes (the mesh
 * replaces its collider, as in the ray casts), queried with the probe's box at every step.  Within a mesh candidate
 * the contacts are taken in ascending triangle index; the cap of 16 per step applies.  hit = -2 - s for the mesh's
 * static s.
 */
int clapgpu_sweep_capsules(void *stream, const clapgpu_geoms *A, const clapgpu_geoms *B, const clapgpu_trimesh *meshes,
                           uint32_t n_sweeps, const uint32_t *sweep_body, const float *delta, const uint32_t *cand_first,
                           const uint32_t *cand, float *frac, float *normal, int32_t *hit);

/*
 * Ray casts against the device scene (__phys_ray_cast / phys_ray_cast2 / phys_ray_cast, physics.c:474-540).
 *
 * clapgpu_bp_index: the grid of the CURRENT boxes without the pair search -- the first three launches of
 * clapgpu_bp_collide and a reduction of the boxes' bounds and of "an edge exceeds `cell`" into control words of the
 * index's own.  Boxes clapgpu_bodies_step_prebin binned are indexed without the bin launch and binned again after the
 * scatter, so the prebin stays for the next collide (also one captured in a graph without its bin launch).  `bp` records
 * the (aabb, n) it indexed; clapgpu_bp_collide, clapgpu_bodies_step_prebin, clapgpu_bp_invalidate, another index and
 * clapgpu_bodies_ground_collide clear that record.  A collide after an index returns the pairs it returns without one.
 * Call it after the last step of a frame (clapgpu_frame_issue runs collide -> contacts -> step, so the grid it leaves
 * describes the boxes from before the step) and again after anything moves bodies.
 * The host cannot see a replayed graph bin the boxes again: the device counts every bin pass, and a ray through an
 * index whose count has moved on scans every geom instead (same results, brute-force time) -- index after replays.
 * clapgpu_bp_index_status: host sync; bit 0: an indexed box's edge exceeds `cell` (this index only, unlike the sticky
 * bit 0 of clapgpu_bp_status); bit 1: the boxes were binned again since the index (a replayed collide or prebinning
 * step); bit 2 (value 4): the object is leveled (clapgpu_bp_create_levels with levels > 1) and its index is switched
 * off: clapgpu_bp_index launched nothing and every query through it scans every geom, as with bp == NULL.  In all
 * three cases rays through this index scan every geom.  CLAPGPU_ERR_INVALID_ARGUMENTS when not indexed.
 *
 * clapgpu_bp_leveled_index (ABI 44): the switch of a leveled object's index; state of the object, off when it is
 * created.  Host only: launches nothing, does not synchronise.  Setting it, on or off, drops the index the object
 * holds: clapgpu_bp_index_status returns CLAPGPU_ERR_INVALID_ARGUMENTS until the next clapgpu_bp_index, as after
 * clapgpu_bp_invalidate.  A one-level object: CLAPGPU_OK, nothing changes.  bp == NULL: CLAPGPU_ERR_INVALID_ARGUMENTS.
 * Off: the object is the leveled object described above, bit 2 included.  On: clapgpu_bp_index runs four launches --
 * the leveled bin, cells and scatter of clapgpu_bp_collide and the bounds reduction, its edge test against the TOP
 * level's cell, cell * 2^(levels - 1) -- and clapgpu_bp_index_status reports bits 0 and 1 as for a one-level object
 * (bit 0: an edge above the top level's cell), never bit 2.  Every query that takes a bp then reads that index, and
 * every call that clears a one-level index's record clears this one.  The lookup rule: for a query box [lo, hi] every
 * level L is looked up with its own cell c_L = cell * 2^L, in the cells floor((lo - g) / c_L) .. floor((hi + g) / c_L)
 * per axis, g = c_L / 2 * (1 + 1e-9); a body of level L has edges of at most c_L and is binned by its centre, so those
 * cells hold every body of that level whose box meets the query; a record counts only when its (level, cell) is the
 * one looked up, because cells of all levels share slots.  The statics are read from ONE level's registration, two
 * below the top (every static is registered on every level; which level is a measured choice and changes no
 * result).  Rays cut their segment into pieces of c_L per level;
 * the caps that send a far-flung ray or a large swept box to the scan hold the lookups of all levels together, so a
 * large mover among small bodies scans.  Results are the scan's, bit for bit, either way.
 *
 * clapgpu_ray_cast: ray k = ray[k][8] (start xyz, direction xyz of any length, normalised as dGeomRaySet does, length,
 * pad) against every body (a geom of `bodies`) and static (`statics`), as dCreateRay + dGeomRaySetClosestHit +
 * dSpaceCollide2 over phys->space + the "closest hit that is not self" loop (physics.c:479-520).  skip[k] (or NULL =
 * none): body i, -2 - s for static s, -1 none.  Out: hit[k] = body i, -2 - s, or -1 (a miss); dist[k] = the hit's depth
 * (*pdist), unchanged on a miss; contact[k][6] (or NULL) = the dContactGeom's pos and normal, unchanged on a miss;
 * flags[k] (or NULL) = CLAPGPU_RAY_*.  bp == NULL: every geom is tested (one wavefront per ray: the right call for a
 * few camera rays); else `bp` must hold an index over bodies->n boxes and have been created with statics->n statics
 * in the same order (CLAPGPU_ERR_INVALID_ARGUMENTS otherwise), and only the grid cells along the ray are looked up --
 * same results bit for bit.  The ray scans every geom instead when an indexed box is larger than a cell, when the boxes
 * were binned again since the index, or when the ray crosses more cells than a scan would test geoms.
 * Colliders (ODE 0.16 ray.cpp; a hit is at 0 <= depth <= length along the unit direction):
 *   sphere   dCollideRaySphere: the entry point, outward normal; a start inside: the exit point, normal flipped
 *            (pointing into the sphere).  The flip follows where the start is (C < 0), not the root taken: a start
 *            exactly on the surface moving outward hits at depth 0 with the outward normal
 *   capsule  dCollideRayCapsule: the cylinder between the caps or a cap's sphere, outward normal; a start inside the
 *            capsule: the exit point, normal flipped
 *   box      dCollideRayBox on the static's AABB: the entry face, its outward axis normal; an edge or corner takes the
 *            first axis (x, y, z) whose slab is entered last; a start inside: the exit face, normal flipped
 *   other    (CLAPGPU_GEOM_OTHER, trimesh): not intersected; see CLAPGPU_RAY_UNRESOLVED.  With a mesh set (`meshes`) a
 *            static that owns a mesh is intersected through its triangles instead
 * Deviations: the hit kept is the smallest depth, ties to bodies before statics and then to the lower index (ODE keeps
 * the first in its hash-space order); NaN geometry never hits.
 * meshes (may be NULL: no mesh set; else a set of clapgpu_trimesh_create, below, created with n_statics == statics->n,
 * CLAPGPU_ERR_INVALID_ARGUMENTS otherwise): the statics that own a mesh of the set are intersected through their
 * triangles (one more launch, one lane per ray).  Such statics raise no CLAPGPU_RAY_UNRESOLVED; OTHER statics without a
 * mesh still do.  With meshes the call takes 8 bytes per ray of stream-ordered scratch (hipMallocAsync) when flags are
 * written.
 * The triangle test (BackfaceCull, ClosestHit: physics.c:485-487): a triangle is hit from its front only,
 * u . n < 0 for the unit direction u and n = (v1 - v0) x (v2 - v0); n == 0 and a ray parallel to the plane never hit;
 * a start inside a closed mesh sees back faces only and misses it.  Contact pos = start + depth * u, normal = n / |n|
 * (towards the start); hit = -2 - s for the mesh's static s; skip = -2 - s skips the whole mesh.
 * Deviation: ODE tests the triangles in float (OPCODE); here in fp64 with the watertight test of Woop, Benthin and Wald
 * (2013), so a ray through a shared edge or vertex of front faces always hits one of them.  Ties extend the rule above:
 * the smallest depth, bodies before statics, the lower static index, the lower triangle index of the mesh.
 */
#define CLAPGPU_RAY_INVALID      1u   /* zero / NaN / infinite direction, NaN start, negative or NaN length: a miss */
#define CLAPGPU_RAY_UNRESOLVED   2u   /* the segment enters an OTHER static's AABB before the hit (or there is no hit):
                                         redo this ray with ODE (the reference's terrain is a trimesh) */
#define CLAPGPU_RAY_MOVED_TARGET 4u   /* clapgpu_bodies_ground_collide: the hit body was itself moved by this batch */
int clapgpu_bp_index(void *stream, clapgpu_bp *bp, uint32_t n, const double *aabb);
int clapgpu_bp_index_status(void *stream, clapgpu_bp *bp, uint32_t *status);
int clapgpu_bp_leveled_index(clapgpu_bp *bp, int on);
int clapgpu_ray_cast(void *stream, clapgpu_bp *bp, const clapgpu_geoms *bodies, const clapgpu_geoms *statics,
                     const clapgpu_trimesh *meshes, uint32_t n_rays, const double *ray, const int32_t *skip,
                     double *dist, int32_t *hit, double *contact, uint32_t *flags);
/*
 * phys_body_ground_collide (physics.c:695-744, called from character_move, character.c:454) for bodies body[k]
 * (each once; see below), ray_off[k] = phys_body.ray_off, grounded[k] = !ch->airborne.  The ray starts at the body position less
 * (ray_off - 0.05) in y, through a float vec3, points down, is 2 * ray_len long (ray_len = yoffset - (ray_off - 0.05)
 * + 1e-3) and skips the body; its bodies are b's geoms.  On a hit normal[k] = the contact normal (float) and the body
 * moves by (float)(ray_len - dist) or (float)(-(dist - ray_len)) per the reference's three branches
 * (dBodySetPosition, then pos / axis / aabb / geom record as clapgpu_bodies_aabb writes them).  Out:
 * grounded_out[k] = the return value, dist[k] (unchanged on a miss), hit[k], flags[k].  Every ray sees the poses from
 * before the call (the reference moves the characters one at a time): CLAPGPU_RAY_MOVED_TARGET marks a ray whose hit
 * body moved in this call -- clapgpu_characters_move_ordered gives the whole move in list order.  INVALID and UNRESOLVED rays move nothing (grounded_out 0).
 * A body listed more than once: all its rays get CLAPGPU_RAY_INVALID and grounded_out 0, and it does not move.
 * scratch: [b->n] uint32 of device memory, overwritten.  bp: NULL or an index over (b->n, b->aabb); cleared on return.
 * meshes (may be NULL): as clapgpu_ray_cast takes it, by the same triangle test, with the same launch more and the same
 * 8 bytes per ray of stream-ordered scratch; the decision and the move see the merged hit.
 */
int clapgpu_bodies_ground_collide(void *stream, clapgpu_bp *bp, const clapgpu_bodies *b, const clapgpu_geoms *statics,
                                  const clapgpu_trimesh *meshes, uint32_t n, const uint32_t *body, const double *ray_off,
                                  const uint8_t *grounded, uint8_t *grounded_out, float *normal, double *dist, int32_t *hit,
                                  uint32_t *flags, uint32_t *scratch);

/*
 * The triangle meshes of static trimesh geoms (phys_geom_trimesh_new, physics.c:882-930): the `meshes` of the ray casts
 * and the sweep above and of the mesh contacts below.
 * clapgpu_trimesh_desc holds DEVICE arrays for mesh m of n_meshes:
 *   static_index[m]       the static (of a statics set of n_statics) the mesh belongs to, meant to be a
 *                         CLAPGPU_GEOM_OTHER static.  The kind is not checked: a sphere, capsule or box static that owns
 *                         a mesh is intersected through its mesh alone (the mesh replaces its collider in the ray casts)
 *   vx_first[m + 1]       ascending from 0: mesh m's vertices are vx[vx_first[m] .. vx_first[m + 1])
 *   tri_first[m + 1]      ascending from 0: its triangles are idx[tri_first[m] .. tri_first[m + 1])
 *   vx[V][3]              model3d.collision_vx: float xyz in model space
 *   idx[T][3]             model3d.collision_idx: u16 vertex indices into the mesh's own vertices, winding as given
 *   scale[m]              entity->scale (float)
 *   pos[m][3]             the geom position: the entity position (dGeomSetPosition; yoffset is 0 for a trimesh)
 *   quat[m][4]            the entity rotation x, y, z, w (dGeomSetQuaternion(w, x, y, z) via phys_body_rotate_xform;
 *                         a geom just created has the identity, 0, 0, 0, 1)
 * The world-space triangle vertex is R * (double)(float)(scale * v) + pos in fp64, R = dQtoR(w, x, y, z).
 * clapgpu_trimesh_create copies the arrays, checks them (may synchronise: a set-up call) and builds one BVH over every
 * triangle of every mesh.  CLAPGPU_ERR_INVALID_ARGUMENTS: a NULL desc or out; n_meshes == 0 with any array given, or
 * n_meshes > 0 with any array missing or n_statics == 0 (all before any HIP call); ranges that do not ascend from 0; a
 * vertex index at or beyond its mesh's vertex count; a static_index >= n_statics or listed twice.
 * clapgpu_trimesh_pose: new pos / quat (device arrays as above) for every mesh, then the same bake and rebuild as create.
 * clapgpu_trimesh_status: host sync; *depth = the tree's height (edges from the root to the deepest leaf; at most 62,
 * 0 without triangles), *n_tris = the triangles of all meshes.
 * A static's broadphase AABB must hold its posed mesh: the mesh contacts below only see pairs the broadphase found.  A
 * mesh that leaves the box it was created with: give the static its new box first (clapgpu_bp_statics_update), then pose.
 * Where few of the meshes move, pose those alone: clapgpu_trimesh_pose_meshes on a set in parts (below).
 */
typedef struct clapgpu_trimesh_desc {
    uint32_t        n_meshes, n_statics;
    const uint32_t *static_index;
    const uint32_t *vx_first, *tri_first;
    const float    *vx;
    const uint16_t *idx;
    const float    *scale;
    const double   *pos;
    const float    *quat;
} clapgpu_trimesh_desc;
int  clapgpu_trimesh_create(void *stream, clapgpu_trimesh **out, const clapgpu_trimesh_desc *d);
int  clapgpu_trimesh_pose(void *stream, clapgpu_trimesh *mesh, const double *pos, const float *quat);
int  clapgpu_trimesh_status(void *stream, const clapgpu_trimesh *mesh, uint32_t *depth, uint32_t *n_tris);
void clapgpu_trimesh_destroy(clapgpu_trimesh *mesh);

/*
 * A mesh set "in parts" (ABI 47): the same object for every entry point that takes a clapgpu_trimesh, with the same
 * answers bit for bit, built so that posing some meshes costs those meshes.  clapgpu_trimesh_create_parts takes the
 * descriptor of clapgpu_trimesh_create, checks it the same way, returns the same errors in the same order and
 * synchronises.  The node array (max(T - 1, 1) nodes of 64 B, the root at node 0) holds one subtree per PART (a mesh
 * with a triangle) and a top tree over the parts:
 *   a part        its leaf slots are [tri_first[m], tri_first[m + 1]); its k - 1 nodes are one BVH2 by the rule of the
 *                 plain set over keys of the UNPOSED mesh (30-bit Morton code of the scaled model-space centroid within
 *                 the mesh's own centroid bounds, the triangle's index below it).  A pose changes no key, leaf order or
 *                 link of it.  A part of one triangle has no node: its root is the leaf link
 *   the top tree  the parts sorted by (30-bit Morton code of the centre of the part's root box within the bounds of all
 *                 such centres, a centre with a NaN: code 0; then mesh index); balanced: a node covering [lo, hi) splits
 *                 at lo + (hi - lo + 1) / 2; height ceil(log2 P); with one part, node 0 is that part's root
 * Boxes as in the plain set (float, rounded outward from the fp64 bake, a child box the exact union of what is below it).
 * The image (nodes, slots, keys) is a function of the descriptor and the poses alone.  CLAPGPU_ERR_TOO_LARGE, no object:
 * top height plus the deepest part's height above 62 (the walk's stack).  Neither height depends on a pose.
 * clapgpu_trimesh_status reports their sum: an upper bound of the tree's height, which is what the stack needs (the
 * balanced top has its leaves on two levels, so where the deepest part hangs from a shorter branch the walked height
 * is one less).  clapgpu_trimesh_pose on a set in parts takes every mesh's pose, bakes and
 * refits (no triangle is sorted) and clears the sticky flags below.
 *
 * clapgpu_trimesh_pose_meshes: mesh[n_moved], pos[n_moved][3], quat[n_moved][4] are DEVICE arrays; row k is the new pose
 * of mesh mesh[k].  Afterwards the set is, byte for byte, the set clapgpu_trimesh_create_parts makes of the same
 * descriptor with those poses replaced: the listed meshes' triangles are baked into their slots, their parts' boxes refit,
 * the P part keys sorted and the top tree rebuilt; no triangle of another mesh is read.  No host synchronisation and no
 * allocation: a captured graph may hold the call.  n_moved == 0: CLAPGPU_OK, nothing launched.  A listed mesh without
 * triangles changes only its stored pose.  CLAPGPU_ERR_INVALID_ARGUMENTS before any HIP call: a NULL set, a plain set, a
 * NULL array with n_moved > 0.  Sticky flags (until the next clapgpu_trimesh_pose): CLAPGPU_TRIMESH_POSE_RANGE a
 * mesh[k] >= n_meshes (skipped); CLAPGPU_TRIMESH_POSE_TWICE a mesh listed more than once (its lowest list position wins).
 * After an error the set may be half posed: a clapgpu_trimesh_pose that succeeds makes it whole.
 *
 * clapgpu_trimesh_parts_status: host sync; out[0] 1 for a set in parts else 0, out[1] the top tree's height, out[2] the
 * deepest part's, out[3] the sticky flags.
 * clapgpu_trimesh_read (tests and tools, either kind of set): host sync; into HOST arrays, each may be NULL: nodes
 * [max(T - 1, 1)][64 B], key [T][2] (static, triangle of its mesh) and tri [T][9] in leaf order, part_root [n_meshes]
 * (the part's root link, 0xffffffff for a mesh without triangles; must be NULL for a plain set).
 */
#define CLAPGPU_TRIMESH_POSE_RANGE 1u
#define CLAPGPU_TRIMESH_POSE_TWICE 2u
int  clapgpu_trimesh_create_parts(void *stream, clapgpu_trimesh **out, const clapgpu_trimesh_desc *d);
int  clapgpu_trimesh_pose_meshes(void *stream, clapgpu_trimesh *set, uint32_t n_moved, const uint32_t *mesh, const double *pos,
                                 const float *quat);
int  clapgpu_trimesh_parts_status(void *stream, const clapgpu_trimesh *set, uint32_t out[4]);
int  clapgpu_trimesh_read(void *stream, const clapgpu_trimesh *set, void *nodes, uint32_t *key, double *tri, uint32_t *part_root);

/*
 * Contacts against the mesh set: near_callback's dCollide for (body, static) pairs whose static owns a mesh, and the
 * capsule sweep against meshes (clapgpu_sweep_capsules with a mesh set).  ODE's trimesh colliders (dCollideSTL,
 * dCollideCCTL, OPCODE) are an absent submodule of the reference: the rule below is this project's own, PARITY UNPINNED.
 *
 * Sphere / capsule against one triangle (tricontact_dev.h).  The body geom is a segment a, b with radius r: a capsule's
 * ends pos + axis * length / 2 and pos - axis * length / 2, a sphere's centre twice (a capsule of length 0).  The
 * triangle (v0, v1, v2) is the mesh set's fp64 bake.  fp64, no FMA contraction.  Normals point from the static towards
 * the body (as in sphere-box); depth >= 0 is a contact.
 *   1. n = (v1 - v0) x (v2 - v0).  n == 0: no contact.  Otherwise n^ = n / |n|.
 *   2. sa, sb = the signed distances (p - v0) . n^ of a and b; m = min(sa, sb); e = the endpoint attaining m, a on a tie.
 *   3. Face: the segment meets the closed triangle, or -r < m <= 0 and e projects into the closed triangle.  One
 *      contact: normal n^, depth r - m, pos e - m n^ (a half-sunk sphere, or a capsule whose foot went through the
 *      ground, is pushed back out along the face).
 *   4. Parallel: a != b, m > 0, |sa - sb| <= 1e-5 |b - a|, both endpoints project into the triangle and
 *      max(sa, sb) <= r.  Two contacts (the record's second slot, as dCollideCapsuleCapsule's parallel case), at a's and
 *      then b's projection: normal n^, depths r - sa and r - sb.  A sphere never takes this case.
 *   5. Otherwise the closest points p on the segment and q on the triangle, at distance d: a contact when 0 < d <= r and
 *      (p - q) . n > 0: normal (p - q) / d, depth r - d, pos q.  A closest point behind the face is no contact (that
 *      is a neighbouring face's contact, or nothing).
 * Depth and normal are unique under the rule; pos may lie anywhere on a tied closest set.  Box bodies and OTHER bodies
 * have no triangle collider here: no mesh contacts.
 *
 * clapgpu_contacts_meshes: for the (body, static) candidate pairs of clapgpu_bp_collide (static_pairs /
 * static_pair_total / static_capacity as clapgpu_contacts_geoms takes them) whose static owns a mesh of `meshes`: the
 * mesh's triangles whose boxes meet the body geom's box (through the BVH), each collided by the rule.  One
 * clapgpu_contact2 per touching (pair, triangle), nc 1 or 2, with mesh_ref[k][2] = (static pair index, triangle index
 * within the mesh).  Canonical order: ascending pair index, then ascending triangle index; the same bits whatever the
 * launch shape.  Surface parameters: phys_contact_surface of the body's and the static's material (as the other lists);
 * touching bodies get CLAPGPU_BODY_HAS_JOINT in body_flags (may be NULL).
 * MAX_CONTACTS (physics.c:150, 413): a pair keeps at most 16 contacts, a two-contact record counting two.  Its records
 * are ordered deeper first (a record's depth: the deeper of its contacts), then lower triangle index, and taken in that
 * order while they fit (the first that does not fit ends the pair's list); the kept ones are written in triangle
 * order.  *capped_pairs (may be NULL) = the pairs that dropped records.  *contact_total (may be NULL) = the records
 * kept, at most `capacity` of them written (16-byte aligned).  scratch: CLAPGPU_MESH_CONTACT_SCRATCH(static_capacity)
 * uint32 of device memory (static_capacity + 1 always suffices), overwritten.  No host synchronisation and no
 * allocation: a captured graph can hold the call.  meshes must have been created with n_statics == statics->n
 * (CLAPGPU_ERR_INVALID_ARGUMENTS otherwise).
 * Precondition: a pair is only found if the static's broadphase AABB holds its posed mesh.
 * The list is additive: clapgpu_contacts_geoms[_both] are unchanged, and a meshed OTHER static still gets nc = 0
 * there.  A mesh given to a sphere, capsule or box static adds mesh contacts on top of that static's own record (the
 * loader meshes only trimesh statics).
 */
#define CLAPGPU_MESH_CONTACT_SCRATCH(static_capacity) (((static_capacity) + 63u) / 64u + 1u)
int  clapgpu_contacts_meshes(void *stream, const clapgpu_geoms *bodies, const clapgpu_geoms *statics,
                             const clapgpu_trimesh *meshes, const uint32_t *static_pairs, const uint32_t *static_pair_total,
                             uint32_t static_capacity, uint32_t *scratch, uint32_t capacity, clapgpu_contact2 *contacts,
                             uint32_t *mesh_ref, uint32_t *contact_total, uint32_t *capped_pairs, uint32_t *body_flags);

/*
 * clapgpu_sweep_capsules_grid: clapgpu_sweep_capsules without candidate lists from the host, as
 * phys_body_sweep_capsule takes none (it collides the probe with phys->space, physics.c:559-670).  Sweep k behaves as
 * clapgpu_sweep_capsules would with this list: every static, then every body (bit 31 set), in ascending index,
 * whose AABB (statics->aabb, b->aabb) meets the probe's swept box -- the union of b->aabb[sweep_body[k]] and the same
 * box moved by delta[k], closed overlap.
 *   - Contacts are taken in candidate order, 16 a step, and a candidate that does not touch contributes none: any
 *     superset of that list in the same relative order gives the same bits.  The gather may hold more than the box asks
 *     for (it grows the box by a relative 2^-40; without b->aabb or statics->aabb every geom of that set is held), never
 *     less.
 *   - The order is canonical whatever the gather: statics before bodies, each ascending, no geom twice.
 * bp == NULL: every geom's box is tested (the brute-force path).  Else `bp` must hold an index over (b->n, b->aabb) and
 * have been created with statics->n statics (CLAPGPU_ERR_INVALID_ARGUMENTS otherwise, as clapgpu_ray_cast), and the
 * swept box's cells and their blocks' static lists are looked up instead; same bits.  A sweep scans every geom when an
 * indexed box is larger than a cell, when the boxes were binned again since the index, or when its swept box covers
 * more cells than a scan tests geoms per lane, or when statics->aabb is NULL.  A list of more than 512 candidates is not kept: that sweep tests every
 * geom's box at every step (same bits).  meshes: NULL, or created with n_statics == statics->n.
 * One wavefront per sweep (with a mesh set: per workgroup); no host synchronisation, no allocation: a captured graph can
 * hold the call.  Nothing moves and the index stays valid.  Out: frac / normal / hit as clapgpu_sweep_capsules, and
 * flags[k] (may be NULL):
 *   CLAPGPU_SLIDE_INVALID     sweep_body[k] >= b->n or a non-finite delta: frac 1, normal (0, 1, 0), hit -1
 *   CLAPGPU_SLIDE_UNRESOLVED  the swept box meets the AABB of a CLAPGPU_GEOM_OTHER static that owns no mesh of `meshes`:
 *                             the sweep saw nothing of it, the host redoes it
 */
#define CLAPGPU_SLIDE_INVALID      1u
#define CLAPGPU_SLIDE_UNRESOLVED   2u
#define CLAPGPU_SLIDE_MOVED_TARGET 4u  /* clapgpu_characters_slide: a mover that gave this one's probe a contact moved too */
int  clapgpu_sweep_capsules_grid(void *stream, clapgpu_bp *bp, const clapgpu_bodies *b, const clapgpu_geoms *statics,
                                 const clapgpu_trimesh *meshes, uint32_t n_sweeps, const uint32_t *sweep_body,
                                 const float *delta, float *frac, float *normal, int32_t *hit, uint32_t *flags);

/*
 * clapgpu_characters_slide: the ENTITY3D_HAS_PHYSICS branch of character_apply_velocity (character.c:254-310) for the
 * bodies body[k] of a batch, each at most once; velocity[k] = ch->velocity (in / out), airborne[k] = ch->airborne.
 *   dt_sec   the raw frame delta: below 1e-6 the call changes nothing at all (:259-260, the goto also skips the
 *            velocity reset); above 1.0 / 30.0 it is 1.0 / 30.0 (:262-263)
 *   deltas   grounded, or airborne with velocity[1] > 0: vec3_scale(velocity, (float)dt), one character_sweep_delta
 *            call (min_normal_y -1, stop_on_block true).  Falling: {0, (float)((double)velocity[1] * dt), 0} with
 *            (0.5, false), then x and z likewise with (-1, true) (:293-298).  velocity[k][1] becomes 0 when the rising
 *            call or the falling call's vertical sweep returns less than 1 (:283, :299)
 *   character_sweep_delta (:193-243) in float as written: the |delta| < 1e-6f exit, the normal[1] < min_normal_y
 *            filter, the move by vec3_scale(delta, frac) when frac > 0 as phys_body_move does it (pos + (double)step),
 *            the two exits, the projection of the remaining delta with linmath's accumulation order; at most three
 *            sweeps a call.  Each sweep is clapgpu_sweep_capsules_grid's from the mover's running position.
 *   first_frac[k][2]  the return value of each character_sweep_delta call, 1 where not made
 *   push_hit[k][6]    per sweep in call order (call * 3 + iteration): the body phys_body_push would push (frac < 1 after
 *                     the filter and a body was hit), else -1.  The push itself (dBodyAddForce): clapgpu_bodies_push, with
 *                     a copy of velocity[] taken BEFORE this call (it zeroes velocity[k][1])
 * Then phys_body_set_velocity(0) (:310): the mover's lvel is 0, and one launch writes its final pos, axis, aabb and
 * geom record as clapgpu_bodies_aabb writes them.  Between the launches a mover's final position travels in its lvel.
 * One batch, poses from before the call (as clapgpu_bodies_ground_collide): a mover sees its own running position and
 * everything else where it was before the call.  flags[k]:
 *   CLAPGPU_SLIDE_INVALID       body[k] >= b->n, a body listed more than once (every listing), or a non-finite delta
 *   CLAPGPU_SLIDE_UNRESOLVED    a sweep's box met an OTHER static without a mesh
 *                               -- both move nothing and keep velocity[k]; first_frac 1, push_hit -1
 *   CLAPGPU_SLIDE_MOVED_TARGET  a body that gave this mover's probe a contact at any step is itself a mover of this
 *                               batch that ended somewhere else.  The flag is a SUPERSET of that: with contacts from
 *                               several movers of the batch it is set without asking whether they moved.  The mover has moved; the call
 *                               that moves a crowd in list order is clapgpu_characters_move_ordered
 * scratch: [b->n] uint32 of device memory, overwritten.  bp: NULL or an index over (b->n, b->aabb); cleared on return
 * (bodies moved) unless dt_sec < 1e-6.  No host synchronisation, no allocation.
 */
typedef struct clapgpu_slide {
    uint32_t        n;
    const uint32_t *body;        /* [n] index into the bodies, each at most once */
    float          *velocity;    /* [n][3] in/out: character.velocity */
    const uint8_t  *airborne;    /* [n] character.airborne */
    float          *first_frac;  /* [n][2] out */
    int32_t        *push_hit;    /* [n][6] out */
    uint32_t       *flags;       /* [n] out: CLAPGPU_SLIDE_* */
} clapgpu_slide;
int  clapgpu_characters_slide(void *stream, clapgpu_bp *bp, const clapgpu_bodies *b, const clapgpu_geoms *statics,
                              const clapgpu_trimesh *meshes, double dt_sec, const clapgpu_slide *s, uint32_t *scratch);

/*
 * clapgpu_bodies_push: the phys_body_push(hit, push_velocity, push_mass) calls of a slide batch (character.c:219-221,
 * physics.c:677-693: dBodyEnable, then dBodyAddForce), applied as the reference applies them: mover 0's pushes in call
 * order (slot q = call * 3 + iteration), then mover 1's, and so on.  PARITY UNPINNED (ODE absent).
 *   pusher[k]     the mover's body (clapgpu_slide.body); its mass is (float)b->mass[pusher[k]], as phys_body_get_mass
 *                 returns it
 *   velocity[k]   the velocity character_sweep_delta was given: the slide's INPUT, copied before the slide zeroed
 *                 velocity[k][1]
 *   push_hit[k][6], flags[k] (may be NULL: all 0)   as clapgpu_characters_slide left them
 * The force of slot (k, q) on body h = push_hit[k][q] is (double)(pusher_mass * velocity[k][j]), the product formed in
 * float.  A slot with h < 0 or h >= b->n pushes nothing; a mover with pusher[k] >= b->n or flags[k] != 0 pushes nothing
 * (an INVALID or UNRESOLVED mover is redone by the host, pushes included; clapgpu_characters_move_ordered leaves no
 * MOVED_TARGET mover).  The same body may stand in
 * many slots and under many movers.  Every pushed body h:
 *   b->facc[h][j] += each force, one fp64 add per push, in ascending (k, q) order -- the reference's sequential sum, bit
 *                 for bit, whatever the scheduling (no atomics on the doubles: the slots are sorted by (h, k, q) and one
 *                 lane walks each body's run)
 *   dBodyEnable, also on a KINEMATIC body: bflags[h] &= ~CLAPGPU_BODY_DISABLED, adis_steps_left[h] = w->adis_steps,
 *                 adis_time_left[h] = w->adis_time; the sample ring is left alone
 *   pushed[h]     (may be NULL) the number of pushes it received; written for all b->n bodies, 0 for the rest
 * b->facc is required.  n == 0 returns CLAPGPU_OK and touches nothing.  n above 2^28 is CLAPGPU_ERR_TOO_LARGE.
 * scratch: clapgpu_bodies_push_scratch_bytes(n) bytes of device memory, 256-byte aligned, overwritten (two key arrays and
 * the sort's work space).  The size depends on the device's sort tuning: the helper needs clapgpu_init to have run and
 * returns 0 when it cannot tell (or for n == 0 or n too large).  No host synchronisation, no allocation: a captured
 * graph can hold the call, after the slide it belongs to.
 */
size_t clapgpu_bodies_push_scratch_bytes(uint32_t n);
int  clapgpu_bodies_push(void *stream, const clapgpu_bodies *b, const clapgpu_world *w, uint32_t n, const uint32_t *pusher,
                         const float *velocity, const int32_t *push_hit, const uint32_t *flags, uint32_t *pushed,
                         void *scratch);

/*
 * clapgpu_bodies_islands: the island pass of dWorldQuickStep (physics.c:769) -- what phys_body_new relies on when it puts
 * every dynamic body on auto-disable: "ODE re-enables them automatically when another enabled body collides with them"
 * (physics.c:1034-1042).  ODE 0.16 util.cpp, dxProcessIslands, restated; PARITY UNPINNED (ODE absent).  Run it after a
 * substep's contact launches (they give the pair list, the records' nc and CLAPGPU_BODY_HAS_JOINT) and before
 * clapgpu_bodies_step / _step_prebin:
 *   seed   every enabled body with CLAPGPU_BODY_AUTO_DISABLE and CLAPGPU_BODY_HAS_JOINT does the auto-disable bookkeeping
 *          of clapgpu_bodies_step (h, the sample ring, both counters, DISABLED and zeroed velocities when both are spent:
 *          the same statements, the same bits); then CLAPGPU_BODY_HAS_JOINT is cleared on EVERY body (dJointGroupEmpty moved
 *          forward), so the step that follows does no bookkeeping of its own and integrates the enabled bodies
 *   link   pair k < min(*pair_total, capacity) joins bodies pairs[2k] and pairs[2k+1] when
 *          (contacts[k].nc & ~CLAPGPU_CONTACT_DEEP) >= 1; a pair with an index >= b->n or with both indices equal is
 *          ignored, a pair listed twice is harmless.  A contact with a static or a mesh links nothing; a KINEMATIC body
 *          links like any other
 *   wake   a DISABLED body whose component holds at least one body that is enabled after the seed loses
 *          CLAPGPU_BODY_DISABLED.  Nothing else of it changes (ODE clears the flag without dBodyEnable): counters, sample
 *          ring, velocities and facc stay.  So a body the seed has just put to sleep beside an awake neighbour is stepped
 *          in this very substep, from zero velocity, with spent counters; a component without an enabled body sleeps on
 *   island[i]     (device, may be NULL) the smallest body index of i's component, i itself for a body in no touching pair:
 *                 the same bits whatever order the atomics took
 *   *woken_total  (device, may be NULL) the number of flags the wake cleared
 * A KINEMATIC, DISABLED character that touches an awake dynamic body is enabled too; it has no AUTO_DISABLE flag, so it
 * stays enabled, and the step treats it as kinematic only when the bodies have an accumulator (b->facc: the rule at
 * clapgpu_bodies_step).
 * scratch: clapgpu_bodies_islands_scratch_bytes(b->n) bytes of device memory, 256-byte aligned, overwritten (the
 * union-find's n parent words, n marks, n roots).  Four launches (three when capacity is 0), no allocation, no host
 * synchronisation: a captured graph can hold the call.  b->n == 0 returns CLAPGPU_OK and launches nothing.  pairs 8-byte,
 * contacts 16-byte aligned.
 */
size_t clapgpu_bodies_islands_scratch_bytes(uint32_t n);
int  clapgpu_bodies_islands(void *stream, const clapgpu_bodies *b, const clapgpu_world *w, double h,
                            const uint32_t *pairs, const uint32_t *pair_total, uint32_t capacity,
                            const clapgpu_contact2 *contacts, void *scratch, uint32_t *island, uint32_t *woken_total);

/*
 * clapgpu_bodies_solve: contact response -- the constraint stage of dWorldQuickStep (physics.c:769) for the contact joints
 * near_callback creates ("rely on contact joints and ERP for penetration resolution", physics.c:433-438).  The records of a
 * substep's three contact lists become quickstep's contact rows and are relaxed by its SOR iteration, one solve per
 * island, islands in parallel.  ODE 0.16 (joints/contact.cpp, quickstep.cpp) restated, with ONE deliberate
 * difference: ODE reorders its rows at random, here the row order is the canonical order of the lists.  The rule below is
 * this library's own contract, restated independently in tests/solveref.py and held to bit equality; PARITY UNPINNED (ODE
 * is absent from the reference).  fp64, no FMA contraction, every sum left to right in the order written.  What the rule
 * means -- the boxed LCP  A = J invM J^T + diag(cfm / h),  b = c / h - J (v / h + invM f_ext) -- is stated densely in
 * tests/lcpref.py, and both the restatement (on the CPU) and these kernels (on the device) are held to its solution.
 *
 * Call it after clapgpu_bodies_islands and before clapgpu_bodies_step[_prebin] of the same substep.  It changes lvel and
 * avel of enabled, non-kinematic bodies that a row names, and nothing else of the bodies.
 *
 * Contacts and their order.  A record contributes min(nc & ~CLAPGPU_CONTACT_DEEP, 2) contacts (a DEEP record: none).
 * Body 1 is the pair's first index; body 2 is the second index of a body pair and nothing for a static or a mesh contact,
 * whose body is static_pairs[2 k] resp. static_pairs[2 mesh_ref[2 k]].  A contact is ACTIVE when body 1 is enabled (after
 * the island pass all bodies of a component share that state).  Ignored like an inactive one: a record past
 * min(*total, capacity) of its list, a body index >= b->n, a body pair with both indices equal, a mesh_ref past the
 * static pairs, island[body 1] >= b->n.  The canonical contact order runs through the static list by record index, then
 * the mesh list, then the body list; within a record slot 1, then slot 2 (the reference's joint-creation order: ground
 * pass first, physics.c:751-753, with list order in place of the hash space's traversal).  A contact has its normal row
 * and, when mu > 0, two friction rows behind it; the ordinal of a row is its position in that order.  The contact's
 * island is island[body 1]; row_key = ((uint64_t)island << 32) | ordinal.
 *
 * Rows (dxJointContact::getInfo2 as the reference configures it: SoftERP | SoftCFM [| Bounce], mu2 unused, no Approx1).
 * With r_i = pos - pos_i (b->pos), x the cross product (r x n = (r1 n2 - r2 n1, r2 n0 - r0 n2, r0 n1 - r1 n0)):
 *   a row along direction u:  J1l = u, J1a = r1 x u, J2l = -u, J2a = -(r2 x u)
 *   normal row    u = n; c = (soft_erp / h) * depth; when mode has CLAPGPU_CONTACT_BOUNCE: out = J . (v1, w1, v2, w2), and if
 *                 bounce_vel >= 0 and -out > bounce_vel then newc = (-bounce) * out, c = newc if newc > c;
 *                 cfm = soft_cfm, lo = 0, hi = +inf
 *   friction rows u = t1, then u = t2, from dPlaneSpace(n): if |n[2]| > M_SQRT1_2: a = n1 n1 + n2 n2, k = 1 / sqrt(a),
 *                 t1 = (0, -n2 k, n1 k), t2 = (a k, -n0 t1[2], n0 t1[1]); else a = n0 n0 + n1 n1, k = 1 / sqrt(a),
 *                 t1 = (-n1 k, n0 k, 0), t2 = (-n2 t1[1], n2 t1[0], a k).  c = 0, cfm = s->cfm, lo = -mu, hi = +mu: a
 *                 force limit, as ODE has it without Approx1
 * n points from the static towards the body and from body 2 to body 1, so a positive lambda pushes body 1 out.
 * Whatever belongs to an absent body 2 is skipped in every sum (not added as zero).
 *
 * Masses.  invM = 1 / mass, 0 for a CLAPGPU_BODY_KINEMATIC body; invI = R diag(1 / inertia) R^T with R = dQtoR(quat),
 * built as the step builds its tensors (tmp = D R^T, invI = R tmp); all zeros for a kinematic body or when b->inertia is
 * NULL.  iMJ = (invM1 J1l, invI1 J1a, invM2 J2l, invI2 J2a), a matrix row times the vector summed left to right.
 * Right-hand side.  f_ext = facc + (NO_GRAVITY ? 0 : m g) (facc taken as 0 when b->facc is NULL); no external torque,
 * the gyroscopic term stays the step's.
 *   rhs = c / h - [ J1l . (v1 / h + invM1 f_ext1) + J1a . (w1 / h) + J2l . (v2 / h + invM2 f_ext2) + J2a . (w2 / h) ]
 * one running sum over the twelve products in that order.  The step that follows adds h invM f_ext itself; the solve
 * anticipates it, as quickstep does.
 * Iteration.  d = iMJ . J (body 1 linear xyz, angular xyz, body 2 linear xyz, angular xyz) + cfm / h; Ad = sor_w / d.  A row
 * with d == 0 is dropped: it keeps its ordinal and lambda = 0.  Each island starts from lambda = 0 and a = 0 (six doubles
 * per body).  For `iterations` sweeps, for each row of the island in canonical order:
 *   delta = Ad * ((rhs - (cfm / h) * lambda) - J . a)      J . a over body 1's six, then body 2's six
 *   lambda' = lambda + delta; if lambda' < lo: lo; if lambda' > hi: hi
 *   a += iMJ * (lambda' - lambda);  lambda = lambda'
 * After the sweeps lvel += h * a_lin and avel += h * a_ang for every enabled, non-kinematic body named by an active row.
 *
 * Levels.  The row order matters only between rows that share a body: a row reads and writes the six a of its one or
 * two bodies and its own lambda, nothing else.  Walking an island's rows in canonical order,
 *   level(row) = 1 + max(level of the latest earlier row of the island naming body 1, the same for body 2)
 * with 0 where no earlier row names the body; an absent body 2 (a static or a mesh contact) is no dependency, a KINEMATIC
 * body is a body like any other, and a dropped row (d == 0) takes part with its bodies like any other row although it does
 * nothing in the sweeps, so the levels depend on the lists alone and never on arithmetic.  Rows of one level name disjoint
 * bodies.  Running every sweep as level 1, then level 2, ..., the rows of a level in any order or at once, gives each row
 * the operands the sequential walk gives it: the same bits, no sum reordered.  tests/solvelevelref.py restates the rule.
 *
 * What is parallel.  Islands run side by side.  An island with fewer than s->wide_rows rows (every island when wide_rows
 * is 0) is walked by one lane, row after row.  An island with at least wide_rows rows is walked by one 256-thread
 * workgroup: its first wavefront takes the levels, 64 rows at a time; the workgroup buckets the rows by level and runs
 * the sweeps level by level with a workgroup barrier behind each level.  CLAPGPU_SOLVE_WIDE_WORKGROUPS workgroups (fewer
 * when rows_capacity is smaller) stride over the wide islands; no grid depends on a count only the device knows.
 * What stays sequential.  The depth: an island costs as many dependent steps per sweep as it has levels, the longest
 * chain of rows that share bodies.  A square grid of piled spheres whose pairs are listed by first index has about four levels per grid line
 * (253 for 64 x 64 spheres and their 12 160 rows); a tower listed bottom-up, where every row shares a body with the row before, has one row per level and
 * gains nothing -- it only pays the barriers.  The order of the pair list decides the depth, the result never.
 *
 * Each list may be absent (a NULL pointer or capacity 0); the mesh list needs static_pairs and static_pair_total.
 * rows_capacity: the most rows the call can hold.  When the rows do not fit, the launches -- which read the total on the
 * device, where alone it is known -- apply nothing and OR 1 into *status (the caller clears it).  row_lambda
 * [rows_capacity] and row_key [rows_capacity] (device, may be NULL) receive lambda and the key of every row at its
 * ordinal; *rows_total (device, may be NULL) the number of rows.  row_level [rows_capacity] (device, may be NULL, 4-byte
 * aligned) receives at every row's ordinal its level (>= 1) when its island was solved by a workgroup and 0 when by one
 * lane (all 0 when the rows do not fit); *wide_total (device, may be NULL, 4-byte aligned) the number of islands solved by
 * a workgroup.
 * scratch: clapgpu_bodies_solve_scratch_bytes(b->n, rows_capacity) bytes of device memory, 256-byte aligned, overwritten;
 * the caller need not clear it between calls; its size does not depend on wide_rows.  Four launches (five when wide_rows
 * is not 0) and a rocPRIM radix sort of the row keys inside the scratch, no allocation, no host synchronisation: a captured graph can hold the call.  b->n == 0 returns CLAPGPU_OK and launches
 * nothing; without any list nothing changes and *rows_total = 0.  Pairs 8-byte, records 16-byte aligned.
 */
#define CLAPGPU_SOLVE_WIDE_WORKGROUPS 1024u    /* the most workgroups the wide sweep launches */
/* wide_rows: an island with at least this many rows is solved by a workgroup, level by level; 0: never */
typedef struct clapgpu_solver { uint32_t iterations; uint32_t wide_rows; double sor_w; double cfm; } clapgpu_solver;
/* 20, 1.3, 1e-10: ODE's dDOUBLE defaults, physics.c:1127-1128 leave them; wide_rows 64: the measured crossover (profiles/solve) */
void   clapgpu_solver_defaults(clapgpu_solver *s);
size_t clapgpu_bodies_solve_scratch_bytes(uint32_t n, uint32_t rows_capacity);
int    clapgpu_bodies_solve(void *stream, const clapgpu_bodies *b, const clapgpu_world *w, const clapgpu_solver *s, double h,
                            const uint32_t *island,   /* required: clapgpu_bodies_islands' output of this substep */
                            const uint32_t *static_pairs, const uint32_t *static_pair_total, uint32_t static_capacity,
                            const clapgpu_contact2 *static_contacts,
                            const clapgpu_contact2 *mesh_contacts, const uint32_t *mesh_ref,
                            const uint32_t *mesh_contact_total, uint32_t mesh_capacity,
                            const uint32_t *pairs, const uint32_t *pair_total, uint32_t capacity,
                            const clapgpu_contact2 *contacts,
                            uint32_t rows_capacity, void *scratch,
                            double *row_lambda, uint64_t *row_key,
                            uint32_t *rows_total, uint32_t *status,
                            uint32_t *row_level, uint32_t *wide_total);

/* ======================================================================== */
/* Characters: the feeder in front of default_update (core/character.c)      */
/* ======================================================================== */

#define CLAPGPU_POS_HISTORY_MAX 8      /* POS_HISTORY_MAX, character.h:21 */

/*
 * struct character's per-frame feeder state (character.h:25-50), SoA over the characters of the
 * scene in list order (scene->characters, character.c:627):
 *   entity[c]         slot of character.entity in the entity SoA
 *   body[c]           index into clapgpu_bodies of its phys body, or -1 (no ENTITY3D_HAS_PHYSICS);
 *                     NULL = no character has one.  Give such bodies body_entity = -1 in
 *                     clapgpu_phys_body_update: characters sync themselves here and keep their rotation
 *   hist_pos[c][8][3], hist_head[c], hist_wrapped[c]   character.history (in/out)
 *   airborne[c]       character.airborne (written by the host's character_move)
 *   moved[c]          out: phys_body_update() reported motion -> host calls character_set_moved()
 *   limbo_height      scene.limbo_height (scene.h:52)
 */
typedef struct clapgpu_characters {
    uint32_t        n;
    float           limbo_height;
    const uint32_t *entity;
    const int32_t  *body;
    float          *hist_pos;
    uint32_t       *hist_head;
    uint8_t        *hist_wrapped;
    const uint8_t  *airborne;
    uint8_t        *moved;
} clapgpu_characters;

/*
 * character_update() (character.c:583-611) for every character, without its tail call: limbo
 * teleport out of the position history, body read-back (position only) + history_push when the
 * body moves.  Writes the entity SoA (pos, CLAPGPU_E_DIRTY) and, on a teleport, the body position
 * (y + yoffset, phys_body_set_position).  Run before clapgpu_entities_update (= the chained
 * orig_update).  b may be NULL when no character has a body.
 */
int clapgpu_characters_update(void *stream, const clapgpu_characters *c, const clapgpu_entities *e,
                              const clapgpu_bodies *b);
/* ... and animated_update's clock (clapgpu_animation_time; now_dev != NULL: clapgpu_animation_time_dev) in the same launch:
 * two per-character passes over different state, both in front of kernels that wait for them.  Same results. */
int clapgpu_characters_update_clock(void *stream, const clapgpu_characters *c, const clapgpu_entities *e, const clapgpu_bodies *b,
                                    const clapgpu_anim_clock *clk, double now, const double *now_dev);

/*
 * clapgpu_characters_move: character_move (character.c:450-537) for a batch of characters that have a body, as one call
 * without host synchronisation: the ground ray (:454), the airborne / jump / walking decision (:464-532) and the
 * ENTITY3D_HAS_PHYSICS branch of character_apply_velocity with its pushes.  It is scene_characters_move's body
 * (clap.c:589), which runs before phys_step.  What stays with the host, from the outputs: the animation side of
 * character_set_state and ch->state itself (request), connect / disconnect (collision), character_set_moved (applied),
 * character_debug, dash and input handling, characters without a body (transform_move).  (From ABI 46 the first of these
 * can follow on the device: clapgpu_characters_state, below.)  PARITY UNPINNED (ODE absent):
 * the rule below is the library's own contract; tests/moveref.py restates it.
 *
 * Mover k, all arithmetic in float exactly as character.c writes it, no FMA, linmath's loops in their own order:
 *   1. Ground ray.  grounded[k] = !airborne[k]; the ray is clapgpu_bodies_ground_collide's and snaps the body as
 *      that call does.  normal[k] is written only on a hit, collision[k] = the hit (body i, -2 - s) or -1 on a miss,
 *      airborne[k] = !grounded_out.  A ray flagged CLAPGPU_RAY_INVALID or CLAPGPU_RAY_UNRESOLVED ends the mover here:
 *      velocity, normal and airborne unchanged, request 0xff, applied 0, first_frac 1, push_hit -1; the host redoes it.
 *      CLAPGPU_RAY_MOVED_TARGET is reported and the mover goes on.
 *   2. Jump protection (:464): state == JUMPING && velocity[1] > 0 sets airborne = 1.
 *   3. Airborne (:467-488): when the raw dt_sec > 1e-6, velocity[1] = (float)((double)velocity[1] +
 *      (double)(float)w->gravity[1] * dt_sec) and the mover slides (applied = 1); either way request = FALLING.
 *   4. Grounded.  jump[k] set (:501, :437-447): velocity = (dx * jump_forward, jump_upward, dz * jump_forward),
 *      request = JUMP_START, airborne = 1 when state == MOVING (:388), no slide.  Else vec3_len(motion) != 0 (:504):
 *      when vec3_len(normal) > 0, newz = cross((1, 0, 0), normal) and newx = cross(normal, newz) as vec3_mul_cross
 *      writes them (the products by 0 and 1 are made), each normalised by k = (float)(1.0 / (double)len) with the
 *      scaling in float (vec3_norm, vec3_scale); coef = 1 if state == MOVING else 0.3f; velocity[i] = newx[i] * (dx *
 *      coef) + newz[i] * (dz * coef) (:526).  Whatever the normal, request = MOVING; the mover slides (applied = 1) only
 *      when state >= IDLE (character_set_state's early return, :319-326).  Else request = IDLE.
 *   5. Slide and push.  The sliding movers go through clapgpu_characters_slide's own launches (dt_sec clamped there);
 *      the others stand in its list under the body index 0xffffffff, which the slide leaves alone, and the
 *      CLAPGPU_SLIDE_INVALID it gives such an entry is cleared.  The pushes go through clapgpu_bodies_push with the
 *      velocity of steps 3 and 4, from before the slide zeroed velocity[1].  A raw dt_sec < 1e-6 issues no slide or push
 *      launch; applied stays 1 for the grounded walkers (the reference still rotates them, :259-260, :312-313).
 *   6. Rotation hand-off (entity and yaw_quat given, both or neither): for every mover with applied == 1,
 *      e->rot[entity[k]] = yaw_quat[k] and e->flags[entity[k]] |= CLAPGPU_E_DIRTY (entity3d_rotate, :313).
 * One batch: every ground ray sees the poses from before the call, every slide the poses after all ground snaps.  The
 * reference moves one character at a time: flags[k] = the ray's CLAPGPU_RAY_* | the slide's CLAPGPU_SLIDE_* << 8, and
 * the MOVED_TARGET bit of either stage marks the movers this batch got wrong; clapgpu_characters_move_ordered (below)
 * moves a crowd in list order and leaves none.  A body listed more than once is INVALID
 * in both stages and stays (its normal[k] may hold its ray's).
 * Launches: the index (bp given), a launch that writes grounded[], the ground rays (+ the mesh pass) and their apply,
 * k_move_decide, the index again, the slide's, the push's, k_move_finish.  No allocation, no host synchronisation: a
 * captured graph can hold the call, dt_sec baked in as for the slide.  n == 0 returns CLAPGPU_OK and launches nothing.
 * CLAPGPU_ERR_INVALID_ARGUMENTS before any HIP call: a NULL m, b, w or statics; with n > 0 a missing array of m, only
 * one of entity / yaw_quat, the pair without e (or e without rot / flags), a missing b->facc or any other array of b the
 * three stages ask for, bp without b->aabb, a scratch that is NULL or not 256-byte aligned.
 * bp: NULL, or created with statics->n statics; the call indexes it itself and leaves it cleared.  meshes: NULL, or
 * created with n_statics == statics->n.  scratch: clapgpu_characters_move_scratch_bytes(b->n, n) bytes of device memory,
 * 256-byte aligned, overwritten: the [b->n] words the ray and the slide use one after the other, the slide's body list
 * and flags, the velocities given to the push, the grounded bytes in and out, the ray's distance and its mesh pass's
 * word, the push's scratch (the helper needs clapgpu_init, and returns 0 when it cannot tell or for n == 0).
 */
typedef struct clapgpu_move {
    uint32_t        n;
    const uint32_t *body;          /* [n] index into the bodies, each at most once */
    const double   *ray_off;       /* [n] phys_body.ray_off, as clapgpu_bodies_ground_collide takes it */
    const float    *motion;        /* [n][2] mctl dx, dz of this frame (ch->motion = {dx, 0, dz}) */
    const uint8_t  *state;         /* [n] ch->state, CS_* of character.h:10-19 (0 START, 1 WAKING, 2 IDLE, 3 MOVING,
                                      4 JUMP_START, 5 JUMPING, 6 FALLING) */
    const uint8_t  *jump;          /* [n] ch->jump && ch->can_jump */
    const float    *jump_params;   /* [n][2] jump_forward, jump_upward */
    float          *velocity;      /* [n][3] in/out ch->velocity */
    float          *normal;        /* [n][3] in/out ch->normal (kept on a ray miss) */
    uint8_t        *airborne;      /* [n] in/out ch->airborne */
    /* out */
    uint8_t        *request;       /* [n] the state character_move asks character_set_state for, or 0xff: none */
    uint8_t        *applied;       /* [n] 1: character_apply_velocity ran (host: character_set_moved, entity3d_rotate) */
    int32_t        *collision;     /* [n] ch->collision: body i, -2 - s, or -1 */
    float          *first_frac;    /* [n][2] as clapgpu_slide */
    int32_t        *push_hit;      /* [n][6] as clapgpu_slide */
    uint32_t       *flags;         /* [n] ray flags | slide flags << 8 */
    /* optional rotation hand-off, both or neither */
    const uint32_t *entity;        /* [n] slot in the entity SoA */
    const float    *yaw_quat;      /* [n][4] the host's quat for entity3d_rotate(e, 0, atan2f(dx, dz), 0), 16-byte aligned */
} clapgpu_move;
#define CLAPGPU_CS_START      0u   /* character_state, character.h:10-19 */
#define CLAPGPU_CS_WAKING     1u
#define CLAPGPU_CS_IDLE       2u
#define CLAPGPU_CS_MOVING     3u
#define CLAPGPU_CS_JUMP_START 4u
#define CLAPGPU_CS_JUMPING    5u
#define CLAPGPU_CS_FALLING    6u
#define CLAPGPU_CS_NONE       0xffu
size_t clapgpu_characters_move_scratch_bytes(uint32_t n_bodies, uint32_t n);
int    clapgpu_characters_move(void *stream, clapgpu_bp *bp, const clapgpu_bodies *b, const clapgpu_world *w,
                               const clapgpu_geoms *statics, const clapgpu_trimesh *meshes,
                               const clapgpu_entities *e /* NULL without the hand-off */,
                               double dt_sec /* raw frame delta */, const clapgpu_move *m, void *scratch);

/*
 * clapgpu_characters_order / clapgpu_characters_move_ordered (ABI 43): a crowd moved in list order.  The reference moves
 * one character at a time: each sees every earlier one where it ended up and every later one where it still stands.
 * clapgpu_characters_move_ordered gives, bit for bit, what clapgpu_characters_move gives when it is called once per mover
 * in list order -- every array of m and every array of b, facc, bflags and the auto-disable counters included -- and moves
 * together the movers that cannot reach each other.  No mover of an ordered call carries a MOVED_TARGET bit.
 *
 * Reach box of mover k: six doubles in the layout of clapgpu_bodies.aabb, from the inputs of the call before anything
 * moves; it holds everything the three stages of mover k can read of another geom or write of its own body, whatever
 * branch the decision takes (the proof stands next to the kernel, clap_amd/csrc/order.hip).  With bb = b->aabb[body[k]],
 * every operation in fp64, in this order, without FMA contraction (tests/orderref.py restates it bit for bit):
 *   roff = ray_off[k] - 0.05;  ray_len = yoffset - roff + 1e-3;  rl = ray_len > 0 ? ray_len : 0   (also for NaN)
 *   start = (double)(float)(pos.y - roff);  end = start - rl * 2
 *   a0 = |vx| + |vy| + |vz|;  A = a0 + |(double)(float)gravity[1]| * dt_sec;  A not finite: A = a0;  still not: A = 0
 *   B = 3 * (|dx| + |dz|);  not finite: B = 0;        S = A > B ? A : B
 *   dtc = dt_sec < 1e-6 ? 0 : dt_sec > 1 / 30 ? 1 / 30 : dt_sec;      T = S * dtc;  not finite: T = 0
 *   mag = fmax over T, |bb[0..5]|, |start|, |end|, rl (fmax skips NaN);      pad = mag * 2^-20 + 1e-6
 *   gx = T + pad;  gy = rl + T + pad
 *   x: [bb[0] - gx, bb[1] + gx]    z: [bb[4] - gx, bb[5] + gx]
 *   y: [min(bb[2] - gy, end - pad), max(bb[3] + gy, start + pad)]   (a NaN ray end leaves the box's own bound)
 * A is the airborne branch after gravity and the walker on a zero normal (the given velocity), B the walking branch; a
 * jump and a state below IDLE do not slide; a delta that is not finite is CLAPGPU_SLIDE_INVALID and moves nothing.
 * Over-estimating only costs levels.
 * Conflict: movers i < j (positions in the list) conflict when their reach boxes overlap (closed).
 * Level: level[j] = 0 without an earlier conflicting mover, else 1 + max level[i] over the earlier movers i that conflict
 * with j: the longest path, unique, whatever the scheduling.  n_levels = 1 + max level (0 for n == 0).
 * Two special cases.  A body listed more than once (and a body[k] >= b->n, whose reach box is NaN) is INVALID in both
 * stages as in the plain call and moves nothing: every such listing is level 0 and conflicts with nobody.  A mover whose
 * reach box is not finite (a NaN or infinite box row, an infinite ray) STANDS ALONE: it conflicts with every other leveled
 * mover, so it has a level to itself -- a body whose box says nothing can still cast a valid ray or slide from a finite
 * position, and nothing bounds what it meets.  The pair search is not given such boxes; the level pass walks n lanes of up
 * to n steps per round while there is one.
 * Ordered move: for L = 0 .. n_levels - 1, stages 1 to 5 of clapgpu_characters_move without the push over the movers of
 * level L in list order (each level takes its own clapgpu_bp_index calls and clears the per-body words, as the plain call
 * does); then ONE clapgpu_bodies_push over all n movers in list order, so facc is the reference's sequential sum in (k, q)
 * order; then the flags and the rotation hand-off.  Why this is the one-at-a-time loop: movers of one level cannot touch
 * each other; a mover's earlier conflicts are done and its later ones have not started; a mover that does not conflict
 * with it cannot be seen by any of its stages; and no stage reads what the push writes (facc, bflags, the auto-disable
 * counters: the ground apply and the slide apply of bodies.hip touch pos, lvel, axis, aabb and the geom record alone).
 *
 * clapgpu_characters_order moves nothing: it reads m's body, ray_off, motion and velocity and b's aabb, pos and yoffset,
 * writes reach[n][6] and level[n] (device) and summary[4] (host): n_levels, pair_total, order_bp's status
 * (clapgpu_bp_status), the relaxation rounds that ran.  pair_total counts the overlapping pairs of leveled boxes, listings
 * of one body included.  order_bp: a second clapgpu_bp of either kind, created with n_static == 0 and n_max >= n; the
 * conflicts are clapgpu_bp_collide's pairs over the reach boxes, the levels a relaxation over them (atomicMax(level[j],
 * level[i] + 1) per pair and round until a round changes nothing, launched in chunks of 8 rounds).
 * BOTH CALLS SYNCHRONISE THE STREAM, for the pair count, the convergence of the rounds and the level count only; neither
 * can be captured in a graph, and neither is a stage of clapgpu_frame.
 * CLAPGPU_ERR_INVALID_ARGUMENTS before any HIP call: what clapgpu_characters_move refuses (clapgpu_characters_order asks
 * only for what it reads, and for reach, level and summary), a NULL order_bp, a missing b->aabb, a NULL n_levels.
 * CLAPGPU_ERR_TOO_LARGE, from either call BEFORE ANY BODY HAS MOVED: pair_total > pair_capacity (summary[1] says how many;
 * retry with more room), or order_bp's status bit 0 (a reach box larger than its top cell; that bit is sticky: retry with
 * another object of a larger cell).  n == 0 returns CLAPGPU_OK, launches nothing and gives n_levels 0.
 * A line of characters at touching distance costs one level per character: the reference's own sequential nature.
 * scratch: *_scratch_bytes bytes of device memory, 256-byte aligned, overwritten; both helpers return 0 for n == 0, the
 * ordered move's also when clapgpu_characters_move_scratch_bytes does.  level (ordered move) may be NULL.
 */
size_t clapgpu_characters_order_scratch_bytes(uint32_t n, uint32_t pair_capacity);
int    clapgpu_characters_order(void *stream, clapgpu_bp *order_bp, const clapgpu_bodies *b, const clapgpu_world *w,
                                double dt_sec, const clapgpu_move *m, uint32_t pair_capacity,
                                double *reach /* [n][6] out */, uint32_t *level /* [n] out */,
                                uint32_t *summary /* host [4]: n_levels, pair_total, order_bp status, rounds */, void *scratch);
size_t clapgpu_characters_move_ordered_scratch_bytes(uint32_t n_bodies, uint32_t n, uint32_t pair_capacity);
int    clapgpu_characters_move_ordered(void *stream, clapgpu_bp *bp, clapgpu_bp *order_bp, const clapgpu_bodies *b,
                                       const clapgpu_world *w, const clapgpu_geoms *statics, const clapgpu_trimesh *meshes,
                                       const clapgpu_entities *e, double dt_sec, const clapgpu_move *m, uint32_t pair_capacity,
                                       uint32_t *level /* [n] device out, may be NULL */, uint32_t *n_levels /* host out */,
                                       void *scratch);

/* ======================================================================== */
/* Clustered lighting: lights x screen tiles bitmask (core/light.c)           */
/* ======================================================================== */

#define CLAPGPU_LIGHTS_MAX 128     /* LIGHTS_MAX, shader_constants.h:8: one bit per slot in an RGBA32UI texel */

/*
 * The slots of struct light (light.h:19-27) that light_grid_compute reads, as device arrays of
 * CLAPGPU_LIGHTS_MAX entries: pos/color/attenuation are float[3] per slot, is_dir is the
 * reference's int flag, active[i] != 0 <=> bit i of light->active is set.
 */
typedef struct clapgpu_lights {
    uint32_t        nr_lights;     /* highest allocated slot + 1 (light.h:46) */
    uint32_t        pad;
    float          *pos;
    const float    *color;
    const float    *attenuation;
    const int32_t  *is_dir;
    const uint32_t *active;
} clapgpu_lights;

/* Tile counts light_grid_update gives the grid (light.c:51-52): ceilf((float)extent / cell).  Host. */
void clapgpu_light_grid_dims(uint32_t width, uint32_t height, uint32_t cell, uint32_t *twidth, uint32_t *theight);

/*
 * light_grid_compute() (light.c:88-154): tiles[gy * twidth + gx][4] (device,
 * the RGBA32UI image the reference uploads with texture_load, light.c:150-153) gets bit idx set
 * iff light idx is active and directional, or is a point light in front of the far plane whose
 * screen-space disc (radius from light_get_radius, light.c:301-309) reaches one of the tile's four
 * corners.  view_mx / proj_mx: the main subview's matrices (host, column-major).
 */
int clapgpu_light_grid_compute(void *stream, const clapgpu_lights *lights, const float view_mx[16],
                               const float proj_mx[16], uint32_t width, uint32_t height, uint32_t cell,
                               uint32_t *tiles);

/*
 * default_update's light hand-off (model.c:1689-1694): carrier k = entity carrier_entity[k] holding
 * light slot carrier_light[k] at offset carrier_off[k] (e->light_idx, e->light_off).  A carrier
 * without a parent whose CLAPGPU_E_DIRTY is set (or any, under CLAPGPU_UPDATE_ALL_DIRTY) writes
 * pos + offset into lights->pos[slot] if the slot is active (light_set_pos, light.c:473-480);
 * carriers apply in list order.  Call BEFORE clapgpu_entities_update, which clears the dirty flags.
 */
int clapgpu_lights_from_entities(void *stream, const clapgpu_entities *e, uint32_t mode, uint32_t n_carriers,
                                 const uint32_t *carrier_entity, const int32_t *carrier_light,
                                 const float *carrier_off, const clapgpu_lights *lights);

/* ======================================================================== */
/* Character states and animation queues (ABI 46)                            */
/* ======================================================================== */

/*
 * character_set_state (character.c:316-426), animation_push_by_name / animation_next / animation_end (model.c:1443-1561),
 * animated_update's control flow (model.c:1563-1592) and the three end callbacks the engine installs itself
 * (character_idle, character_start_motion, character_any_to_jump, character.c:86-121), per character, on the device.
 * The rule is stated once in clap_amd/csrc/aniq_dev.h and restated in tests/aniqref.py.
 *
 * The queue of a character (entity3d.aniq): up to CLAPGPU_ANIQ_MAX entries of 8 bytes.  struct queued_animation
 * (model.h:352-361) maps to an entry as: animation -> animation, repeat -> repeat, speed -> speed, end -> a code
 * (CLAPGPU_ANI_END_*: the function pointer's name; end_priv is always the character), delay is unused by the reference,
 * sfx_state and frame_cb stay with the host (events: CLAPGPU_ANIQ_STARTED tells it when to reset sfx_state).
 * Per character: len (aniq.da.nr_el), cur (e->animation, -1 allowed), cleared (e->ani_cleared), ani_time (e->ani_time).
 * The joint cursors animation_start resets (model.c:1419-1422) have no device counterpart: clapgpu_pose_update
 * brackets a key time without a cursor.
 *
 * name_anim[CLAPGPU_ANI_NAMES]: animation_by_name (model.c:1426-1434) of the model for each of the twelve names
 * character.c pushes, -1 where the model has none; the host fills it once (device memory).
 *
 * Host-owned characters.  A call leaves a character untouched -- none of its arrays written but events, which gets
 * CLAPGPU_ANIQ_HOST -- when, on entry, len == 0, len > CLAPGPU_ANIQ_MAX, cur < 0, cur >= len or an entry's animation >=
 * n_anims (animation_next would push "idle" with a drand48 phase, model.c:1458-1469: that stream is the host's), or when
 * the step would call an end code CLAPGPU_ANI_END_HOST, push a fifth entry (CLAPGPU_ANIQ_OVERFLOW is set too), push an
 * animation >= n_anims, or advance an emptied queue ((cur + 1) % 0, model.c:1478).  The step runs on a copy in
 * registers and commits only when none of these arose; the host then does for that character what it did before ABI 46.
 *
 * state, airborne, velocity and jump_params may be the very arrays of a clapgpu_move when mover is NULL (character c is
 * mover c): the move of the next frame then reads the state this frame's calls left.
 */
#define CLAPGPU_ANIQ_MAX 4u
#define CLAPGPU_ANI_END_NONE         0u
#define CLAPGPU_ANI_END_IDLE         1u     /* character_idle, character.c:86-92 */
#define CLAPGPU_ANI_END_START_MOTION 2u     /* character_start_motion, :94-99 */
#define CLAPGPU_ANI_END_ANY_TO_JUMP  3u     /* character_any_to_jump, :103-121 */
#define CLAPGPU_ANI_END_HOST         0xffu  /* a callback of the host's */
/* the slots of name_anim[], in the order character.c first uses the names */
#define CLAPGPU_ANI_IDLE           0u
#define CLAPGPU_ANI_START_TO_IDLE  1u
#define CLAPGPU_ANI_MOTION_STOP    2u
#define CLAPGPU_ANI_JUMP_TO_IDLE   3u
#define CLAPGPU_ANI_FALL_TO_IDLE   4u
#define CLAPGPU_ANI_MOTION         5u
#define CLAPGPU_ANI_MOTION_START   6u
#define CLAPGPU_ANI_JUMP_TO_MOTION 7u
#define CLAPGPU_ANI_IDLE_TO_JUMP   8u
#define CLAPGPU_ANI_MOTION_TO_JUMP 9u
#define CLAPGPU_ANI_JUMP           10u
#define CLAPGPU_ANI_FALL           11u
#define CLAPGPU_ANI_NAMES          12u
/* events[c]: bits 0-7 are the last clapgpu_animation_queue_time's, bits 8-15 (the same bits << CLAPGPU_ANIQ_STATE_SHIFT)
 * the last clapgpu_characters_state's, which clears the low byte: one word holds the frame's both steps */
#define CLAPGPU_ANIQ_ENDED           (1u << 0)   /* frame_time >= time_end (model.c:1590) */
#define CLAPGPU_ANIQ_STARTED         (1u << 1)   /* an animation_start ran: the host resets sfx_state */
#define CLAPGPU_ANIQ_ADVANCED        (1u << 2)   /* cur = (cur + 1) % len (model.c:1478) */
#define CLAPGPU_ANIQ_CB_IDLE         (1u << 3)
#define CLAPGPU_ANIQ_CB_START_MOTION (1u << 4)
#define CLAPGPU_ANIQ_CB_ANY_TO_JUMP  (1u << 5)
#define CLAPGPU_ANIQ_HOST            (1u << 6)   /* untouched: the host does this step */
#define CLAPGPU_ANIQ_OVERFLOW        (1u << 7)   /* ... because a push found CLAPGPU_ANIQ_MAX entries */
#define CLAPGPU_ANIQ_STATE_SHIFT     8u

typedef struct clapgpu_aniq_entry {
    uint16_t animation;
    uint8_t  repeat;
    uint8_t  end;                  /* CLAPGPU_ANI_END_* */
    float    speed;
} clapgpu_aniq_entry;

/* One animated model's characters, in the order of its clapgpu_anim_clock / clapgpu_pose_batch. */
typedef struct clapgpu_aniq {
    uint32_t            n;
    uint32_t            n_anims;
    const int32_t      *name_anim;     /* [CLAPGPU_ANI_NAMES] */
    const float        *time_end;      /* [n_anims] animation.time_end */
    clapgpu_aniq_entry *queue;         /* [n][CLAPGPU_ANIQ_MAX], 16-byte aligned */
    uint8_t            *len;           /* [n] */
    int8_t             *cur;           /* [n] */
    uint8_t            *cleared;       /* [n] */
    double             *ani_time;      /* [n] */
    uint8_t            *state;         /* [n] ch->state, CLAPGPU_CS_* */
    uint8_t            *airborne;      /* [n] ch->airborne */
    float              *velocity;      /* [n][3] ch->velocity */
    float              *ch_motion;     /* [n][2] ch->motion's x and z: persistent, written at character.c:499 */
    const float        *jump_params;   /* [n][2] jump_forward, jump_upward */
    const int32_t      *mover;         /* [n] index into the clapgpu_move, -1: none; NULL: character c is mover c */
    /* out */
    uint32_t           *pose_anim;     /* [n] queue[cur].animation: clapgpu_pose_batch.anim */
    float              *frame_time;    /* [n] clapgpu_pose_batch.frame_time */
    uint32_t           *events;        /* [n] CLAPGPU_ANIQ_* */
} clapgpu_aniq;

/*
 * What character_move does with its request, directly behind clapgpu_characters_move: for every character with a mover
 * k whose request[k] is not 0xff, ch_motion[c] = motion[k] when request[k] is JUMP_START, MOVING or IDLE (the grounded
 * path writes ch->motion, character.c:499; FALLING keeps the old value), then character_set_state(request[k])
 * (character.c:316-426) with every push, ignored return value, goto fail_fallback and end callback it makes.  Left out
 * of case CS_MOVING: character_apply_velocity and character_set_moved (:350-351), which the move has done (applied[k]).
 * airborne = 1 of :388 is written again (idempotent: the call can be used without the move).
 * now: clap_get_current_time(), the frame's one clock (clap.c:212-237, 557): what animation_start stores; now_dev != NULL:
 * read from that device double instead (a captured graph).  events[c] = the step's bits << CLAPGPU_ANIQ_STATE_SHIFT, 0 for
 * a character without a mover or a request.  One lane per character, no host synchronisation, no allocation.
 * CLAPGPU_ERR_INVALID_ARGUMENTS before any HIP call: q or m NULL; with q->n > 0 a missing array of q (mover, pose_anim,
 * frame_time and time_end may be NULL here), a queue that is not 16-byte aligned, m->n > 0 without m->request or
 * m->motion, a NULL mover with q->n > m->n.  A mover index outside [0, m->n) is no mover.  q->n == 0 launches nothing.
 */
int clapgpu_characters_state(void *stream, const clapgpu_aniq *q, const clapgpu_move *m, double now, const double *now_dev);

/*
 * animated_update (model.c:1563-1592) for the model's characters, in place of clapgpu_animation_time: per character
 *   pose_anim[c]  = queue[cur].animation
 *   frame_time[c] = (float)((now - ani_time[c]) * speed)          (double arithmetic, before the advance: channels_transform
 *                                                                  runs before animation_next)
 * and, when (now - ani_time[c]) * speed >= time_end[animation], animation_next (model.c:1454-1483) with its callbacks:
 * a repeating entry restarts; another one has its end code called (nulled first), then ani_cleared clears and returns,
 * or cur = (cur + 1) % len and animation_start.  frame_cb / frame_sfx stay with the host, which runs them from
 * frame_time; they change no queue.  events[c] = (events[c] & 0xff00) | the step's bits.  A host-owned character's
 * pose_anim and frame_time are not written either.  Arguments as above (every array but mover needed, and time_end);
 * q->n == 0 launches nothing.
 */
int clapgpu_animation_queue_time(void *stream, const clapgpu_aniq *q, double now, const double *now_dev);

/* ======================================================================== */
/* Views in device memory (ABI 49)                                           */
/* ======================================================================== */

/*
 * Everything a frame knows about its views -- the frusta of the cull, the view and projection matrices of the light grid
 * and the particles' billboards, the camera position of the LOD pick -- reaches the kernels above by value, from host
 * memory, as kernel arguments; a captured graph holds them frozen.  The view block is the same knowledge in device memory:
 *   clapgpu_views_source   what a view IS: matrices, or a pose.  Written by one small copy from the host or by a kernel
 *                          of the caller's.
 *   clapgpu_views_state    what the kernels READ: per slot the frustum, the matrices, the camera position and the cull's
 *                          constants.  Written by clapgpu_views_calc alone.
 * Slot 0 is the main view, slot 1 + k further view k in the order of clapgpu_views.  Both blocks are 16-byte aligned.
 *
 * THE RULE: clapgpu_views_calc does per slot the arithmetic of clapgpu_view_matrix (when FROM_POSE), mvp = proj * view
 * and clapgpu_frustum_calc, by the same functions (csrc/lm_dev.h) in the same order, and every *_views entry point
 * below gives the bits of its twin called with those host values.  Every NaN these functions store is the one quiet NaN
 * 0x7fc00000, on the host and on the device: what an invalid operation (0 * inf of a singular mvp) leaves in the sign and
 * payload of a NaN differs between the two machines and no consumer reads it.
 * The main view's pose can come from the camera controller on the device (clapgpu_camera_calc, ABI 50, below) and the
 * shadow light's view from the cascades' fit (clapgpu_cascades_calc, ABI 51, below), and a spotlight's view from the
 * entity that carries it (clapgpu_lights_update, ABI 52, below).  clapgpu_entities.bv (the bounding-volume pick's camera and control positions) is an argument
 * of the fused update kernel, which the view block does not reach: clapgpu_entities_bv_views is its twin over the block.
 */
#define CLAPGPU_VIEW_SLOTS (1 + CLAPGPU_EXTRA_VIEWS_MAX)
#define CLAPGPU_VIEW_FROM_POSE        1u     /* view matrix = clapgpu_view_matrix(pos, quat); view_mx is not read */
#define CLAPGPU_VIEW_NDC_Z_ZERO_ONE   2u     /* the ndc_z_zero_one argument of clapgpu_frustum_calc */

typedef struct clapgpu_view_source {
    float    view_mx[16], proj_mx[16];
    float    pos[3];                         /* the camera position the LOD pick uses (and the pose's, when FROM_POSE) */
    uint32_t flags;                          /* CLAPGPU_VIEW_* */
    float    quat[4];                        /* x y z w; read only when FROM_POSE */
} clapgpu_view_source;
typedef struct clapgpu_views_source {
    clapgpu_view_source slot[CLAPGPU_VIEW_SLOTS];
} clapgpu_views_source;

typedef struct clapgpu_view_state {
    clapgpu_frustum frustum;                 /* clapgpu_frustum_calc(view_mx, proj_mx, NDC_Z_ZERO_ONE) */
    uint32_t cull[8];                        /* reserved to the library: the cull's constants (per-axis extremes of the
                                              * corners, "every plane component finite") */
    float    view_mx[16], proj_mx[16], mvp[16];
    float    cam_pos[3];
    uint32_t pad;
} clapgpu_view_state;
typedef struct clapgpu_views_state {
    clapgpu_view_state slot[CLAPGPU_VIEW_SLOTS];
} clapgpu_views_state;

#define CLAPGPU_VIEWS_SOURCE_BYTES 800
#define CLAPGPU_VIEWS_STATE_BYTES  2320
#ifdef __cplusplus
static_assert(sizeof(clapgpu_views_source) == CLAPGPU_VIEWS_SOURCE_BYTES && sizeof(clapgpu_views_state) == CLAPGPU_VIEWS_STATE_BYTES,
              "the view block's layout is ABI");
#else
_Static_assert(sizeof(clapgpu_views_source) == CLAPGPU_VIEWS_SOURCE_BYTES && sizeof(clapgpu_views_state) == CLAPGPU_VIEWS_STATE_BYTES,
               "the view block's layout is ABI");
#endif

/* state->slot[0 .. n_views-1] from source->slot[same]; the other slots are left untouched.  n_views is 1 ..
 * CLAPGPU_VIEW_SLOTS.  One launch, no allocation, no host synchronisation: it can be captured.  A NULL or misaligned
 * block or an n_views out of range: CLAPGPU_ERR_INVALID_ARGUMENTS before any HIP call (as for every entry point below). */
int clapgpu_views_calc(void *stream, const clapgpu_views_source *source, clapgpu_views_state *state, uint32_t n_views);

/* The twins: each takes the view block where its original takes host values, validates as its original does and leaves
 * the bits its original leaves when called with the host-computed values of the same source. */
/* clapgpu_entities_cull: the main plane from slot 0, plane k of e->views (mask pointers and n from the host struct)
 * from slot 1 + k; e->views->frustum[] is not read */
int clapgpu_entities_cull_views(void *stream, const clapgpu_entities *e, const clapgpu_views_state *state);
/* clapgpu_entities_lod / clapgpu_visible_compact_lod: cam_pos from slot 0 */
int clapgpu_entities_lod_views(void *stream, const clapgpu_entities *e, const uint32_t *visible, const uint32_t *count,
                               uint32_t index_base, const clapgpu_views_state *state, const int32_t *force_lod,
                               int32_t *cur_lod, int32_t *draw_lod);
int clapgpu_visible_compact_lod_views(void *stream, const clapgpu_entities *e, uint32_t index_base,
                                      const clapgpu_views_state *state, const int32_t *force_lod, int32_t *cur_lod,
                                      uint32_t *visible, uint32_t *count, int32_t *draw_lod, void *scratch);
/* clapgpu_light_grid_compute: view, mvp and proj_mx[0] from slot 0 */
int clapgpu_light_grid_compute_views(void *stream, const clapgpu_lights *lights, const clapgpu_views_state *state,
                                     uint32_t width, uint32_t height, uint32_t cell, uint32_t *tiles);
/* clapgpu_particles_update: the billboards' view matrix from slot 0 */
int clapgpu_particles_update_views(void *stream, const clapgpu_particles *p, const clapgpu_views_state *state);

/* ======================================================================== */
/* The camera controller on the device (ABI 50)                              */
/* ======================================================================== */

/*
 * camera_update (core/camera.c:208-246, called from scene_camera_calc, scene.c:1013) for a camera that follows a control
 * entity: camera_target, the loop that casts four rays from the target to the near-plane corners of the orbiting camera
 * and shortens the orbit until none is blocked, and transform_orbit.  camera_move (yaw and pitch from input) stays with
 * the host: it writes quat.  clapgpu_camera is a block in DEVICE memory, 16-byte aligned; the host writes the inputs,
 * clapgpu_camera_calc the outputs.
 *
 * THE RULE.  clapgpu_camera_calc does camera_update's arithmetic in its order, in fp32 and fp64 exactly where the
 * reference has them, with no FMA contraction, by the functions the host twins below call (csrc/lm_dev.h), so the block
 * holds the host's bits; every NaN stored is 0x7fc00000 (as for the view block).
 *   moved == 0 (camera_has_moved() is false): status = 0 and iterations = 0 are written and nothing else; slot 0 of the
 *       source is left alone.
 *   camera_target (camera.c:174-206), for entity ctl_entity of `e`:
 *       IS_CHARACTER: target = pos_scale.xyz; height = entity3d_aabb_Y = |model box Y| * pos_scale.w (model.c:1190,
 *           model_table); HAS_HEAD_JOINT: target = joint_pos[head_joint].xyz + (0, height * 0.2f, 0), else
 *           target.y += height * 0.75f
 *       otherwise: target = center[ctl_entity], height = aabb_Y / 2.0f
 *       dist_cap = fmaxf(10.0f, cbrtf(X * Y * Z)); dist = fminf(height * 3.0f, fminf(dist_cap, far_plane - 10.0f))
 *   the loop (camera.c:232-236, 93-117, 68-91, 51-66), dist a double: while dist > 0.1 --
 *       the pose is cloned and orbits: pos = quat * (0, 0, (float)dist) + target; the view matrix (clapgpu_view_matrix)
 *       is inverted; corner[k] = inverse * (+-w, +-h, 0, 1) in the order (w,h) (-w,h) (w,-h) (-w,-h), w = near_plane,
 *       h = near_plane / aspect; ray k starts at target, has direction corner[k].xyz - target (float) and length
 *       (double)vec3_len(direction); a hit gives scale = depth / length, min_scale = fmin(...) from 1.0;
 *       min_scale < 0.99: dist = (double)(float)dist * min_scale (camera_position_is_good takes dist as a float) and
 *       round again, else stop
 *   updated = ((double)dist_of_camera_target != dist) (camera.c:238), dist = (float)dist, pos = the final orbit;
 *   pos and quat are then written into source->slot[0], whose flags must already hold CLAPGPU_VIEW_FROM_POSE; its
 *   proj_mx and flags are left alone.
 * THE RAYS are clapgpu_ray_cast's: the same colliders, tie rule and mesh test, with skip = ctl_skip; the result is, bit
 * for bit, what a host gets by running the loop itself with one clapgpu_ray_cast of four rays (flags asked for) per
 * iteration.  A ray flagged CLAPGPU_RAY_INVALID is a miss; one flagged CLAPGPU_RAY_UNRESOLVED counts by the hit it
 * returned and sets CLAPGPU_CAMERA_UNRESOLVED.  ctl_skip == -1 says the control entity has no physics: phys_ray_cast
 * returns NULL (physics.c:536), no ray is cast and none ever hits.
 * TERMINATION is unconditional.  A continuing iteration multiplies a finite dist by less than 0.99 and the loop ends at
 * or below 0.1: at most ln(3.4e39) / -ln(0.99) ~ 9 040 iterations from the largest float.  A NaN dist fails `> 0.1`;
 * an infinite dist or a NaN quaternion gives non-finite corners, whose rays are INVALID and miss, so the loop stops after
 * that iteration.  CLAPGPU_CAMERA_ITER_MAX therefore never binds on any input; the loop carries it (here and in
 * clapgpu_camera_update_host) so that a kernel's end does not rest on an argument about rounding, and reports
 * CLAPGPU_CAMERA_CAPPED if it ever did.
 * What the host cannot see before a HIP call it cannot refuse: ctl_entity >= e->n, or HAS_HEAD_JOINT without joint_pos,
 * is found by the kernel, which then writes status = CLAPGPU_CAMERA_INVALID and iterations = 0 and nothing else.
 */
#define CLAPGPU_CAMERA_IS_CHARACTER   1u     /* flags: entity3d_matches(control, ENTITY3D_IS_CHARACTER) */
#define CLAPGPU_CAMERA_HAS_HEAD_JOINT 2u     /* flags: model3d_get_joint(model, JOINT_HEAD) succeeds */
#define CLAPGPU_CAMERA_UNRESOLVED     1u     /* status: a ray of some iteration was CLAPGPU_RAY_UNRESOLVED */
#define CLAPGPU_CAMERA_CAPPED         2u     /* status: the loop was cut at CLAPGPU_CAMERA_ITER_MAX (cannot happen, above) */
#define CLAPGPU_CAMERA_INVALID        4u     /* status: ctl_entity out of range, or a head joint without joint_pos */
#define CLAPGPU_CAMERA_ITER_MAX       16384u

typedef struct clapgpu_camera {
    /* in */
    float    quat[4];                        /* c->xform.rotation (x y z w), after camera_move */
    float    pos[3];                         /* in: c->xform.pos (not read: the orbit replaces it); out: the camera position */
    float    dist;                           /* in: c->dist (not read: camera_target replaces it); out: c->dist */
    float    near_plane, far_plane, aspect;
    uint32_t moved;                          /* camera_has_moved() */
    uint32_t ctl_entity;                     /* index into the frame's clapgpu_entities */
    int32_t  ctl_skip;                       /* the rays' skip, as clapgpu_ray_cast codes it; -1: the control has no physics */
    uint32_t flags;                          /* CLAPGPU_CAMERA_IS_CHARACTER | CLAPGPU_CAMERA_HAS_HEAD_JOINT */
    uint32_t head_joint;                     /* index into the pose batch's joint_pos ([4] floats per joint) */
    /* out */
    float    target[3];
    uint32_t updated;                        /* c->dist != dist, camera.c:238 */
    float    corner[4][4];                   /* c->frustum_corner of the last iteration (untouched when there was none) */
    uint32_t iterations, status;             /* calls of camera_position_is_good; CLAPGPU_CAMERA_* */
    uint32_t pad[2];
} clapgpu_camera;

#define CLAPGPU_CAMERA_BYTES 160
#ifdef __cplusplus
static_assert(sizeof(clapgpu_camera) == CLAPGPU_CAMERA_BYTES, "the camera block's layout is ABI");
#else
_Static_assert(sizeof(clapgpu_camera) == CLAPGPU_CAMERA_BYTES, "the camera block's layout is ABI");
#endif

/* One launch (one workgroup of four wavefronts, a wavefront per corner ray), no allocation, no host synchronisation: it
 * can be captured.  e: pos_scale, model, model_table and center are read.  joint_pos (may be NULL without a head joint):
 * the pose batch's WORLD joint positions (clapgpu_pose_batch.joint_pos, behind clapgpu_joint_pos_world where the pose
 * left model space).  bp, bodies, statics and meshes as clapgpu_ray_cast takes and validates them (bp NULL: every geom
 * is scanned).  A NULL or misaligned cam or source, a NULL e / bodies / statics or an e without those four arrays:
 * CLAPGPU_ERR_INVALID_ARGUMENTS before any HIP call. */
int clapgpu_camera_calc(void *stream, clapgpu_camera *cam, const clapgpu_entities *e, const float *joint_pos,
                        clapgpu_bp *bp, const clapgpu_geoms *bodies, const clapgpu_geoms *statics,
                        const clapgpu_trimesh *meshes, clapgpu_views_source *source);

/* The host twins: the kernel's own functions on the host's values (host memory throughout).
 * clapgpu_camera_target: camera_target from the control entity's pos_scale[4], model box lo[3] / hi[3], world centre[3]
 * and head joint position head[3] (read when HAS_HEAD_JOINT; may be NULL otherwise) -> target[3], *dist.
 * clapgpu_camera_rays: one iteration's corners [4][4] and rays [4][8] (as clapgpu_ray_cast takes them) for the pose
 * quat, target and dist.  clapgpu_camera_decide: from the four rays' answers (hit[k] != 0: a hit at depth[k]) and the
 * rays cast, *min_scale and *next_dist; returns 1 when the position is good (the loop stops), 0 when the loop goes on
 * with *next_dist. */
void clapgpu_camera_target(uint32_t flags, const float pos_scale[4], const float lo[3], const float hi[3], const float center[3],
                           const float head[3], float far_plane, float target[3], float *dist);
void clapgpu_camera_rays(const float quat[4], const float target[3], float dist, float near_plane, float aspect,
                         float corner[16], double ray[32]);
int clapgpu_camera_decide(float dist, const int32_t hit[4], const double depth[4], const double ray[32], double *min_scale,
                          double *next_dist);
/* ... and the whole of camera_update behind camera_target on a HOST copy of the block (target and dist in, as
 * clapgpu_camera_target left them): the loop with its cap, the final orbit, updated / iterations / status.  cast(user,
 * ray[32], hit[4], depth[4]) answers one iteration's four rays (hit[k] != 0: a hit; preset to misses) and returns the OR
 * of their CLAPGPU_RAY_* flags; it is not called when ctl_skip == -1.  moved == 0: as the kernel.  `cast` is a
 * clapgpu_camera_cast_fn, passed as the object pointer POSIX lets a function pointer travel in. */
typedef uint32_t (*clapgpu_camera_cast_fn)(void *user, const double *ray, int32_t *hit, double *depth);
void clapgpu_camera_update_host(clapgpu_camera *cam, void *cast, void *user);

/* ======================================================================== */
/* The shadow cascades on the device (ABI 51)                                */
/* ======================================================================== */

/*
 * What scene_camera_calc (scene.c:1004-1048) does behind camera_update: the camera's cascade sub-frusta
 * (view_update_perspective_subviews, view.c:11-37), near_backup from the bounding volume this frame's default_update
 * picked (scene.c:1021-1038, model.c:1703-1713), and the shadow light's views fitted to those frusta
 * (view_update_from_frustum, view.c:195-246, 129-163).  clapgpu_cascades is a block in DEVICE memory, 16-byte aligned;
 * the host writes the inputs, clapgpu_cascades_calc the outputs.  The inputs change with the window, the light and the
 * render options, not with the camera: a frame whose camera is the device's needs no host between the camera and the
 * shadow passes' cull, and a replayed graph's light view follows its camera.
 *
 * THE RULE.  clapgpu_cascades_calc does that arithmetic in the reference's order, in fp32 and fp64 exactly where the
 * reference has them, with no FMA contraction, by the functions the host twins below call (csrc/lm_dev.h), so the block
 * holds the host's bits; every NaN stored is 0x7fc00000 (as for the view block).  nr = nr_cascades, 0 meaning 4.
 *   the camera's view matrix: slot 0 of `source` -- clapgpu_view_matrix(pos, quat) when its flags hold
 *       CLAPGPU_VIEW_FROM_POSE, else its view_mx.
 *   cam_corners[v], v < nr: the corners of clapgpu_frustum_calc(that matrix, persp[v], NDC_Z_ZERO_ONE); cam_corners[4]:
 *       those of the main frustum, with slot 0's own proj_mx.  persp[] is the host's (clapgpu_cascades_persp): the
 *       reference's mat4x4_perspective takes 1 / tan(fov / 2) through libm in double, which the device does not
 *       reproduce bit for bit, and the four matrices change only with the window.  No libm function is called.
 *   near_backup: the input field, or with NEAR_BACKUP_FROM_BV the value of scene.c:1030-1037 for the entity `env` of
 *       *bv_result (the key of clapgpu_bv_query: 0 = no volume, near_backup 0; else env = 0xFFFFFFFF - low word):
 *       X / Y / Z = |model box edge| * pos_scale.w (as camera_target); d = vec3_norm_safe(light_dir);
 *       xz_mix = linf_interp(Z, X, fabsf(d . (1,0,0))) with the blend's complement and the sum in double;
 *       ycos = fmaxf(fabsf(d . (0,1,0)), 0.2f); near_backup = min(xz_mix / ycos, cbrtf(X * Y * Z)), min the ternary
 *       a < b ? a : b.  The inner products are the literal sums with their zero factors (inf * 0 is NaN, as there).
 *   each fit (subview_update_from_target), once per cascade v < nr from cam_corners[v] and once for the light's main
 *       view from cam_corners[4]: the world box of the eight corners from +-INFINITY by min(v, cur) / max(v, cur) as
 *       ternaries; light_pos = aabb_center with y = the box's lowest; target = -light_dir through vec3_norm_safe, scaled
 *       by fmaxf(near_backup, 1.0f); mat4x4_look_at_safe(light_pos + that, light_pos, (0,1,0)) -- the up vector becomes
 *       (0,0,-1) where |forward . up| > 0.999f, vec3_norm takes 1.0 / len in double; the light-space box of the corners
 *       under that matrix (mat4x4_mul_vec4_post, then * (1.0f / w)); the direction is scaled again by (near_backup +
 *       |z extent|) / near_backup, the second look_at gives view_mx, mat4x4_invert inv_view_mx.
 *   each cascade's projection (subview_projection_update): the light-space box of cam_corners[v] under view_mx;
 *       near_plane = 0.1f, far_plane = -box.min.z; mat4x4_ortho_ndc_z_1 (NDC_Z_ZERO_ONE) or _2 over the box's x and y
 *       with (near, far), or (far, near) under Z_REVERSE; inv_proj_mx = mat4x4_invert; mvp = proj_mx * view_mx
 *       (UNIFORM_SHADOW_MVP, model.c:864-869; far_plane is UNIFORM_LIGHT_FAR).
 *   the light's main view_mx is also written into source->slot[light_slot].view_mx; that slot's proj_mx, pos and flags
 *       are left alone (view_update_from_frustum never writes light.view[0].main.proj_mx either).
 * The reference fits every view->subview[] whatever nr_cascades is; nothing reads the surplus ones, and the device leaves
 * cascade[v], and cam_corners[v], for nr <= v < 4 untouched.  The light sub-views' own frusta (view.c:145) are read by the
 * debug UI alone and are not produced.
 * What the host cannot see before a HIP call it cannot refuse: the flags, light_slot and nr_cascades live in the device
 * block.  A light_slot outside 1 .. CLAPGPU_VIEW_SLOTS - 1, a light slot whose flags hold CLAPGPU_VIEW_FROM_POSE, an
 * nr_cascades above 4, and with NEAR_BACKUP_FROM_BV a NULL bv_result or a key naming an entity at or past e->n: the
 * kernel writes status = CLAPGPU_CASCADES_INVALID and nothing else.
 */
#define CLAPGPU_CASCADES_MAX                  4      /* CASCADES_MAX, shader_constants.h:9 */
#define CLAPGPU_CASCADES_Z_REVERSE            1u     /* flags: the z_reverse of view.c:137 (!shadow_vsm) */
#define CLAPGPU_CASCADES_NDC_Z_ZERO_ONE       2u     /* flags: renderer_get_caps()->ndc_z_zero_one */
#define CLAPGPU_CASCADES_NEAR_BACKUP_FROM_BV  4u     /* flags: near_backup from *bv_result, not from the field */
#define CLAPGPU_CASCADES_INVALID              1u     /* status */
#define CLAPGPU_CASCADES_NO_ENTITY            0xFFFFFFFFu

typedef struct clapgpu_cascade_view {        /* one light sub-view, out */
    float    view_mx[16], inv_view_mx[16], proj_mx[16], inv_proj_mx[16];
    float    mvp[16];                        /* proj_mx * view_mx */
    float    near_plane, far_plane;
    uint32_t pad[2];
} clapgpu_cascade_view;

typedef struct clapgpu_cascades {
    /* in */
    float    light_dir[3];                   /* s->light.dir[0..2] */
    uint32_t nr_cascades;                    /* 1 .. 4; 0: 4 */
    float    persp[CLAPGPU_CASCADES_MAX][16];/* the camera sub-frusta's projections (view.c:33): clapgpu_cascades_persp */
    float    near_backup;                    /* used unless NEAR_BACKUP_FROM_BV */
    uint32_t light_slot;                     /* 1 .. CLAPGPU_VIEW_SLOTS - 1: the source slot of the light's main view */
    uint32_t flags;                          /* CLAPGPU_CASCADES_* */
    uint32_t pad0;
    /* out */
    clapgpu_cascade_view cascade[CLAPGPU_CASCADES_MAX];
    float    view_mx[16], inv_view_mx[16];   /* the light's main view */
    float    near_backup_used;               /* scene.c's near_backup, before the fit's fmaxf(.., 1.0f) */
    uint32_t bv_entity;                      /* the entity of *bv_result, or CLAPGPU_CASCADES_NO_ENTITY */
    uint32_t status;                         /* 0 or CLAPGPU_CASCADES_INVALID */
    uint32_t pad1;
    float    cam_corners[CLAPGPU_CASCADES_MAX + 1][8][4];    /* the camera's sub-frusta's corners, [4]: the main frustum's */
} clapgpu_cascades;

#define CLAPGPU_CASCADE_VIEW_BYTES 336
#define CLAPGPU_CASCADES_BYTES     2416
#ifdef __cplusplus
static_assert(sizeof(clapgpu_cascade_view) == CLAPGPU_CASCADE_VIEW_BYTES && sizeof(clapgpu_cascades) == CLAPGPU_CASCADES_BYTES,
              "the cascades block's layout is ABI");
#else
_Static_assert(sizeof(clapgpu_cascade_view) == CLAPGPU_CASCADE_VIEW_BYTES && sizeof(clapgpu_cascades) == CLAPGPU_CASCADES_BYTES,
               "the cascades block's layout is ABI");
#endif

/* One launch (one wavefront, a lane per fit), no allocation, no host synchronisation: it can be captured.  e: pos_scale,
 * model and model_table are read when the key of *bv_result names an entity.  bv_result (device; may be NULL without
 * NEAR_BACKUP_FROM_BV): what clapgpu_entities_bv_views or the update's fused pick left.  A NULL or misaligned c or source,
 * a NULL e, or a bv_result next to an e without those three arrays: CLAPGPU_ERR_INVALID_ARGUMENTS before any HIP call. */
int clapgpu_cascades_calc(void *stream, clapgpu_cascades *c, clapgpu_views_source *source, const clapgpu_entities *e,
                          const uint64_t *bv_result);

/* The host twins: the kernel's own functions on the host's values (host memory throughout).
 * clapgpu_cascades_calc_host: the whole of clapgpu_cascades_calc on HOST copies of the block and the source.  The bounding
 * volume is given by value: has_env == 0 is the key 0; else env's MODEL box and scale (near_backup is read from the field
 * without NEAR_BACKUP_FROM_BV, as in the kernel); bv_entity is then set to 0, which the caller overwrites with the entity
 * it meant.  clapgpu_cascades_near_backup: scene.c:1030-1037 alone.  clapgpu_cascades_persp: persp[] of the block from the
 * main view's fov, aspect, near and far planes by the splits of view.c:13-26 (15, 50, 150, then far) and
 * clapgpu_perspective. */
void clapgpu_cascades_calc_host(clapgpu_cascades *c, clapgpu_views_source *source, const float env_box_lo[3],
                                const float env_box_hi[3], float env_scale, int has_env);
float clapgpu_cascades_near_backup(const float light_dir[3], const float env_box_lo[3], const float env_box_hi[3], float env_scale);
void clapgpu_cascades_persp(float fov, float aspect, float near_plane, float far_plane, uint32_t nr_cascades, int ndc_z_zero_one,
                            float persp[64]);

/* The bounding-volume pick with its positions in device memory: the twin of the pick the fused update does for
 * clapgpu_entities.bv, as a pass of its own over the boxes the update stored (it stands to the update as
 * clapgpu_entities_cull_views stands to the fused cull).  The camera position is state->slot[0].cam_pos, the control
 * position e->pos_scale[ctl_entity].xyz, read by the kernel; ctl_entity >= e->n with has_ctl set: no control.  *result
 * (cleared on the stream first) and inside_mask get the bits the fused pick gives when clapgpu_bv_query holds those two
 * positions; result may be NULL when inside_mask is given; both NULL: nothing is asked for and nothing is launched.  e:
 * flags, aabb, model, model_table and pos_scale are read.  One launch, one wavefront per 64 entities; it can be captured. */
int clapgpu_entities_bv_views(void *stream, const clapgpu_entities *e, const clapgpu_views_state *state, uint32_t has_ctl,
                              uint32_t ctl_entity, uint64_t *result, uint64_t *inside_mask);

/* ======================================================================== */
/* Spotlights on the device (ABI 52)                                         */
/* ======================================================================== */

/*
 * light_update (core/light.c:462-471, called from scene_update ahead of mq_update, scene.c:1170) for the lights that
 * track an entity: every light slot made from scene.json registers light_update_from_entity (light.c:385-422) on its
 * entity's transform (scene.c:1626-1631), and when that transform has moved the callback writes the light's position,
 * a spotlight's direction and the pose of a spotlight's own shadow view -- the view that culls the shadow passes when
 * light 0 is a spotlight (scene.c:1043 skips the cascade fit then).  clapgpu_spots is a HOST struct of DEVICE pointers:
 * the tracked lights in entity order, the slots' dir and cutoff (clapgpu_lights stays as it is: callers build it
 * positionally), and one status word.  A frame whose spotlight rides a body, a character or an animated entity needs no
 * host between the body read-back and the shadow passes' cull, and a replayed graph's spot view follows its carrier.
 *
 * THE RULE.  clapgpu_lights_update does the callback's arithmetic in its order, in fp32, with no FMA contraction, by
 * the function its host twin calls (csrc/lm_dev.h), so the arrays hold the host's bits; every NaN stored in dir is
 * 0x7fc00000 (as for the view block).
 *   which carriers apply (light.c:464-467): carrier k applies iff 0 <= carrier_light[k] < nr_lights, carrier_entity[k] <
 *       e->n, active[light] is set, and the entity's CLAPGPU_E_DIRTY is set (this mirror's transform_is_updated,
 *       light.c:467) or mode has CLAPGPU_UPDATE_ALL_DIRTY.  There is NO parent test: light_update has none and the
 *       transform it reads is the local one (light.c:391) -- this is where the call differs from
 *       clapgpu_lights_from_entities.
 *   who writes a slot (light.c:464: one callback per slot, the last registered): per light slot the last applying
 *       carrier in list order writes it, and the same holds per view slot.
 *   position (light.c:391-393, 473-480): lights->pos[l] = pos + carrier_off per component -- the bits
 *       clapgpu_lights_from_entities leaves, so a carrier in both lists is written twice with one value.
 *   the spotlight test (light.c:395, 516-522): is_dir[l] && (double)cutoff[l] > 0.0; a NaN cutoff is no spotlight.
 *   direction, spotlights only (light.c:398-400, 508-514): r = quat_mul_vec3(rot[e], (0,0,1)) in linmath's order with
 *       every product kept (inf * 0 stays NaN); dir[l][i] = 0.0f - r[i] -- vec3_sub from a zero vector, not a negation:
 *       -0 becomes +0.
 *   view pose, a spotlight with a nonzero view slot v (light.c:409, view_update_from_angles on e->xform):
 *       source->slot[v].pos gets the entity's position bits (NOT + carrier_off) and source->slot[v].quat its rotation
 *       bits, copies bit for bit, NaNs included; nothing else of the slot is touched.  The host writes that slot's
 *       proj_mx once (clapgpu_spot_persp, light.c:404-408) and its flags once (CLAPGPU_VIEW_FROM_POSE, plus
 *       NDC_Z_ZERO_ONE as the renderer has it).  A slot that is no spotlight writes no view: the callback has returned
 *       by then (light.c:395-396).
 * The copies of subview[0] into subview[1..3] and their dividers (light.c:418-421) are not produced: a consumer reads the
 * slot's clapgpu_view_state for every cascade.  light_update_from_camera (light.c:430-460) has no user in the reference
 * and none here.
 * What the host cannot see before a HIP call it cannot refuse: carrier_view_slot[] and the slots' flags live in device
 * memory.  If any carrier, applying or not, has a nonzero view slot outside 1 .. CLAPGPU_VIEW_SLOTS - 1, or one naming a
 * slot whose flags lack CLAPGPU_VIEW_FROM_POSE, the kernel writes *status = CLAPGPU_SPOTS_INVALID and nothing else;
 * otherwise *status = 0.
 */
#define CLAPGPU_SPOTS_INVALID 1u             /* status */

typedef struct clapgpu_spots {
    uint32_t        n, pad;             /* tracked lights, in entity order */
    const uint32_t *carrier_entity;     /* [n] */
    const int32_t  *carrier_light;      /* [n] */
    const float    *carrier_off;        /* [3n] e->light_off */
    const uint32_t *carrier_view_slot;  /* [n] 0: no view; 1 .. CLAPGPU_VIEW_SLOTS-1: the source slot of light.view[idx].main; may be NULL (all 0) */
    float          *dir;                /* [3 * CLAPGPU_LIGHTS_MAX] light->dir, written */
    const float    *cutoff;             /* [CLAPGPU_LIGHTS_MAX] light->cutoff, radians */
    uint32_t       *status;             /* one device word: 0 or CLAPGPU_SPOTS_INVALID, written by every launch */
} clapgpu_spots;

#define CLAPGPU_SPOTS_BYTES 64
#ifdef __cplusplus
static_assert(sizeof(clapgpu_spots) == CLAPGPU_SPOTS_BYTES, "the spots descriptor's layout is ABI");
#else
_Static_assert(sizeof(clapgpu_spots) == CLAPGPU_SPOTS_BYTES, "the spots descriptor's layout is ABI");
#endif

/* One launch (one workgroup of CLAPGPU_LIGHTS_MAX lanes), no allocation, no host synchronisation: it can be captured.
 * e: pos_scale, rot and flags are read.  source may be NULL iff s->carrier_view_slot is NULL.  Call BEFORE
 * clapgpu_entities_update, which clears the dirty flags.  Refused with CLAPGPU_ERR_INVALID_ARGUMENTS before any HIP
 * call: a NULL e / s / lights (or a lights without its arrays); an e without pos_scale / rot / flags; n > 0 with a NULL
 * carrier_entity / carrier_light / carrier_off; a NULL dir / cutoff / status; a NULL or misaligned source next to a
 * carrier_view_slot.  nr_lights > CLAPGPU_LIGHTS_MAX: CLAPGPU_ERR_TOO_LARGE.  n == 0 or nr_lights == 0: nothing is
 * launched (status keeps its value) and CLAPGPU_OK. */
int clapgpu_lights_update(void *stream, const clapgpu_entities *e, uint32_t mode, const clapgpu_spots *s,
                          const clapgpu_lights *lights, clapgpu_views_source *source);
/* The host twin: the kernel's own function on the host's values -- the same structs with HOST pointers, e's pos_scale /
 * rot / flags as host arrays.  Arguments the device call refuses make it return without writing. */
void clapgpu_lights_update_host(const clapgpu_entities *e, uint32_t mode, const clapgpu_spots *s,
                                const clapgpu_lights *lights, clapgpu_views_source *source);
/* A spotlight view's projection (light.c:404-408, view.c:178-193): clapgpu_perspective(cutoff * 1.0f, 1.0f / 1.0f, 0.1f,
 * 200.0f, ndc_z_zero_one).  Host. */
void clapgpu_spot_persp(float cutoff, int ndc_z_zero_one, float proj[16]);

/* ======================================================================== */
/* Draw records on the device (ABI 53)                                       */
/* ======================================================================== */

/*
 * What _models_render (core/model.c:742-1086) sets per drawn entity, for one render pass, in the order it draws: txmodel
 * by txmodel in list order (model.c:784) and inside a txmodel in the order of its entity list (model.c:959).  The
 * frame's visible list is in device index order and carries no uniforms; clapgpu_draw_records leaves one fixed-size
 * record per draw in the reference's order, and the range of every txmodel, so a renderer reads device buffers and no
 * host pass walks what is drawn.
 *
 * clapgpu_draw_order is a HOST struct of DEVICE pointers, static while the topology stands (the caller builds it where
 * it builds tile_row_start): the walk of model.c:784 / :959 flattened.  order[r] is the entity at render position r;
 * entities that belong to no txmodel (padding lanes) are simply absent.  group_start[g] .. group_start[g + 1] are the
 * positions of txmodel g: ascending, group_start[0] == 0, group_start[n_groups] == n_order; an empty group is legal.
 * group_flags[g] has CLAPGPU_DRAW_GROUP_SKIP_SHADOW where model3d.skip_shadow is set.
 *
 * clapgpu_draw_inputs is a HOST struct of DEVICE pointers indexed by ENTITY, so that entity3d_color() and friends stay
 * one store.  Any of them may be NULL: zeros then, and -1 for character.
 *
 * clapgpu_draw_pass holds HOST values: what models_render_options says about the pass.
 *
 * THE RULE, followed by the kernels and by the host twin through the same functions (csrc/draw_dev.h):
 *   which groups draw (model.c:786): a group with CLAPGPU_DRAW_GROUP_SKIP_SHADOW emits nothing in a pass with
 *       CLAPGPU_DRAW_PASS_SHADOW (opts->shader_override).
 *   which positions draw (model.c:960-973): position r is drawn iff bit order[r] of vis_mask is set -- the planes hold
 *       ALIVE && VISIBLE && (SKIP_CULLING || in the view's frustum) -- or, with vis_mask == NULL (the pass without a
 *       view, model.c:969-970: `view &&`), iff flags[order[r]] has CLAPGPU_E_ALIVE and CLAPGPU_E_VISIBLE.  The records
 *       are the drawn positions in ascending r.  (nr_ents, model.c:1049, is *count.)
 *   group_first[g] is the number of records in front of group g; group_first[n_groups] == *count, the total.
 *   mx, inv_mx (model.c:1027-1028), color and color_pt (model.c:1017-1018) are moved as 32-bit words: NaN payloads
 *       survive, this is a copy and not arithmetic.
 *   lod = lod[i] (model.c:993-997, 1042: e->cur_lod), or 0 with lod == NULL; character = character[i]; group = g;
 *       entity = index_base + i.
 *   bloom intensity (model.c:1000-1003): if (double)fabsf(e.bloom_intensity) > 1e-3 the entity's value, else with
 *       CLAPGPU_DRAW_PASS_HAS_ROPTS (`else if (ropts)`) the pass's; in both cases CLAPGPU_DRAW_SET_BLOOM_INTENSITY is
 *       set in the record's flags.  Otherwise the field is 0 and the bit clear: the reference leaves the uniform at
 *       whatever the previous draw set, and a consumer has to know that.  The comparison is the reference's: the float
 *       promoted to double against the double constant 1e-3, so (float)1e-3, which lies above it, passes and the float
 *       below it does not; a NaN does not pass.
 *   bloom threshold (model.c:1005-1008): the same rule, CLAPGPU_DRAW_SET_BLOOM_THRESHOLD.
 *   edge_mode (model.c:1010-1016, shader_constants.h:57-62): CLAPGPU_DRAW_OUTLINE_EXCLUDE gives EDGE_EXCLUDE, 1u << 7;
 *       with CLAPGPU_DRAW_IS_CHARACTER and mq_nr_characters != 0 it also gets (k & 15u), k the 1-based ordinal of this
 *       draw among the DRAWN characters of its group in render order (nr_characters restarts per txmodel, model.c:956,
 *       and counts only what passed the cull): the 16th drawn character of a txmodel gets 0, the 17th 1.
 *   the three words at offset 180 are zero.
 * Not produced: the LOD's buffer binds (a consumer compares lod with the record in front), joint_transforms (the
 * record's character indexes the pose batch), the particle instance count.  Alpha-blended models are not sorted; the
 * reference does not sort either.
 *
 * Capacity: records at or past `capacity` are not written; *count still holds the total, group_first is complete and
 * *status has CLAPGPU_DRAW_CAPPED.  What the host cannot see it cannot refuse: an order[r] >= entities->n, a
 * group_start that does not ascend, does not start at 0 or does not end at n_order give *status = CLAPGPU_DRAW_INVALID,
 * *count = 0, group_first all zeros and nothing else written (the rule of CLAPGPU_SPOTS_INVALID).
 */
#define CLAPGPU_DRAW_GROUP_SKIP_SHADOW   1u  /* group_flags: model3d.skip_shadow */
#define CLAPGPU_DRAW_IS_CHARACTER        1u  /* draw_flags: ENTITY3D_IS_CHARACTER */
#define CLAPGPU_DRAW_OUTLINE_EXCLUDE     2u  /* draw_flags: e->outline_exclude */
#define CLAPGPU_DRAW_PASS_SHADOW         1u  /* pass flags: opts->shader_override */
#define CLAPGPU_DRAW_PASS_HAS_ROPTS      2u  /* pass flags: opts->render_options != NULL */
#define CLAPGPU_DRAW_SET_BLOOM_INTENSITY 1u  /* record flags: this draw sets the uniform */
#define CLAPGPU_DRAW_SET_BLOOM_THRESHOLD 2u
#define CLAPGPU_DRAW_CAPPED              1u  /* status */
#define CLAPGPU_DRAW_INVALID             2u  /* status */

typedef struct clapgpu_draw_order {
    uint32_t        n_order, n_groups;
    const uint32_t *order;              /* [n_order] entity at render position r */
    const uint32_t *group_start;        /* [n_groups + 1] */
    const uint32_t *group_flags;        /* [n_groups] */
} clapgpu_draw_order;

typedef struct clapgpu_draw_inputs {
    const float    *color;              /* [4n] e->color */
    const int32_t  *color_pt;           /* [n] e->color_pt */
    const float    *bloom_intensity;    /* [n] */
    const float    *bloom_threshold;    /* [n] */
    const uint32_t *draw_flags;         /* [n] CLAPGPU_DRAW_IS_CHARACTER | CLAPGPU_DRAW_OUTLINE_EXCLUDE */
    const int32_t  *character;          /* [n] index into the pose batch, or -1 */
} clapgpu_draw_inputs;

typedef struct clapgpu_draw_pass {
    uint32_t flags;                     /* CLAPGPU_DRAW_PASS_* */
    float    bloom_intensity;           /* ropts->bloom_intensity */
    float    bloom_threshold;           /* ropts->bloom_threshold */
    uint32_t mq_nr_characters;          /* mq->nr_characters */
    uint32_t index_base;
} clapgpu_draw_pass;

typedef struct clapgpu_draw_record {    /* three 64-byte lines */
    float    mx[16];                    /*   0 UNIFORM_TRS */
    float    inv_mx[16];                /*  64 UNIFORM_INVERSE_TRS */
    float    color[4];                  /* 128 UNIFORM_IN_COLOR */
    float    bloom_intensity;           /* 144 */
    float    bloom_threshold;           /* 148 */
    uint32_t edge_mode;                 /* 152 UNIFORM_EDGE_MODE */
    int32_t  color_pt;                  /* 156 UNIFORM_COLOR_PASSTHROUGH */
    uint32_t entity;                    /* 160 index_base + i */
    int32_t  lod;                       /* 164 */
    uint32_t group;                     /* 168 */
    int32_t  character;                 /* 172 */
    uint32_t flags;                     /* 176 CLAPGPU_DRAW_SET_* */
    uint32_t zero[3];                   /* 180 */
} clapgpu_draw_record;

#define CLAPGPU_DRAW_RECORD_BYTES 192
#ifdef __cplusplus
#define CLAPGPU_DRAW_ASSERT(c) static_assert(c, "the draw record's layout is ABI")
#else
#define CLAPGPU_DRAW_ASSERT(c) _Static_assert(c, "the draw record's layout is ABI")
#endif
CLAPGPU_DRAW_ASSERT(sizeof(clapgpu_draw_record) == CLAPGPU_DRAW_RECORD_BYTES);
CLAPGPU_DRAW_ASSERT(offsetof(clapgpu_draw_record, inv_mx) == 64 && offsetof(clapgpu_draw_record, color) == 128);
CLAPGPU_DRAW_ASSERT(offsetof(clapgpu_draw_record, bloom_intensity) == 144 && offsetof(clapgpu_draw_record, bloom_threshold) == 148);
CLAPGPU_DRAW_ASSERT(offsetof(clapgpu_draw_record, edge_mode) == 152 && offsetof(clapgpu_draw_record, color_pt) == 156);
CLAPGPU_DRAW_ASSERT(offsetof(clapgpu_draw_record, entity) == 160 && offsetof(clapgpu_draw_record, lod) == 164);
CLAPGPU_DRAW_ASSERT(offsetof(clapgpu_draw_record, group) == 168 && offsetof(clapgpu_draw_record, character) == 172);
CLAPGPU_DRAW_ASSERT(offsetof(clapgpu_draw_record, flags) == 176 && offsetof(clapgpu_draw_record, zero) == 180);

/* Bytes of device scratch (256-byte aligned) a call with these sizes needs: the render-space masks, their row counts and
 * prefixes, the per-group character counts.  Never 0. */
size_t clapgpu_draw_records_scratch_bytes(uint32_t n_order, uint32_t n_groups);
/* Three launches (render-space masks; prefixes per group; record fill), no allocation, no host synchronisation: it can
 * be captured.  entities: n, mx and inv_mx are read, and flags when vis_mask is NULL.  vis_mask: any entity-space plane
 * of ceil(n / 64) words (entities->vis_mask, a plane of entities->views), or NULL: the pass without a view.  lod: the
 * per-entity cur_lod array, NULL: 0.  inputs may be NULL (every array absent).  records: [capacity], 64-byte aligned.
 * count, status: one device word each; group_first: [n_groups + 1] device words.  scratch: 256-byte aligned,
 * clapgpu_draw_records_scratch_bytes(n_order, n_groups).  Refused with CLAPGPU_ERR_INVALID_ARGUMENTS before any HIP
 * call: a NULL entities / order / pass / count / group_first / status; NULL records with capacity > 0; a misaligned
 * records or scratch, or a NULL scratch; entities without mx / inv_mx (or without flags beside a NULL vis_mask);
 * n_order > 0 with a NULL order->order or n_groups == 0; n_groups > 0 with a NULL group_start / group_flags.
 * n_order == 0 or entities->n == 0 still leaves *count = 0, *status = 0 and a zeroed group_first. */
int clapgpu_draw_records(void *stream, const clapgpu_entities *entities, const uint64_t *vis_mask, const int32_t *lod,
                         const clapgpu_draw_order *order, const clapgpu_draw_inputs *inputs, const clapgpu_draw_pass *pass,
                         clapgpu_draw_record *records, uint32_t capacity, uint32_t *count, uint32_t *group_first,
                         uint32_t *status, void *scratch);
/* The host twin: the kernels' own decision functions over HOST pointers (every struct as above with host arrays; no
 * stream, no scratch).  Arguments the device call refuses make it return without writing. */
void clapgpu_draw_records_host(const clapgpu_entities *entities, const uint64_t *vis_mask, const int32_t *lod,
                               const clapgpu_draw_order *order, const clapgpu_draw_inputs *inputs, const clapgpu_draw_pass *pass,
                               clapgpu_draw_record *records, uint32_t capacity, uint32_t *count, uint32_t *group_first,
                               uint32_t *status);

/* One pass's outputs inside a frame: the arguments of clapgpu_draw_records behind `inputs`.  A block with count == NULL
 * is not issued.  NULL records with capacity == 0 and a count is legal: counts and ranges only. */
typedef struct clapgpu_frame_draw_pass {
    clapgpu_draw_pass    pass;
    uint32_t             capacity;
    clapgpu_draw_record *records;       /* device */
    uint32_t            *count;         /* device */
    uint32_t            *group_first;   /* device */
    uint32_t            *status;        /* device */
} clapgpu_frame_draw_pass;

/* clapgpu_frame.draw: a HOST struct.  main is the model pass over entities->vis_mask; view[v] is the pass of further
 * view v over entities->views->vis_mask[v] (the shadow passes).  scratch is shared: the passes run one after the other. */
typedef struct clapgpu_frame_draw {
    const clapgpu_draw_order  *order;
    const clapgpu_draw_inputs *inputs;  /* may be NULL */
    clapgpu_frame_draw_pass    main;
    clapgpu_frame_draw_pass    view[CLAPGPU_EXTRA_VIEWS_MAX];
    void                      *scratch; /* device, clapgpu_draw_records_scratch_bytes(order->n_order, order->n_groups) */
} clapgpu_frame_draw;

/* ======================================================================== */
/* One frame (core/clap.c:551-665)                                           */
/* ======================================================================== */

/*
 * Everything clap_frame() does on the batched path, as one C call that issues the launches in the reference's
 * order on `stream` -- scene_characters_move (when `move` is set), phys_step's substeps (broadphase x2, contact records, world step), character hooks, body
 * read-back + rotation push + light hand-off, the entity update with the main view's cull, animation clock + pose +
 * skinning, particles, the light grid, the ordered visible list + LOD pick -- without reading anything back.
 * Every pointer except `entities` may be NULL: that part of the frame is skipped.  The descriptor holds no state: a
 * caller builds it once and reuses it; capturing the call in a HIP graph (now_dev for the clock) replays the frame
 * with one launch.
 */
typedef struct clapgpu_frame {
    /* entities: tile layout (tile_row_start, device) or level-major (level_start, host) */
    const clapgpu_entities   *entities;
    const uint32_t           *tile_row_start;  uint32_t n_tiles;
    const uint32_t           *level_start;     uint32_t n_levels;
    const clapgpu_frustum    *frustum;         /* main view: fused cull; NULL = no cull, no visible list */
    /* physics (physics.c:746-812) */
    const clapgpu_bodies     *bodies;
    const clapgpu_world      *world;
    clapgpu_bp               *bp;
    uint32_t *pairs, pair_capacity, *pair_total;
    uint32_t *static_pairs, static_pair_capacity, *static_pair_total;
    const clapgpu_geoms      *body_geoms, *static_geoms;
    clapgpu_contact2 *contacts, *static_contacts;
    uint32_t *contact_total, *static_contact_total;
    uint32_t n_body_links; const uint32_t *link_body, *link_entity;
    /* character feeder (character.c:583-611) */
    const clapgpu_characters *characters;
    /* lights: hand-off from their carrier entities, then the tile masks */
    const clapgpu_lights     *lights;
    uint32_t n_light_carriers; const uint32_t *carrier_entity; const int32_t *carrier_light; const float *carrier_offset;
    uint32_t light_width, light_height, light_cell; uint32_t *light_tiles;
    const float              *view_mx, *proj_mx;     /* HOST, 16 floats each */
    /* skeletal animation */
    const clapgpu_anim_clock *anim_clock;      const double *now_dev;   /* device clock for graph replay, or NULL: `now` */
    const clapgpu_skeleton   *skeleton;
    const clapgpu_animations *animations;
    const clapgpu_pose_batch *pose;
    const clapgpu_skin_batch *skin;
    /* particles */
    const clapgpu_particles  *particles;
    /* render-pass glue */
    uint32_t index_base; uint32_t *visible, *visible_count; void *visible_scratch;
    float cam_pos[3]; const int32_t *force_lod; int32_t *cur_lod, *draw_lod;
    uint32_t flags;                            /* CLAPGPU_FRAME_* */
    /* contacts against static meshes (clapgpu_contacts_meshes) after each substep's static contacts; meshes NULL: none.
     * Needs body_geoms, static_geoms, static_pairs and static_pair_total */
    const clapgpu_trimesh    *meshes;
    clapgpu_contact2 *mesh_contacts; uint32_t *mesh_ref; uint32_t mesh_contact_capacity;
    uint32_t *mesh_contact_total, *mesh_capped;
    uint32_t *mesh_scratch;                    /* CLAPGPU_MESH_CONTACT_SCRATCH(static_pair_capacity) uint32 */
    /* waking by contact (clapgpu_bodies_islands) in every substep, after its last contact launch and before its step;
     * island_scratch NULL: this stage is skipped.  Needs pairs, pair_total, contacts and body_geoms; island / island_woken
     * may be NULL */
    void     *island_scratch;                  /* clapgpu_bodies_islands_scratch_bytes(bodies->n) bytes, 256-byte aligned */
    uint32_t *island, *island_woken;
    /* contact response (clapgpu_bodies_solve) in every substep, between its island pass and its step; solve_scratch NULL:
     * this stage is skipped.  Needs island_scratch and island; solver NULL: clapgpu_solver_defaults.  solve_status (may be
     * NULL) as *status of clapgpu_bodies_solve; its other outputs are not asked for */
    const clapgpu_solver *solver;
    void     *solve_scratch;                   /* clapgpu_bodies_solve_scratch_bytes(bodies->n, solve_rows_capacity), 256-byte aligned */
    uint32_t  solve_rows_capacity;
    uint32_t *solve_status;
    /* scene_characters_move (clap.c:589, before phys_step): clapgpu_characters_move as the frame's first stage, on the
     * physics chain under CLAPGPU_FRAME_OVERLAP, over bodies, world, bp, static_geoms and meshes of this descriptor and,
     * for the rotation hand-off, entities.  move NULL: this stage is skipped.  clapgpu_characters.airborne may alias
     * move->airborne when both lists are in the same order: the hooks then see what this frame's move left */
    const clapgpu_move *move;
    double    move_dt_sec;                     /* the raw frame delta, as clapgpu_characters_move takes it */
    void     *move_scratch;                    /* clapgpu_characters_move_scratch_bytes(bodies->n, move->n), 256-byte aligned */
    /* character states and animation queues on the device (ABI 46); NULL: the frame as before, launch for launch.  Set:
     * clapgpu_characters_state(aniq, move) follows the move stage (when move is set), and clapgpu_animation_queue_time
     * takes the place of the clock (anim_clock is not read).  The queue clock is a launch of its own behind the character
     * hooks, which read airborne before animated_update's callback can set it; under CLAPGPU_FRAME_OVERLAP the animation
     * chain is forked behind it.  Needs skeleton, animations and pose, with pose->anim == aniq->pose_anim, pose->frame_time
     * == aniq->frame_time and pose->n_chars == aniq->n: CLAPGPU_ERR_INVALID_ARGUMENTS otherwise, before any launch */
    const clapgpu_aniq *aniq;
    /* skinning that follows the cull and the LOD (ABI 48); NULL: the frame as before, launch for launch.  Set: the
     * animation chain no longer issues clapgpu_skin, and clapgpu_skin_drawn(skin, skin_select) is the frame's LAST stage:
     * behind the visible list and the LOD pick, and behind the join under CLAPGPU_FRAME_OVERLAP.  n_planes == 0 in the
     * descriptor: the frame supplies the planes and n_entities itself -- entities->vis_mask and the planes of
     * entities->views; cur_lod == NULL there: this descriptor's cur_lod is used when it has one.  Needs skin, pose (with
     * skeleton and animations) and frustum: CLAPGPU_ERR_INVALID_ARGUMENTS otherwise, before any launch */
    const clapgpu_skin_select *skin_select;
    /* views in device memory (ABI 49); both NULL: the frame as before, launch for launch.  Both set (one alone, or
     * views_state next to a non-NULL frustum: CLAPGPU_ERR_INVALID_ARGUMENTS before any launch): clapgpu_views_calc(
     * views_source, views_state, 1 + entities->views->n) is the frame's FIRST launch on the caller's stream, ahead of any
     * fork of CLAPGPU_FRAME_OVERLAP; the entity update runs without its fused cull and clapgpu_entities_cull_views follows
     * it over the boxes it stored (the same masks: the fused kernel's frustum is a kernel argument); the light grid, the
     * particles and the LOD pick use their *_views twins.  frustum (NULL), view_mx, proj_mx, cam_pos and
     * entities->views->frustum[] are not read, and "the frame has a main view" (visible list, LOD pick, skin_select)
     * means frustum || views_state.  A replayed graph of such a frame follows whatever was written into views_source
     * before the replay.  entities->bv stays host-valued (its twin over the block: bv_result, below) */
    const clapgpu_views_source *views_source;  /* device */
    clapgpu_views_state        *views_state;   /* device */
    /* the shadow cascades on the device (ABI 51); cascades NULL: the frame as before, launch for launch (the three fields
     * behind it are not read).  Set: it needs views_source, views_state and entities->views with n >= 1 (the light's
     * slot; light_slot itself lives in the device block: a slot the frame's views do not reach is fitted and not culled):
     * CLAPGPU_ERR_INVALID_ARGUMENTS otherwise, before any launch.  The tail of the frame takes the camera frame's shape
     * whether or not `camera` is set -- the head clapgpu_views_calc stays, the update runs without its cull -- and
     * behind the join, clapgpu_joint_pos_world and the light grid the frame issues, in this order:
     * clapgpu_entities_bv_views(entities, views_state, bv_has_ctl, bv_ctl_entity, bv_result, NULL) when bv_result is set
     * (the flag that asks for the volume lives in the device block, so "bv_result set" means "the frame runs the pick";
     * it reads the head's cam_pos, the camera the previous frame left, which is the position default_update sees:
     * scene_update runs before scene_cameras_calc); clapgpu_bp_index and clapgpu_camera_calc when `camera` is set;
     * clapgpu_cascades_calc(cascades, views_source, entities, bv_result); the second clapgpu_views_calc over all slots;
     * clapgpu_entities_cull_views, the visible list with the LOD pick, and skin_select.  bv_has_ctl / bv_ctl_entity are
     * host values: camera->ctl_entity is in device memory */
    clapgpu_cascades           *cascades;      /* device */
    uint64_t                   *bv_result;     /* device, or NULL: no pick */
    uint32_t                    bv_has_ctl, bv_ctl_entity;
    /* spotlights on the device (ABI 52); spots NULL: the frame as before, launch for launch.  Set: it needs lights, and
     * with a spots->carrier_view_slot also views_source and views_state (CLAPGPU_ERR_INVALID_ARGUMENTS otherwise, before
     * any launch).  clapgpu_lights_update(entities, 0, spots, lights, views_source) is issued directly before the light
     * hand-off: behind the body read-back and the character hooks, which set DIRTY, and ahead of the entity update, which
     * clears it -- light_update before mq_update (scene.c:1170).  With a carrier_view_slot the tail takes the cascades
     * frame's shape whether or not camera / cascades are set: the head clapgpu_views_calc stays, the update runs without
     * its cull, and behind the join come the second clapgpu_views_calc over all slots, clapgpu_entities_cull_views, the
     * list with the LOD pick and skin_select -- the shadow passes are culled against THIS frame's spot.  A spot's view
     * slot equal to cascades->light_slot is the caller's contradiction (the reference never fits light 0 when it is a
     * spotlight, scene.c:1043): both write the slot, the fit last.
     * view_visible[v] set: behind the main list the frame issues clapgpu_visible_compact(views->vis_mask[v],
     * views->vis_row_pop[v], n, index_base, view_visible[v], view_visible_count[v], visible_scratch): the ordered list of
     * shadow pass v, which _models_render walks with view = &light->view[0].  No LOD is picked: a shadow pass has no
     * camera (model.c:752-760, 975) and draws with the cur_lod the entity has.  It needs a main view (frustum or
     * views_state), v < entities->views->n, view_visible_count[v] and visible_scratch: CLAPGPU_ERR_INVALID_ARGUMENTS
     * otherwise, before any launch.
     * (These fields stand in front of `camera`, as the cascades' do: the descriptor's version is CLAPGPU_ABI_VERSION.) */
    const clapgpu_spots        *spots;
    uint32_t *view_visible[CLAPGPU_EXTRA_VIEWS_MAX], *view_visible_count[CLAPGPU_EXTRA_VIEWS_MAX];
    /* draw records on the device (ABI 53); draw NULL: the frame as before, launch for launch.  Set: it needs a main view
     * (frustum or views_state), draw->order, draw->scratch, and for every further view's block with a count
     * v < entities->views->n: CLAPGPU_ERR_INVALID_ARGUMENTS otherwise, before any launch, as for anything
     * clapgpu_draw_records itself refuses.  The further views' records are issued BEHIND THE CULL AND AHEAD OF the visible
     * list and the LOD pick: pipeline_render runs the shadow passes before the model pass (pipeline-builder.c:246-272),
     * and without a camera they draw with the cur_lod the last model pass left (model.c:975) -- clapgpu_draw_records(
     * entities, views->vis_mask[v], cur_lod, order, inputs, &view[v].pass, ...).  The main pass's records are issued
     * BEHIND the LOD pick, over entities->vis_mask with lod = cur_lod: this frame's LODs.  skin_select stays last.
     * (The field stands in front of `camera`, as the spots' do.) */
    const clapgpu_frame_draw   *draw;
    /* the camera controller on the device (ABI 50); camera NULL: the frame as before, launch for launch (camera_bp is not
     * read).  Set: it needs views_source and views_state (CLAPGPU_ERR_INVALID_ARGUMENTS otherwise, before any launch),
     * and writes slot 0 of views_source.  The rays see body_geoms, or the geoms of bodies when that is NULL, or no body,
     * and static_geoms, or no static.  The head clapgpu_views_calc stays -- particles and the light grid read it: the
     * camera the previous frame left, which is the reference's order (scene_update before scene_cameras_calc,
     * clap.c:614-616) -- and clapgpu_entities_cull_views moves from behind the update to behind the camera: after the
     * join, clapgpu_joint_pos_world and the light grid the frame issues clapgpu_bp_index(camera_bp, bodies->n,
     * bodies->aabb) when camera_bp is set (it needs bodies then), clapgpu_camera_calc(camera, entities, pose->joint_pos,
     * camera_bp, those geoms, meshes, views_source), a second clapgpu_views_calc, the cull, the visible
     * list with the LOD pick, and skin_select.  Slots 1.. of the source keep what the host wrote */
    clapgpu_camera             *camera;        /* device */
    clapgpu_bp                 *camera_bp;     /* may be NULL: the rays scan every geom */
} clapgpu_frame;

/* Default (0): everything on the caller's stream in the reference's order.  CLAPGPU_FRAME_OVERLAP: the frame's three
 * independent chains -- physics -> entity update; animation clock -> pose -> skinning; particles -- run on the caller's
 * stream and two helper streams forked from and joined into it by events (graph capture records the same edges); joint
 * world positions, light grid, visible list and LOD pick follow the join.  Results are identical either way; on one
 * MI355X the overlapped frame is NOT shorter (0.64 against 0.62 ms at BASELINE sizes: csrc/frame.hip). */
#define CLAPGPU_FRAME_OVERLAP 1u
/* CLAPGPU_FRAME_PREBIN: every substep's body step also bins the boxes it writes for the NEXT broadphase pass
 * (clapgpu_bodies_step_prebin): one launch less per substep.  The caller promises that nothing but this frame call writes
 * bodies->aabb between frames (or calls clapgpu_bp_invalidate after doing so). */
#define CLAPGPU_FRAME_PREBIN  2u

int clapgpu_frame_issue(void *stream, const clapgpu_frame *f, double now, uint32_t physics_substeps);

#ifdef __cplusplus
}
#endif
#endif /* CLAPGPU_H */
