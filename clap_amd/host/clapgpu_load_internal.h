/*
 * clapgpu_load_internal.h -- what the loader's files share (include/clapgpu_load.h is the public side).
 *
 *   clapgpu_load_json.c    JSON text -> node tree, typed getters
 *   clapgpu_load_gltf.c    file reader, base64, GLB container, glTF document -> struct gltf, mesh choice
 *   clapgpu_load_model.c   struct gltf -> struct ld_model (geometry, skin, animations, collision mesh), its snapshot arrays
 *   clapgpu_load.c         scene.json walk, lights, the scene's snapshot arrays, the two entry points
 */
#ifndef CLAPGPU_LOAD_INTERNAL_H
#define CLAPGPU_LOAD_INTERNAL_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "clapgpu_snapshot.h"

#define LOAD_LOCAL __attribute__((visibility("hidden")))       /* shared by the loader's files, not exported */

#define LD_OK            0
#define LD_NOMEM        (-1)        /* CERR_NOMEM */
#define LD_NOT_FOUND    (-2)
#define LD_INVALID      (-3)        /* CERR_INVALID_ARGUMENTS */
#define LD_PARSE        (-4)        /* CERR_PARSE_FAILED */

#define JOINT_TYPE_MAX   6          /* model.h:31-37 */
#define LIGHTS_MAX       128
#define E_VISIBLE        (1u << 0)  /* model.h:294-310 */
#define E_IS_CHARACTER   (1u << 1)
#define E_HAS_PHYSICS    (1u << 4)
#define E_PHYS_IS_BODY   (1u << 5)
#define E_LIGHT_SOURCE   (1u << 8)
#define E_HAS_ARMATURE   (1u << 12)
#define E_IS_ANIMATED    (1u << 13)
#define E_SKIP_CULLING   (1u << 14)
#define E_ALIVE          (1u << 31)

struct ld_err { char *buf; size_t len; };
LOAD_LOCAL int fail(struct ld_err *e, int rc, const char *fmt, ...) __attribute__((format(printf, 3, 4)));     /* writes the text, returns rc */

/* every array the loader allocates may have no elements: one element is asked for then, zeroed like the rest */
static inline void *ld_alloc(size_t n, size_t el) { return calloc(n ? n : 1, el); }

/* ---------------------------------------------------------------------------------- clapgpu_load_json.c */
enum { J_NULL, J_BOOL, J_NUMBER, J_STRING, J_ARRAY, J_OBJECT };
struct jnode {
    int           tag;
    char         *key, *str;
    double        num;
    int           b;
    unsigned      count;
    struct jnode *head, *tail, *next;
};
struct jparse { const char *p, *end; int bad; struct jnode **all; size_t n_all, cap_all; };

LOAD_LOCAL struct jnode *jdecode(struct jparse *jp, const char *buf, size_t len);     /* NULL: no tree, nothing to free */
LOAD_LOCAL void jfree(struct jparse *jp);
LOAD_LOCAL struct jnode *jfind(const struct jnode *obj, const char *key);
LOAD_LOCAL int jdoubles(const struct jnode *arr, double *out, unsigned n);
LOAD_LOCAL bool jfloats(const struct jnode *arr, float *out, unsigned n);
LOAD_LOCAL int *jints_alloc(const struct jnode *arr, unsigned *count);
LOAD_LOCAL bool jnum_index(const struct jnode *n, double *out);
LOAD_LOCAL int jnum_i(const struct jnode *n, int dflt);
LOAD_LOCAL char *jstrdup(const struct jnode *n);

/* ---------------------------------------------------------------------------------- clapgpu_load_gltf.c */
enum { PATH_TRANSLATION, PATH_ROTATION, PATH_SCALE, PATH_NONE };         /* model.h chan_path order, gltf.c:131-136 */

struct g_bufview { unsigned buffer; size_t offset, length; };
struct g_accessor { unsigned bufview, comptype, count, comps; size_t offset; };
struct g_node { char *name; float rotation[4], scale[3], translation[3]; int mesh, skin; unsigned id, nr_children; int *ch_arr; };
struct g_skin { const float *invmxs; char *name; int *joints, *nodes; unsigned nr_joints, nr_invmxs; };
struct g_mesh { char *name; int indices, material, POSITION, NORMAL, JOINTS_0, WEIGHTS_0; };
struct g_sampler { int input, output, interp; };
struct g_channel { int sampler, node, path; };
struct g_anim { char *name; struct g_sampler *samplers; unsigned n_samplers; struct g_channel *channels; unsigned n_channels; };

struct gltf {
    uint8_t *file; size_t file_size;
    const uint8_t *bin; size_t bin_size;
    uint8_t **buffers; size_t *buffer_size; unsigned n_buffers;
    struct g_bufview *bufvws; unsigned n_bufvws;
    struct g_accessor *accrs; unsigned n_accrs;
    struct g_node *nodes; unsigned n_nodes;
    struct g_skin *skins; unsigned n_skins;
    struct g_mesh *meshes; unsigned n_meshes;
    struct g_anim *anis; unsigned n_anis;
    int root_node;
};

#define GL_U8   0x1401u             /* accessor componentType */
#define GL_U16  0x1403u
#define GL_U32  0x1405u

LOAD_LOCAL int read_file(const char *path, uint8_t **out, size_t *size);
LOAD_LOCAL int gltf_load_file(struct gltf *g, const char *path, struct ld_err *e);    /* on failure nothing is left to free */
LOAD_LOCAL void gltf_free(struct gltf *g);
LOAD_LOCAL const void *accr_buf(const struct gltf *g, int accr, size_t *elsz, unsigned *count);
LOAD_LOCAL uint32_t accr_uint(const void *base, unsigned comptype, size_t i);
LOAD_LOCAL int gltf_pick_mesh(const struct gltf *g);
LOAD_LOCAL int gltf_mesh_skin(const struct gltf *g, int mesh);

/* ---------------------------------------------------------------------------------- clapgpu_load_model.c */
struct ld_anim {
    uint32_t n_channels, n_times, n_data;
    uint32_t *ch_target, *ch_path, *ch_nr, *ch_time_off, *ch_data_off;
    float *times, *data, time_end;
};

struct ld_model {
    char *name;
    float aabb[6];                       /* min xyz, max xyz */
    uint32_t nr_joints;                  /* 0: not skinned */
    int32_t *joint_parent;
    char **joint_name;
    float *invmx, *bind, root_pose[16];
    int32_t joint_types[JOINT_TYPE_MAX];
    uint32_t n_verts;
    float *position, *normal, *weights;
    uint8_t *joints;
    struct ld_anim *anims; uint32_t n_anims;
    char **anim_name;
    uint16_t *cidx; uint32_t n_ctri;     /* "geom": "trimesh": model3d.collision_idx (the vertices are `position`) */
    int has_collision;
};

/* snapshot output: the first failure sticks in rc and turns every later add into a no-op */
struct ld_out { clapgpu_snapshot_writer *w; int rc; };
LOAD_LOCAL void add(struct ld_out *o, const char *comp, const char *key, uint32_t dt, uint32_t nd, uint64_t d0, uint64_t d1, const void *p);
LOAD_LOCAL void add_i64(struct ld_out *o, const char *comp, const char *key, int64_t v);

LOAD_LOCAL int model_from_gltf(struct ld_model *m, const struct gltf *g, int mesh, int fix_origin, struct ld_err *e);
LOAD_LOCAL int collision_from_gltf(struct ld_model *m, const struct gltf *g, int mesh, struct ld_err *e);
LOAD_LOCAL void model_free(struct ld_model *m);
LOAD_LOCAL void write_model(struct ld_out *o, unsigned k, const struct ld_model *m);

#endif
