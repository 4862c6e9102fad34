/*
 * clapgpu_load.c -- scene.json + glTF -> SoA scene snapshot (include/clapgpu_load.h).
 *
 * Follows, rule by rule, what the engine's loaders read and in which order they create things:
 *   scene_onload              scene.c:1816-1884   clapgpu_load.c        top level: "name", "model" [..], "light" [..]
 *   model_new_from_json       scene.c:1318-1724   clapgpu_load.c        one model: keys, defaults, physics, armature, entity / character arrays
 *                             scene.c:1391-1419   clapgpu_load_gltf.c   the mesh choice (gltf_pick_mesh)
 *   scene_add_light_from_json scene.c:1726-1813   clapgpu_load.c
 *   gltf_json_parse           gltf.c:666-1064     clapgpu_load_gltf.c   nodes, scenes, buffers, bufferViews, accessors, animations, skins, meshes
 *   gltf_bin_parse            gltf.c:1065-1096    clapgpu_load_gltf.c   GLB container
 *   gltf_instantiate_one      gltf.c:1158-1331    clapgpu_load_model.c  vertex attributes, skin -> joints / root pose, animations -> channels
 *   model3d_add_skinning      model.c:524-537, animation_add_channel model.c:725-742: clapgpu_load_model.c; light_get light.c:311-340: here
 *   json.c                                        clapgpu_load_json.c   the node tree and its getters
 * Nothing here is executed per frame; the arithmetic that has to match the engine's bits (euler -> quaternion,
 * mat4x4_invert, mat4x4_from_quat, the mesh AABB) goes through the same helpers as the rest of the library.
 */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "clapgpu.h"
#include "clapgpu_load.h"
#include "clapgpu_scene.h"
#include "clapgpu_load_internal.h"

int fail(struct ld_err *e, int rc, const char *fmt, ...)
{
    if (e && e->buf && e->len) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(e->buf, e->len, fmt, ap);
        va_end(ap);
    }
    return rc;
}

/* ================================================================================== the scene being built */
struct vec { void *p; size_t n, cap, el; };
static void *vpush(struct vec *v)
{
    if (v->n == v->cap) {
        const size_t cap = v->cap ? v->cap * 2 : 64;
        void *p = realloc(v->p, cap * v->el);
        if (!p) return NULL;
        v->p = p; v->cap = cap;
    }
    void *slot = (char *)v->p + v->n++ * v->el;
    memset(slot, 0, v->el);
    return slot;
}

struct ld_entity { float pos_scale[4], rot[4]; int32_t parent, parent_joint, model; uint32_t flags; char *name; int32_t light_idx; };
struct ld_carrier { uint32_t entity; int32_t light; float off[3]; };
struct ld_attach { uint32_t entity, parent, joint; };
struct ld_body { uint32_t entity; int32_t geom_class, phys_type; double mass, radius, length, yoffset, bounce, bounce_vel; };
struct ld_char { uint32_t entity, model; double speed; uint8_t can_jump, can_dash; };

struct ld_lights {
    uint32_t nr_lights;
    float pos[LIGHTS_MAX][3], color[LIGHTS_MAX][3], attenuation[LIGHTS_MAX][3], dir[LIGHTS_MAX][3], cutoff[LIGHTS_MAX];
    int32_t is_dir[LIGHTS_MAX];
    uint32_t active[LIGHTS_MAX];
    float ambient[3], shadow_tint[3];
};

struct ld_scene {
    struct vec models, entities, carriers, attaches, bodies, chars;     /* ld_model, ld_entity, ... */
    struct ld_lights lights;
    const char *asset_dir;
};

static int light_get(struct ld_lights *l)                                /* light.c:311-340 */
{
    int idx = -1;
    for (int i = 0; i < LIGHTS_MAX; i++) if (!l->active[i]) { idx = i; break; }    /* bitmap_set_lowest */
    if (idx < 0) return -1;
    l->active[idx] = 1;
    if ((uint32_t)idx >= l->nr_lights) l->nr_lights = (uint32_t)idx + 1;
    memset(l->pos[idx], 0, 12); memset(l->color[idx], 0, 12); memset(l->dir[idx], 0, 12);
    l->attenuation[idx][0] = 1; l->attenuation[idx][1] = 0; l->attenuation[idx][2] = 0;
    l->cutoff[idx] = 0;
    l->is_dir[idx] = 1;
    return idx;
}

static float to_radians(float degrees) { return (float)(degrees * M_PI / 180.0); }     /* util.h:77-80 */

/* transform_rotate_vec3 for light_update_from_entity's spot direction (light.c:398-400): v' = q v q^-1 via linmath's
 * quat_mul_vec3 (linmath.h: t = 2 cross(q.xyz, v); v' = v + w t + cross(q.xyz, t)) */
static void quat_mul_vec3(float r[3], const float q[4], const float v[3])
{
    float t[3] = { q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0] };
    for (int i = 0; i < 3; i++) t[i] = t[i] * 2.0f;
    const float u[3] = { q[1] * t[2] - q[2] * t[1], q[2] * t[0] - q[0] * t[2], q[0] * t[1] - q[1] * t[0] };
    for (int i = 0; i < 3; i++) { const float wt = t[i] * q[3]; r[i] = v[i] + wt; r[i] = r[i] + u[i]; }
}

static int find_entity(const struct ld_scene *s, const char *name)       /* mq_find_entity: the first entity so named */
{
    const struct ld_entity *e = s->entities.p;
    for (size_t i = 0; i < s->entities.n; i++) if (e[i].name && !strcmp(e[i].name, name)) return (int)i;
    return -1;
}

static void scene_init(struct ld_scene *s, const char *asset_dir)
{
    memset(s, 0, sizeof(*s));
    s->models.el = sizeof(struct ld_model); s->entities.el = sizeof(struct ld_entity); s->carriers.el = sizeof(struct ld_carrier);
    s->attaches.el = sizeof(struct ld_attach); s->bodies.el = sizeof(struct ld_body); s->chars.el = sizeof(struct ld_char);
    s->asset_dir = asset_dir;
}

static void scene_free(struct ld_scene *s)
{
    for (size_t i = 0; i < s->models.n; i++) model_free((struct ld_model *)s->models.p + i);
    for (size_t i = 0; i < s->entities.n; i++) free(((struct ld_entity *)s->entities.p)[i].name);
    free(s->models.p); free(s->entities.p); free(s->carriers.p); free(s->attaches.p); free(s->bodies.p); free(s->chars.p);
}

/* the asset at `path` and the mesh the engine would instantiate from it; `shown` is how the caller named the file.
 * On failure nothing is left to free. */
static int gltf_load_pick(struct gltf *g, const char *path, const char *shown, int *mesh, struct ld_err *e)
{
    const int rc = gltf_load_file(g, path, e);
    if (rc) return rc;
    *mesh = gltf_pick_mesh(g);
    if (*mesh >= 0) return LD_OK;
    gltf_free(g);
    return fail(e, LD_PARSE, "'%s': no mesh to instantiate", shown);
}

/* ================================================================================== one "model" entry */
static const char *const jt_str[JOINT_TYPE_MAX] = { NULL, "head", "foot_left", "foot_right", "hand_left", "hand_right" };

struct model_keys {                  /* scene.c:1318-1390, with the engine's defaults */
    const char *name, *gltf;
    const struct jnode *phys, *ent, *ch;
    double speed;
    int can_jump, can_dash, fix_origin;
};

static void model_keys_from_json(struct model_keys *k, const struct jnode *node)
{
    *k = (struct model_keys){ .speed = 0.75 };
    for (const struct jnode *p = node->head; p; p = p->next) {
        if (p->tag == J_STRING && !strcmp(p->key, "name")) k->name = p->str;
        else if (p->tag == J_STRING && !strcmp(p->key, "gltf")) k->gltf = p->str;
        else if (p->tag == J_OBJECT && !strcmp(p->key, "physics")) k->phys = p;
        else if (p->tag == J_BOOL && !strcmp(p->key, "can_dash")) k->can_dash = p->b;
        else if (p->tag == J_BOOL && !strcmp(p->key, "can_jump")) k->can_jump = p->b;
        else if (p->tag == J_ARRAY && !strcmp(p->key, "entity")) k->ent = p->head;
        else if (p->tag == J_ARRAY && !strcmp(p->key, "character")) k->ch = p->head;
        else if (p->tag == J_NUMBER && !strcmp(p->key, "speed")) k->speed = p->num;
        else if (p->tag == J_BOOL && !strcmp(p->key, "fix_origin")) k->fix_origin = p->b;
    }
}

struct phys_keys { double mass, bounce, bounce_vel, yoffset, radius, length; int geom_class, type; };

/* the "physics" block; `phys` NULL: the defaults */
static void physics_from_json(struct phys_keys *k, const struct jnode *phys)
{
    *k = (struct phys_keys){ .mass = 1.0, .bounce_vel = INFINITY, .radius = 1.0, .length = 1.0, .geom_class = 0 /* GEOM_SPHERE */, .type = 0 /* PHYS_BODY */ };
    for (const struct jnode *p = phys ? phys->head : NULL; p; p = p->next) {
        if (p->tag == J_NUMBER && !strcmp(p->key, "bounce")) k->bounce = p->num;
        else if (p->tag == J_NUMBER && !strcmp(p->key, "bounce_vel")) k->bounce_vel = p->num;
        else if (p->tag == J_NUMBER && !strcmp(p->key, "mass")) k->mass = p->num;
        else if (p->tag == J_NUMBER && !strcmp(p->key, "yoffset")) k->yoffset = p->num;
        else if (p->tag == J_NUMBER && !strcmp(p->key, "radius")) k->radius = p->num;
        else if (p->tag == J_NUMBER && !strcmp(p->key, "length")) k->length = p->num;
        else if (p->tag == J_STRING && !strcmp(p->key, "geom")) {
            if (!strcmp(p->str, "trimesh")) k->geom_class = 2;           /* physics.h:31-39 geom_class: SPHERE, CAPSULE, TRIMESH */
            else if (!strcmp(p->str, "sphere")) k->geom_class = 0;
            else if (!strcmp(p->str, "capsule")) k->geom_class = 1;
        } else if (p->tag == J_STRING && !strcmp(p->key, "type")) {
            if (!strcmp(p->str, "body")) k->type = 0;
            else if (!strcmp(p->str, "geom")) k->type = 1;
        }
    }
}

/* "armature": semantic joint roles by joint name (scene.c:1476-1492) */
static void armature_from_json(struct ld_model *m, const struct jnode *arm)
{
    if (!arm || arm->tag != J_OBJECT) return;
    for (int i = 1; i < JOINT_TYPE_MAX; i++) {
        const struct jnode *jj = jfind(arm, jt_str[i]);
        if (!jj || jj->tag != J_STRING) continue;
        for (uint32_t j = 0; j < m->nr_joints; j++)
            if (!strcmp(jj->str, m->joint_name[j])) { m->joint_types[i] = (int32_t)j; break; }
    }
}

/* "position": [x, y, z, scale, degrees about y]: the leading numbers count.  Three place the entity; false: fewer than
 * four -- the engine goes on to the next entity there, so this one keeps its slot but gets no light, body or attach record */
static bool entity_position_from_json(struct ld_entity *en, const struct jnode *j)
{
    if (!j || j->tag != J_ARRAY) return false;
    float v[5];
    unsigned n = 0;
    for (const struct jnode *pos = j->head; pos && pos->tag == J_NUMBER && n < 5; pos = pos->next) v[n++] = (float)pos->num;
    if (n >= 3) memcpy(en->pos_scale, v, 12);                            /* entity3d_position */
    if (n >= 4) en->pos_scale[3] = v[3];                                 /* entity3d_scale */
    if (n >= 5) {                                                        /* entity3d_rotate(e, 0, to_radians(deg), 0) */
        const float ang[3] = { 0.0f, to_radians(v[4]), 0.0f };
        clapgpu_quat_from_angles(ang, 0, en->rot);
    }
    return n >= 4;
}

/* the light an entity carries (scene.c:1587-1632): "light_color" takes the slot -- also when the colour itself is
 * malformed -- and a malformed array ends the reading of the light's keys */
static void entity_light_from_json(struct ld_lights *L, struct ld_entity *en, const struct jnode *it, float off[3])
{
    const struct jnode *j;
    if ((j = jfind(it, "light_color")) && j->tag == J_ARRAY) {
        en->light_idx = light_get(L);
        if (en->light_idx < 0 || !jfloats(j, L->color[en->light_idx], 3)) return;
    }
    const int idx = en->light_idx;
    if (idx < 0) return;
    if ((j = jfind(it, "light_offset")) && j->tag == J_ARRAY && !jfloats(j, off, 3)) return;
    if (jfloats(jfind(it, "light_attenuation"), L->attenuation[idx], 3)) L->is_dir[idx] = 0;
    if ((j = jfind(it, "light_cutoff")) && j->tag == J_NUMBER) {
        L->cutoff[idx] = to_radians((float)j->num);
        L->is_dir[idx] = 1;
    }
}

/* one element of "entity" / "character" (scene.c:1494-1700) */
static int entity_from_json(struct ld_scene *s, const struct jnode *it, int32_t model_idx, const struct model_keys *mk, const struct phys_keys *pk)
{
    struct ld_entity *en = vpush(&s->entities);
    if (!en) return LD_NOMEM;
    const struct ld_model *m = (struct ld_model *)s->models.p + model_idx;
    const uint32_t ei = (uint32_t)(s->entities.n - 1);
    /* entity3d_make (model.c:1730-1762) */
    en->rot[3] = 1.0f; en->pos_scale[3] = 1.0f;
    en->parent = -1; en->parent_joint = -1; en->light_idx = -1; en->model = model_idx;
    en->flags = E_ALIVE | E_VISIBLE | (m->nr_joints ? E_HAS_ARMATURE : 0) | (m->n_anims ? E_IS_ANIMATED : 0);
    if (mk->ch) {                                                        /* character: skips culling (scene.c:1508-1515) */
        en->flags |= E_IS_CHARACTER | E_SKIP_CULLING;
        struct ld_char *c = vpush(&s->chars);
        if (!c) return LD_NOMEM;
        c->entity = ei; c->model = (uint32_t)model_idx; c->speed = mk->speed; c->can_jump = (uint8_t)mk->can_jump; c->can_dash = (uint8_t)mk->can_dash;
    }
    const struct jnode *j;
    if ((j = jfind(it, "name")) && j->tag == J_STRING) en->name = strdup(j->str);
    if ((j = jfind(it, "attach")) && j->tag == J_STRING) {
        const int p = find_entity(s, j->str);
        if (p < 0 || (uint32_t)p == ei) return LD_OK;                    /* CRES_RET(mq_find_entity(...), continue) */
        en->parent = p;
    }
    if ((j = jfind(it, "attach_joint")) && j->tag == J_STRING && en->parent >= 0) {
        const struct ld_entity *pe = (struct ld_entity *)s->entities.p + en->parent;
        const struct ld_model *pm = (struct ld_model *)s->models.p + pe->model;
        int jt = -1;
        for (int i = 1; i < JOINT_TYPE_MAX; i++) if (!strcmp(jt_str[i], j->str)) jt = i;
        if (jt < 0 || !pm->nr_joints || pm->joint_types[jt] < 0) return LD_OK;       /* model3d_joint_by_type fails: continue */
        en->parent_joint = pm->joint_types[jt];
    }
    float ang[3];
    if (jfloats(jfind(it, "rotate"), ang, 3)) clapgpu_quat_from_angles(ang, 1, en->rot);
    if (!entity_position_from_json(en, jfind(it, "position"))) return LD_OK;
    struct ld_lights *L = &s->lights;
    float light_off[3] = { 0, 0, 0 };
    entity_light_from_json(L, en, it, light_off);
    if (en->light_idx >= 0) {
        en->flags |= E_LIGHT_SOURCE;
        struct ld_carrier *c = vpush(&s->carriers);
        if (!c) return LD_NOMEM;
        c->entity = ei; c->light = en->light_idx; memcpy(c->off, light_off, 12);
        for (int i = 0; i < 3; i++) L->pos[en->light_idx][i] = en->pos_scale[i] + light_off[i];      /* light_update_from_entity */
        if (L->is_dir[en->light_idx] && L->cutoff[en->light_idx] > 0.0f) {                        /* spotlight: direction */
            const float fwd[3] = { 0, 0, 1 };
            float dir[3];
            quat_mul_vec3(dir, en->rot, fwd);
            for (int i = 0; i < 3; i++) L->dir[en->light_idx][i] = 0.0f - dir[i];                   /* light_set_direction */
        }
    }
    /* entity3d_add_physics (model.c:1799-1808).  phys_body_new (physics.c:953-985) creates a geom for the capsule and
     * trimesh classes only: with "geom": "sphere" (the default) it returns NULL and the entity stays without physics. */
    if (mk->phys && pk->geom_class != 0) {
        struct ld_body *b = vpush(&s->bodies);
        if (!b) return LD_NOMEM;
        b->entity = ei; b->geom_class = pk->geom_class; b->phys_type = pk->type; b->mass = pk->mass; b->radius = pk->radius;
        b->length = pk->length; b->yoffset = pk->yoffset; b->bounce = pk->bounce; b->bounce_vel = pk->bounce_vel;
        en->flags |= E_HAS_PHYSICS | (pk->type == 0 ? E_PHYS_IS_BODY : 0);       /* phys_body_has_body: type == PHYS_BODY */
    }
    if (en->parent >= 0 && en->parent_joint >= 0) {
        struct ld_attach *a = vpush(&s->attaches);
        if (!a) return LD_NOMEM;
        a->entity = ei; a->parent = (uint32_t)en->parent; a->joint = (uint32_t)en->parent_joint;
    }
    return LD_OK;
}

/* model_new_from_json, scene.c:1318-1724 */
static int model_from_json(struct ld_scene *s, const struct jnode *node, struct ld_err *e)
{
    struct model_keys mk;
    struct phys_keys pk;
    if (node->tag != J_OBJECT) return fail(e, LD_PARSE, "scene: model is not an object");
    model_keys_from_json(&mk, node);
    if (!mk.name || !mk.gltf) return fail(e, LD_PARSE, "scene: model without 'name' or 'gltf'");

    char path[4096];
    snprintf(path, sizeof(path), "%s/%s", s->asset_dir, mk.gltf);
    struct gltf g;
    int mesh;
    int rc = gltf_load_pick(&g, path, mk.gltf, &mesh, e);
    if (rc) return rc;
    struct ld_model *m = vpush(&s->models);
    rc = m ? model_from_gltf(m, &g, mesh, mk.fix_origin, e) : LD_NOMEM;
    if (rc) goto out;
    free(m->name);
    m->name = strdup(mk.name);                                           /* model3d_set_name */
    physics_from_json(&pk, mk.phys);
    if (mk.phys && pk.geom_class == 2) {                                 /* a trimesh body: its collision mesh */
        rc = collision_from_gltf(m, &g, mesh, e);
        if (rc) goto out;
    }
    armature_from_json(m, jfind(node, "armature"));
    for (const struct jnode *it = mk.ent ? mk.ent : mk.ch; it && !rc; it = it->next)
        if (it->tag == J_OBJECT) rc = entity_from_json(s, it, (int32_t)(s->models.n - 1), &mk, &pk);
out:
    gltf_free(&g);
    return rc;
}

/* scene_add_light_from_json, scene.c:1726-1813 */
static int light_from_json(struct ld_scene *s, const struct jnode *light, struct ld_err *e)
{
    if (light->tag != J_OBJECT) return fail(e, LD_PARSE, "scene: light is not an object");
    struct ld_lights *L = &s->lights;
    float pos[3], color[3], dir[3];
    const struct jnode *j;
    if ((j = jfind(light, "ambient_color"))) return jfloats(j, L->ambient, 3) ? LD_OK : fail(e, LD_PARSE, "scene: bad ambient_color");
    if ((j = jfind(light, "shadow_tint"))) return jfloats(j, L->shadow_tint, 3) ? LD_OK : fail(e, LD_PARSE, "scene: bad shadow_tint");
    if (!jfloats(jfind(light, "position"), pos, 3) || !jfloats(jfind(light, "color"), color, 3))
        return fail(e, LD_PARSE, "scene: light without position / color");
    const int idx = light_get(L);
    if (idx < 0) return fail(e, LD_INVALID, "scene: more than %d lights", LIGHTS_MAX);
    L->is_dir[idx] = 1;
    memcpy(L->pos[idx], pos, 12); memcpy(L->color[idx], color, 12);
    if (jfloats(jfind(light, "direction"), dir, 3))
        for (int i = 0; i < 3; i++) L->dir[idx][i] = 0.0f - dir[i];                                   /* light_set_direction: 0 - dir */
    if (jfloats(jfind(light, "attenuation"), L->attenuation[idx], 3)) L->is_dir[idx] = 0;
    if ((j = jfind(light, "cutoff")) && j->tag == J_NUMBER) { L->cutoff[idx] = (float)j->num; L->is_dir[idx] = 1; }
    return LD_OK;
}

/* ================================================================================== snapshot output */
static void write_entities(struct ld_out *o, const struct ld_scene *s)
{
    const size_t n = s->entities.n, nm = s->models.n;
    const struct ld_entity *en = s->entities.p;
    const struct ld_model *md = s->models.p;
    float *ps = ld_alloc(n, 16), *rot = ld_alloc(n, 16), *maabb = ld_alloc(nm, 24);
    int32_t *parent = ld_alloc(n, 4), *pj = ld_alloc(n, 4), *model = ld_alloc(n, 4);
    uint32_t *flags = ld_alloc(n, 4), *seqs = ld_alloc(n, 4);
    uint8_t *mskip = ld_alloc(nm, 1);
    if (!ps || !rot || !maabb || !parent || !pj || !model || !flags || !seqs || !mskip) o->rc = LD_NOMEM;
    for (size_t i = 0; !o->rc && i < n; i++) {
        memcpy(ps + 4 * i, en[i].pos_scale, 16); memcpy(rot + 4 * i, en[i].rot, 16);
        parent[i] = en[i].parent; pj[i] = en[i].parent_joint; model[i] = en[i].model;
        flags[i] = en[i].flags | CLAPGPU_E_DIRTY | (en[i].parent >= 0 && en[i].parent_joint >= 0 ? CLAPGPU_E_JOINT_ATTACHED : 0);
    }
    for (size_t k = 0; !o->rc && k < nm; k++) memcpy(maabb + 6 * k, md[k].aabb, 24);
    add_i64(o, "entities", "n", (int64_t)n);
    add(o, "entities", "pos_scale", CLAPGPU_DT_F32, 2, n, 4, ps);
    add(o, "entities", "rot", CLAPGPU_DT_F32, 2, n, 4, rot);
    add(o, "entities", "parent", CLAPGPU_DT_I32, 1, n, 0, parent);
    add(o, "entities", "parent_joint", CLAPGPU_DT_I32, 1, n, 0, pj);
    add(o, "entities", "model", CLAPGPU_DT_I32, 1, n, 0, model);
    add(o, "entities", "flags", CLAPGPU_DT_U32, 1, n, 0, flags);
    add(o, "entities", "seqs", CLAPGPU_DT_U32, 1, n, 0, seqs);
    add(o, "entities", "model_aabb", CLAPGPU_DT_F32, 2, nm, 6, maabb);
    add(o, "entities", "model_skip", CLAPGPU_DT_U8, 1, nm, 0, mskip);
    add_i64(o, "scene", "n_models", (int64_t)nm);
    free(ps); free(rot); free(maabb); free(parent); free(pj); free(model); free(flags); free(seqs); free(mskip);
}

/* collision meshes of the trimesh bodies' models: model k's are vx[vx_first[k] ..), idx[tri_first[k] ..) */
static void write_collision(struct ld_out *o, const struct ld_model *md, size_t nm)
{
    uint32_t *vf = calloc(nm + 1, 4), *tf = calloc(nm + 1, 4);
    if (!vf || !tf) o->rc = o->rc ? o->rc : LD_NOMEM;
    for (size_t k = 0; vf && tf && k < nm; k++) {
        vf[k + 1] = vf[k] + (md[k].has_collision ? md[k].n_verts : 0);
        tf[k + 1] = tf[k] + (md[k].has_collision ? md[k].n_ctri : 0);
    }
    float *cv = vf ? ld_alloc(vf[nm], 12) : NULL;
    uint32_t *ci = tf ? ld_alloc(tf[nm], 12) : NULL;                 /* u16 values: the snapshot has no u16 */
    if (!cv || !ci) o->rc = o->rc ? o->rc : LD_NOMEM;
    else
        for (size_t k = 0; k < nm; k++) {
            if (!md[k].has_collision) continue;
            memcpy(cv + 3 * (size_t)vf[k], md[k].position, (size_t)md[k].n_verts * 12);
            for (size_t i = 0; i < (size_t)md[k].n_ctri * 3; i++) ci[3 * (size_t)tf[k] + i] = md[k].cidx[i];
        }
    add(o, "collision", "vx_first", CLAPGPU_DT_U32, 1, nm + 1, 0, vf);
    add(o, "collision", "tri_first", CLAPGPU_DT_U32, 1, nm + 1, 0, tf);
    if (cv && ci) {
        add(o, "collision", "vx", CLAPGPU_DT_F32, 2, vf[nm], 3, cv);
        add(o, "collision", "idx", CLAPGPU_DT_U32, 2, tf[nm], 3, ci);
    }
    free(vf); free(tf); free(cv); free(ci);
}

static void write_lights(struct ld_out *o, const struct ld_lights *L)
{
    add_i64(o, "lights", "nr_lights", L->nr_lights);
    add(o, "lights", "pos", CLAPGPU_DT_F32, 2, LIGHTS_MAX, 3, L->pos);
    add(o, "lights", "color", CLAPGPU_DT_F32, 2, LIGHTS_MAX, 3, L->color);
    add(o, "lights", "attenuation", CLAPGPU_DT_F32, 2, LIGHTS_MAX, 3, L->attenuation);
    add(o, "lights", "dir", CLAPGPU_DT_F32, 2, LIGHTS_MAX, 3, L->dir);
    add(o, "lights", "cutoff", CLAPGPU_DT_F32, 1, LIGHTS_MAX, 0, L->cutoff);
    add(o, "lights", "is_dir", CLAPGPU_DT_I32, 1, LIGHTS_MAX, 0, L->is_dir);
    add(o, "lights", "active", CLAPGPU_DT_U32, 1, LIGHTS_MAX, 0, L->active);
    add(o, "lights", "ambient", CLAPGPU_DT_F32, 1, 3, 0, L->ambient);
    add(o, "lights", "shadow_tint", CLAPGPU_DT_F32, 1, 3, 0, L->shadow_tint);
}

/* the side tables, one array per field */
static void write_records(struct ld_out *o, const struct ld_scene *s)
{
#define COL(vec, type, field, ctype, dt, comp, key) do { \
        const size_t cn = (vec).n; ctype *col = ld_alloc(cn, sizeof(ctype)); \
        if (!col) o->rc = o->rc ? o->rc : LD_NOMEM; \
        else { for (size_t q = 0; q < cn; q++) col[q] = (ctype)((const type *)(vec).p)[q].field; \
               add(o, comp, key, dt, 1, cn, 0, col); free(col); } } while (0)
    COL(s->carriers, struct ld_carrier, entity, uint32_t, CLAPGPU_DT_U32, "carriers", "entity");
    COL(s->carriers, struct ld_carrier, light, int32_t, CLAPGPU_DT_I32, "carriers", "light");
    {
        const size_t cn = s->carriers.n;
        float *off = ld_alloc(cn, 12);
        if (!off) o->rc = o->rc ? o->rc : LD_NOMEM;
        else { for (size_t q = 0; q < cn; q++) memcpy(off + 3 * q, ((const struct ld_carrier *)s->carriers.p)[q].off, 12);
               add(o, "carriers", "offset", CLAPGPU_DT_F32, 2, cn, 3, off); free(off); }
    }
    COL(s->attaches, struct ld_attach, entity, uint32_t, CLAPGPU_DT_U32, "attach", "entity");
    COL(s->attaches, struct ld_attach, parent, uint32_t, CLAPGPU_DT_U32, "attach", "parent");
    COL(s->attaches, struct ld_attach, joint, uint32_t, CLAPGPU_DT_U32, "attach", "joint");
    COL(s->bodies, struct ld_body, entity, uint32_t, CLAPGPU_DT_U32, "bodies", "entity");
    COL(s->bodies, struct ld_body, geom_class, int32_t, CLAPGPU_DT_I32, "bodies", "geom_class");
    COL(s->bodies, struct ld_body, phys_type, int32_t, CLAPGPU_DT_I32, "bodies", "phys_type");
    COL(s->bodies, struct ld_body, mass, double, CLAPGPU_DT_F64, "bodies", "mass");
    COL(s->bodies, struct ld_body, radius, double, CLAPGPU_DT_F64, "bodies", "radius");
    COL(s->bodies, struct ld_body, length, double, CLAPGPU_DT_F64, "bodies", "length");
    COL(s->bodies, struct ld_body, yoffset, double, CLAPGPU_DT_F64, "bodies", "yoffset");
    COL(s->bodies, struct ld_body, bounce, double, CLAPGPU_DT_F64, "bodies", "bounce");
    COL(s->bodies, struct ld_body, bounce_vel, double, CLAPGPU_DT_F64, "bodies", "bounce_vel");
    COL(s->chars, struct ld_char, entity, uint32_t, CLAPGPU_DT_U32, "characters", "entity");
    COL(s->chars, struct ld_char, model, uint32_t, CLAPGPU_DT_U32, "characters", "model");
    COL(s->chars, struct ld_char, speed, double, CLAPGPU_DT_F64, "characters", "speed");
    COL(s->chars, struct ld_char, can_jump, uint8_t, CLAPGPU_DT_U8, "characters", "can_jump");
    COL(s->chars, struct ld_char, can_dash, uint8_t, CLAPGPU_DT_U8, "characters", "can_dash");
#undef COL
}

static int write_scene(const struct ld_scene *s, const char *snapshot_path)
{
    struct ld_out o = { NULL, 0 };
    const int rc = clapgpu_snapshot_create(&o.w, snapshot_path);
    if (rc) return rc;
    const struct ld_model *md = s->models.p;
    write_entities(&o, s);
    write_collision(&o, md, s->models.n);
    for (size_t k = 0; k < s->models.n && !o.rc; k++) write_model(&o, (unsigned)k, &md[k]);
    write_lights(&o, &s->lights);
    write_records(&o, s);
    if (o.rc) { clapgpu_snapshot_abort(o.w); return o.rc; }
    return clapgpu_snapshot_finish(o.w);
}

/* the scene as a snapshot file, then the scene freed: what both entry points end with */
static int scene_finish(struct ld_scene *s, int rc, const char *snapshot_path, struct ld_err *e)
{
    if (!rc) {
        rc = write_scene(s, snapshot_path);
        if (rc) fail(e, rc, "cannot write '%s'", snapshot_path);
    }
    scene_free(s);
    return rc;
}

/* ================================================================================== the entry points */
int clapgpu_load_scene(const char *scene_json, const char *asset_dir, const char *snapshot_path, char *err, size_t err_len)
{
    struct ld_err e = { err, err_len };
    if (err && err_len) err[0] = 0;
    if (!scene_json || !snapshot_path) return fail(&e, LD_INVALID, "missing path");
    uint8_t *buf = NULL;
    size_t size = 0;
    int rc = read_file(scene_json, &buf, &size);
    if (rc) return fail(&e, rc, "cannot read '%s'", scene_json);
    struct jparse jp;
    struct jnode *root = jdecode(&jp, (const char *)buf, size);
    if (!root) { free(buf); return fail(&e, LD_PARSE, "couldn't parse '%s'", scene_json); }
    char dir[4096];
    if (asset_dir) snprintf(dir, sizeof(dir), "%s", asset_dir);
    else {
        snprintf(dir, sizeof(dir), "%s", scene_json);
        char *slash = strrchr(dir, '/');
        if (slash) *slash = 0; else strcpy(dir, ".");
    }
    struct ld_scene s;
    scene_init(&s, dir);
    rc = LD_OK;
    if (root->tag != J_OBJECT) rc = fail(&e, LD_PARSE, "parse error in '%s'", scene_json);
    for (struct jnode *p = rc ? NULL : root->head; p && !rc; p = p->next) {          /* scene_onload, scene.c:1846-1873 */
        if (!strcmp(p->key, "name")) {
            if (p->tag != J_STRING) rc = fail(&e, LD_PARSE, "parse error in '%s': name", scene_json);
        } else if (!strcmp(p->key, "model")) {
            if (p->tag != J_ARRAY) { rc = fail(&e, LD_PARSE, "parse error in '%s': model", scene_json); break; }
            for (struct jnode *m = p->head; m && !rc; m = m->next) rc = model_from_json(&s, m, &e);
        } else if (!strcmp(p->key, "light") && p->tag == J_ARRAY) {
            for (struct jnode *l = p->head; l && !rc; l = l->next) rc = light_from_json(&s, l, &e);
        }
    }
    rc = scene_finish(&s, rc, snapshot_path, &e);
    jfree(&jp);
    free(buf);
    return rc;
}

int clapgpu_load_gltf(const char *gltf_path, int fix_origin, const char *snapshot_path, char *err, size_t err_len)
{
    struct ld_err e = { err, err_len };
    if (err && err_len) err[0] = 0;
    if (!gltf_path || !snapshot_path) return fail(&e, LD_INVALID, "missing path");
    struct gltf g;
    int mesh;
    int rc = gltf_load_pick(&g, gltf_path, gltf_path, &mesh, &e);
    if (rc) return rc;
    struct ld_scene s;
    scene_init(&s, NULL);
    struct ld_model *m = vpush(&s.models);
    rc = m ? model_from_gltf(m, &g, mesh, fix_origin, &e) : LD_NOMEM;
    gltf_free(&g);
    return scene_finish(&s, rc, snapshot_path, &e);
}
