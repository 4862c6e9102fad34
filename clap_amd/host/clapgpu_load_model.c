/*
 * clapgpu_load_model.c -- one mesh of a struct gltf -> struct ld_model, and the model's arrays in the snapshot.
 *
 * gltf_instantiate_one (gltf.c:1158-1331) without the renderer objects, in its order: vertex attributes, then -- for
 * a skinned mesh -- vertex joints / weights, the skeleton, the animations' channels.  The arithmetic that has to match
 * the engine's bits (mat4x4_invert, mat4x4_from_quat) goes through the same helpers as the rest of the library.
 */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "clapgpu.h"
#include "clapgpu_load_internal.h"

static void anim_free(struct ld_anim *an)
{
    free(an->ch_target); free(an->ch_path); free(an->ch_nr); free(an->ch_time_off); free(an->ch_data_off); free(an->times); free(an->data);
}

void model_free(struct ld_model *m)
{
    free(m->name); free(m->joint_parent); free(m->invmx); free(m->bind); free(m->position); free(m->normal);
    free(m->weights); free(m->joints); free(m->cidx);
    for (uint32_t j = 0; m->joint_name && j < m->nr_joints; j++) free(m->joint_name[j]);
    free(m->joint_name);
    for (uint32_t a = 0; a < m->n_anims; a++) {
        anim_free(&m->anims[a]);
        if (m->anim_name) free(m->anim_name[a]);
    }
    free(m->anims); free(m->anim_name);
    memset(m, 0, sizeof(*m));
}

/* vertex_array_aabb_calc (util.c, util.h:133) over tightly packed positions */
static void aabb_calc(float aabb[6], const float *vx, uint32_t n)
{
    aabb[0] = aabb[1] = aabb[2] = INFINITY;
    aabb[3] = aabb[4] = aabb[5] = -INFINITY;
    for (uint32_t i = 0; i < n; i++)
        for (int j = 0; j < 3; j++) {
            const float v = vx[3 * (size_t)i + j];
            aabb[j] = v < aabb[j] ? v : aabb[j];                        /* min(v, aabb) / max(v, aabb) as util.h's macros evaluate */
            aabb[3 + j] = v > aabb[3 + j] ? v : aabb[3 + j];
        }
}

/* a copy of `count` tightly packed elements of `elsz` bytes */
static void *dup_elems(const void *src, unsigned count, size_t elsz)
{
    void *p = ld_alloc(count, elsz);
    if (p) memcpy(p, src, (size_t)count * elsz);
    return p;
}

/* POSITION, fix_origin, the AABB, NORMAL (gltf.c:1158-1230) */
static int geometry_from_gltf(struct ld_model *m, const struct gltf *g, const struct g_mesh *gm, int fix_origin, struct ld_err *e)
{
    size_t es; unsigned cnt;
    const float *vx = accr_buf(g, gm->POSITION, &es, &cnt);
    if (!vx || es != 12) return fail(e, LD_PARSE, "mesh '%s': POSITION is not a readable float VEC3 accessor", gm->name);
    m->n_verts = cnt;
    m->position = dup_elems(vx, cnt, 12);
    if (!m->position) return LD_NOMEM;
    aabb_calc(m->aabb, m->position, cnt);                               /* mesh_attr_dup(MESH_VX), mesh.c:128 */
    if (fix_origin) {                                                   /* vertex_array_fix_origin, util.c:77-92 */
        const float c[3] = { (m->aabb[0] + m->aabb[3]) / 2.0f, m->aabb[1], (m->aabb[2] + m->aabb[5]) / 2.0f };
        for (uint32_t i = 0; i < cnt; i++) for (int j = 0; j < 3; j++) m->position[3 * (size_t)i + j] -= c[j];
        aabb_calc(m->aabb, m->position, cnt);
    }
    if (gm->NORMAL >= 0) {
        const float *nx = accr_buf(g, gm->NORMAL, &es, &cnt);
        if (!nx || es != 12 || cnt != m->n_verts) return fail(e, LD_PARSE, "mesh '%s': NORMAL does not match POSITION", gm->name);
        m->normal = dup_elems(nx, cnt, 12);
        if (!m->normal) return LD_NOMEM;
    }
    return LD_OK;
}

/* vertex joints / weights: mesh_attr_dup widens u8x4 joints to ints (mesh.c:112-121); u8 is kept here, u16 narrowed */
static int vertex_skin_from_gltf(struct ld_model *m, const struct gltf *g, const struct g_mesh *gm, const struct g_skin *s, struct ld_err *e)
{
    size_t es; unsigned cnt;
    const struct g_accessor *ja = &g->accrs[gm->JOINTS_0];
    const void *jb = accr_buf(g, gm->JOINTS_0, &es, &cnt);
    if (!jb || ja->comps != 4 || cnt != m->n_verts || (ja->comptype != GL_U8 && ja->comptype != GL_U16))
        return fail(e, LD_PARSE, "mesh '%s': JOINTS_0 is not u8 / u16 VEC4 matching POSITION", gm->name);
    m->joints = ld_alloc(cnt, 4);
    if (!m->joints) return LD_NOMEM;
    for (size_t i = 0; i < (size_t)cnt * 4; i++) {
        const unsigned v = accr_uint(jb, ja->comptype, i);
        if (v >= s->nr_joints || v > 255) return fail(e, LD_PARSE, "mesh '%s': vertex joint %u outside the skin's %u joints", gm->name, v, s->nr_joints);
        m->joints[i] = (uint8_t)v;
    }
    const float *wb = accr_buf(g, gm->WEIGHTS_0, &es, &cnt);
    if (!wb || es != 16 || cnt != m->n_verts) return fail(e, LD_PARSE, "mesh '%s': WEIGHTS_0 is not float VEC4 matching POSITION", gm->name);
    m->weights = dup_elems(wb, cnt, 16);
    return m->weights ? LD_OK : LD_NOMEM;
}

/* model3d_add_skinning (model.c:524-537), the root pose, joint names and parent links */
static int skeleton_from_gltf(struct ld_model *m, const struct gltf *g, const struct g_skin *s)
{
    const uint32_t J = m->nr_joints = s->nr_joints;
    m->invmx = malloc((size_t)J * 64); m->bind = malloc((size_t)J * 64);
    m->joint_parent = malloc(sizeof(int32_t) * J); m->joint_name = calloc(J, sizeof(char *));
    if (!m->invmx || !m->bind || !m->joint_parent || !m->joint_name) return LD_NOMEM;
    for (int i = 0; i < JOINT_TYPE_MAX; i++) m->joint_types[i] = -1;
    memcpy(m->invmx, s->invmxs, (size_t)J * 64);
    for (uint32_t j = 0; j < J; j++) clapgpu_mat4_invert(m->invmx + 16 * (size_t)j, m->bind + 16 * (size_t)j);
    /* root pose: the node named like the skin (gltf.c:1243-1258) */
    static const float ident[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    memcpy(m->root_pose, ident, sizeof(ident));
    for (unsigned i = 0; i < g->n_nodes && s->name; i++) {
        const struct g_node *nd = &g->nodes[i];
        if (strcmp(nd->name, s->name)) continue;
        const float *r = nd->rotation;
        if (sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]) != 0.0f) {     /* vec4_len(): truthiness only */
            clapgpu_mat4_from_quat(r, m->root_pose);
            m->root_pose[12] = nd->translation[0]; m->root_pose[13] = nd->translation[1];
            m->root_pose[14] = nd->translation[2]; m->root_pose[15] = 1.0f;
        }
        break;
    }
    /* joints: names and children (gltf.c:1263-1274) -> parent links.  gltf_skin_node_to_joint (gltf.c:1150-1156):
     * a node numbered >= nr_joints is no joint (-1: the engine stores that child and never follows it to a real joint) */
    for (uint32_t j = 0; j < J; j++) m->joint_parent[j] = -1;
    for (uint32_t j = 0; j < J; j++) {
        const struct g_node *nd = &g->nodes[s->joints[j]];
        m->joint_name[j] = strdup(nd->name);
        for (unsigned c = 0; c < nd->nr_children; c++) {
            const int cn = nd->ch_arr[c];
            if (cn < 0 || (unsigned)cn >= J) continue;
            const int cj = s->nodes[cn];
            if (cj > 0 && (uint32_t)cj != j) m->joint_parent[cj] = (int32_t)j;     /* joint 0 is where the walk starts (model.c:1583): it has no parent */
        }
    }
    return LD_OK;
}

/* room for `need` floats in all: at least twice that when the array has to grow */
static int grow_floats(float **arr, size_t *cap, size_t need)
{
    if (need <= *cap) return LD_OK;
    float *t = realloc(*arr, 4 * need * 2);
    if (!t) return LD_NOMEM;
    *arr = t; *cap = need * 2;
    return LD_OK;
}

/* one animation's channels on joints of skin `s` (animation_add_channel, model.c:725-742); channels on other nodes
 * are skipped ("references a non-existent joint") */
static int anim_from_gltf(struct ld_anim *an, const struct gltf *g, const struct g_anim *ga, const struct g_skin *s, struct ld_err *e)
{
    const uint32_t J = s->nr_joints;
    an->ch_target = ld_alloc(ga->n_channels, 4); an->ch_path = ld_alloc(ga->n_channels, 4); an->ch_nr = ld_alloc(ga->n_channels, 4);
    an->ch_time_off = ld_alloc(ga->n_channels, 4); an->ch_data_off = ld_alloc(ga->n_channels, 4);
    if (!an->ch_target || !an->ch_path || !an->ch_nr || !an->ch_time_off || !an->ch_data_off) return LD_NOMEM;
    size_t t_cap = 0, d_cap = 0;
    for (unsigned c = 0; c < ga->n_channels; c++) {
        const struct g_channel *ch = &ga->channels[c];
        if (ch->sampler < 0 || (unsigned)ch->sampler >= ga->n_samplers) return fail(e, LD_PARSE, "animation '%s': channel %u has no sampler", ga->name ? ga->name : "", c);
        const struct g_sampler *sm = &ga->samplers[ch->sampler];
        size_t tes, des; unsigned frames, dcnt;
        const float *time = accr_buf(g, sm->input, &tes, &frames);
        const float *data = accr_buf(g, sm->output, &des, &dcnt);
        if (!time || tes != 4 || !data || !frames || dcnt < frames || des % 4)
            return fail(e, LD_PARSE, "animation '%s': channel %u has unreadable key times / values", ga->name ? ga->name : "", c);
        const int joint = ch->node >= 0 && (unsigned)ch->node < J ? s->nodes[ch->node] : -1;      /* gltf_skin_node_to_joint */
        if (joint < 0) continue;
        const uint32_t dfl = (uint32_t)(des / 4);                       /* floats per key: 3 (T, S) or 4 (R) */
        if (grow_floats(&an->times, &t_cap, an->n_times + frames) || grow_floats(&an->data, &d_cap, an->n_data + (size_t)frames * dfl)) return LD_NOMEM;
        const uint32_t k = an->n_channels++;
        an->ch_target[k] = (uint32_t)joint; an->ch_path[k] = (uint32_t)ch->path; an->ch_nr[k] = frames;
        an->ch_time_off[k] = an->n_times; an->ch_data_off[k] = an->n_data;
        memcpy(an->times + an->n_times, time, 4 * (size_t)frames);
        memcpy(an->data + an->n_data, data, 4 * (size_t)frames * dfl);
        an->n_times += frames; an->n_data += frames * dfl;
        float last;
        memcpy(&last, (const uint8_t *)time + 4 * (size_t)(frames - 1), 4);
        an->time_end = an->time_end > last ? an->time_end : last;        /* max(an->time_end, time[frames - 1]) */
    }
    return LD_OK;
}

/* animations -> channels (gltf.c:1276-1320) */
static int anims_from_gltf(struct ld_model *m, const struct gltf *g, const struct g_skin *s, struct ld_err *e)
{
    m->anims = ld_alloc(g->n_anis, sizeof(*m->anims));
    m->anim_name = ld_alloc(g->n_anis, sizeof(char *));
    if (!m->anims || !m->anim_name) return LD_NOMEM;
    for (unsigned a = 0; a < g->n_anis; a++) {
        const struct g_anim *ga = &g->anis[a];
        struct ld_anim an;
        memset(&an, 0, sizeof(an));
        const int rc = anim_from_gltf(&an, g, ga, s, e);
        if (rc || !an.n_channels) {                                     /* "an animation with no channels has no reason to exist" */
            anim_free(&an);
            if (rc) return rc;
            continue;
        }
        m->anim_name[m->n_anims] = ga->name ? strdup(ga->name) : NULL;
        m->anims[m->n_anims++] = an;
    }
    return LD_OK;
}

int model_from_gltf(struct ld_model *m, const struct gltf *g, int mesh, int fix_origin, struct ld_err *e)
{
    memset(m, 0, sizeof(*m));
    const struct g_mesh *gm = &g->meshes[mesh];
    m->name = strdup(gm->name);
    int rc = geometry_from_gltf(m, g, gm, fix_origin, e);
    if (rc) return rc;
    const int skin = gltf_mesh_skin(g, mesh);
    if (skin < 0 || (unsigned)skin >= g->n_skins) return LD_OK;
    const struct g_skin *s = &g->skins[skin];
    if (!s->nr_joints || !s->invmxs || s->nr_invmxs < s->nr_joints)
        return fail(e, LD_PARSE, "mesh '%s': skin without joints or with fewer inverse bind matrices than joints", gm->name);
    rc = vertex_skin_from_gltf(m, g, gm, s, e);
    if (!rc) rc = skeleton_from_gltf(m, g, s);
    if (!rc) rc = anims_from_gltf(m, g, s, e);
    return rc;
}

/* model3d_make keeps the instantiated mesh's vertices (after fix_origin) and u16 indices as the collision mesh
 * (model.c:99-102); phys_geom_trimesh_new reads them (physics.c:882-930).  Indices of another width are narrowed when
 * they fit in u16; a trailing partial triple is dropped (ODE takes whole triangles). */
int collision_from_gltf(struct ld_model *m, const struct gltf *g, int mesh, struct ld_err *e)
{
    const struct g_mesh *gm = &g->meshes[mesh];
    const int ia = gm->indices;
    size_t es; unsigned cnt;
    const uint8_t *ib = accr_buf(g, ia, &es, &cnt);
    if (!ib || g->accrs[ia].comps != 1) return fail(e, LD_PARSE, "mesh '%s': indices are not a readable scalar accessor", gm->name);
    const unsigned ct = g->accrs[ia].comptype;
    if (ct != GL_U8 && ct != GL_U16 && ct != GL_U32) return fail(e, LD_PARSE, "mesh '%s': indices are not u8 / u16 / u32", gm->name);
    m->n_ctri = cnt / 3;
    m->cidx = ld_alloc(m->n_ctri, 6);
    if (!m->cidx) return LD_NOMEM;
    for (size_t i = 0; i < (size_t)m->n_ctri * 3; i++) {
        const uint32_t v = accr_uint(ib, ct, i);
        if (v >= m->n_verts || v > 0xffffu) return fail(e, LD_PARSE, "mesh '%s': index %u outside the mesh's %u vertices", gm->name, v, m->n_verts);
        m->cidx[i] = (uint16_t)v;
    }
    m->has_collision = 1;
    return LD_OK;
}

/* ================================================================================== snapshot output */
void add(struct ld_out *o, const char *comp, const char *key, uint32_t dt, uint32_t nd, uint64_t d0, uint64_t d1, const void *p)
{
    char name[CLAPGPU_SNAPSHOT_NAME_MAX];
    const uint64_t dims[2] = { d0, d1 };
    static const uint64_t zero8[2];
    if (o->rc) return;
    if ((size_t)snprintf(name, sizeof(name), "%s.%s", comp, key) >= sizeof(name)) o->rc = LD_INVALID;
    else o->rc = clapgpu_snapshot_add(o->w, name, dt, nd, dims, p ? p : zero8);
}

void add_i64(struct ld_out *o, const char *comp, const char *key, int64_t v)
{
    add(o, comp, key, CLAPGPU_DT_I64, 1, 1, 0, &v);
}

/* model.vert:36-38 never renormalises: total_local_pos.w = sum of the weights.  How far this mesh is from 1
 * decides whether a pre-skinned draw may feed vec4(p, 1) (clapgpu_skin_batch.out_w, clapgpu.h) */
static float weight_sum_max_dev(const struct ld_model *m)
{
    float dev = 0.f;
    for (uint32_t v = 0; v < m->n_verts; v++) {
        const float *q = m->weights + 4 * (size_t)v;
        float sum = 0.f;
        for (int i = 0; i < 4; i++) sum += q[i];                  /* the shader's accumulation order */
        const float d = fabsf(sum - 1.f);
        if (!(d <= dev)) dev = d;                                 /* NaN weights surface as NaN */
    }
    return dev;
}

/* animation `a`'s arrays; returns its count of keys with t[i] <= t[i-1].  channel_time_to_idx scans from the cursor
 * joint->off[path] (model.c:1266-1288, 1310): with key times that do not strictly increase the bracket it finds depends
 * on that cursor's history, which the stateless device search (pose.hip) does not have.  Such channels are flagged. */
static uint64_t write_anim(struct ld_out *o, const char *comp, uint32_t a, const struct ld_anim *an)
{
    char key[40];
#define AK(suffix, dt, n, p) do { snprintf(key, sizeof(key), "a%u_%s", a, suffix); add(o, comp, key, dt, 1, n, 0, p); } while (0)
    AK("ch_target", CLAPGPU_DT_U32, an->n_channels, an->ch_target);
    AK("ch_path", CLAPGPU_DT_U32, an->n_channels, an->ch_path);
    AK("ch_nr", CLAPGPU_DT_U32, an->n_channels, an->ch_nr);
    AK("ch_time_off", CLAPGPU_DT_U32, an->n_channels, an->ch_time_off);
    AK("ch_data_off", CLAPGPU_DT_U32, an->n_channels, an->ch_data_off);
    AK("times", CLAPGPU_DT_F32, an->n_times, an->times);
    AK("data", CLAPGPU_DT_F32, an->n_data, an->data);
    AK("time_end", CLAPGPU_DT_F32, 1, &an->time_end);
    uint32_t *ns = ld_alloc(an->n_channels, sizeof(*ns)), total = 0;
    if (!ns) { o->rc = LD_NOMEM; return 0; }
    for (uint32_t c = 0; c < an->n_channels; c++) {
        const float *t = an->times + an->ch_time_off[c];
        for (uint32_t i = 1; i < an->ch_nr[c]; i++)
            ns[c] += !(t[i] > t[i - 1]);
        total += ns[c];
    }
    AK("ch_nonstrict", CLAPGPU_DT_U32, an->n_channels, ns);
#undef AK
    free(ns);
    return total;
}

void write_model(struct ld_out *o, unsigned k, const struct ld_model *m)
{
    char comp[24];
    snprintf(comp, sizeof(comp), "model%u", k);
    const uint32_t J = m->nr_joints, V = m->n_verts;
    add_i64(o, comp, "nr_joints", J);
    add_i64(o, comp, "n_verts", V);
    add(o, comp, "aabb", CLAPGPU_DT_F32, 1, 6, 0, m->aabb);
    add(o, comp, "position", CLAPGPU_DT_F32, 2, V, 3, m->position);
    if (m->normal) add(o, comp, "normal", CLAPGPU_DT_F32, 2, V, 3, m->normal);
    if (!J) return;
    const float dev = weight_sum_max_dev(m);
    add(o, comp, "joints", CLAPGPU_DT_U8, 2, V, 4, m->joints);
    add(o, comp, "weights", CLAPGPU_DT_F32, 2, V, 4, m->weights);
    add(o, comp, "weight_sum_max_dev", CLAPGPU_DT_F32, 1, 1, 0, &dev);
    add(o, comp, "joint_parent", CLAPGPU_DT_I32, 1, J, 0, m->joint_parent);
    add(o, comp, "invmx", CLAPGPU_DT_F32, 2, J, 16, m->invmx);
    add(o, comp, "bind", CLAPGPU_DT_F32, 2, J, 16, m->bind);
    add(o, comp, "root_pose", CLAPGPU_DT_F32, 1, 16, 0, m->root_pose);
    add(o, comp, "joint_types", CLAPGPU_DT_I32, 1, JOINT_TYPE_MAX, 0, m->joint_types);
    add_i64(o, comp, "n_anims", m->n_anims);
    uint64_t nonstrict_total = 0;
    for (uint32_t a = 0; a < m->n_anims && !o->rc; a++) nonstrict_total += write_anim(o, comp, a, &m->anims[a]);
    add_i64(o, comp, "key_times_nonstrict", (int64_t)nonstrict_total);
}
