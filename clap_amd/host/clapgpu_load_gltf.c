/*
 * clapgpu_load_gltf.c -- a .gltf / .glb file -> struct gltf, and which of its meshes the engine instantiates.
 *
 * One function per section of the engine's gltf_json_parse (gltf.c:666-1064), called in its order: later sections
 * read what earlier ones numbered (bufferViews count buffers, accessors count bufferViews, skins read accessors).
 */
#include <ctype.h>
#include <stdio.h>
#include <string.h>
#include <strings.h>

#include "clapgpu_load_internal.h"

/* ================================================================================== files, base64 */
int read_file(const char *path, uint8_t **out, size_t *size)
{
    FILE *f = fopen(path, "rb");
    if (!f) return LD_NOT_FOUND;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *b = n >= 0 ? malloc((size_t)n + 1) : NULL;
    if (!b) { fclose(f); return LD_NOMEM; }
    if (fread(b, 1, (size_t)n, f) != (size_t)n) { fclose(f); free(b); return LD_PARSE; }
    fclose(f);
    b[n] = 0;
    *out = b; *size = (size_t)n;
    return LD_OK;
}

static long b64_decode(uint8_t *dst, size_t cap, const char *src, size_t slen)
{
    unsigned acc = 0, bits = 0;
    size_t n = 0;
    for (size_t i = 0; i < slen; i++) {
        const int c = (unsigned char)src[i];
        int v;
        if (c >= 'A' && c <= 'Z') v = c - 'A';
        else if (c >= 'a' && c <= 'z') v = c - 'a' + 26;
        else if (c >= '0' && c <= '9') v = c - '0' + 52;
        else if (c == '+' || c == '-') v = 62;
        else if (c == '/' || c == '_') v = 63;
        else if (c == '=') break;
        else if (isspace(c)) continue;
        else return -1;
        acc = acc << 6 | (unsigned)v;
        bits += 6;
        if (bits >= 8) {
            bits -= 8;
            if (n >= cap) return -1;
            dst[n++] = (uint8_t)(acc >> bits);
        }
    }
    return (long)n;
}

/* ================================================================================== accessors */
#define DATA_URI "data:application/octet-stream;base64,"                 /* gltf.c:13 */

void gltf_free(struct gltf *g)
{
    for (unsigned i = 0; i < g->n_buffers; i++) free(g->buffers[i]);
    free(g->buffers); free(g->buffer_size); free(g->bufvws); free(g->accrs);
    for (unsigned i = 0; i < g->n_nodes; i++) { free(g->nodes[i].name); free(g->nodes[i].ch_arr); }
    free(g->nodes);
    for (unsigned i = 0; i < g->n_skins; i++) { free(g->skins[i].name); free(g->skins[i].joints); free(g->skins[i].nodes); }
    free(g->skins);
    for (unsigned i = 0; i < g->n_meshes; i++) free(g->meshes[i].name);
    free(g->meshes);
    for (unsigned i = 0; i < g->n_anis; i++) { free(g->anis[i].name); free(g->anis[i].samplers); free(g->anis[i].channels); }
    free(g->anis);
    free(g->file);
    memset(g, 0, sizeof(*g));
}

static size_t comp_size(unsigned t)                                      /* gltf_type_size, gltf.c:21-50 */
{
    switch (t) {
    case 0x1400: case 0x1401: return 1;
    case 0x1402: case 0x1403: return 2;
    case 0x1404: case 0x1405: case 0x1406: return 4;
    case 0x140a: return 8;
    default: return 0;
    }
}

static unsigned comps_of(const char *type)                               /* data_type_by_name + data_comp_count */
{
    if (!strcasecmp(type, "SCALAR")) return 1;
    if (!strcasecmp(type, "VEC2")) return 2;
    if (!strcasecmp(type, "VEC3")) return 3;
    if (!strcasecmp(type, "VEC4")) return 4;
    if (!strcasecmp(type, "MAT4")) return 16;
    if (!strcasecmp(type, "MAT3")) return 9;
    if (!strcasecmp(type, "MAT2")) return 4;
    return 0;
}

/* gltf_accessor_buf (gltf.c:313-323) with the bounds the engine does not check */
const void *accr_buf(const struct gltf *g, int accr, size_t *elsz, unsigned *count)
{
    if (accr < 0 || (unsigned)accr >= g->n_accrs) return NULL;
    const struct g_accessor *a = &g->accrs[accr];
    if (a->bufview >= g->n_bufvws) return NULL;
    const struct g_bufview *bv = &g->bufvws[a->bufview];
    if (bv->buffer >= g->n_buffers || !g->buffers[bv->buffer]) return NULL;
    const size_t es = a->comps * comp_size(a->comptype);                /* gltf_accessor_stride: tightly packed */
    const size_t size = g->buffer_size[bv->buffer];
    /* overflow-safe: every term is checked against what is left of the buffer before it is added */
    if (!es || bv->offset > size || a->offset > size - bv->offset) return NULL;
    const size_t room = size - bv->offset - a->offset;
    if (a->count > room / es) return NULL;
    if (elsz) *elsz = es;
    if (count) *count = a->count;
    return g->buffers[bv->buffer] + a->offset + bv->offset;
}

/* element `i` of tightly packed u8 / u16 / u32 values; accessor offsets need not be aligned */
uint32_t accr_uint(const void *base, unsigned comptype, size_t i)
{
    const uint8_t *b = base;
    if (comptype == GL_U8) return b[i];
    if (comptype == GL_U16) { uint16_t h; memcpy(&h, b + 2 * i, 2); return h; }
    uint32_t v;
    memcpy(&v, b + 4 * i, 4);
    return v;
}

/* ================================================================================== the document, section by section */
/* nodes (gltf.c:728-760).  The engine skips nameless nodes and then indexes its array with glTF node numbers:
 * files it reads correctly name every node.  A nameless node is an error here instead of a silent shift. */
static int parse_nodes(struct gltf *g, const struct jnode *nodes, struct ld_err *e)
{
    g->nodes = ld_alloc(nodes->count, sizeof(*g->nodes));
    if (!g->nodes) return LD_NOMEM;
    unsigned nid = 0;
    for (struct jnode *n = nodes->head; n; n = n->next, nid++) {
        struct jnode *jname = jfind(n, "name");
        if (n->tag != J_OBJECT || !jname || jname->tag != J_STRING) return fail(e, LD_PARSE, "glTF: node %u has no name (the engine's node table would shift)", nid);
        struct g_node *nd = &g->nodes[g->n_nodes++];
        nd->name = strdup(jname->str);
        nd->id = nid;
        nd->mesh = jnum_i(jfind(n, "mesh"), 0);                         /* absent: the zeroed darray slot, i.e. 0 */
        nd->skin = jnum_i(jfind(n, "skin"), 0);
        jfloats(jfind(n, "rotation"), nd->rotation, 4);
        jfloats(jfind(n, "translation"), nd->translation, 3);
        jfloats(jfind(n, "scale"), nd->scale, 3);
        struct jnode *j = jfind(n, "children");
        if (j && j->tag == J_ARRAY) nd->ch_arr = jints_alloc(j, &nd->nr_children);
    }
    return LD_OK;
}

/* scenes (gltf.c:764-795): the first listed node that is not "Light" / "Camera" is the root; later scenes override */
static void parse_scenes(struct gltf *g, const struct jnode *scenes)
{
    g->root_node = -1;
    for (struct jnode *n = scenes->head; n; n = n->next) {
        struct jnode *jname = jfind(n, "name"), *jnodes = jfind(n, "nodes");
        if (n->tag != J_OBJECT || !jname || jname->tag != J_STRING || !jnodes || jnodes->tag != J_ARRAY) continue;
        unsigned cnt = 0;
        int *ids = jints_alloc(jnodes, &cnt);
        for (unsigned i = 0; ids && i < cnt; i++) {
            if (ids[i] < 0 || (unsigned)ids[i] >= g->n_nodes) continue;
            const struct g_node *nd = &g->nodes[ids[i]];
            if (!strcmp(nd->name, "Light") || !strcmp(nd->name, "Camera")) continue;
            g->root_node = ids[i];
            break;
        }
        free(ids);
    }
}

/* buffers (gltf.c:798-846).  Skipped entries take no number. */
static int parse_buffers(struct gltf *g, const struct jnode *bufs, struct ld_err *e)
{
    g->buffers = ld_alloc(bufs->count, sizeof(*g->buffers));
    g->buffer_size = ld_alloc(bufs->count, sizeof(*g->buffer_size));
    if (!g->buffers || !g->buffer_size) return LD_NOMEM;
    for (struct jnode *n = bufs->head; n; n = n->next) {
        struct jnode *jlen = jfind(n, "byteLength"), *juri = jfind(n, "uri");
        if (n->tag != J_OBJECT || !jlen) continue;
        if (!g->n_buffers && g->bin && juri) continue;                  /* the GLB bin buffer has no uri; the others must */
        if ((g->n_buffers || !g->bin) && !juri) continue;
        size_t blen = (size_t)jlen->num;
        uint8_t *b;
        if (juri) {
            const size_t pre = sizeof(DATA_URI) - 1;
            if (juri->tag != J_STRING || strlen(juri->str) < pre || strncmp(juri->str, DATA_URI, pre)) continue;
            const size_t slen = strlen(juri->str) - pre, cap = slen / 4 * 3 + 3;
            if (cap > blen) blen = cap;
            b = ld_alloc(blen, 1);
            if (!b) return LD_NOMEM;
            if (b64_decode(b, blen, juri->str + pre, slen) < 0) { free(b); b = NULL; }   /* a hole keeps the buffer numbering */
        } else {
            if (blen > g->bin_size) return fail(e, LD_PARSE, "glTF: GLB buffer of %zu bytes in a %zu-byte BIN chunk", blen, g->bin_size);
            b = ld_alloc(blen, 1);
            if (!b) return LD_NOMEM;
            memcpy(b, g->bin, blen);
        }
        g->buffers[g->n_buffers] = b;
        g->buffer_size[g->n_buffers++] = blen;
    }
    return LD_OK;
}

/* bufferViews (gltf.c:849-866): all three members are required by the engine, byteOffset included */
static int parse_bufviews(struct gltf *g, const struct jnode *bufvws)
{
    g->bufvws = ld_alloc(bufvws->count, sizeof(*g->bufvws));
    if (!g->bufvws) return LD_NOMEM;
    for (struct jnode *n = bufvws->head; n; n = n->next) {
        struct jnode *jbuf = jfind(n, "buffer"), *jlen = jfind(n, "byteLength"), *joff = jfind(n, "byteOffset");
        /* skipped entries do not take a number, as in the engine (gltf.c:857-861); on top of its rules, numbers that are
         * negative, non-finite or fractional are skipped too (the engine would cast them: undefined behaviour) */
        double vbuf, vlen, voff;
        if (!jnum_index(jbuf, &vbuf) || !jnum_index(jlen, &vlen) || !jnum_index(joff, &voff)) continue;
        if (vbuf >= g->n_buffers) continue;
        struct g_bufview *bv = &g->bufvws[g->n_bufvws++];
        bv->buffer = (unsigned)vbuf; bv->offset = (size_t)voff; bv->length = (size_t)vlen;
    }
    return LD_OK;
}

/* accessors (gltf.c:869-897).  Skipped entries take no number. */
static int parse_accessors(struct gltf *g, const struct jnode *accrs)
{
    g->accrs = ld_alloc(accrs->count, sizeof(*g->accrs));
    if (!g->accrs) return LD_NOMEM;
    for (struct jnode *n = accrs->head; n; n = n->next) {
        struct jnode *jbv = jfind(n, "bufferView"), *joff = jfind(n, "byteOffset"), *jcount = jfind(n, "count"),
                     *jtype = jfind(n, "type"), *jct = jfind(n, "componentType");
        double vbv, vcount, vct, voff = 0.0;
        if (!jtype || jtype->tag != J_STRING || !jnum_index(jbv, &vbv) || !jnum_index(jcount, &vcount) || !jnum_index(jct, &vct)) continue;
        if (joff && joff->tag == J_NUMBER && !jnum_index(joff, &voff)) continue;
        if (vbv >= g->n_bufvws || vcount > 4294967295.0 || vct > 65535.0) continue;
        const unsigned comps = comps_of(jtype->str);
        if (!comps) continue;
        struct g_accessor *a = &g->accrs[g->n_accrs++];
        a->bufview = (unsigned)vbv; a->comptype = (unsigned)vct; a->count = (unsigned)vcount; a->comps = comps;
        a->offset = (size_t)voff;
    }
    return LD_OK;
}

static int name_index(const char *const names[4], const struct jnode *j, int dflt)
{
    if (j && j->tag == J_STRING)
        for (int i = 0; i < 4; i++) if (!strcmp(names[i], j->str)) return i;
    return dflt;
}

/* animations (gltf.c:491-581) */
static int parse_animations(struct gltf *g, const struct jnode *anis, struct ld_err *e)
{
    static const char *const paths[4] = { "translation", "rotation", "scale", "none" };
    static const char *const interps[4] = { "STEP", "LINEAR", "CUBICSPLINE", "NONE" };
    g->anis = ld_alloc(anis->count, sizeof(*g->anis));
    if (!g->anis) return LD_NOMEM;
    for (struct jnode *n = anis->head; n; n = n->next) {
        struct jnode *jch = jfind(n, "channels"), *jsm = jfind(n, "samplers");
        if (!jch || jch->tag != J_ARRAY || !jsm || jsm->tag != J_ARRAY) return fail(e, LD_PARSE, "glTF: animation without channels / samplers");
        struct g_anim *an = &g->anis[g->n_anis++];
        an->name = jstrdup(jfind(n, "name"));
        an->channels = ld_alloc(jch->count, sizeof(*an->channels));
        an->samplers = ld_alloc(jsm->count, sizeof(*an->samplers));
        if (!an->channels || !an->samplers) return LD_NOMEM;
        for (struct jnode *c = jch->head; c; c = c->next) {
            struct g_channel *ch = &an->channels[an->n_channels++];
            ch->sampler = -1; ch->node = -1; ch->path = PATH_NONE;
            if (c->tag != J_OBJECT) continue;
            ch->sampler = jnum_i(jfind(c, "sampler"), -1);
            struct jnode *jt = jfind(c, "target");
            if (jt && jt->tag == J_OBJECT) {
                ch->node = jnum_i(jfind(jt, "node"), -1);
                ch->path = name_index(paths, jfind(jt, "path"), PATH_NONE);
            }
        }
        for (struct jnode *c = jsm->head; c; c = c->next) {
            struct g_sampler *sm = &an->samplers[an->n_samplers++];
            sm->input = sm->output = sm->interp = -1;
            if (c->tag != J_OBJECT) continue;
            sm->input = jnum_i(jfind(c, "input"), -1);
            sm->output = jnum_i(jfind(c, "output"), -1);
            sm->interp = name_index(interps, jfind(c, "interpolation"), -1);
        }
    }
    return LD_OK;
}

/* skins (gltf.c:583-617).  skin->nodes[] maps a NODE number to its joint and is sized nr_joints by the engine:
 * a joint node numbered >= nr_joints would be written out of bounds there, so it is refused here. */
static int parse_skins(struct gltf *g, const struct jnode *skins, struct ld_err *e)
{
    g->skins = ld_alloc(skins->count, sizeof(*g->skins));
    if (!g->skins) return LD_NOMEM;
    for (struct jnode *n = skins->head; n; n = n->next) {
        struct g_skin *sk = &g->skins[g->n_skins++];
        struct jnode *jmat = jfind(n, "inverseBindMatrices"), *jj = jfind(n, "joints");
        if (jmat && jmat->tag == J_NUMBER) {
            size_t es; unsigned cnt;
            const void *b = accr_buf(g, (int)jmat->num, &es, &cnt);
            if (!b || es != 64) return fail(e, LD_PARSE, "glTF: inverseBindMatrices accessor is not a readable MAT4 float array");
            sk->invmxs = b; sk->nr_invmxs = cnt;
        }
        sk->name = jstrdup(jfind(n, "name"));
        if (!jj || jj->tag != J_ARRAY) continue;
        sk->joints = jints_alloc(jj, &sk->nr_joints);
        if (!sk->joints) return fail(e, LD_PARSE, "glTF: skin joints are not numbers");
        sk->nodes = calloc(sk->nr_joints, sizeof(int));
        if (!sk->nodes) return LD_NOMEM;
        for (unsigned j = 0; j < sk->nr_joints; j++) {
            if (sk->joints[j] < 0 || (unsigned)sk->joints[j] >= sk->nr_joints || (unsigned)sk->joints[j] >= g->n_nodes)
                return fail(e, LD_PARSE, "glTF: skin joint %u is node %d; the engine's node->joint table holds %u entries", j, sk->joints[j], sk->nr_joints);
            sk->nodes[sk->joints[j]] = (int)j;
        }
    }
    return LD_OK;
}

/* meshes (gltf.c:994-1037): the first primitive only; "indices" and "material" are required by the engine */
static int parse_meshes(struct gltf *g, const struct jnode *meshes)
{
    g->meshes = ld_alloc(meshes->count, sizeof(*g->meshes));
    if (!g->meshes) return LD_NOMEM;
    for (struct jnode *n = meshes->head; n; n = n->next) {
        struct jnode *jname = jfind(n, "name"), *jprim = jfind(n, "primitives");
        if (!jname || jname->tag != J_STRING || !jprim || jprim->tag != J_ARRAY || !jprim->head) continue;
        jprim = jprim->head;
        struct jnode *jidx = jfind(jprim, "indices"), *jmat = jfind(jprim, "material"), *jattr = jfind(jprim, "attributes");
        if (!jattr || jattr->tag != J_OBJECT || !jidx || !jmat) continue;
        struct g_mesh *m = &g->meshes[g->n_meshes++];
        m->name = strdup(jname->str);
        m->indices = (int)jidx->num; m->material = (int)jmat->num;
        m->POSITION = m->NORMAL = m->JOINTS_0 = m->WEIGHTS_0 = -1;
        for (struct jnode *p = jattr->head; p; p = p->next) {
            if (p->tag != J_NUMBER) continue;
            if (!strcmp(p->key, "POSITION")) m->POSITION = (int)p->num;
            else if (!strcmp(p->key, "NORMAL")) m->NORMAL = (int)p->num;
            else if (!strcmp(p->key, "JOINTS_0")) m->JOINTS_0 = (int)p->num;
            else if (!strcmp(p->key, "WEIGHTS_0")) m->WEIGHTS_0 = (int)p->num;
        }
    }
    return LD_OK;
}

/* gltf_json_parse (gltf.c:666-1064) */
static int gltf_sections(struct gltf *g, const struct jnode *root, struct ld_err *e)
{
    static const struct { const char *name; int tag; } need[8] = {         /* GLTF_CHECK_PROP, gltf.c:703-720: the engine refuses a file without any of these */
        { "scenes", J_ARRAY }, { "scene", J_NUMBER }, { "nodes", J_ARRAY }, { "materials", J_ARRAY }, { "meshes", J_ARRAY },
        { "accessors", J_ARRAY }, { "bufferViews", J_ARRAY }, { "buffers", J_ARRAY },
    };
    for (int i = 0; i < 8; i++) {
        const struct jnode *n = jfind(root, need[i].name);
        if (!n || n->tag != need[i].tag) return fail(e, LD_PARSE, "glTF: no '%s' property of the expected type", need[i].name);
    }
    const struct jnode *anis = jfind(root, "animations"), *skins = jfind(root, "skins");
    if (anis && anis->tag != J_ARRAY) return fail(e, LD_PARSE, "glTF: 'animations' is not an array");
    int rc = parse_nodes(g, jfind(root, "nodes"), e);
    if (!rc) parse_scenes(g, jfind(root, "scenes"));
    if (!rc) rc = parse_buffers(g, jfind(root, "buffers"), e);
    if (!rc) rc = parse_bufviews(g, jfind(root, "bufferViews"));
    if (!rc) rc = parse_accessors(g, jfind(root, "accessors"));
    if (!rc && anis) rc = parse_animations(g, anis, e);
    if (!rc && skins && skins->tag == J_ARRAY) rc = parse_skins(g, skins, e);
    if (!rc) rc = parse_meshes(g, jfind(root, "meshes"));
    return rc;
}

static int gltf_json_parse(struct gltf *g, const char *buf, size_t len, struct ld_err *e)
{
    struct jparse jp;
    struct jnode *root = jdecode(&jp, buf, len);
    if (!root) return fail(e, LD_PARSE, "glTF: JSON does not parse");
    const int rc = gltf_sections(g, root, e);
    jfree(&jp);
    return rc;
}

/* gltf_bin_parse (gltf.c:1065-1096): a well-formed GLB container gives its JSON chunk and sets g->bin; any other file
 * is JSON text as a whole */
static const char *glb_json_chunk(struct gltf *g, size_t *len)
{
    struct glb_header { uint32_t magic, version, length; } hdr;
    *len = g->file_size;
    if (g->file_size < 12 + 8) return (const char *)g->file;
    memcpy(&hdr, g->file, sizeof(hdr));
    if (hdr.magic != 0x46546C67u || hdr.version < 2 || hdr.length != g->file_size) return (const char *)g->file;
    uint32_t jlen, jtype, blen, btype;
    memcpy(&jlen, g->file + 12, 4); memcpy(&jtype, g->file + 16, 4);
    if (jtype != 0x4E4F534Au || (size_t)12 + 8 + jlen + 8 > g->file_size) return (const char *)g->file;
    memcpy(&blen, g->file + 20 + jlen, 4); memcpy(&btype, g->file + 24 + jlen, 4);
    if (btype != 0x004E4942u || (size_t)jlen + blen + 12 + 16 != g->file_size) return (const char *)g->file;
    g->bin = g->file + 28 + jlen; g->bin_size = blen;
    *len = jlen;
    return (const char *)g->file + 20;
}

/* gltf_onload (gltf.c:1098-1124): GLB first, plain JSON with data: URIs second */
int gltf_load_file(struct gltf *g, const char *path, struct ld_err *e)
{
    memset(g, 0, sizeof(*g));
    int rc = read_file(path, &g->file, &g->file_size);
    if (rc) return fail(e, rc, "cannot read '%s'", path);
    size_t len;
    const char *json = glb_json_chunk(g, &len);
    rc = gltf_json_parse(g, json, len, e);
    if (rc) gltf_free(g);
    return rc;
}

/* ================================================================================== the mesh choice */
static int gltf_mesh_by_name(const struct gltf *g, const char *name)
{
    for (unsigned i = 0; i < g->n_meshes; i++) if (!strcmp(g->meshes[i].name, name)) return (int)i;
    return -1;
}

/* which mesh model_new_from_json instantiates (scene.c:1391-1419) */
int gltf_pick_mesh(const struct gltf *g)
{
    if (!g->n_meshes) return -1;
    if (g->n_meshes == 1) return 0;
    const int collision = gltf_mesh_by_name(g, "collision");
    const int root = g->root_node < 0 ? 0 : g->nodes[g->root_node].mesh;     /* gltf_root_mesh, gltf.c:445-454 */
    if (root < 0) {                                                      /* the first mesh that is not the collision mesh */
        for (unsigned i = 0; i < g->n_meshes; i++) if ((int)i != collision) return (int)i;
        return -1;
    }
    return (unsigned)root < g->n_meshes ? root : -1;
}

int gltf_mesh_skin(const struct gltf *g, int mesh)                        /* gltf.c:456-467 */
{
    if (g->meshes[mesh].JOINTS_0 < 0 || g->meshes[mesh].WEIGHTS_0 < 0) return -1;
    for (unsigned i = 0; i < g->n_nodes; i++)
        if (g->nodes[i].mesh == mesh && g->nodes[i].skin >= 0) return g->nodes[i].skin;
    return -1;
}
