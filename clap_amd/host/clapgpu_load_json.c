/*
 * clapgpu_load_json.c -- JSON text -> node tree, and the typed getters the loader reads it with.
 *
 * The tree is what the engine's json.c gives its loaders: objects and arrays as lists in file order (json_find_member
 * takes the first match), numbers through strtod.  Nesting deeper than 64 levels below the root is refused.
 */
#include <ctype.h>
#include <math.h>
#include <string.h>

#include "clapgpu_load_internal.h"

static struct jnode *jnew(struct jparse *jp, int tag)
{
    struct jnode *n = calloc(1, sizeof(*n));
    if (!n) { jp->bad = 1; return NULL; }
    if (jp->n_all == jp->cap_all) {
        size_t cap = jp->cap_all ? jp->cap_all * 2 : 256;
        struct jnode **a = realloc(jp->all, cap * sizeof(*a));
        if (!a) { free(n); jp->bad = 1; return NULL; }
        jp->all = a; jp->cap_all = cap;
    }
    jp->all[jp->n_all++] = n;
    n->tag = tag;
    return n;
}

void jfree(struct jparse *jp)
{
    for (size_t i = 0; i < jp->n_all; i++) { free(jp->all[i]->key); free(jp->all[i]->str); free(jp->all[i]); }
    free(jp->all);
    memset(jp, 0, sizeof(*jp));
}

static void jskip(struct jparse *jp) { while (jp->p < jp->end && isspace((unsigned char)*jp->p)) jp->p++; }

static int hex4(const char *s, unsigned *out)
{
    unsigned v = 0;
    for (int i = 0; i < 4; i++) {
        const int c = (unsigned char)s[i];
        if (!isxdigit(c)) return -1;
        v = v * 16 + (unsigned)(isdigit(c) ? c - '0' : tolower(c) - 'a' + 10);
    }
    *out = v;
    return 0;
}

static char *jstring(struct jparse *jp)
{
    if (jp->p >= jp->end || *jp->p != '"') { jp->bad = 1; return NULL; }
    jp->p++;
    size_t cap = 32, n = 0;
    char *s = malloc(cap);
    if (!s) { jp->bad = 1; return NULL; }
    while (jp->p < jp->end && *jp->p != '"') {
        unsigned cp = (unsigned char)*jp->p++;
        if (cp == '\\') {
            if (jp->p >= jp->end) break;
            const char c = *jp->p++;
            switch (c) {
            case 'b': cp = '\b'; break; case 'f': cp = '\f'; break; case 'n': cp = '\n'; break;
            case 'r': cp = '\r'; break; case 't': cp = '\t'; break;
            case 'u':
                if (jp->end - jp->p < 4 || hex4(jp->p, &cp)) { jp->bad = 1; free(s); return NULL; }
                jp->p += 4;
                if (cp >= 0xD800 && cp < 0xDC00 && jp->end - jp->p >= 6 && jp->p[0] == '\\' && jp->p[1] == 'u') {
                    unsigned lo;
                    if (!hex4(jp->p + 2, &lo) && lo >= 0xDC00 && lo < 0xE000) {
                        cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
                        jp->p += 6;
                    }
                }
                break;
            default: cp = (unsigned char)c; break;            /* \" \\ \/ */
            }
        }
        if (n + 5 > cap) { cap *= 2; char *t = realloc(s, cap); if (!t) { free(s); jp->bad = 1; return NULL; } s = t; }
        if (cp < 0x80) s[n++] = (char)cp;
        else if (cp < 0x800) { s[n++] = (char)(0xC0 | cp >> 6); s[n++] = (char)(0x80 | (cp & 0x3F)); }
        else if (cp < 0x10000) { s[n++] = (char)(0xE0 | cp >> 12); s[n++] = (char)(0x80 | ((cp >> 6) & 0x3F)); s[n++] = (char)(0x80 | (cp & 0x3F)); }
        else { s[n++] = (char)(0xF0 | cp >> 18); s[n++] = (char)(0x80 | ((cp >> 12) & 0x3F)); s[n++] = (char)(0x80 | ((cp >> 6) & 0x3F)); s[n++] = (char)(0x80 | (cp & 0x3F)); }
    }
    if (jp->p >= jp->end) { free(s); jp->bad = 1; return NULL; }
    jp->p++;                                                   /* closing quote */
    s[n] = 0;
    return s;
}

static struct jnode *jvalue(struct jparse *jp, int depth);

static void jappend(struct jnode *parent, struct jnode *child)
{
    if (parent->tail) parent->tail->next = child; else parent->head = child;
    parent->tail = child;
    parent->count++;
}

static struct jnode *jvalue(struct jparse *jp, int depth)
{
    if (depth > 64) { jp->bad = 1; return NULL; }
    jskip(jp);
    if (jp->p >= jp->end) { jp->bad = 1; return NULL; }
    const char c = *jp->p;
    if (c == '{' || c == '[') {
        struct jnode *n = jnew(jp, c == '{' ? J_OBJECT : J_ARRAY);
        if (!n) return NULL;
        const char close = c == '{' ? '}' : ']';
        jp->p++;
        jskip(jp);
        if (jp->p < jp->end && *jp->p == close) { jp->p++; return n; }
        for (;;) {
            char *key = NULL;
            jskip(jp);
            if (c == '{') {
                key = jstring(jp);
                if (!key) return NULL;
                jskip(jp);
                if (jp->p >= jp->end || *jp->p != ':') { free(key); jp->bad = 1; return NULL; }
                jp->p++;
            }
            struct jnode *v = jvalue(jp, depth + 1);
            if (!v) { free(key); return NULL; }
            v->key = key;
            jappend(n, v);
            jskip(jp);
            if (jp->p >= jp->end) { jp->bad = 1; return NULL; }
            if (*jp->p == ',') { jp->p++; continue; }
            if (*jp->p == close) { jp->p++; return n; }
            jp->bad = 1;
            return NULL;
        }
    }
    if (c == '"') {
        struct jnode *n = jnew(jp, J_STRING);
        if (!n) return NULL;
        n->str = jstring(jp);
        return n->str ? n : NULL;
    }
    if ((size_t)(jp->end - jp->p) >= 4 && !strncmp(jp->p, "true", 4)) { struct jnode *n = jnew(jp, J_BOOL); if (n) n->b = 1; jp->p += 4; return n; }
    if ((size_t)(jp->end - jp->p) >= 5 && !strncmp(jp->p, "false", 5)) { struct jnode *n = jnew(jp, J_BOOL); jp->p += 5; return n; }
    if ((size_t)(jp->end - jp->p) >= 4 && !strncmp(jp->p, "null", 4)) { struct jnode *n = jnew(jp, J_NULL); jp->p += 4; return n; }
    if (c == '-' || isdigit((unsigned char)c)) {
        char tmp[64];
        size_t k = 0;
        while (jp->p + k < jp->end && k < sizeof(tmp) - 1 && (isdigit((unsigned char)jp->p[k]) || strchr("+-.eE", jp->p[k]))) k++;
        memcpy(tmp, jp->p, k);
        tmp[k] = 0;
        char *endp;
        const double v = strtod(tmp, &endp);                 /* json.c parses numbers with strtod as well */
        if (endp == tmp) { jp->bad = 1; return NULL; }
        jp->p += endp - tmp;
        struct jnode *n = jnew(jp, J_NUMBER);
        if (n) n->num = v;
        return n;
    }
    jp->bad = 1;
    return NULL;
}

struct jnode *jdecode(struct jparse *jp, const char *buf, size_t len)
{
    memset(jp, 0, sizeof(*jp));
    jp->p = buf; jp->end = buf + len;
    struct jnode *root = jvalue(jp, 0);
    if (root) { jskip(jp); if (jp->p != jp->end) jp->bad = 1; }
    if (jp->bad || !root) { jfree(jp); return NULL; }
    return root;
}

struct jnode *jfind(const struct jnode *obj, const char *key)      /* json_find_member: the first match */
{
    if (!obj || obj->tag != J_OBJECT) return NULL;
    for (struct jnode *p = obj->head; p; p = p->next)
        if (p->key && !strcmp(p->key, key)) return p;
    return NULL;
}

/* json_double_array (json.c:1373-1392): every element must be a number; here at most `n` are taken */
int jdoubles(const struct jnode *arr, double *out, unsigned n)
{
    if (!arr || arr->tag != J_ARRAY) return -1;
    unsigned i = 0;
    for (struct jnode *p = arr->head; p; p = p->next, i++) {
        if (p->tag != J_NUMBER || i >= n) return -1;
        out[i] = p->num;
    }
    return 0;
}

int *jints_alloc(const struct jnode *arr, unsigned *count)          /* json_int_array_alloc */
{
    if (!arr || arr->tag != J_ARRAY || !arr->count) return NULL;
    int *a = malloc(sizeof(int) * arr->count);
    if (!a) return NULL;
    unsigned i = 0;
    for (struct jnode *p = arr->head; p; p = p->next, i++) {
        if (p->tag != J_NUMBER) { free(a); return NULL; }
        a[i] = (int)p->num;
    }
    *count = arr->count;
    return a;
}

/* A JSON number usable as an index / size / offset: a finite, non-negative integer value below 2^53 (negative, NaN or
 * huge doubles cast to unsigned / size_t are undefined behaviour, and (unsigned)-1 would index wildly). */
bool jnum_index(const struct jnode *n, double *out)
{
    if (!n || n->tag != J_NUMBER) return false;
    const double v = n->num;
    if (!(v >= 0.0) || !(v < 9007199254740992.0) || v != floor(v)) return false;
    if (out) *out = v;
    return true;
}

char *jstrdup(const struct jnode *n) { return n && n->tag == J_STRING ? strdup(n->str) : NULL; }
int jnum_i(const struct jnode *n, int dflt) { return n && n->tag == J_NUMBER ? (int)n->num : dflt; }

/* a JSON array of up to `n` <= 4 numbers as floats (a vector, a colour, a quaternion): the engine's loaders take
 * json_double_array into doubles and narrow; components the array does not have read as 0.  false: `out` is untouched */
bool jfloats(const struct jnode *arr, float *out, unsigned n)
{
    double d[4] = { 0, 0, 0, 0 };
    if (n > 4 || jdoubles(arr, d, n)) return false;
    for (unsigned i = 0; i < n; i++) out[i] = (float)d[i];
    return true;
}
