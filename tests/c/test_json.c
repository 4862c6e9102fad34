/*
 * tests/c/test_json.c -- the loader's JSON module (clap_amd/host/clapgpu_load_json.c) alone.
 *
 *   test_json
 *
 * Links nothing but clapgpu_load_json.c; tests/test_load_scene.py builds it with AddressSanitizer + UBSan and runs it.
 * Every text is handed to the parser in a heap block of exactly its length (no terminator), so a read past the end of
 * the input is a sanitizer error.  The expected values were recorded from the loader as it was before it was split into
 * files (the same cases against its then-static functions), not from this module.  Exit code 0 and "PASS" = pass.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "clapgpu_load_internal.h"

static int fails;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); fails++; } } while (0)

static char *held;                                           /* the exact-length copy the tree's parse read from */

static struct jnode *parse_n(struct jparse *jp, const char *text, size_t len)
{
    free(held);
    held = malloc(len ? len : 1);
    memcpy(held, text, len);
    return jdecode(jp, held, len);
}

static struct jnode *parse(struct jparse *jp, const char *text) { return parse_n(jp, text, strlen(text)); }

static void accepts(const char *what, const char *text, int want)
{
    struct jparse jp;
    struct jnode *root = parse(&jp, text);
    CHECK(!!root == want, "%s: %s, expected %s", what, root ? "parsed" : "refused", want ? "a tree" : "a refusal");
    if (root) jfree(&jp);
}

/* `n` opening brackets, a 0, `n` closing ones */
static void nesting(unsigned n, char open, char close, int want)
{
    char text[512], what[32];
    size_t k = 0;
    for (unsigned i = 0; i < n; i++) { if (open == '{') { memcpy(text + k, "{\"k\":", 5); k += 5; } else text[k++] = open; }
    text[k++] = '0';
    for (unsigned i = 0; i < n; i++) text[k++] = close;
    text[k] = 0;
    snprintf(what, sizeof(what), "%u nested '%c'", n, open);
    accepts(what, text, want);
}

static void string_is(const char *what, const char *text, const char *bytes, size_t len)
{
    struct jparse jp;
    struct jnode *root = parse(&jp, text);
    CHECK(root && root->tag == J_STRING, "%s: no string", what);
    if (!root) return;
    if (root->tag == J_STRING) {
        CHECK(strlen(root->str) == len && !memcmp(root->str, bytes, len), "%s: %zu bytes '%s', expected %zu", what, strlen(root->str), root->str, len);
    }
    jfree(&jp);
}

/* a string of `plain` letters and `euros` \u20ac escapes (6 characters in, 3 bytes out) */
static void string_of(unsigned plain, unsigned euros)
{
    char text[1024], want[512], what[48];
    size_t k = 0, w = 0;
    text[k++] = '"';
    for (unsigned i = 0; i < plain; i++) { text[k++] = (char)('a' + i % 26); want[w++] = (char)('a' + i % 26); }
    for (unsigned i = 0; i < euros; i++) { memcpy(text + k, "\\u20ac", 6); k += 6; memcpy(want + w, "\xE2\x82\xAC", 3); w += 3; }
    text[k++] = '"';
    text[k] = 0;
    snprintf(what, sizeof(what), "string of %u letters + %u escapes", plain, euros);
    string_is(what, text, want, w);
}

/* a number literal of `len` characters: 1 and zeros */
static void long_number(unsigned len, int want, double value)
{
    char text[128], what[48];
    memset(text, '0', len);
    text[0] = '1';
    text[len] = 0;
    snprintf(what, sizeof(what), "number of %u characters", len);
    struct jparse jp;
    struct jnode *root = parse(&jp, text);
    CHECK(!!root == want, "%s: %s", what, root ? "parsed" : "refused");
    if (!root) return;
    CHECK(root->tag == J_NUMBER && root->num == value, "%s: %g, expected %g", what, root->num, value);
    jfree(&jp);
    /* the same literal as an array element: what follows the copied part must be ',' or ']' */
    char arr[160];
    snprintf(arr, sizeof(arr), "[%s]", text);
    accepts(what, arr, want);
}

static void index_is(const char *what, double v, int want)
{
    struct jnode n = { .tag = J_NUMBER, .num = v };
    double out = -7.0;
    CHECK(jnum_index(&n, &out) == !!want, "jnum_index(%s): expected %d", what, want);
    if (want) CHECK(!memcmp(&out, &v, sizeof(v)), "jnum_index(%s): gave %g", what, out);
    else CHECK(out == -7.0, "jnum_index(%s): wrote %g on refusal", what, out);
    CHECK(jnum_index(&n, NULL) == !!want, "jnum_index(%s, NULL)", what);
}

int main(void)
{
    struct jparse jp;
    struct jnode *root;

    /* ---- nesting: the root is level 0, level 64 is the deepest accepted ---- */
    nesting(64, '[', ']', 1);
    nesting(65, '[', ']', 0);
    nesting(64, '{', '}', 1);
    nesting(65, '{', '}', 0);

    /* ---- escapes ---- */
    string_is("simple escapes", "\"\\b\\f\\n\\r\\t\\\"\\\\\\/\"", "\b\f\n\r\t\"\\/", 8);
    string_is("an unknown escape keeps its letter", "\"\\q\"", "q", 1);
    string_is("\\u below 0x80", "\"\\u0041\"", "A", 1);
    string_is("\\u below 0x800", "\"\\u00e9\\u07FF\"", "\xC3\xA9\xDF\xBF", 4);
    string_is("\\u in the BMP", "\"\\u0800\\u20AC\\uffff\"", "\xE0\xA0\x80\xE2\x82\xAC\xEF\xBF\xBF", 9);
    string_is("surrogate pair", "\"\\ud83d\\ude00\"", "\xF0\x9F\x98\x80", 4);
    string_is("lone high surrogate: three bytes of its own", "\"\\ud83d\"", "\xED\xA0\xBD", 3);
    string_is("high surrogate, then no low one", "\"\\ud83d\\u0041\"", "\xED\xA0\xBD" "A", 4);
    accepts("high surrogate, then a \\u cut short", "\"\\ud83d\\ude\"", 0);
    accepts("\\u cut short by the end of input", "\"\\u12", 0);
    accepts("\\u cut short by the quote", "\"\\u12\"", 0);
    accepts("\\u with a non-hex digit", "\"\\u12g4\"", 0);
    accepts("backslash at the end of input", "\"abc\\", 0);
    accepts("unterminated string", "\"abc", 0);
    string_of(31, 0);
    string_of(32, 0);                                         /* the buffer starts at 32 bytes */
    string_of(33, 0);
    string_of(0, 40);                                         /* grows by escapes only: 240 characters in, 120 bytes out */
    string_of(27, 1);
    string_of(26, 2);
    string_is("empty string", "\"\"", "", 0);

    /* ---- numbers: the literal is copied into 64 bytes, i.e. at most 63 characters of it ---- */
    long_number(62, 1, 1e61);
    long_number(63, 1, 1e62);
    long_number(64, 0, 0);
    long_number(100, 0, 0);
    accepts("-", "-", 0);
    accepts("1e", "1e", 0);
    accepts("[1e]", "[1e]", 0);
    accepts("--1", "--1", 0);
    accepts("-nan", "-nan", 0);
    accepts("+1", "+1", 0);
    accepts(".5", ".5", 0);
    accepts("1.", "1.", 1);
    accepts("-0", "-0", 1);
    accepts("1e999", "1e999", 1);                             /* strtod's infinity */
    root = parse(&jp, "[-1.5e2, 0x10]");
    CHECK(!root, "a hexadecimal literal stops at the x");
    if (root) jfree(&jp);
    root = parse(&jp, "[-1.5e2,7]");
    CHECK(root && root->count == 2 && root->head->num == -150.0 && root->tail->num == 7.0, "[-1.5e2,7]");
    if (root) jfree(&jp);

    /* ---- structure ---- */
    accepts("empty input", "", 0);
    accepts("blank input", " \n\t", 0);
    accepts("trailing bytes after the root", "{} x", 0);
    accepts("trailing blanks after the root", " {} \n", 1);
    accepts("two roots", "1 2", 0);
    accepts("missing ':'", "{\"a\" 1}", 0);
    accepts("missing ','", "[1 2]", 0);
    accepts("missing ',' between members", "{\"a\":1 \"b\":2}", 0);
    accepts("missing ']'", "[1", 0);
    accepts("missing '}'", "{\"a\":1", 0);
    accepts("']' for '}'", "{\"a\":1]", 0);
    accepts("trailing ','", "[1,]", 0);
    accepts("a key that is no string", "{1:2}", 0);
    accepts("tru", "tru", 0);
    accepts("nul", "nul", 0);
    accepts("[tru]", "[tru]", 0);
    accepts("fals", "fals", 0);
    accepts("true", "true", 1);
    accepts("[true,false,null]", "[true,false,null]", 1);
    accepts("empty object and array", "{\"a\":[],\"b\":{}}", 1);
    root = parse(&jp, "[true,false,null]");
    CHECK(root && root->head->tag == J_BOOL && root->head->b == 1 && root->head->next->tag == J_BOOL && root->head->next->b == 0 &&
          root->tail->tag == J_NULL, "the bare words");
    if (root) jfree(&jp);

    /* ---- getters ---- */
    root = parse(&jp, "{\"a\":1,\"b\":\"s\",\"a\":2,\"v\":[1,2,3],\"long\":[1,2,3,4],\"short\":[1,2],\"mixed\":[1,\"x\",3],"
                      "\"none\":[],\"ints\":[3,-4,5.9]}");
    CHECK(root != NULL, "the getters' document");
    if (root) {
        double d[4] = { -1, -1, -1, -1 };
        float f[4] = { -1, -1, -1, -1 };
        unsigned cnt = 77;
        int *ints;
        CHECK(jfind(root, "a") && jfind(root, "a")->num == 1.0, "jfind: the first of duplicate keys");
        CHECK(!jfind(root, "zz") && !jfind(NULL, "a") && !jfind(jfind(root, "v"), "a"), "jfind: absent key, no object");
        CHECK(!jdoubles(jfind(root, "v"), d, 3) && d[0] == 1 && d[1] == 2 && d[2] == 3 && d[3] == -1, "jdoubles: three of three");
        CHECK(jdoubles(jfind(root, "long"), d, 3) == -1, "jdoubles: too many elements");
        d[0] = d[1] = d[2] = -1;
        CHECK(!jdoubles(jfind(root, "short"), d, 3) && d[0] == 1 && d[1] == 2 && d[2] == -1, "jdoubles: too few are taken, the rest is left");
        CHECK(jdoubles(jfind(root, "mixed"), d, 3) == -1, "jdoubles: a non-number");
        CHECK(!jdoubles(jfind(root, "none"), d, 3), "jdoubles: an empty array");
        CHECK(jdoubles(jfind(root, "a"), d, 3) == -1 && jdoubles(NULL, d, 3) == -1, "jdoubles: no array");
        /* jfloats is jdoubles narrowed: the same refusals, absent components 0, nothing written on refusal */
        CHECK(jfloats(jfind(root, "v"), f, 3) && f[0] == 1 && f[1] == 2 && f[2] == 3 && f[3] == -1, "jfloats: three of three");
        CHECK(jfloats(jfind(root, "short"), f, 3) && f[0] == 1 && f[1] == 2 && f[2] == 0, "jfloats: too few");
        f[0] = f[1] = f[2] = -1;
        CHECK(!jfloats(jfind(root, "long"), f, 3) && !jfloats(jfind(root, "mixed"), f, 3) && !jfloats(jfind(root, "a"), f, 3) &&
              !jfloats(NULL, f, 3) && f[0] == -1 && f[1] == -1 && f[2] == -1, "jfloats: refusals leave the floats alone");
        CHECK(jfloats(jfind(root, "long"), f, 4) && f[3] == 4, "jfloats: four");
        CHECK(!jints_alloc(jfind(root, "none"), &cnt) && cnt == 77, "jints_alloc: an empty array");
        CHECK(!jints_alloc(jfind(root, "mixed"), &cnt) && cnt == 77, "jints_alloc: a string among the numbers");
        CHECK(!jints_alloc(jfind(root, "a"), &cnt) && !jints_alloc(NULL, &cnt) && cnt == 77, "jints_alloc: no array");
        ints = jints_alloc(jfind(root, "ints"), &cnt);
        CHECK(ints && cnt == 3 && ints[0] == 3 && ints[1] == -4 && ints[2] == 5, "jints_alloc: numbers truncate toward zero");
        free(ints);
        CHECK(jnum_i(jfind(root, "a"), -9) == 1 && jnum_i(jfind(root, "b"), -9) == -9 && jnum_i(NULL, -9) == -9, "jnum_i");
        char *s = jstrdup(jfind(root, "b"));
        CHECK(s && !strcmp(s, "s") && !jstrdup(jfind(root, "a")) && !jstrdup(NULL), "jstrdup");
        free(s);
        CHECK(!jnum_index(jfind(root, "b"), d) && !jnum_index(NULL, d), "jnum_index: no number");
        jfree(&jp);
    }
    index_is("0", 0.0, 1);
    index_is("-0.0", -0.0, 1);
    index_is("0.5", 0.5, 0);
    index_is("-1", -1.0, 0);
    index_is("2^53 - 1", 9007199254740991.0, 1);
    index_is("2^53", 9007199254740992.0, 0);
    index_is("NaN", NAN, 0);
    index_is("infinity", INFINITY, 0);

    free(held);
    if (fails) return 1;
    printf("PASS\n");
    return 0;
}
