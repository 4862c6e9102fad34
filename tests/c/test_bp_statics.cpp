// test_bp_statics -- the host binning of a broadphase's static boxes (clap_amd/csrc/bp_statics.h) checked on its own:
// no HIP call, no GPU.  Built as host code with -fsanitize=address,undefined by tests/test_bp_statics.py.
// Exits non-zero with a message on the first violation.
#include <stdio.h>
#include <stdlib.h>
#include "bp_statics.h"

using namespace clapgpu;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "test_bp_statics: " __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform(double lo, double hi)                               // splitmix64
{
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return lo + (hi - lo) * (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// the device's boxes_overlap (bp_grid.h), restated for the host: NaN overlaps everything
static bool overlap(const double *a, const double *b)
{
    return !(a[0] > b[1] || a[1] < b[0] || a[2] > b[3] || a[3] < b[2] || a[4] > b[5] || a[5] < b[4]);
}

static void run(uint32_t buckets, double cell, uint32_t ns, uint32_t n_bodies)
{
    const double world = 40.0 * cell;
    std::vector<double> st(6 * (size_t)ns);
    for (uint32_t s = 0; s < ns; s++) {
        // edges well below, around and far above `cell` (and a few cells: registered in several blocks)
        const int kind = s % 8;
        const double e_lo = kind < 3 ? 0.02 : kind < 6 ? 0.7 : kind == 6 ? 2.0 : 8.0;
        const double e_hi = kind < 3 ? 0.3 : kind < 6 ? 1.5 : kind == 6 ? 7.0 : 60.0;
        for (int a = 0; a < 3; a++) {
            const double lo = uniform(-world, world);
            st[6 * (size_t)s + 2 * a] = lo;
            st[6 * (size_t)s + 2 * a + 1] = lo + uniform(e_lo, e_hi) * cell;
        }
    }
    const double degenerate[4][6] = {
        { 10, 10, 10, 10, 10, 10 },                                      // a point
        { 12, 11, 12, 11, 12, 11 },                                      // inverted
        { -1e300, 1e300, -1e300, 1e300, -1e300, 1e300 },
        { NAN, 1.0, 0.0, 1.0, 0.0, 1.0 },
    };
    for (int d = 0; d < 4; d++) memcpy(&st[6 * (size_t)(2 + 5 * d)], degenerate[d], sizeof(degenerate[d]));

    const StaticsImage im = bp_statics_image(buckets, cell, ns, st.data());

    // 1. the CSR
    CHECK(im.start.size() == (size_t)buckets + 1 && im.start[0] == 0, "start has %zu words", im.start.size());
    for (uint32_t b = 0; b < buckets; b++) CHECK(im.start[b] <= im.start[b + 1], "start not monotone at bucket %u", b);
    const uint32_t n_entries = im.start[buckets];
    CHECK(n_entries > 0 && n_entries == im.entries.size(), "start ends at %u, %zu entries", n_entries, im.entries.size());
    CHECK(im.n_large > 0 && im.n_large == im.large.size(), "n_large %u, %zu in the list", im.n_large, im.large.size());
    CHECK(im.recs.size() == im.entries.size() && im.lrecs.size() == im.large.size(), "records and lists differ in length");
    // 2. ascending inside a bucket (strictly: no static twice in one bucket)
    for (uint32_t b = 0; b < buckets; b++)
        for (uint32_t e = im.start[b] + 1; e < im.start[b + 1]; e++)
            CHECK(im.entries[e - 1] < im.entries[e], "bucket %u: entry %u after %u", b, im.entries[e], im.entries[e - 1]);
    // 3. every static in exactly one of "large" and "registered"
    std::vector<uint8_t> is_large(ns, 0), is_reg(ns, 0);
    for (uint32_t e = 0; e < im.n_large; e++) {
        CHECK(im.large[e] < ns && !is_large[im.large[e]], "large list: static %u out of range or twice", im.large[e]);
        is_large[im.large[e]] = 1;
    }
    for (uint32_t e = 0; e < n_entries; e++) {
        CHECK(im.entries[e] < ns, "entry %u out of range", im.entries[e]);
        is_reg[im.entries[e]] = 1;
    }
    for (uint32_t s = 0; s < ns; s++) CHECK(is_large[s] + is_reg[s] == 1, "static %u: large %d, registered %d", s, is_large[s], is_reg[s]);
    for (int d = 0; d < 4; d++)
        CHECK(d == 0 ? is_reg[2] : is_large[2 + 5 * d], "degenerate row %d is in the wrong list", d);
    // 4. the records carry box and index
    for (uint32_t e = 0; e < n_entries; e++)
        CHECK(im.recs[e].idx == im.entries[e] && !memcmp(im.recs[e].bb, &st[6 * (size_t)im.entries[e]], 48), "record %u", e);
    for (uint32_t e = 0; e < im.n_large; e++)
        CHECK(im.lrecs[e].idx == im.large[e] && !memcmp(im.lrecs[e].bb, &st[6 * (size_t)im.large[e]], 48), "large record %u", e);
    // 5. bounds = union of the registered boxes
    double u[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    for (uint32_t s = 0; s < ns; s++)
        for (int a = 0; a < 3 && is_reg[s]; a++) {
            u[a] = fmin(u[a], st[6 * (size_t)s + 2 * a]);
            u[3 + a] = fmax(u[3 + a], st[6 * (size_t)s + 2 * a + 1]);
        }
    for (int a = 0; a < 6; a++) CHECK(u[a] == im.bounds[a], "bounds[%d] = %.17g, union %.17g", a, im.bounds[a], u[a]);
    // 6. what the grid rests on: a body (every edge <= cell) finds every static it overlaps in the large list or in the
    // bucket of its own block
    uint64_t overlaps = 0, from_bucket = 0;
    for (uint32_t i = 0; i < n_bodies; i++) {
        double bb[6];
        const uint32_t near = (uint32_t)uniform(0, ns);                  // half of them next to a static
        for (int a = 0; a < 3; a++) {
            const double e = i % 5 == 0 ? cell : uniform(0.0, cell);
            double lo = uniform(-world - cell, world + cell);
            const double s_lo = st[6 * (size_t)near + 2 * a], s_hi = st[6 * (size_t)near + 2 * a + 1];
            if (i % 2 && near < ns && s_lo <= s_hi && s_hi - s_lo < 100.0 * cell) lo = uniform(s_lo - e, s_hi);
            bb[2 * a] = lo; bb[2 * a + 1] = lo + e;
            while (bb[2 * a + 1] - lo > cell) bb[2 * a + 1] = nextafter(bb[2 * a + 1], lo);   // the sum may round up past cell
            CHECK(bb[2 * a + 1] - bb[2 * a] <= cell, "test body %u has an edge above cell", i);
        }
        const int32_t cx = cell_coord((bb[0] + bb[1]) * 0.5, cell), cy = cell_coord((bb[2] + bb[3]) * 0.5, cell),
                      cz = cell_coord((bb[4] + bb[5]) * 0.5, cell);
        const uint32_t ob = block_hash(cx >> 2, cy >> 2, cz >> 2, buckets - 1);
        for (uint32_t s = 0; s < ns; s++) {
            if (!overlap(bb, &st[6 * (size_t)s])) continue;
            overlaps++;
            if (is_large[s]) continue;
            bool found = false;
            for (uint32_t e = im.start[ob]; e < im.start[ob + 1]; e++) found |= im.entries[e] == s;
            CHECK(found, "body %u (cell %d %d %d, bucket %u) overlaps static %u, which is neither large nor in its bucket", i, cx, cy, cz, ob, s);
            from_bucket++;
        }
    }
    CHECK(from_bucket > n_bodies / 4, "only %llu overlaps with registered statics: the bodies miss them", (unsigned long long)from_bucket);
    printf("cell %g: %u statics, %u entries, %u large, %llu overlaps (%llu through a bucket)\n", cell, ns, n_entries, im.n_large,
           (unsigned long long)overlaps, (unsigned long long)from_bucket);
}

int main()
{
    run(1024, 1.0, 2000, 20000);
    run(1024, 3.7, 2000, 20000);
    // no statics at all: the placeholders
    const StaticsImage none = bp_statics_image(1024, 1.0, 0, nullptr);
    CHECK(none.start[1024] == 0 && none.n_large == 0 && none.entries.size() == 1 && none.large.size() == 1 &&
          none.recs.size() == 1 && none.lrecs.size() == 1 && none.bounds[0] > none.bounds[3], "the image without statics");
    printf("test_bp_statics OK\n");
    return 0;
}
