// test_bp_levels -- the per-level statics image of a leveled broadphase (clap_amd/csrc/bp_statics.h's
// bp_statics_level_images / bp_statics_concat, read as bp_levels.hip's search reads it) checked on its own: no HIP call,
// no GPU.  Built as host code with -fsanitize=address,undefined by tests/test_bp_levels.py.
// Exits non-zero with a message on the first violation.
#include <stdio.h>
#include <stdlib.h>
#include "bp_statics.h"
#include "bp_levels.h"

using namespace clapgpu;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "test_bp_levels: " __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform(double lo, double hi)                               // splitmix64
{
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return lo + (hi - lo) * (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

static bool overlap(const double *a, const double *b)
{
    return !(a[0] > b[1] || a[1] < b[0] || a[2] > b[3] || a[3] < b[2] || a[4] > b[5] || a[5] < b[4]);
}

template <typename T>
static bool same_bytes(const std::vector<T> &a, const std::vector<T> &b)
{
    return a.size() == b.size() && !memcmp(a.data(), b.data(), a.size() * sizeof(T));
}

static void run(uint32_t buckets, double cell, uint32_t levels, uint32_t ns, uint32_t n_bodies)
{
    const double top = ldexp(cell, (int)levels - 1), world = 6.0 * top;
    std::vector<double> st(6 * (size_t)ns);
    for (uint32_t s = 0; s < ns; s++) {
        // edges from below the finest cell to several top-level blocks (large on every level)
        const double scale = ldexp(cell, (int)(s % (levels + 4)) - 1);
        for (int a = 0; a < 3; a++) {
            const double lo = uniform(-world, world);
            st[6 * (size_t)s + 2 * a] = lo;
            st[6 * (size_t)s + 2 * a + 1] = lo + uniform(0.3, 1.7) * scale;
        }
    }
    const double nan_box[6] = { NAN, 1.0, 0.0, 1.0, 0.0, 1.0 };
    memcpy(&st[6 * 7], nan_box, sizeof(nan_box));

    const std::vector<StaticsImage> ims = bp_statics_level_images(buckets, cell, levels, ns, st.data());
    CHECK(ims.size() == levels, "%zu images for %u levels", ims.size(), levels);
    // level 0 is today's image, byte for byte (and every level the image of its own cell)
    for (uint32_t l = 0; l < levels; l++) {
        const StaticsImage one = bp_statics_image(buckets, ldexp(cell, (int)l), ns, st.data());
        CHECK(same_bytes(one.start, ims[l].start) && same_bytes(one.entries, ims[l].entries) && same_bytes(one.large, ims[l].large) &&
              same_bytes(one.recs, ims[l].recs) && same_bytes(one.lrecs, ims[l].lrecs) && one.n_large == ims[l].n_large &&
              !memcmp(one.bounds, ims[l].bounds, sizeof(one.bounds)), "level %u is not the one-level image of its cell", l);
    }
    std::vector<uint32_t> large_start;
    const StaticsImage all = bp_statics_concat(ims, &large_start);
    CHECK(all.start.size() == (size_t)levels * (buckets + 1) && large_start.size() == levels + 1 && large_start[0] == 0,
          "the concatenated image: %zu starts, %zu large starts", all.start.size(), large_start.size());
    CHECK(all.start.back() == all.entries.size() && all.recs.size() == all.entries.size(), "entries and their starts");
    CHECK(large_start[levels] == all.n_large && all.large.size() == all.n_large && all.lrecs.size() == all.n_large, "the large lists");

    uint32_t n_large_levels = 0;
    for (uint32_t l = 0; l < levels; l++) {
        const uint32_t *ss = &all.start[(size_t)l * (buckets + 1)];
        CHECK(ss[0] == (l ? all.start[(size_t)l * (buckets + 1) - 1] : 0u), "level %u does not start where level %u ends", l, l - 1);
        std::vector<uint8_t> is_large(ns, 0), is_reg(ns, 0);
        for (uint32_t b = 0; b < buckets; b++) {
            CHECK(ss[b] <= ss[b + 1], "level %u: start not monotone at bucket %u", l, b);
            for (uint32_t e = ss[b]; e < ss[b + 1]; e++) {
                CHECK(all.entries[e] < ns && (e == ss[b] || all.entries[e - 1] < all.entries[e]), "level %u bucket %u: not ascending", l, b);
                CHECK(all.recs[e].idx == all.entries[e] && !memcmp(all.recs[e].bb, &st[6 * (size_t)all.entries[e]], 48), "level %u record %u", l, e);
                is_reg[all.entries[e]] = 1;
            }
        }
        // the large lists are ascending
        for (uint32_t e = large_start[l]; e < large_start[l + 1]; e++) {
            CHECK(all.large[e] < ns && (e == large_start[l] || all.large[e - 1] < all.large[e]), "level %u: large list not ascending at %u", l, e);
            CHECK(all.lrecs[e].idx == all.large[e] && !memcmp(all.lrecs[e].bb, &st[6 * (size_t)all.large[e]], 48), "level %u large record %u", l, e);
            is_large[all.large[e]] = 1;
        }
        for (uint32_t s = 0; s < ns; s++) CHECK(is_large[s] + is_reg[s] == 1, "level %u static %u: large %d, registered %d", l, s, is_large[s], is_reg[s]);
        CHECK(is_large[7], "level %u: the NaN static is not in the large list", l);
        n_large_levels += large_start[l + 1] > large_start[l];

        // every static is registered, on this level, in every block whose bodies could touch it: a body of this level
        // (largest edge in (cell / 2, cell], level 0: (0, cell]) finds each static it overlaps in its block's bucket
        // or in the level's large list
        const double c = ldexp(cell, (int)l);
        uint64_t from_bucket = 0;
        for (uint32_t i = 0; i < n_bodies; i++) {
            double bb[6];
            const uint32_t near = (uint32_t)uniform(0, ns);
            for (int a = 0; a < 3; a++) {
                const double e = a == (int)(i % 3) ? (i % 5 == 0 ? c : uniform(l ? 0.5 * c : 0.0, c)) : uniform(0.0, c);
                double lo = uniform(-world - c, world + c);
                const double s_lo = st[6 * (size_t)near + 2 * a], s_hi = st[6 * (size_t)near + 2 * a + 1];
                if (i % 2 && s_lo <= s_hi) lo = uniform(s_lo - e, s_hi);
                bb[2 * a] = lo; bb[2 * a + 1] = lo + e;
                while (bb[2 * a + 1] - lo > c) bb[2 * a + 1] = nextafter(bb[2 * a + 1], lo);
            }
            double cl;
            bool over;
            const uint32_t lv = box_level(bb, cell, levels, &cl, &over);
            CHECK(!over && lv <= l && cl <= c, "test body %u of level %u got level %u", i, l, lv);
            if (lv != l) continue;                                           // the largest edge rounded below the level
            const uint32_t ob = block_hash(cell_coord((bb[0] + bb[1]) * 0.5, c) >> 2, cell_coord((bb[2] + bb[3]) * 0.5, c) >> 2,
                                           cell_coord((bb[4] + bb[5]) * 0.5, c) >> 2, buckets - 1);
            for (uint32_t s = 0; s < ns; s++) {
                if (is_large[s] || !overlap(bb, &st[6 * (size_t)s])) continue;
                bool found = false;
                for (uint32_t e = ss[ob]; e < ss[ob + 1]; e++) found |= all.entries[e] == s;
                CHECK(found, "level %u body %u (bucket %u) overlaps static %u, which is neither large nor in its bucket", l, i, ob, s);
                from_bucket++;
            }
        }
        CHECK(from_bucket > n_bodies / 20, "level %u: only %llu overlaps with registered statics", l, (unsigned long long)from_bucket);
        printf("level %u (cell %g): %u entries, %u large, %llu overlaps through a bucket\n", l, c, ss[buckets] - ss[0],
               large_start[l + 1] - large_start[l], (unsigned long long)from_bucket);
    }
    CHECK(n_large_levels == levels, "only %u levels have a large static", n_large_levels);
}

int main()
{
    run(1024, 0.25, 6, 600, 6000);
    run(1024, 0.37, 3, 300, 6000);
    // no statics: the placeholders of the concatenated image
    std::vector<uint32_t> ls;
    const StaticsImage none = bp_statics_concat(bp_statics_level_images(1024, 1.0, 4, 0, nullptr), &ls);
    CHECK(none.start.size() == 4 * 1025 && none.start.back() == 0 && none.n_large == 0 && none.entries.size() == 1 && none.large.size() == 1 &&
          none.recs.size() == 1 && none.lrecs.size() == 1 && ls.size() == 5 && ls[4] == 0, "the leveled image without statics");
    // the level of a box: an edge equal to cell * 2^l is level l, the next double above is level l + 1; NaN is level 0
    for (uint32_t l = 0; l < 6; l++) {
        const double c = ldexp(0.25, (int)l);
        double cl;
        bool over;
        const double at[6] = { 0, c, 0, 0.1, 0, 0.1 }, above[6] = { 0, nextafter(c, INFINITY), 0, 0.1, 0, 0.1 },
                     below[6] = { 0, 0.1, 0, nextafter(c, 0.0), 0, 0.1 };
        CHECK(box_level(at, 0.25, 6, &cl, &over) == l && cl == c && !over, "edge = cell of level %u", l);
        CHECK(box_level(below, 0.25, 6, &cl, &over) == l && !over, "edge just below the cell of level %u", l);
        CHECK(box_level(above, 0.25, 6, &cl, &over) == (l < 5 ? l + 1 : 5) && over == (l == 5), "edge just above the cell of level %u", l);
    }
    {
        double cl;
        bool over;
        const double nan_edge[6] = { 0, NAN, 0, 0.1, 0, 0.1 };
        CHECK(box_level(nan_edge, 0.25, 6, &cl, &over) == 0 && !over, "a NaN edge");
    }
    printf("test_bp_levels OK\n");
    return 0;
}
