// dump_bp_statics -- prints the statics image the host makes of a set of boxes (clap_amd/csrc/bp_statics.h:
// bp_statics_image for one level, bp_statics_level_images + bp_statics_concat for more), for
// tests/test_bp_statics_update.py to hold against tests/bpstaticsref.py.  No HIP call, no GPU; built as host code with
// -fsanitize=address,undefined.
// Input file: uint32 buckets, levels, n_static, 0; double cell; n_static * 6 doubles.  Output: one line per array, doubles
// as the hexadecimal of their bits.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include "bp_statics.h"

using namespace clapgpu;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "dump_bp_statics: " __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static void print_recs(const char *name, const std::vector<GridRec> &recs, const std::vector<uint32_t> &idx, uint32_t n)
{
    printf("%s", name);
    for (uint32_t e = 0; e < n; e++) {
        CHECK(recs[e].idx == idx[e], "%s %u: record of %u, entry %u", name, e, recs[e].idx, idx[e]);
        CHECK(!recs[e].cell[0] && !recs[e].cell[1] && !recs[e].cell[2], "%s %u: cell words", name, e);
        for (int a = 0; a < 6; a++) {
            uint64_t u;
            memcpy(&u, &recs[e].bb[a], sizeof(u));
            printf(" %016" PRIx64, u);
        }
    }
    printf("\n");
}

int main(int argc, char **argv)
{
    CHECK(argc == 2, "usage: dump_bp_statics FILE");
    FILE *f = fopen(argv[1], "rb");
    CHECK(f, "cannot open %s", argv[1]);
    uint32_t head[4];
    double cell;
    CHECK(fread(head, sizeof(head), 1, f) == 1 && fread(&cell, sizeof(cell), 1, f) == 1, "short header");
    const uint32_t buckets = head[0], levels = head[1], n = head[2];
    CHECK(buckets && !(buckets & (buckets - 1)) && levels >= 1 && levels <= 16 && cell > 0.0, "bad header");
    std::vector<double> boxes(6 * (size_t)n + 1);
    CHECK(n == 0 || fread(boxes.data(), 6 * sizeof(double), n, f) == n, "short box array");
    fclose(f);

    std::vector<uint32_t> large_start{ 0u };
    StaticsImage im;
    if (levels == 1) {
        im = bp_statics_image(buckets, cell, n, boxes.data());
        large_start.push_back(im.n_large);
    } else {
        im = bp_statics_concat(bp_statics_level_images(buckets, cell, levels, n, boxes.data()), &large_start);
    }
    CHECK(im.start.size() == (size_t)levels * (buckets + 1), "%zu starts", im.start.size());
    const uint32_t n_entries = im.start.back();
    CHECK(im.entries.size() >= n_entries && im.recs.size() >= n_entries && im.large.size() >= im.n_large &&
          im.lrecs.size() >= im.n_large && large_start.size() == levels + 1 && large_start.back() == im.n_large, "sizes");
    printf("n_entries %u\nn_large %u\n", n_entries, im.n_large);
    printf("start");
    for (uint32_t v : im.start) printf(" %u", v);
    printf("\nentries");
    for (uint32_t e = 0; e < n_entries; e++) printf(" %u", im.entries[e]);
    printf("\nlarge");
    for (uint32_t e = 0; e < im.n_large; e++) printf(" %u", im.large[e]);
    printf("\nlarge_start");
    for (uint32_t v : large_start) printf(" %u", v);
    printf("\nbounds");
    for (int a = 0; a < 6; a++) {
        uint64_t u;
        memcpy(&u, &im.bounds[a], sizeof(u));
        printf(" %016" PRIx64, u);
    }
    printf("\n");
    print_recs("entry_boxes", im.recs, im.entries, n_entries);
    print_recs("large_boxes", im.lrecs, im.large, im.n_large);
    printf("dump_bp_statics OK\n");
    return 0;
}
