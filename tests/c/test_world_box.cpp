// test_world_box.cpp -- lmd::world_aabb (the box from its extreme corners, lm_dev.h) against lmd::world_aabb_literal
// (all eight corners, the reference's order), bit for bit, on the host.  Stand-alone: no HIP call.
//   test_world_box [cases]   prints the differences, how many cases took each path and what the cases covered;
//   exit status 0 iff no case differs.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "lm_dev.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd64()                                         // splitmix64
{
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static uint32_t rndu(uint32_t n) { return (uint32_t)(rnd64() % n); }
static float rndf(float lo, float hi) { return lo + (hi - lo) * (float)((rnd64() >> 40) * (1.0 / 16777216.0)); }
static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

static const float SPECIAL[] = { NAN, INFINITY, -INFINITY, 0.0f, -0.0f, 1e-42f, -1e-42f, 3e38f, -3e38f, 1e20f, 1e-20f, 1.0f, -1.0f };
constexpr int N_SPECIAL = sizeof(SPECIAL) / sizeof(SPECIAL[0]);

int main(int argc, char **argv)
{
    const long cases = argc > 1 ? atol(argv[1]) : 3000000;
    long diffs = 0, n_fast = 0, n_literal = 0;
    long cov_neg0_translation = 0, cov_inverted_box = 0, cov_negative_scale = 0, cov_zero_scale = 0, cov_overflow = 0,
         cov_nan = 0, cov_ties = 0;
    for (long c = 0; c < cases; c++) {
        float m[16], b[6];                                       // b = lx ly lz hx hy hz
        lmd::identity(m);
        const uint32_t kind = rndu(8);
        if (kind == 0) {                                         // small integers: equal corner values, exact cancellation
            for (int col = 0; col < 4; col++)
                for (int r = 0; r < 3; r++) E_(m, col, r) = (float)((int)rndu(5) - 2);
            for (int k = 0; k < 6; k++) b[k] = (float)((int)rndu(7) - 3);
            cov_ties++;
        } else if (kind == 1) {                                  // a TRS as the kernels build it, any sign of scale, or none
            const float s = rndu(4) == 0 ? 0.0f : rndf(-3.f, 3.f);
            float q[4] = { rndf(-1, 1), rndf(-1, 1), rndf(-1, 1), rndf(-1, 1) };
            const float ql = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) + 1e-9f;
            if (rndu(3) == 0) { q[0] = q[1] = q[2] = 0.f; q[3] = ql; }      // unrotated: exact zeros off the diagonal
            lmd::trs(m, rndf(-100, 100), rndf(-100, 100), rndf(-100, 100), s, q[0] / ql, q[1] / ql, q[2] / ql, q[3] / ql);
            for (int k = 0; k < 3; k++) { b[k] = rndf(-5, 0); b[3 + k] = rndf(0, 5); }
        } else {                                                 // any affine matrix, entries over many magnitudes
            const float mag = powf(10.f, rndf(-3, 3));
            for (int col = 0; col < 4; col++)
                for (int r = 0; r < 3; r++) E_(m, col, r) = rndf(-1, 1) * mag;
            const float bmag = powf(10.f, rndf(-3, 3));
            for (int k = 0; k < 3; k++) { b[k] = rndf(-1, 1) * bmag; b[3 + k] = rndf(-1, 1) * bmag; }   // lo > hi half the time
        }
        if (rndu(3)) {                                           // up to six of the 18 values become special ones
            const uint32_t n = rndu(7);
            for (uint32_t k = 0; k < n; k++) {
                const uint32_t at = rndu(18);
                const float v = SPECIAL[rndu(N_SPECIAL)];
                if (at < 12) E_(m, at / 3, at % 3) = v; else b[at - 12] = v;
            }
        }
        if (rndu(16) == 0) E_(m, 3, rndu(3)) = -0.0f;

        bool neg0 = false, inverted = false, negs = false, zeros = false, ovf = false, nan = false;
        for (int a = 0; a < 3; a++) {
            neg0 |= bits(E_(m, 3, a)) == 0x80000000u;
            inverted |= b[a] > b[3 + a];
            for (int col = 0; col < 3; col++) {
                const float e = E_(m, col, a);
                negs |= col == a && e < 0.f;
                zeros |= col == a && e == 0.f;
                for (int h = 0; h < 2; h++) {
                    const float x = b[col + 3 * h];
                    ovf |= isfinite(e) && isfinite(x) && isinf(e * x);
                }
            }
        }
        for (int k = 0; k < 16; k++) nan |= isnan(m[k]);
        for (int k = 0; k < 6; k++) nan |= isnan(b[k]);
        cov_neg0_translation += neg0; cov_inverted_box += inverted; cov_negative_scale += negs; cov_zero_scale += zeros;
        cov_overflow += ovf; cov_nan += nan;

        float bb[6], ctr[3], bb_l[6], ctr_l[3], scratch[6];
        if (lmd::world_box_extremes(scratch, m, b[0], b[1], b[2], b[3], b[4], b[5])) n_fast++; else n_literal++;
        lmd::world_aabb(bb, ctr, m, b[0], b[1], b[2], b[3], b[4], b[5]);
        lmd::world_aabb_literal(bb_l, ctr_l, m, b[0], b[1], b[2], b[3], b[4], b[5]);
        bool same = true;
        for (int k = 0; k < 6; k++) same &= bits(bb[k]) == bits(bb_l[k]);
        for (int k = 0; k < 3; k++) same &= bits(ctr[k]) == bits(ctr_l[k]);
        if (!same && diffs++ < 5) {
            printf("case %ld differs:\n  m  ", c);
            for (int k = 0; k < 16; k++) printf(" %a", m[k]);
            printf("\n  box");
            for (int k = 0; k < 6; k++) printf(" %a", b[k]);
            printf("\n  got");
            for (int k = 0; k < 6; k++) printf(" %08x", bits(bb[k]));
            for (int k = 0; k < 3; k++) printf(" %08x", bits(ctr[k]));
            printf("\n  want");
            for (int k = 0; k < 6; k++) printf(" %08x", bits(bb_l[k]));
            for (int k = 0; k < 3; k++) printf(" %08x", bits(ctr_l[k]));
            printf("\n");
        }
    }
    printf("cases %ld differences %ld fast %ld literal %ld\n", cases, diffs, n_fast, n_literal);
    printf("covered neg0_translation %ld inverted_box %ld negative_scale %ld zero_scale %ld overflow %ld nan %ld ties %ld\n",
           cov_neg0_translation, cov_inverted_box, cov_negative_scale, cov_zero_scale, cov_overflow, cov_nan, cov_ties);
    return diffs ? 1 : 0;
}
