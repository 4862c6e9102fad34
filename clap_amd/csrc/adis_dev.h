// adis_dev.h -- dInternalHandleAutoDisabling for one body (ODE 0.16 util.cpp, restated; PARITY UNPINNED: ODE is absent from
// the reference), as a function: what k_islands_seed (islands.hip) runs ahead of the island pass, which needs to know who
// is asleep.  k_bodies_step (bodies.hip) holds the same statements written out: with the call in it the step needed 130
// VGPRs instead of 128 (three waves per SIMD instead of four) and measured outside the parent's spread
// (profiles/islands/README.md).  tests/test_islands_gpu.py holds the two to the same bits.
#pragma once
#include "common.h"

namespace clapgpu {

// b: anything with samples, lvel, avel, bflags, adis_steps_left, adis_time_left, adis_samples, adis_counter (BodiesK,
// IslandsK).  The caller has found body i enabled, with CLAPGPU_BODY_AUTO_DISABLE and CLAPGPU_BODY_HAS_JOINT in fl; v / om
// are its lvel / avel as loaded.  One sample into the ring, the counters, and when both are spent the body is
// disabled (HAS_JOINT dropped with it) and its velocities are zeroed: returns true.
template <class K>
__device__ __forceinline__ bool auto_disable(const K &b, const clapgpu_world &w, double h, uint32_t i, uint32_t fl,
                                             const double (&v)[3], const double (&om)[3])
{
    bool idle = false;
    double al[3], aa[3];
    const uint32_t S = b.samples > 1 ? b.samples : 1;
    if (S == 1) {
        for (int a = 0; a < 3; a++) { al[a] = v[a]; aa[a] = om[a]; }
        idle = true;
    } else {
        double *ring = b.adis_samples + (size_t)i * S * 6;
        uint32_t c = b.adis_counter[i] & 0x7fffffffu, ready = b.adis_counter[i] >> 31;
        for (int a = 0; a < 3; a++) { ring[6 * (size_t)c + a] = v[a]; ring[6 * (size_t)c + 3 + a] = om[a]; }
        if (++c >= S) { c = 0; ready = 1; }
        b.adis_counter[i] = c | ready << 31;
        if (ready) {
            idle = true;
            for (int a = 0; a < 3; a++) { al[a] = ring[a]; aa[a] = ring[3 + a]; }
            for (uint32_t s = 1; s < S; s++)
                for (int a = 0; a < 3; a++) { al[a] += ring[6 * (size_t)s + a]; aa[a] += ring[6 * (size_t)s + 3 + a]; }
            const double r1 = 1.0 / (double)S;
            for (int a = 0; a < 3; a++) { al[a] *= r1; aa[a] *= r1; }
        }
    }
    if (idle) {
        if (al[0] * al[0] + al[1] * al[1] + al[2] * al[2] > w.adis_linear_threshold_sq) idle = false;
        else if (aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2] > w.adis_angular_threshold_sq) idle = false;
    }
    int32_t sl = b.adis_steps_left[i];
    double tl = b.adis_time_left[i];
    if (idle) { sl--; tl -= h; } else { sl = w.adis_steps; tl = w.adis_time; }
    b.adis_steps_left[i] = sl;
    b.adis_time_left[i] = tl;
    const bool sleeps = sl <= 0 && tl <= 0;
    if (sleeps) {
        b.bflags[i] = (fl | CLAPGPU_BODY_DISABLED) & ~CLAPGPU_BODY_HAS_JOINT;
        double *vp = b.lvel + 3 * (size_t)i, *op = b.avel + 3 * (size_t)i;
        vp[0] = vp[1] = vp[2] = 0;
        op[0] = op[1] = op[2] = 0;
    }
    return sleeps;
}

} // namespace clapgpu
