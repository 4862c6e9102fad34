// push.hip -- phys_body_push for a slide batch on gfx950: the forces a batch of movers puts on the bodies their sweeps
// hit, summed into the bodies' accumulators in the reference's order, and the wake-up of what they hit.
//
// character_sweep_delta calls phys_body_push(hit, push_velocity, push_mass) for every blocked sweep that hit a body
// (character.c:219-221); that is dBodyEnable + dBodyAddForce (physics.c:677-693).  The reference walks its characters
// one after the other, so body h's accumulator receives its forces in ascending (mover k, slot q) order, and fp64
// addition is not associative: the sum has to be made in that order, whatever the scheduling.
//   k_push_keys    one lane per slot s = 6 k + q: the key (target << shift) | s, target = b->n for a slot that pushes
//                  nothing; the same launch clears pushed[]
//   (rocPRIM radix sort of the keys, inside the caller's scratch: the keys are distinct, so the order is the same
//    whichever algorithm the sort picks)
//   k_push_apply   one lane per sorted key; the first key of a body's run walks the run, which is that body's slots in
//                  ascending order: one add per push into registers, then facc, the enable and the count
// No atomics anywhere.  float product, fp64 sum, no FMA contraction.  ODE is absent from the reference: PARITY UNPINNED.
#include <rocprim/device/device_radix_sort.hpp>
#include "common.h"

namespace clapgpu {

constexpr int UB = 256;
constexpr uint32_t PUSH_MAX_MOVERS = 1u << 28;          // 6 n stays inside 32 bits

struct PushK {
    uint32_t n_slots, n_bodies, shift;                  // shift: bits of a slot index
    const uint32_t *pusher;
    const float *velocity;
    const int32_t *push_hit;
    const uint32_t *flags;
    const double *mass;
    double *facc;
    uint32_t *bflags;
    int32_t *adis_steps_left;
    double *adis_time_left;
    int32_t adis_steps;
    double adis_time;
    uint32_t *pushed;
};

__global__ __launch_bounds__(UB)
void k_push_keys(PushK p, uint64_t *keys)
{
    const uint32_t s = blockIdx.x * UB + threadIdx.x;
    if (p.pushed && s < p.n_bodies) p.pushed[s] = 0;
    if (s >= p.n_slots) return;
    const uint32_t k = s / 6;
    uint32_t target = p.n_bodies;
    if (p.pusher[k] < p.n_bodies && (!p.flags || p.flags[k] == 0)) {
        const int32_t h = p.push_hit[s];
        if (h >= 0 && (uint32_t)h < p.n_bodies) target = (uint32_t)h;
    }
    keys[s] = (uint64_t)target << p.shift | s;
}

__global__ __launch_bounds__(UB)
void k_push_apply(PushK p, const uint64_t *keys)
{
    const uint32_t i = blockIdx.x * UB + threadIdx.x;
    if (i >= p.n_slots) return;
    const uint32_t t = (uint32_t)(keys[i] >> p.shift);
    if (t >= p.n_bodies) return;                                             // the slots that push nothing sort last
    if (i > 0 && (uint32_t)(keys[i - 1] >> p.shift) == t) return;            // not the head of its body's run
    const uint64_t slot_mask = (1ull << p.shift) - 1;
    double *fp = p.facc + 3 * (size_t)t;
    double f[3] = { fp[0], fp[1], fp[2] };
    uint32_t count = 0;
    for (uint32_t j = i; j < p.n_slots; j++) {
        const uint64_t key = keys[j];
        if ((uint32_t)(key >> p.shift) != t) break;
        const uint32_t k = (uint32_t)(key & slot_mask) / 6;                  // < n: the key kernel wrote it
        const float m = (float)p.mass[p.pusher[k]];                          // phys_body_get_mass
        const float *v = p.velocity + 3 * (size_t)k;
        for (int a = 0; a < 3; a++) {
            const float force = m * v[a];                                    // vec3_scale(force, push_velocity, push_mass)
            f[a] += (double)force;                                           // dBodyAddForce
        }
        count++;
    }
    fp[0] = f[0]; fp[1] = f[1]; fp[2] = f[2];
    p.bflags[t] &= ~CLAPGPU_BODY_DISABLED;                                   // dBodyEnable
    p.adis_steps_left[t] = p.adis_steps;
    p.adis_time_left[t] = p.adis_time;
    if (p.pushed) p.pushed[t] = count;
}

// the scratch: keys [6 n] | keys [6 n] | the sort's work space, sized for every key bit (the most it asks for)
struct PushLayout { size_t keys0, keys1, sort, sort_bytes, total; };

static hipError_t push_layout(uint32_t n_slots, hipStream_t s, PushLayout &l)
{
    Carve c;
    l.keys0 = c.take((size_t)n_slots * sizeof(uint64_t));
    l.keys1 = c.take((size_t)n_slots * sizeof(uint64_t));
    rocprim::double_buffer<uint64_t> none(nullptr, nullptr);
    l.sort_bytes = 0;
    const hipError_t err = rocprim::radix_sort_keys(nullptr, l.sort_bytes, none, (size_t)n_slots, 0, 64, s);
    l.sort = c.take(l.sort_bytes);
    l.total = c.bytes();
    return err;
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" size_t clapgpu_bodies_push_scratch_bytes(uint32_t n)
{
    if (n == 0 || n > PUSH_MAX_MOVERS) return 0;
    PushLayout l;
    if (push_layout(6 * n, nullptr, l) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return l.total;
}

extern "C" int clapgpu_bodies_push(void *stream, const clapgpu_bodies *b, const clapgpu_world *w, uint32_t n,
                                   const uint32_t *pusher, const float *velocity, const int32_t *push_hit, const uint32_t *flags,
                                   uint32_t *pushed, void *scratch)
{
    if (!b || !w || !b->facc || !b->mass || !b->bflags || !b->adis_steps_left || !b->adis_time_left)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (n == 0) return CLAPGPU_OK;
    if (!pusher || !velocity || !push_hit || !scratch || (reinterpret_cast<uintptr_t>(scratch) & 255u))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (n > PUSH_MAX_MOVERS) return CLAPGPU_ERR_TOO_LARGE;
    hipStream_t s = as_stream(stream);
    const uint32_t n_slots = 6 * n;
    PushLayout l;
    CLAPGPU_HIP(push_layout(n_slots, s, l));
    uint8_t *base = static_cast<uint8_t *>(scratch);
    rocprim::double_buffer<uint64_t> keys(reinterpret_cast<uint64_t *>(base + l.keys0),
                                          reinterpret_cast<uint64_t *>(base + l.keys1));

    PushK p;
    p.n_slots = n_slots; p.n_bodies = b->n; p.shift = bits_of(n_slots - 1);
    p.pusher = pusher; p.velocity = velocity; p.push_hit = push_hit; p.flags = flags;
    p.mass = b->mass; p.facc = b->facc; p.bflags = b->bflags;
    p.adis_steps_left = b->adis_steps_left; p.adis_time_left = b->adis_time_left;
    p.adis_steps = w->adis_steps; p.adis_time = w->adis_time;
    p.pushed = pushed;
    const uint32_t lanes = pushed && b->n > n_slots ? b->n : n_slots;
    hipLaunchKernelGGL(k_push_keys, dim3((lanes + UB - 1) / UB), dim3(UB), 0, s, p, keys.current());
    CLAPGPU_LAUNCH_CHECK("k_push_keys");
    CLAPGPU_HIP(rocprim::radix_sort_keys(base + l.sort, l.sort_bytes, keys, (size_t)n_slots, 0, p.shift + bits_of(b->n), s));
    hipLaunchKernelGGL(k_push_apply, dim3((n_slots + UB - 1) / UB), dim3(UB), 0, s, p, keys.current());
    CLAPGPU_LAUNCH_CHECK("k_push_apply");
    return CLAPGPU_OK;
}
