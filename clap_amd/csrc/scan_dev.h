// scan_dev.h -- a single-pass exclusive scan over the totals of a launch's tiles, with decoupled look-back.  Device only.
// A tile's offset = the sum of everything before it.  Tile b publishes (flag, epoch, value) as ONE 64-bit word -- its own
// sum first (AGGREGATE), its inclusive prefix once known (PREFIX) -- and a wavefront walks back over its predecessors'
// words, 64 at a time, until it meets a PREFIX.  Workgroups are dispatched in index order and wait only on lower indices,
// so the walk always terminates; the caller's epoch in the word (one value per pass over the same words) makes the last
// pass's entries read as empty: no clearing pass.
#pragma once
#include "common.h"

namespace clapgpu {

constexpr uint64_t LB_AGG = 1ull << 62, LB_PREFIX = 2ull << 62, LB_FLAGS = 3ull << 62;
__device__ __forceinline__ uint64_t lb_word(uint64_t flag, uint32_t epoch, uint32_t value)
{
    return flag | ((uint64_t)(epoch & 0x3fffffffu) << 32) | value;
}

// exclusive prefix of tile `b` (called by one whole wavefront); publishes the tile's own words.  A word that never
// arrives sets `status_bit` in *status.
__device__ __forceinline__ uint32_t lb_exclusive(uint64_t *state, uint32_t b, uint32_t sum, uint32_t epoch, uint32_t *status,
                                                 uint32_t status_bit)
{
    const int lane = lane_id();
    if (b == 0) {
        if (lane == 0) __hip_atomic_store(&state[0], lb_word(LB_PREFIX, epoch, sum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return 0;
    }
    if (lane == 0) __hip_atomic_store(&state[b], lb_word(LB_AGG, epoch, sum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t excl = 0;
    for (int64_t top = (int64_t)b - 1; top >= 0; top -= WAVE) {         // window: tiles top, top-1, ..., top-63
        const int64_t t = top - lane;
        uint64_t w = 0;
        if (t >= 0) {
            uint32_t spins = 0;
            do {
                w = __hip_atomic_load(&state[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((w & LB_FLAGS) && (uint32_t)((w >> 32) & 0x3fffffffu) == (epoch & 0x3fffffffu)) break;
                w = 0;
                __builtin_amdgcn_s_sleep(1);
            } while (++spins < (1u << 22));                               // a bound, not an expectation: see above
            if (!w) atomicOr(status, status_bit);
        }
        const uint64_t is_prefix = __ballot(t >= 0 && (w & LB_FLAGS) == LB_PREFIX);
        const int stop = is_prefix ? __builtin_ctzll(is_prefix) : WAVE - 1;   // nearest predecessor that knows its prefix
        uint32_t v = (t >= 0 && lane <= stop) ? (uint32_t)w : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        excl += v;
        if (is_prefix) break;
    }
    if (lane == 0) __hip_atomic_store(&state[b], lb_word(LB_PREFIX, epoch, excl + sum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return excl;
}

} // namespace clapgpu
