// views_dev.h -- the view block (include/clapgpu.h, "Views in device memory") as the kernels read it.  A slot of
// clapgpu_views_state begins with the cull's own lmd::FrustumK -- the frustum, then the constants k_views_calc left in
// the reserved words -- so a twin kernel hands the SAME functions (lmd::aabb_in_frustum_fast, cull_extra_views) a
// reference into the block where its original hands them a kernel argument.
#pragma once
#include <stddef.h>
#include "common.h"
#include "lm_dev.h"

namespace clapgpu {

static_assert(sizeof(lmd::Frustum) == sizeof(clapgpu_frustum) && offsetof(clapgpu_view_state, frustum) == 0 &&
              offsetof(clapgpu_view_state, cull) == offsetof(lmd::FrustumK, cmin) &&
              sizeof(lmd::FrustumK) <= offsetof(clapgpu_view_state, view_mx) && alignof(lmd::FrustumK) <= 16 &&
              sizeof(clapgpu_view_state) % 16 == 0,
              "a view slot begins with the cull's FrustumK");

__device__ __forceinline__ const lmd::FrustumK &view_frustum_k(const clapgpu_views_state *st, uint32_t slot)
{
    return *reinterpret_cast<const lmd::FrustumK *>(&st->slot[slot]);
}

// what every entry point asks of a block before any HIP call
static inline bool view_block_ok(const void *p) { return p && (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

} // namespace clapgpu
