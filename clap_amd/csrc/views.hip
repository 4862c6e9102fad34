// views.hip -- the producer of the view block: clapgpu_views_state from clapgpu_views_source, one lane per slot.
//
// Replaces, per view, what the host did once a frame and handed to the kernels by value: transform_view_mat4x4
// (transform.c:132-138) when the slot is a pose, mvp = proj * view, subview_calc_frustum (view.c:248-289) and the cull's
// constants.  The arithmetic is lm_dev.h's -- the functions clapgpu_view_matrix, clapgpu_frustum_calc and
// make_frustum_k call on the host -- so the block holds the host's bits, non-finite inputs included.
//
// A few hundred flops in a single wavefront: the launch is latency, not work.  What it buys is that nothing about a view
// is a kernel argument any more, so a captured frame follows its camera.  The source is the host's to write, or a
// kernel's: slot 0's pose is k_camera_calc's (camera.hip) in a frame with clapgpu_frame.camera.
#include "common.h"
#include "lm_dev.h"
#include "views_dev.h"

namespace clapgpu {

__global__ __launch_bounds__(WAVE)
void k_views_calc(const clapgpu_views_source *__restrict__ src, clapgpu_views_state *__restrict__ dst, uint32_t n_views)
{
    const uint32_t s = threadIdx.x;
    if (s >= n_views) return;
    const clapgpu_view_source &in = src->slot[s];
    clapgpu_view_state &out = dst->slot[s];
    const uint32_t flags = in.flags;
    const float pos[3] = { in.pos[0], in.pos[1], in.pos[2] };
    float v[16], p[16], mvp[16];
    if (flags & CLAPGPU_VIEW_FROM_POSE) {
        const float q[4] = { in.quat[0], in.quat[1], in.quat[2], in.quat[3] };
        lmd::view_matrix(v, pos, q);
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) v[i] = in.view_mx[i];
    }
#pragma unroll
    for (int i = 0; i < 16; i++) p[i] = in.proj_mx[i];

    lmd::FrustumK k;
    lmd::frustum_calc(k.f, mvp, v, p, (flags & CLAPGPU_VIEW_NDC_Z_ZERO_ONE) != 0);
    lmd::frustum_constants(k);

#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int c = 0; c < 4; c++) out.frustum.planes[i][c] = k.f.planes[i][c];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int c = 0; c < 4; c++) out.frustum.corners[i][c] = k.f.corners[i][c];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        out.cull[a] = __float_as_uint(k.cmin[a]);
        out.cull[3 + a] = __float_as_uint(k.cmax[a]);
    }
    out.cull[6] = k.finite;
    out.cull[7] = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        out.view_mx[i] = v[i];
        out.proj_mx[i] = p[i];
        out.mvp[i] = mvp[i];
    }
#pragma unroll
    for (int a = 0; a < 3; a++) out.cam_pos[a] = pos[a];
    out.pad = 0;
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" int clapgpu_views_calc(void *stream, const clapgpu_views_source *source, clapgpu_views_state *state, uint32_t n_views)
{
    if (!view_block_ok(source) || !view_block_ok(state) || n_views < 1 || n_views > CLAPGPU_VIEW_SLOTS)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    hipLaunchKernelGGL(k_views_calc, dim3(1), dim3(WAVE), 0, as_stream(stream), source, state, n_views);
    CLAPGPU_LAUNCH_CHECK("k_views_calc");
    return CLAPGPU_OK;
}
