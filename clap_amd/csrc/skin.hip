// skin.hip -- vertex skinning for gfx950.
//
// Materialises what the reference leaves to its vertex shader (shaders/model.vert:32-48, also
// shadow.vert:19-23 and shadow_vsm.vert:19-23, i.e. recomputed in every geometry pass):
//     p' = sum_{i<4} w_i * (J[j_i] * (p,1)),   n' = sum_{i<4} w_i * (J[j_i] * (n,0))
// with J = the entity's joint_transforms, accumulated i = 0..3 in order, fp32, no weight
// renormalisation.  The shader goes on with the vec4 (model.vert:44: proj * view * trs * total_local_pos), whose
// w = sum_i w_i * (row 3 of J[j_i] . (p,1)) -- the sum of the weights for affine palettes, NOT 1 unless the
// asset's weights are normalised: out_w (optional) carries it, so a pre-skinned draw can feed the same vec4.
// Inputs are the reference's vertex attribute formats (mesh.h:125-131,
// gltf.c:387-388): position f32x3, normal f32x3, joints u8x4, weights f32x4.
//
// Mapping: one workgroup per character; its palette (nr_joints x 64 B) is staged once in LDS
// with an 80-byte row pitch (conflict-free 16-B column reads for lanes hitting different
// joints) and every lane skins one vertex.  HBM: 44 B in + 24 B out per vertex + the palette
// once per character (88.5 B / vertex at 64 joints, 200 vertices).
#include "common.h"
#include "lm_dev.h"
#include "skin_dev.h"

namespace clapgpu {

constexpr int SKIN_BLOCK = 256;
constexpr int SKIN_WAVES = 8;           // 56 VGPRs: eight workgroups per CU keep the vertex stream in flight
template <bool W>                      // W: also total_local_pos.w (4 B / vertex more)
__global__ __launch_bounds__(SKIN_BLOCK, SKIN_WAVES)
void k_skin(SkinArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float pal[];   // J rows of PAL_PITCH floats (5 KiB at 64 joints)

    const uint32_t c = blockIdx.x;
    const uint32_t J = a.J;
    const uint32_t vfirst = a.vert_first[c], vcount = a.vert_count[c], ofirst = a.out_first[c];

    stage_palette(pal, a.joint_transforms + (size_t)c * J * 4, J, threadIdx.x, SKIN_BLOCK);
    uint32_t k = threadIdx.x;
    SkinVert cur;
    if (k < vcount)
        cur = load_vert(a, (size_t)vfirst + k);                   // in flight across the barrier, beside the palette loads
    __syncthreads();

    while (k < vcount) {
        skin_vertex<W>(a, pal, cur, (size_t)ofirst + k);
        k += SKIN_BLOCK;
        if (k < vcount)
            cur = load_vert(a, (size_t)vfirst + k);
    }
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" int clapgpu_skin(void *stream, const clapgpu_skin_batch *b)
{
    if (!b)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (b->n_chars == 0)
        return CLAPGPU_OK;
    const int rc = check_skin_batch(b);
    if (rc) return rc;
    const SkinArgs a = make_skin_args(b);
    if (b->out_w)
        hipLaunchKernelGGL(k_skin<true>, dim3(b->n_chars), dim3(SKIN_BLOCK), b->nr_joints * PAL_PITCH * sizeof(float),
                           as_stream(stream), a);
    else
        hipLaunchKernelGGL(k_skin<false>, dim3(b->n_chars), dim3(SKIN_BLOCK), b->nr_joints * PAL_PITCH * sizeof(float),
                           as_stream(stream), a);
    CLAPGPU_LAUNCH_CHECK("k_skin");
    return CLAPGPU_OK;
}
