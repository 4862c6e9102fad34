// skin_dev.h -- the skinning of ONE vertex, stated once for every kernel that skins (skin.hip: every vertex of every
// character; skin_drawn.hip: the vertices the frame draws).  Device only.
//     p' = sum_{i<4} w_i * (J[j_i] * (p,1)),   n' = sum_{i<4} w_i * (J[j_i] * (n,0))
// accumulated i = 0..3 in order, fp32, no contraction (-ffp-contract=off, the Makefile), no weight renormalisation: the
// arithmetic of shaders/model.vert:32-48 as oracle/skin.c states it.  The palette is read from LDS rows of PAL_PITCH floats.
#pragma once
#include "common.h"

namespace clapgpu {

constexpr int PAL_PITCH = 20;          // floats per palette row in LDS (16 + 4 pad): conflict-free 16-B column reads
constexpr int PAL_MAX_JOINTS = 256;

struct SkinArgs {
    uint32_t        n_chars, J;
    const uint32_t *vert_first, *vert_count, *out_first;
    const float    *position, *normal;
    const uint32_t *joints;            // u8x4 packed
    const float4   *weights;
    const float4   *joint_transforms;
    float          *out_position, *out_normal, *out_w;
};

struct SkinVert {
    float    px, py, pz, nx, ny, nz;
    uint32_t jj;
    float4   w;
};

__device__ __forceinline__ SkinVert load_vert(const SkinArgs &a, size_t v)
{
    // vertex attributes are read once per frame: non-temporal loads keep them from evicting the
    // palette (and everything else that is reused) from the infinity cache
    SkinVert r;
    r.px = __builtin_nontemporal_load(&a.position[3 * v]);
    r.py = __builtin_nontemporal_load(&a.position[3 * v + 1]);
    r.pz = __builtin_nontemporal_load(&a.position[3 * v + 2]);
    r.nx = __builtin_nontemporal_load(&a.normal[3 * v]);
    r.ny = __builtin_nontemporal_load(&a.normal[3 * v + 1]);
    r.nz = __builtin_nontemporal_load(&a.normal[3 * v + 2]);
    r.jj = __builtin_nontemporal_load(&a.joints[v]);
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 w = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(&a.weights[v]));
    r.w = make_float4(w.x, w.y, w.z, w.w);
    return r;
}

// stage rows [0, J) of a character's palette into `pal` with `lanes` lanes (lane = this lane's index among them): J * 4
// float4, coalesced.  The caller orders the writes before the reads (a barrier, or the wave's own fence).
__device__ __forceinline__ void stage_palette(float *pal, const float4 *src, uint32_t J, uint32_t lane, uint32_t lanes)
{
    for (uint32_t q = lane; q < J * 4; q += lanes) {
        const float4 v = src[q];
        *reinterpret_cast<float4 *>(pal + (q >> 2) * PAL_PITCH + (q & 3) * 4) = v;
    }
}

// blend vertex `cur` by the palette in `pal` and write it at output vertex `o`.  W: also total_local_pos.w
template <bool W>
__device__ __forceinline__ void skin_vertex(const SkinArgs &a, const float *pal, const SkinVert &cur, size_t o)
{
    const float w[4] = { cur.w.x, cur.w.y, cur.w.z, cur.w.w };
    float tp[3] = { 0, 0, 0 }, tn[3] = { 0, 0, 0 }, tw = 0.f;
#pragma unroll 1
    for (int i = 0; i < 4; i++) {
        const uint32_t ji = (cur.jj >> (8 * i)) & 0xffu;
        const float4 *m = reinterpret_cast<const float4 *>(pal + ji * PAL_PITCH);
        const float4 c0 = m[0], c1 = m[1], c2 = m[2], c3 = m[3];
        const float wi = i == 0 ? w[0] : i == 1 ? w[1] : i == 2 ? w[2] : w[3];
        // ((M0 x + M1 y) + M2 z) + M3 w per component; w = 1 for positions, 0 for normals
        const float lx = ((c0.x * cur.px + c1.x * cur.py) + c2.x * cur.pz) + c3.x * 1.0f;
        const float ly = ((c0.y * cur.px + c1.y * cur.py) + c2.y * cur.pz) + c3.y * 1.0f;
        const float lz = ((c0.z * cur.px + c1.z * cur.py) + c2.z * cur.pz) + c3.z * 1.0f;
        const float mx = ((c0.x * cur.nx + c1.x * cur.ny) + c2.x * cur.nz) + c3.x * 0.0f;
        const float my = ((c0.y * cur.nx + c1.y * cur.ny) + c2.y * cur.nz) + c3.y * 0.0f;
        const float mz = ((c0.z * cur.nx + c1.z * cur.ny) + c2.z * cur.nz) + c3.z * 0.0f;
        tp[0] += lx * wi; tp[1] += ly * wi; tp[2] += lz * wi;
        tn[0] += mx * wi; tn[1] += my * wi; tn[2] += mz * wi;
        if (W) {
            const float lw = ((c0.w * cur.px + c1.w * cur.py) + c2.w * cur.pz) + c3.w * 1.0f;
            tw += lw * wi;
        }
    }
    // written once, read by the draw path: streaming stores keep them out of the infinity cache
    __builtin_nontemporal_store(tp[0], &a.out_position[3 * o]);
    __builtin_nontemporal_store(tp[1], &a.out_position[3 * o + 1]);
    __builtin_nontemporal_store(tp[2], &a.out_position[3 * o + 2]);
    __builtin_nontemporal_store(tn[0], &a.out_normal[3 * o]);
    __builtin_nontemporal_store(tn[1], &a.out_normal[3 * o + 1]);
    __builtin_nontemporal_store(tn[2], &a.out_normal[3 * o + 2]);
    if (W)
        __builtin_nontemporal_store(tw, &a.out_w[o]);
}

// a clapgpu_skin_batch as the kernels take it; the caller has checked its pointers
static inline SkinArgs make_skin_args(const clapgpu_skin_batch *b)
{
    SkinArgs a;
    a.n_chars = b->n_chars;
    a.J = b->nr_joints;
    a.vert_first = b->vert_first;
    a.vert_count = b->vert_count;
    a.out_first = b->out_first;
    a.position = b->position;
    a.normal = b->normal;
    a.joints = reinterpret_cast<const uint32_t *>(b->joints);
    a.weights = reinterpret_cast<const float4 *>(b->weights);
    a.joint_transforms = reinterpret_cast<const float4 *>(b->joint_transforms);
    a.out_position = b->out_position;
    a.out_normal = b->out_normal;
    a.out_w = b->out_w;
    return a;
}

// what clapgpu_skin and clapgpu_skin_drawn ask of a batch (n_chars != 0)
static inline int check_skin_batch(const clapgpu_skin_batch *b)
{
    if (!b->vert_first || !b->vert_count || !b->out_first || !b->position || !b->normal || !b->joints ||
        !b->weights || !b->joint_transforms || !b->out_position || !b->out_normal)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (b->nr_joints == 0 || b->nr_joints > PAL_MAX_JOINTS)
        return CLAPGPU_ERR_TOO_LARGE;
    return CLAPGPU_OK;
}

} // namespace clapgpu
