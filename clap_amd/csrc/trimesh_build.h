// trimesh_build.h -- what the two builds of a mesh set share: the object, the bake arithmetic, the Morton code, the Karras
// rule, the outward rounding and the arrival step of a bottom-up refit.  trimesh.hip builds the plain set (one BVH2 over
// every triangle, rebuilt by every pose); trimesh_parts.hip builds the set in parts (one subtree per mesh under a small
// top tree; a pose refits).  Kernels read either through trimesh_dev.h alone.
#pragma once
#include <math.h>
#include "common.h"
#include "phys_dev.h"
#include "bp_grid.h"
#include "trimesh_dev.h"

struct clapgpu_trimesh {
    uint32_t n_meshes, n_statics, n_vx, n_tris;
    uint32_t *static_index, *vx_first, *tri_first, *tri_mesh;
    float *vx, *scale, *quat;
    uint16_t *idx;
    double *pos;
    int32_t *static_mesh;                               // [n_statics]: the static's mesh or -1
    double *tri, *stri;                                 // [T][9]: input order (plain set only), leaf order
    uint2 *skey;
    uint64_t *keys[2];                                  // [T] each (plain set only)
    clapgpu::Node *nodes;                               // [max(T - 1, 1)]
    uint32_t *parent;                                   // [T - 1 + T]: of the internal nodes, then of the leaves
    uint32_t *counter, *height;                         // [T - 1] each
    uint64_t *bounds;                                   // [6]: centroid min xyz, max xyz as order keys
    uint32_t *ctl;                                      // [0] check error, [1] tree height; in parts: [2] the deepest
                                                        // part's height, [3] the sticky flags of clapgpu_trimesh_pose_meshes
    void *sort_tmp;
    size_t sort_bytes;
    // ---- a set in parts (trimesh_parts.hip); all zero in a plain set
    uint32_t parts;                                     // 1: in parts
    uint32_t n_parts, top_height, part_height;          // P; ceil(log2 P); the deepest part's (fixed at creation)
    uint32_t mesh_bits;                                 // bits of a mesh index in a top key
    uint32_t *slot_tri;                                 // [T]: the input triangle baked into each leaf slot
    uint32_t *part_root, *part_mesh;                    // [M]: the part's root link or TM_NONE; [P]: the parts' meshes
    float *part_box;                                    // [M][6]: the part's root box
    uint32_t *top_leaf;                                 // [P]: sorted position -> its top node | side << 31
    uint64_t *top_keys[2];                              // [P] each
    uint32_t *stamp;                                    // [M]: lowest list position of a listed mesh, else TM_NONE
};

namespace clapgpu {

constexpr int TB = 256;                                 // set-up kernels
constexpr uint32_t TM_NONE = 0xffffffffu;               // no parent (a subtree's root), no part, not listed

// trimesh.hip: the one creation path (arguments, ranges, copies, k_tm_check) of both kinds of set
__attribute__((visibility("hidden"))) int trimesh_create(void *stream, clapgpu_trimesh **out, const clapgpu_trimesh_desc *d,
                                                         bool parts);
// trimesh_parts.hip: what creation, the full pose and destroy do for a set in parts
__attribute__((visibility("hidden"))) int parts_build(hipStream_t s, clapgpu_trimesh *m, const uint32_t *host_tri_first);
__attribute__((visibility("hidden"))) int parts_pose_all(hipStream_t s, clapgpu_trimesh *m);
__attribute__((visibility("hidden"))) void parts_free(clapgpu_trimesh *m);

template <typename T> static int dev_alloc(T *&p, size_t n)
{
    CLAPGPU_HIP(hipMalloc(reinterpret_cast<void **>(&p), (n ? n : 1) * sizeof(T)));
    return CLAPGPU_OK;
}

// mat4x4_scale_aniso(identity, s, s, s) then mat4x4_mul_vec4 on (x, y, z, 1): each row from 0.f plus the four
// products in order, then vec3_scale by 1 / w
__device__ __forceinline__ void scaled(float s, const float *v, double (&o)[3])
{
    const float v4[4] = { v[0], v[1], v[2], 1.0f };
    float r[4];
    for (int j = 0; j < 4; j++) {
        r[j] = 0.f;
        for (int i = 0; i < 4; i++) r[j] += (i == j ? (j < 3 ? s : 1.0f) : 0.0f) * v4[i];
    }
    const float w = 1.0f / r[3];
    for (int j = 0; j < 3; j++) o[j] = r[j] * w;
}

// triangle t of mesh m in world space: R * scaled(v) + pos in fp64, R = dQtoR(w, x, y, z)
__device__ __forceinline__ void bake_tri(uint32_t t, uint32_t m, const uint32_t *vx_first, const float *vx, const uint16_t *idx,
                                         const float *scale, const double *pos, const float *quat, double (&w)[9])
{
    const double q[4] = { quat[4 * (size_t)m + 3], quat[4 * (size_t)m], quat[4 * (size_t)m + 1], quat[4 * (size_t)m + 2] };
    double R[12];
    phd::q_to_R(q, R);
    const double p[3] = { pos[3 * (size_t)m], pos[3 * (size_t)m + 1], pos[3 * (size_t)m + 2] };
    const float s = scale[m];
    for (int k = 0; k < 3; k++) {
        const float *v = vx + 3 * ((size_t)vx_first[m] + idx[3 * (size_t)t + k]);
        double ms[3];
        scaled(s, v, ms);
        for (int a = 0; a < 3; a++)
            w[3 * k + a] = R[4 * a] * ms[0] + R[4 * a + 1] * ms[1] + R[4 * a + 2] * ms[2] + p[a];
    }
}

// the bounds of one point per thread (NaN coordinates left out): the wave's, then the workgroup's in LDS, then one atomic
// per workgroup and side on bounds[6] (min xyz, max xyz as order keys).  Every thread of the TB-wide workgroup calls it.
__device__ __forceinline__ void block_bounds(const double (&c)[3], uint64_t *bounds)
{
    __shared__ double red[TB / WAVE][6];
    const int wv = threadIdx.x / WAVE;
    for (int a = 0; a < 3; a++) {
        double lo = c[a] == c[a] ? c[a] : INFINITY, hi = c[a] == c[a] ? c[a] : -INFINITY;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = fmin(lo, __shfl_xor(lo, o));
            hi = fmax(hi, __shfl_xor(hi, o));
        }
        if (lane_id() == 0) { red[wv][a] = lo; red[wv][3 + a] = hi; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        double lo = red[0][a], hi = red[0][3 + a];
        for (int k = 1; k < TB / WAVE; k++) { lo = fmin(lo, red[k][a]); hi = fmax(hi, red[k][3 + a]); }
        if (lo <= hi) {
            atomicMin((unsigned long long *)&bounds[a], (unsigned long long)order_key(lo));
            atomicMax((unsigned long long *)&bounds[3 + a], (unsigned long long)order_key(hi));
        }
    }
}

__device__ __forceinline__ uint32_t spread10(uint32_t x)                // 10 bits -> every third bit
{
    x &= 0x3ffu;
    x = (x | (x << 16)) & 0x030000ffu;
    x = (x | (x << 8)) & 0x0300f00fu;
    x = (x | (x << 4)) & 0x030c30c3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// 30-bit Morton code of c within bounds[6] (order keys; bounds[0] all ones: no point was counted, code 0)
__device__ __forceinline__ uint32_t morton30(const double (&c)[3], const uint64_t *bounds)
{
    uint32_t code = 0;
    if (bounds[0] != ~0ull) {
        for (int a = 0; a < 3; a++) {
            const double lo = order_value(bounds[a]), hi = order_value(bounds[3 + a]);
            double f = hi > lo ? (c[a] - lo) / (hi - lo) : 0.0;
            f = f >= 0.0 ? (f <= 1.0 ? f : 1.0) : 0.0;  // NaN: 0
            const uint32_t q = (uint32_t)fmin(f * 1024.0, 1023.0);
            code |= spread10(q) << (2 - a);
        }
    }
    return code;
}

__device__ __forceinline__ int delta(const uint64_t *k, int64_t T, int64_t i, int64_t j)
{
    return (j < 0 || j >= T) ? -1 : __clzll((long long)(k[i] ^ k[j]));
}

// Karras 2012, "Maximizing parallelism in the construction of BVHs, octrees, and k-d trees": internal node i of the n - 1
// over n sorted distinct keys covers [lo, hi] and splits after g (children: g when lo == g it is leaf g, g + 1 likewise)
__device__ __forceinline__ void karras_node(const uint64_t *k, int64_t n, int64_t i, int64_t &lo, int64_t &hi, int64_t &g)
{
    const int d = delta(k, n, i, i + 1) - delta(k, n, i, i - 1) >= 0 ? 1 : -1;
    const int dmin = delta(k, n, i, i - d);
    int64_t lmax = 2;
    while (delta(k, n, i, i + lmax * d) > dmin) lmax <<= 1;
    int64_t l = 0;
    for (int64_t t = lmax >> 1; t >= 1; t >>= 1)
        if (delta(k, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = delta(k, n, i, j);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(k, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    g = i + s * d + (d < 0 ? -1 : 0);
    lo = i < j ? i : j;
    hi = i < j ? j : i;
}

__device__ __forceinline__ float round_down(double d)
{
    float f = (float)d;
    if ((double)f > d) f = nextafterf(f, -INFINITY);
    return f;
}

__device__ __forceinline__ float round_up(double d)
{
    float f = (float)d;
    if ((double)f < d) f = nextafterf(f, INFINITY);
    return f;
}

// a triangle's box (min xyz, max xyz), rounded outward
__device__ __forceinline__ void leaf_box(const double *v, float (&b)[6])
{
    for (int a = 0; a < 3; a++) {
        b[a] = round_down(fmin(fmin(v[a], v[3 + a]), v[6 + a]));
        b[3 + a] = round_up(fmax(fmax(v[a], v[3 + a]), v[6 + a]));
    }
}

__device__ __forceinline__ float load_agent(const float *p)
{
    return __uint_as_float(__hip_atomic_load(reinterpret_cast<const uint32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

} // namespace clapgpu
