// trimesh.hip -- the triangle meshes of static trimesh geoms on the device, for gfx950: the mesh set, its bake and its
// BVH.  The kernels that read the set are elsewhere: ray casts in ray_trimesh.hip (k_ray_trimesh), contacts and the capsule
// sweep in contacts.hip, all through trimesh_dev.h (the node layout, the MeshSet view, the walk).
//
//   k_tm_check      the index check of clapgpu_trimesh_create: every vertex index below its mesh's vertex count, every
//                   static at most once and in range; fills static -> mesh and triangle -> mesh
//   k_tm_bake       phys_geom_trimesh_new (physics.c:882-930) + the geom's pose: world-space fp64 triangles (72 B each)
//   k_tm_morton     30-bit Morton code of each centroid in the centroids' bounds, the triangle index below it (64-bit key)
//   (rocPRIM)       radix sort of the keys
//   k_tm_gather     the triangles and their (static, triangle of its mesh) in leaf order
//   k_tm_hierarchy  Karras 2012: the binary radix tree over the sorted keys (all distinct: the index breaks ties)
//   k_tm_boxes      bottom-up: each node's two child boxes (float, rounded outward) and its subtree height
// The arithmetic of these (bake, Morton code, Karras rule, rounding) is in trimesh_build.h, shared with trimesh_parts.hip:
// the set "in parts" of clapgpu_trimesh_create_parts, whose pose refits and sorts nothing but its parts.
//
// The mesh: model3d.collision_vx scaled by the entity's scale in float the way mat4x4_scale_aniso + mat4x4_mul_vec4
// compute it (each row starts from 0.f and adds the products, so -0 becomes +0; w == 1), widened to double, then
// R * v + pos in fp64 with R = dQtoR(w, x, y, z) of the entity quaternion and pos the entity position (yoffset is 0 for a
// trimesh).  Triangles are the u16 index triples in order, winding kept (physics.c:898-903).
//
// Tree: one BVH2 over every triangle of every mesh, nodes as trimesh_dev.h lays them out.  The keys are distinct and the
// Morton part leaves the top two bits clear, so the prefix length grows by at least one per level: the height is at most
// 62 (see clapgpu_trimesh_status), within the walk's stack.
#include <string.h>
#include <stdlib.h>
#include <rocprim/device/device_radix_sort.hpp>
#include "trimesh_build.h"

namespace clapgpu {

// ------------------------------------------------------------------------------------------------- set-up kernels
__global__ __launch_bounds__(TB)
void k_tm_check(uint32_t M, uint32_t T, uint32_t n_statics, const uint32_t *static_index, const uint32_t *vx_first,
                const uint32_t *tri_first, const uint16_t *idx, uint32_t *tri_mesh, int32_t *static_mesh, uint32_t *ctl)
{
    const uint32_t t = blockIdx.x * TB + threadIdx.x;
    if (t < T) {
        uint32_t lo = 0, hi = M;                        // the last mesh whose first triangle is <= t (tri_first ascending)
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) / 2;
            if (tri_first[mid] <= t) lo = mid; else hi = mid;
        }
        tri_mesh[t] = lo;
        const uint32_t nv = vx_first[lo + 1] - vx_first[lo];
        for (int c = 0; c < 3; c++)
            if (idx[3 * (size_t)t + c] >= nv) atomicOr(&ctl[0], 1u);
    }
    if (t < M) {
        const uint32_t s = static_index[t];
        if (s >= n_statics) atomicOr(&ctl[0], 2u);
        else if (atomicCAS(&static_mesh[s], -1, (int32_t)t) != -1) atomicOr(&ctl[0], 4u);
    }
}

__global__ __launch_bounds__(TB)
void k_tm_bake(uint32_t T, const uint32_t *tri_mesh, const uint32_t *vx_first, const float *vx, const uint16_t *idx,
               const float *scale, const double *pos, const float *quat, double *tri, uint64_t *bounds)
{
    const uint32_t t = blockIdx.x * TB + threadIdx.x;
    double c[3] = { NAN, NAN, NAN };
    if (t < T) {
        double w[9];
        bake_tri(t, tri_mesh[t], vx_first, vx, idx, scale, pos, quat, w);
        for (int a = 0; a < 9; a++) tri[9 * (size_t)t + a] = w[a];
        for (int a = 0; a < 3; a++) c[a] = (w[a] + w[3 + a] + w[6 + a]) / 3.0;
    }
    block_bounds(c, bounds);                            // the centroids' bounds (NaN centroids left out)
}

__global__ __launch_bounds__(TB)
void k_tm_morton(uint32_t T, const double *tri, const uint64_t *bounds, uint64_t *keys)
{
    const uint32_t t = blockIdx.x * TB + threadIdx.x;
    if (t >= T) return;
    double c[3];
    for (int a = 0; a < 3; a++) c[a] = (tri[9 * (size_t)t + a] + tri[9 * (size_t)t + 3 + a] + tri[9 * (size_t)t + 6 + a]) / 3.0;
    const uint32_t code = morton30(c, bounds);          // every centroid NaN: code 0
    keys[t] = ((uint64_t)code << 32) | t;
}

__global__ __launch_bounds__(TB)
void k_tm_gather(uint32_t T, const uint64_t *keys, const double *tri, const uint32_t *tri_mesh, const uint32_t *tri_first,
                 const uint32_t *static_index, double *stri, uint2 *skey)
{
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= T) return;
    const uint32_t t = (uint32_t)keys[i], m = tri_mesh[t];
    for (int a = 0; a < 9; a++) stri[9 * (size_t)i + a] = tri[9 * (size_t)t + a];
    skey[i] = make_uint2(static_index[m], t - tri_first[m]);
}

// Karras 2012, "Maximizing parallelism in the construction of BVHs, octrees, and k-d trees", internal node i of T - 1
__global__ __launch_bounds__(TB)
void k_tm_hierarchy(uint32_t T, const uint64_t *k, Node *nodes, uint32_t *parent)
{
    const int64_t i = blockIdx.x * (int64_t)TB + threadIdx.x, n = T;
    if (i >= n - 1) return;
    int64_t lo, hi, g;
    karras_node(k, n, i, lo, hi, g);
    const uint32_t c0 = lo == g ? TM_LEAF | (uint32_t)g : (uint32_t)g;
    const uint32_t c1 = hi == g + 1 ? TM_LEAF | (uint32_t)(g + 1) : (uint32_t)(g + 1);
    nodes[i].child[0] = c0;
    nodes[i].child[1] = c1;
    nodes[i].pad[0] = nodes[i].pad[1] = 0;
    parent[(c0 & TM_LEAF) ? (n - 1) + (c0 & ~TM_LEAF) : c0] = (uint32_t)i;
    parent[(c1 & TM_LEAF) ? (n - 1) + (c1 & ~TM_LEAF) : c1] = (uint32_t)i;
}

// one thread per leaf climbs while it is the second child to arrive at a node
__global__ __launch_bounds__(TB)
void k_tm_boxes(uint32_t T, const double *stri, Node *nodes, const uint32_t *parent, uint32_t *counter, uint32_t *height,
                uint32_t *ctl)
{
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= T) return;
    float b[6];
    leaf_box(stri + 9 * (size_t)i, b);
    if (T == 1) {                                       // a root holding the one leaf twice
        for (int a = 0; a < 6; a++) { nodes[0].box[a] = b[a]; nodes[0].box[6 + a] = b[a]; }
        nodes[0].child[0] = nodes[0].child[1] = TM_LEAF;
        nodes[0].pad[0] = nodes[0].pad[1] = 0;
        ctl[1] = 1;
        return;
    }
    uint32_t x = TM_LEAF | i, h = 0, p = parent[(T - 1) + i];
    for (;;) {
        Node &n = nodes[p];
        const int side = n.child[0] == x ? 0 : 1;
        for (int a = 0; a < 6; a++) n.box[6 * side + a] = b[a];
        const uint32_t old = __hip_atomic_fetch_add(&counter[p], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (old == 0) return;                           // the sibling finishes this node
        const uint32_t sib = n.child[1 - side];
        for (int a = 0; a < 3; a++) {
            b[a] = fminf(b[a], load_agent(&n.box[6 * (1 - side) + a]));
            b[3 + a] = fmaxf(b[3 + a], load_agent(&n.box[6 * (1 - side) + 3 + a]));
        }
        const uint32_t hs = (sib & TM_LEAF) ? 0u : __hip_atomic_load(&height[sib], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        h = 1 + (h > hs ? h : hs);
        __hip_atomic_store(&height[p], h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == 0) { ctl[1] = h; return; }
        x = p;
        p = parent[p];
    }
}
// the one place a kernel's view of the set is filled
MeshSet trimesh_set(const clapgpu_trimesh *m)
{
    MeshSet s;
    s.nodes = m->nodes; s.tri = m->stri; s.key = m->skey; s.static_mesh = m->static_mesh;
    s.n_tris = m->n_tris; s.n_statics = m->n_statics;
    return s;
}

// bake + tree from the current poses: the one rebuild path of create and pose
static int build(hipStream_t s, clapgpu_trimesh *m)
{
    const uint32_t T = m->n_tris;
    if (T == 0) return CLAPGPU_OK;
    const dim3 g((T + TB - 1) / TB);
    CLAPGPU_HIP(hipMemsetAsync(m->bounds, 0xff, 3 * sizeof(uint64_t), s));
    CLAPGPU_HIP(hipMemsetAsync(m->bounds + 3, 0, 3 * sizeof(uint64_t), s));
    hipLaunchKernelGGL(k_tm_bake, g, dim3(TB), 0, s, T, m->tri_mesh, m->vx_first, m->vx, m->idx, m->scale, m->pos, m->quat, m->tri,
                       m->bounds);
    CLAPGPU_LAUNCH_CHECK("k_tm_bake");
    hipLaunchKernelGGL(k_tm_morton, g, dim3(TB), 0, s, T, m->tri, m->bounds, m->keys[0]);
    CLAPGPU_LAUNCH_CHECK("k_tm_morton");
    size_t bytes = m->sort_bytes;
    CLAPGPU_HIP(rocprim::radix_sort_keys(m->sort_tmp, bytes, m->keys[0], m->keys[1], T, 0, 62, s));
    hipLaunchKernelGGL(k_tm_gather, g, dim3(TB), 0, s, T, m->keys[1], m->tri, m->tri_mesh, m->tri_first, m->static_index, m->stri,
                       m->skey);
    CLAPGPU_LAUNCH_CHECK("k_tm_gather");
    if (T > 1) {
        CLAPGPU_HIP(hipMemsetAsync(m->counter, 0, (size_t)(T - 1) * sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_tm_hierarchy, dim3((T - 1 + TB - 1) / TB), dim3(TB), 0, s, T, m->keys[1], m->nodes, m->parent);
        CLAPGPU_LAUNCH_CHECK("k_tm_hierarchy");
    }
    hipLaunchKernelGGL(k_tm_boxes, g, dim3(TB), 0, s, T, m->stri, m->nodes, m->parent, m->counter, m->height, m->ctl);
    CLAPGPU_LAUNCH_CHECK("k_tm_boxes");
    return CLAPGPU_OK;
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" void clapgpu_trimesh_destroy(clapgpu_trimesh *m)
{
    if (!m) return;
    void *p[] = { m->static_index, m->vx_first, m->tri_first, m->tri_mesh, m->vx, m->scale, m->quat, m->idx, m->pos,
                  m->static_mesh, m->tri, m->stri, m->skey, m->keys[0], m->keys[1], m->nodes, m->parent, m->counter,
                  m->height, m->bounds, m->ctl, m->sort_tmp };
    for (void *q : p)
        if (q) (void)hipFree(q);
    parts_free(m);
    free(m);
}

// the arguments, the ranges, the copies and the device check of both kinds of set, then the kind's own build
int clapgpu::trimesh_create(void *stream, clapgpu_trimesh **out, const clapgpu_trimesh_desc *d, bool parts)
{
    if (!out || !d) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    *out = nullptr;
    const uint32_t M = d->n_meshes;
    const bool any = d->static_index || d->vx_first || d->tri_first || d->vx || d->idx || d->scale || d->pos || d->quat;
    const bool all = d->static_index && d->vx_first && d->tri_first && d->vx && d->idx && d->scale && d->pos && d->quat;
    if (M == 0 ? any : !all) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (M > 0 && d->n_statics == 0) return CLAPGPU_ERR_INVALID_ARGUMENTS;     // every static_index would be out of range
    hipStream_t s = as_stream(stream);
    clapgpu_trimesh *m = static_cast<clapgpu_trimesh *>(calloc(1, sizeof(clapgpu_trimesh)));
    if (!m) return CLAPGPU_ERR_NOMEM;
    m->n_meshes = M;
    m->n_statics = d->n_statics;
    int rc = CLAPGPU_OK;
#define TRY(x) do { rc = (x); if (rc) { clapgpu_trimesh_destroy(m); return rc; } } while (0)
    uint32_t *hf = static_cast<uint32_t *>(malloc(2 * ((size_t)M + 1) * sizeof(uint32_t)));
    if (!hf) { clapgpu_trimesh_destroy(m); return CLAPGPU_ERR_NOMEM; }
    struct Hold { void *p; ~Hold() { free(p); } } hold{ hf };                  // the ranges live to the end: a set in parts reads them
    hf[0] = hf[M + 1] = 0;
    if (M) {                                                                   // the ranges, on the host: they size everything
        hipError_t e = hipMemcpyAsync(hf, d->vx_first, ((size_t)M + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(hf + M + 1, d->tri_first, ((size_t)M + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { clapgpu_trimesh_destroy(m); return hip_fail(e, "clapgpu_trimesh_create: ranges"); }
    }
    bool ok = hf[0] == 0 && hf[M + 1] == 0;
    for (uint32_t k = 0; k < M && ok; k++) ok = hf[k + 1] >= hf[k] && hf[M + 2 + k] >= hf[M + 1 + k];
    m->n_vx = hf[M];
    m->n_tris = hf[2 * M + 1];
    if (!ok || m->n_tris >= TM_LEAF) { clapgpu_trimesh_destroy(m); return CLAPGPU_ERR_INVALID_ARGUMENTS; }
    const size_t V = m->n_vx, T = m->n_tris;
    TRY(dev_alloc(m->static_index, M)); TRY(dev_alloc(m->vx_first, M + 1)); TRY(dev_alloc(m->tri_first, M + 1));
    TRY(dev_alloc(m->tri_mesh, T)); TRY(dev_alloc(m->vx, 3 * V)); TRY(dev_alloc(m->scale, M)); TRY(dev_alloc(m->quat, 4 * M));
    TRY(dev_alloc(m->idx, 3 * T)); TRY(dev_alloc(m->pos, 3 * M)); TRY(dev_alloc(m->static_mesh, m->n_statics));
    TRY(dev_alloc(m->tri, parts ? 0 : 9 * T)); TRY(dev_alloc(m->stri, 9 * T)); TRY(dev_alloc(m->skey, T));
    TRY(dev_alloc(m->keys[0], parts ? 0 : T)); TRY(dev_alloc(m->keys[1], parts ? 0 : T)); TRY(dev_alloc(m->nodes, T > 1 ? T - 1 : 1));
    TRY(dev_alloc(m->parent, 2 * T)); TRY(dev_alloc(m->counter, T)); TRY(dev_alloc(m->height, T));
    TRY(dev_alloc(m->bounds, 6)); TRY(dev_alloc(m->ctl, 4));
    if (T && !parts) {
        size_t bytes = 0;
        if (rocprim::radix_sort_keys(nullptr, bytes, m->keys[0], m->keys[1], (size_t)T, 0, 62, s) != hipSuccess)
            TRY(CLAPGPU_ERR_UNKNOWN);
        m->sort_bytes = bytes;
        TRY(dev_alloc(reinterpret_cast<uint8_t *&>(m->sort_tmp), bytes));
    }
    auto cp = [&](void *dst, const void *src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) : hipSuccess;
    };
    hipError_t e = hipSuccess;
    if (M) {
        const hipError_t es[] = { cp(m->static_index, d->static_index, M * 4), cp(m->vx_first, d->vx_first, (M + 1) * 4),
                                  cp(m->tri_first, d->tri_first, (M + 1) * 4), cp(m->vx, d->vx, 12 * V), cp(m->idx, d->idx, 6 * T),
                                  cp(m->scale, d->scale, 4 * (size_t)M), cp(m->pos, d->pos, 24 * (size_t)M),
                                  cp(m->quat, d->quat, 16 * (size_t)M) };
        for (hipError_t x : es) if (x != hipSuccess) e = x;
    }
    if (e == hipSuccess && m->n_statics) e = hipMemsetAsync(m->static_mesh, 0xff, (size_t)m->n_statics * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(m->ctl, 0, 4 * sizeof(uint32_t), s);
    if (e != hipSuccess) { clapgpu_trimesh_destroy(m); return hip_fail(e, "clapgpu_trimesh_create: copies"); }
    const size_t nt = T > M ? T : M;
    if (nt) {
        hipLaunchKernelGGL(k_tm_check, dim3((unsigned)((nt + TB - 1) / TB)), dim3(TB), 0, s, M, (uint32_t)T, m->n_statics,
                           m->static_index, m->vx_first, m->tri_first, m->idx, m->tri_mesh, m->static_mesh, m->ctl);
        e = launch_error();
        uint32_t err = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&err, m->ctl, sizeof(err), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { clapgpu_trimesh_destroy(m); return hip_fail(e, "k_tm_check"); }
        if (err) {
            set_last_error(err & 1 ? "clapgpu_trimesh_create: a vertex index at or beyond its mesh's vertex count"
                                   : err & 2 ? "clapgpu_trimesh_create: a static_index out of range"
                                             : "clapgpu_trimesh_create: a static listed twice");
            clapgpu_trimesh_destroy(m);
            return CLAPGPU_ERR_INVALID_ARGUMENTS;
        }
    }
    TRY(parts ? parts_build(s, m, hf + M + 1) : build(s, m));
#undef TRY
    *out = m;
    return CLAPGPU_OK;
}

extern "C" int clapgpu_trimesh_create(void *stream, clapgpu_trimesh **out, const clapgpu_trimesh_desc *d)
{
    return trimesh_create(stream, out, d, false);
}

extern "C" int clapgpu_trimesh_pose(void *stream, clapgpu_trimesh *m, const double *pos, const float *quat)
{
    if (!m || (m->n_meshes && (!pos || !quat))) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    hipStream_t s = as_stream(stream);
    if (m->n_meshes == 0) return m->parts ? parts_pose_all(s, m) : CLAPGPU_OK;
    CLAPGPU_HIP(hipMemcpyAsync(m->pos, pos, 24 * (size_t)m->n_meshes, hipMemcpyDeviceToDevice, s));
    CLAPGPU_HIP(hipMemcpyAsync(m->quat, quat, 16 * (size_t)m->n_meshes, hipMemcpyDeviceToDevice, s));
    return m->parts ? parts_pose_all(s, m) : build(s, m);
}

extern "C" int clapgpu_trimesh_status(void *stream, const clapgpu_trimesh *m, uint32_t *depth, uint32_t *n_tris)
{
    if (!m || !depth || !n_tris) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    *n_tris = m->n_tris;
    *depth = 0;
    if (m->n_tris == 0) return CLAPGPU_OK;
    hipStream_t s = as_stream(stream);
    if (m->parts) {                                     // top plus deepest part: both fixed at creation
        CLAPGPU_HIP(hipStreamSynchronize(s));
        *depth = m->top_height + m->part_height;
        return CLAPGPU_OK;
    }
    CLAPGPU_HIP(hipMemcpyAsync(depth, m->ctl + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    CLAPGPU_HIP(hipStreamSynchronize(s));
    return CLAPGPU_OK;
}
