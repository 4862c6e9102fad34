// trimesh_parts.hip -- the mesh set "in parts" (clapgpu_trimesh_create_parts), for gfx950: the same node array, leaf
// slots and view as the plain set of trimesh.hip (trimesh_dev.h; the kernels that walk it cannot tell the two apart), built
// so that a pose moves no leaf and no link of a mesh: a moving mesh costs a re-bake and a refit of its own triangles
// and a rebuild of a tree over the parts, not a sort of every triangle of the set.
//
// Layout (P parts = meshes with a triangle, T triangles, T - 1 nodes, the root at node 0):
//   nodes [0, P - 1)        the top tree: balanced over the parts in sorted order, in preorder (a node covering
//                           [lo, hi) splits at s = lo + (hi - lo + 1) / 2; its left child is the next node, its right
//                           child s - lo nodes on).  Its SHAPE depends on P alone; a pose changes which part hangs
//                           where and the boxes.  Height ceil(log2 P).
//   nodes [P - 1, T - 1)    the parts in mesh order: mesh m with k >= 2 triangles owns k - 1 nodes from
//                           part_root[m] = (P - 1) + tri_first[m] - (parts before m), a Karras tree whose root is the
//                           first of them.  A part of one triangle owns no node: its root is the leaf link.
//   leaf slots              mesh m's are [tri_first[m], tri_first[m + 1]), ordered by the key of the UNPOSED mesh (30-bit
//                           Morton code of the scaled model-space centroid in the mesh's own centroid bounds, the
//                           triangle's index below it): fixed at creation, like the links and the part's height.
//
//   creation    k_tp_model_bounds, k_tp_model_keys, (rocPRIM pairs sort by mesh and code), k_tp_slots, k_tp_hierarchy,
//               k_tp_top_shape, then the refit below for every mesh
//   refit       k_tp_bake_refit   one thread per leaf slot of a listed mesh: bakes its triangle, climbs its part (the
//                                 second arriver at a node goes on and re-arms the node's counter), hands the root box on
//               k_tp_centres, k_tp_top_keys, (rocPRIM keys sort of P keys), k_tp_top_refit: the top tree's links and boxes
//   listing     k_tp_fill (the stamps; no memset on a pose path), k_tp_mark, k_tp_take: the lowest list position of a mesh wins (an atomicMin stamp), its pose is taken
//
// Determinism: a node's box is min / max of its children's in child order whoever arrives last, the bounds are atomic
// min / max, the sorts are of distinct keys: the image is a function of the descriptor and the poses.
#include <string.h>
#include <stdlib.h>
#include <vector>
#include <rocprim/device/device_radix_sort.hpp>
#include "trimesh_build.h"

namespace clapgpu {

// ------------------------------------------------------------------------------------------------- creation
// the centroid of triangle t of mesh m, scaled and unposed (model space)
__device__ __forceinline__ void model_centroid(uint32_t t, uint32_t m, const uint32_t *vx_first, const float *vx,
                                               const uint16_t *idx, const float *scale, double (&c)[3])
{
    const float s = scale[m];
    double ms[3];
    for (int k = 0; k < 3; k++) {
        scaled(s, vx + 3 * ((size_t)vx_first[m] + idx[3 * (size_t)t + k]), ms);
        for (int a = 0; a < 3; a++) c[a] = k == 0 ? ms[a] : c[a] + ms[a];
    }
    for (int a = 0; a < 3; a++) c[a] = c[a] / 3.0;
}

// per mesh: the bounds of its triangles' model-space centroids (NaN coordinates left out).  A wavefront whose lanes
// all belong to one mesh (nearly all of a large mesh's) reduces first and makes one atomic per side; the others make
// theirs per lane.  Min and max do not depend on the order, so neither do the bounds.
__global__ __launch_bounds__(TB)
void k_tp_model_bounds(uint32_t T, const uint32_t *tri_mesh, const uint32_t *vx_first, const float *vx, const uint16_t *idx,
                       const float *scale, uint64_t *mbounds)
{
    const uint32_t t = blockIdx.x * TB + threadIdx.x;
    const bool live = t < T;
    const uint32_t m = live ? tri_mesh[t] : TM_NONE;
    double c[3] = { NAN, NAN, NAN };
    if (live) model_centroid(t, m, vx_first, vx, idx, scale, c);
    const uint32_t m0 = __shfl(m, 0);                   // lane 0 is live in every wavefront that has a live lane
    const bool one = __all(m == m0 || !live);
    for (int a = 0; a < 3; a++) {
        double lo = c[a] == c[a] ? c[a] : INFINITY, hi = c[a] == c[a] ? c[a] : -INFINITY;
        if (one) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                lo = fmin(lo, __shfl_xor(lo, o));
                hi = fmax(hi, __shfl_xor(hi, o));
            }
        }
        if (live && lo <= hi && (!one || lane_id() == 0)) {
            atomicMin((unsigned long long *)&mbounds[6 * (size_t)m + a], (unsigned long long)order_key(lo));
            atomicMax((unsigned long long *)&mbounds[6 * (size_t)m + 3 + a], (unsigned long long)order_key(hi));
        }
    }
}

// the creation sort's key (mesh, code) and value (the triangle): the sort is stable, so equal codes keep triangle order
__global__ __launch_bounds__(TB)
void k_tp_model_keys(uint32_t T, const uint32_t *tri_mesh, const uint32_t *vx_first, const float *vx, const uint16_t *idx,
                     const float *scale, const uint64_t *mbounds, uint64_t *keys, uint32_t *vals)
{
    const uint32_t t = blockIdx.x * TB + threadIdx.x;
    if (t >= T) return;
    const uint32_t m = tri_mesh[t];
    double c[3];
    model_centroid(t, m, vx_first, vx, idx, scale, c);
    keys[t] = ((uint64_t)m << 30) | morton30(c, mbounds + 6 * (size_t)m);
    vals[t] = t;
}

// leaf slot i: its Karras key within the part (code, triangle of its mesh) and what the kernels read of it
__global__ __launch_bounds__(TB)
void k_tp_slots(uint32_t T, const uint64_t *sorted, const uint32_t *slot_tri, const uint32_t *tri_mesh, const uint32_t *tri_first,
                const uint32_t *static_index, uint64_t *pkey, uint2 *skey)
{
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= T) return;
    const uint32_t t = slot_tri[i], m = tri_mesh[i];    // slots and triangles of a mesh share their range
    pkey[i] = ((sorted[i] & 0x3fffffffull) << 32) | (t - tri_first[m]);
    skey[i] = make_uint2(static_index[m], t - tri_first[m]);
}

// the Karras rule (trimesh_build.h) within each part: slot i is inner node i - first of its part's k - 1
__global__ __launch_bounds__(TB)
void k_tp_hierarchy(uint32_t T, const uint64_t *pkey, const uint32_t *tri_mesh, const uint32_t *tri_first,
                    const uint32_t *part_root, Node *nodes, uint32_t *parent)
{
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= T) return;
    const uint32_t m = tri_mesh[i], f = tri_first[m], k = tri_first[m + 1] - f, li = i - f;
    if (li + 1 >= k) return;                            // k - 1 inner nodes; none for a part of one triangle
    int64_t lo, hi, g;
    karras_node(pkey + f, k, li, lo, hi, g);
    const uint32_t base = part_root[m], self = base + li;
    const uint32_t c0 = lo == g ? TM_LEAF | (f + (uint32_t)g) : base + (uint32_t)g;
    const uint32_t c1 = hi == g + 1 ? TM_LEAF | (f + (uint32_t)g + 1) : base + (uint32_t)g + 1;
    nodes[self].child[0] = c0;
    nodes[self].child[1] = c1;
    parent[(c0 & TM_LEAF) ? (size_t)(T - 1) + (c0 & ~TM_LEAF) : c0] = self;
    parent[(c1 & TM_LEAF) ? (size_t)(T - 1) + (c1 & ~TM_LEAF) : c1] = self;
}

// top node j of P - 1 in preorder: its range by descent from the root, its inner links, its children's parents
__global__ __launch_bounds__(TB)
void k_tp_top_shape(uint32_t P, Node *nodes, uint32_t *parent, uint32_t *top_leaf)
{
    const uint32_t j = blockIdx.x * TB + threadIdx.x;
    if (j + 1 >= P) return;
    uint32_t at = 0, lo = 0, hi = P;
    while (at != j) {
        const uint32_t s = lo + (hi - lo + 1) / 2, right = at + (s - lo);
        if (j < right) { at = at + 1; hi = s; }         // (a left leaf: right == at + 1 <= j)
        else { at = right; lo = s; }
    }
    const uint32_t s = lo + (hi - lo + 1) / 2;
    if (s - lo == 1) top_leaf[lo] = j;
    else { nodes[j].child[0] = j + 1; parent[j + 1] = j; }
    if (hi - s == 1) top_leaf[s] = j | TM_LEAF;
    else { nodes[j].child[1] = j + (s - lo); parent[j + (s - lo)] = j; }
}

// ------------------------------------------------------------------------------------------------- refit
// An arrival at node p on `side` with the child's box b (and height h): stores the box, and while this thread is the
// second child to arrive goes on upward with the union, re-arming the counter it passed.  The union is min / max in child
// order, so its bits do not depend on who arrives last.  True at a node without a parent: b (h) are the subtree's.
template <bool HEIGHT>
__device__ __forceinline__ bool refit_climb(Node *nodes, const uint32_t *parent, uint32_t *counter, uint32_t *height,
                                            uint32_t p, int side, float (&b)[6], uint32_t &h)
{
    for (;;) {
        Node &n = nodes[p];
        for (int a = 0; a < 6; a++) n.box[6 * side + a] = b[a];
        const uint32_t old = __hip_atomic_fetch_add(&counter[p], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (old == 0) return false;                     // the sibling finishes this node
        __hip_atomic_store(&counter[p], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // both came: armed for the next refit
        float o[6];
        for (int a = 0; a < 6; a++) o[a] = load_agent(&n.box[6 * (1 - side) + a]);
        for (int a = 0; a < 3; a++) {
            b[a] = side == 0 ? fminf(b[a], o[a]) : fminf(o[a], b[a]);
            b[3 + a] = side == 0 ? fmaxf(b[3 + a], o[3 + a]) : fmaxf(o[3 + a], b[3 + a]);
        }
        if (HEIGHT) {
            const uint32_t sib = n.child[1 - side];
            const uint32_t hs = (sib & TM_LEAF) ? 0u : __hip_atomic_load(&height[sib], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            h = 1 + (h > hs ? h : hs);
            __hip_atomic_store(&height[p], h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const uint32_t up = parent[p];
        if (up == TM_NONE) return true;
        side = nodes[up].child[0] == p ? 0 : 1;
        p = up;
    }
}

// leaf slot i of a listed mesh (stamp NULL: of every mesh): bake, the part's boxes, the root box handed to the top pass
__global__ __launch_bounds__(TB)
void k_tp_bake_refit(uint32_t T, const uint32_t *tri_mesh, const uint32_t *slot_tri, const uint32_t *vx_first, const float *vx,
                     const uint16_t *idx, const float *scale, const double *pos, const float *quat, const uint32_t *stamp,
                     double *stri, Node *nodes, const uint32_t *parent, uint32_t *counter, uint32_t *height, float *part_box,
                     uint32_t *ctl, uint64_t *bounds)
{
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= T) return;
    if (i == 0)                                         // the centres' bounds for the top pass: none yet
        for (int a = 0; a < 3; a++) { bounds[a] = ~0ull; bounds[3 + a] = 0; }
    const uint32_t m = tri_mesh[i];
    if (stamp && stamp[m] == TM_NONE) return;           // not listed: neither read nor written
    double w[9];
    bake_tri(slot_tri[i], m, vx_first, vx, idx, scale, pos, quat, w);
    for (int a = 0; a < 9; a++) stri[9 * (size_t)i + a] = w[a];
    float b[6];
    leaf_box(w, b);
    if (T == 1) {                                       // a root holding the one leaf twice
        for (int a = 0; a < 6; a++) { nodes[0].box[a] = b[a]; nodes[0].box[6 + a] = b[a]; }
        nodes[0].child[0] = nodes[0].child[1] = TM_LEAF;
        ctl[2] = 1;
        return;
    }
    const uint32_t p = parent[(size_t)(T - 1) + i];
    uint32_t h = 0;
    if (p == TM_NONE || refit_climb<true>(nodes, parent, counter, height, p, nodes[p].child[0] == (TM_LEAF | i) ? 0 : 1, b, h)) {
        for (int a = 0; a < 6; a++) part_box[6 * (size_t)m + a] = b[a];
        atomicMax(&ctl[2], h);
    }
}

// the centre of a part's root box; any NaN coordinate: no centre
__device__ __forceinline__ bool part_centre(const float *b, double (&c)[3])
{
    for (int a = 0; a < 3; a++) c[a] = ((double)b[a] + (double)b[3 + a]) * 0.5;
    const bool ok = c[0] == c[0] && c[1] == c[1] && c[2] == c[2];
    if (!ok) c[0] = c[1] = c[2] = NAN;
    return ok;
}

__global__ __launch_bounds__(TB)
void k_tp_centres(uint32_t P, const uint32_t *part_mesh, const float *part_box, uint64_t *bounds)
{
    const uint32_t q = blockIdx.x * TB + threadIdx.x;
    double c[3] = { NAN, NAN, NAN };
    if (q < P) part_centre(part_box + 6 * (size_t)part_mesh[q], c);
    block_bounds(c, bounds);
}

// a part's key: the code of its centre in the centres' bounds (no centre: 0), its mesh below it
__global__ __launch_bounds__(TB)
void k_tp_top_keys(uint32_t P, uint32_t mesh_bits, const uint32_t *part_mesh, const float *part_box, const uint64_t *bounds,
                   uint64_t *keys)
{
    const uint32_t q = blockIdx.x * TB + threadIdx.x;
    if (q >= P) return;
    const uint32_t m = part_mesh[q];
    double c[3];
    const uint32_t code = part_centre(part_box + 6 * (size_t)m, c) ? morton30(c, bounds) : 0u;
    keys[q] = ((uint64_t)code << mesh_bits) | m;
}

// sorted position p: hangs its part under its top node and climbs the top tree
__global__ __launch_bounds__(TB)
void k_tp_top_refit(uint32_t P, uint32_t mesh_bits, const uint64_t *sorted, const uint32_t *part_root, const float *part_box,
                    const uint32_t *top_leaf, Node *nodes, const uint32_t *parent, uint32_t *counter)
{
    const uint32_t p = blockIdx.x * TB + threadIdx.x;
    if (p >= P) return;
    const uint32_t m = (uint32_t)(sorted[p] & ((1ull << mesh_bits) - 1));
    const uint32_t at = top_leaf[p] & ~TM_LEAF;
    const int side = top_leaf[p] >> 31;
    float b[6];
    for (int a = 0; a < 6; a++) b[a] = part_box[6 * (size_t)m + a];
    nodes[at].child[side] = part_root[m];
    uint32_t h = 0;
    refit_climb<false>(nodes, parent, counter, nullptr, at, side, b, h);
}

// ------------------------------------------------------------------------------------------------- listing
// In place of hipMemsetAsync on the pose paths.  Observed once (ROCm 7.2, torch's stream capture, gfx950): with the stamps
// and the bounds set by captured 0xff memsets, a graph's first replay left the direct call's image and its second did
// not (the TWICE flag came up, so the stamps of the replay before were still there; the top nodes differed).  With
// kernels in their place both replays do.  That the memset nodes are the cause is a supposition: no stand-alone
// reproducer was made, and the order of memset and kernel nodes on the captured stream was not examined.
__global__ __launch_bounds__(TB)
void k_tp_fill(uint32_t n, uint32_t *p, uint32_t v)
{
    const uint32_t k = blockIdx.x * TB + threadIdx.x;
    if (k < n) p[k] = v;
}

__global__ __launch_bounds__(TB)
void k_tp_mark(uint32_t n, uint32_t M, const uint32_t *mesh, uint32_t *stamp, uint32_t *ctl)
{
    const uint32_t k = blockIdx.x * TB + threadIdx.x;
    if (k >= n) return;
    const uint32_t m = mesh[k];
    if (m >= M) atomicOr(&ctl[3], CLAPGPU_TRIMESH_POSE_RANGE);
    else if (atomicMin(&stamp[m], k) != TM_NONE) atomicOr(&ctl[3], CLAPGPU_TRIMESH_POSE_TWICE);
}

__global__ __launch_bounds__(TB)
void k_tp_take(uint32_t n, uint32_t M, const uint32_t *mesh, const uint32_t *stamp, const double *pos_in, const float *quat_in,
               double *pos, float *quat)
{
    const uint32_t k = blockIdx.x * TB + threadIdx.x;
    if (k >= n) return;
    const uint32_t m = mesh[k];
    if (m >= M || stamp[m] != k) return;
    for (int a = 0; a < 3; a++) pos[3 * (size_t)m + a] = pos_in[3 * (size_t)k + a];
    for (int a = 0; a < 4; a++) quat[4 * (size_t)m + a] = quat_in[4 * (size_t)k + a];
}

// ------------------------------------------------------------------------------------------------- host
static dim3 grid(size_t n) { return dim3((unsigned)((n + TB - 1) / TB)); }

// the listed meshes' triangles and parts (stamp NULL: every mesh's), then the top tree
static int refit(hipStream_t s, clapgpu_trimesh *m, const uint32_t *stamp)
{
    const uint32_t T = m->n_tris, P = m->n_parts;
    if (T == 0) return CLAPGPU_OK;
    hipLaunchKernelGGL(k_tp_bake_refit, grid(T), dim3(TB), 0, s, T, m->tri_mesh, m->slot_tri, m->vx_first, m->vx, m->idx, m->scale,
                       m->pos, m->quat, stamp, m->stri, m->nodes, m->parent, m->counter, m->height, m->part_box, m->ctl,
                       m->bounds);
    CLAPGPU_LAUNCH_CHECK("k_tp_bake_refit");
    if (P < 2) return CLAPGPU_OK;                       // node 0 is the one part's root
    hipLaunchKernelGGL(k_tp_centres, grid(P), dim3(TB), 0, s, P, m->part_mesh, m->part_box, m->bounds);
    CLAPGPU_LAUNCH_CHECK("k_tp_centres");
    hipLaunchKernelGGL(k_tp_top_keys, grid(P), dim3(TB), 0, s, P, m->mesh_bits, m->part_mesh, m->part_box, m->bounds, m->top_keys[0]);
    CLAPGPU_LAUNCH_CHECK("k_tp_top_keys");
    size_t bytes = m->sort_bytes;
    CLAPGPU_HIP(rocprim::radix_sort_keys(m->sort_tmp, bytes, m->top_keys[0], m->top_keys[1], P, 0, 30 + m->mesh_bits, s));
    hipLaunchKernelGGL(k_tp_top_refit, grid(P), dim3(TB), 0, s, P, m->mesh_bits, m->top_keys[1], m->part_root, m->part_box,
                       m->top_leaf, m->nodes, m->parent, m->counter);
    CLAPGPU_LAUNCH_CHECK("k_tp_top_refit");
    return CLAPGPU_OK;
}

static uint32_t ceil_log2(uint32_t v)
{
    uint32_t h = 0;
    while (h < 32 && (1ull << h) < v) h++;
    return h;
}

int parts_build(hipStream_t s, clapgpu_trimesh *m, const uint32_t *tf)
{
    const uint32_t M = m->n_meshes, T = m->n_tris;
    m->parts = 1;
    std::vector<uint32_t> root(M ? M : 1, TM_NONE), pmesh;
    for (uint32_t k = 0; k < M; k++)
        if (tf[k + 1] > tf[k]) pmesh.push_back(k);
    const uint32_t P = (uint32_t)pmesh.size();
    for (uint32_t q = 0; q < P; q++) {
        const uint32_t k = pmesh[q], n = tf[k + 1] - tf[k];
        root[k] = n == 1 ? TM_LEAF | tf[k] : (P - 1) + tf[k] - q;
    }
    m->n_parts = P;
    m->top_height = ceil_log2(P);
    m->mesh_bits = bits_of(M ? M - 1 : 0);
    CLAPGPU_HIP(hipMemsetAsync(m->nodes, 0, (T > 1 ? (size_t)T - 1 : 1) * sizeof(Node), s));
    if (int rc = dev_alloc(m->slot_tri, T)) return rc;
    if (int rc = dev_alloc(m->part_root, M)) return rc;
    if (int rc = dev_alloc(m->part_mesh, P)) return rc;
    if (int rc = dev_alloc(m->part_box, 6 * (size_t)M)) return rc;
    if (int rc = dev_alloc(m->top_leaf, P)) return rc;
    if (int rc = dev_alloc(m->top_keys[0], P)) return rc;
    if (int rc = dev_alloc(m->top_keys[1], P)) return rc;
    if (int rc = dev_alloc(m->stamp, M)) return rc;
    if (M) CLAPGPU_HIP(hipMemcpy(m->part_root, root.data(), (size_t)M * 4, hipMemcpyHostToDevice));
    if (P) CLAPGPU_HIP(hipMemcpy(m->part_mesh, pmesh.data(), (size_t)P * 4, hipMemcpyHostToDevice));
    if (T == 0) {
        CLAPGPU_HIP(hipStreamSynchronize(s));
        return CLAPGPU_OK;
    }
    size_t bytes = 0;                                   // the pose's sort of the P part keys: sized and allocated here
    if (rocprim::radix_sort_keys(nullptr, bytes, m->top_keys[0], m->top_keys[1], (size_t)P, 0, 30 + m->mesh_bits, s) != hipSuccess)
        return CLAPGPU_ERR_UNKNOWN;
    m->sort_bytes = bytes;
    if (int rc = dev_alloc(reinterpret_cast<uint8_t *&>(m->sort_tmp), bytes)) return rc;

    // creation's own temporaries: the per-mesh bounds, the sort's values and storage
    uint64_t *mbounds = nullptr, *key[2] = { nullptr, nullptr };       // key[0]: the sort's input, then the parts' Karras keys
    uint32_t *vals = nullptr;
    void *tmp = nullptr;
    struct Free {
        uint64_t *&a, *&k0, *&k1; uint32_t *&b; void *&c;
        ~Free() { (void)hipFree(a); (void)hipFree(k0); (void)hipFree(k1); (void)hipFree(b); (void)hipFree(c); }
    } hold{ mbounds, key[0], key[1], vals, tmp };
    if (int rc = dev_alloc(mbounds, 6 * (size_t)M)) return rc;
    if (int rc = dev_alloc(key[0], T)) return rc;
    if (int rc = dev_alloc(key[1], T)) return rc;
    if (int rc = dev_alloc(vals, T)) return rc;
    const int end_bit = 30 + (int)m->mesh_bits;
    size_t cbytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, cbytes, key[0], key[1], vals, m->slot_tri, (size_t)T, 0, end_bit, s) != hipSuccess)
        return CLAPGPU_ERR_UNKNOWN;
    if (int rc = dev_alloc(reinterpret_cast<uint8_t *&>(tmp), cbytes)) return rc;

    CLAPGPU_HIP(hipMemsetAsync(m->parent, 0xff, 2 * (size_t)T * sizeof(uint32_t), s));
    CLAPGPU_HIP(hipMemsetAsync(m->counter, 0, (size_t)T * sizeof(uint32_t), s));
    CLAPGPU_HIP(hipMemsetAsync(mbounds, 0, 6 * (size_t)M * sizeof(uint64_t), s));       // per mesh: min keys all ones, max keys zero
    CLAPGPU_HIP(hipMemset2DAsync(mbounds, 6 * sizeof(uint64_t), 0xff, 3 * sizeof(uint64_t), M, s));
    hipLaunchKernelGGL(k_tp_model_bounds, grid(T), dim3(TB), 0, s, T, m->tri_mesh, m->vx_first, m->vx, m->idx, m->scale, mbounds);
    CLAPGPU_LAUNCH_CHECK("k_tp_model_bounds");
    hipLaunchKernelGGL(k_tp_model_keys, grid(T), dim3(TB), 0, s, T, m->tri_mesh, m->vx_first, m->vx, m->idx, m->scale, mbounds,
                       key[0], vals);
    CLAPGPU_LAUNCH_CHECK("k_tp_model_keys");
    CLAPGPU_HIP(rocprim::radix_sort_pairs(tmp, cbytes, key[0], key[1], vals, m->slot_tri, (size_t)T, 0, end_bit, s));
    hipLaunchKernelGGL(k_tp_slots, grid(T), dim3(TB), 0, s, T, key[1], m->slot_tri, m->tri_mesh, m->tri_first, m->static_index,
                       key[0], m->skey);
    CLAPGPU_LAUNCH_CHECK("k_tp_slots");
    if (T > 1) {
        hipLaunchKernelGGL(k_tp_hierarchy, grid(T), dim3(TB), 0, s, T, key[0], m->tri_mesh, m->tri_first, m->part_root, m->nodes,
                           m->parent);
        CLAPGPU_LAUNCH_CHECK("k_tp_hierarchy");
    }
    if (P > 1) {
        hipLaunchKernelGGL(k_tp_top_shape, grid(P - 1), dim3(TB), 0, s, P, m->nodes, m->parent, m->top_leaf);
        CLAPGPU_LAUNCH_CHECK("k_tp_top_shape");
    }
    if (int rc = refit(s, m, nullptr)) return rc;
    uint32_t deepest = 0;
    CLAPGPU_HIP(hipMemcpyAsync(&deepest, m->ctl + 2, sizeof(deepest), hipMemcpyDeviceToHost, s));
    CLAPGPU_HIP(hipStreamSynchronize(s));
    m->part_height = deepest;
    // The walk's stack holds TM_STACK = 64 entries and bvh_walk drops a push beyond it without a word, so a taller tree
    // would answer wrongly: the plain set's bound of 62 edges holds here too.  A part's height is at most 62 by its keys
    // (trimesh.hip), the top adds ceil(log2 P): only some 2^20 parts above a degenerate part get there.  Neither height
    // depends on a pose, so this is the one place the bound is checked.
    if (m->top_height + m->part_height > 62) {
        set_last_error("clapgpu_trimesh_create_parts: the tree (top plus deepest part) is more than 62 high");
        return CLAPGPU_ERR_TOO_LARGE;
    }
    return CLAPGPU_OK;
}

int parts_pose_all(hipStream_t s, clapgpu_trimesh *m)
{
    // the sticky flags, and whatever a pose that failed half-way left armed
    hipLaunchKernelGGL(k_tp_fill, grid(1), dim3(TB), 0, s, 1u, m->ctl + 3, 0u);
    CLAPGPU_LAUNCH_CHECK("k_tp_fill");
    if (m->n_tris == 0) return CLAPGPU_OK;
    hipLaunchKernelGGL(k_tp_fill, grid(m->n_tris), dim3(TB), 0, s, m->n_tris, m->counter, 0u);
    CLAPGPU_LAUNCH_CHECK("k_tp_fill");
    return refit(s, m, nullptr);
}

void parts_free(clapgpu_trimesh *m)
{
    void *p[] = { m->slot_tri, m->part_root, m->part_mesh, m->part_box, m->top_leaf, m->top_keys[0], m->top_keys[1], m->stamp };
    for (void *q : p)
        if (q) (void)hipFree(q);
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" int clapgpu_trimesh_create_parts(void *stream, clapgpu_trimesh **out, const clapgpu_trimesh_desc *d)
{
    return trimesh_create(stream, out, d, true);
}

extern "C" int clapgpu_trimesh_pose_meshes(void *stream, clapgpu_trimesh *m, uint32_t n_moved, const uint32_t *mesh,
                                           const double *pos, const float *quat)
{
    if (!m || !m->parts) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (n_moved == 0) return CLAPGPU_OK;
    if (!mesh || !pos || !quat) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    hipStream_t s = as_stream(stream);
    const uint32_t M = m->n_meshes;
    if (M) {
        hipLaunchKernelGGL(k_tp_fill, grid(M), dim3(TB), 0, s, M, m->stamp, TM_NONE);
        CLAPGPU_LAUNCH_CHECK("k_tp_fill");
    }
    hipLaunchKernelGGL(k_tp_mark, grid(n_moved), dim3(TB), 0, s, n_moved, M, mesh, m->stamp, m->ctl);
    CLAPGPU_LAUNCH_CHECK("k_tp_mark");
    hipLaunchKernelGGL(k_tp_take, grid(n_moved), dim3(TB), 0, s, n_moved, M, mesh, m->stamp, pos, quat, m->pos, m->quat);
    CLAPGPU_LAUNCH_CHECK("k_tp_take");
    return refit(s, m, m->stamp);
}

extern "C" int clapgpu_trimesh_parts_status(void *stream, const clapgpu_trimesh *m, uint32_t out[4])
{
    if (!m || !out) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    out[0] = m->parts ? 1u : 0u;
    out[1] = m->top_height;
    out[2] = m->part_height;
    out[3] = 0;
    hipStream_t s = as_stream(stream);
    if (m->parts) CLAPGPU_HIP(hipMemcpyAsync(&out[3], m->ctl + 3, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    CLAPGPU_HIP(hipStreamSynchronize(s));
    return CLAPGPU_OK;
}

extern "C" int clapgpu_trimesh_read(void *stream, const clapgpu_trimesh *m, void *nodes, uint32_t *key, double *tri,
                                    uint32_t *part_root)
{
    if (!m || (part_root && !m->parts)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    hipStream_t s = as_stream(stream);
    const size_t T = m->n_tris;
    if (nodes) CLAPGPU_HIP(hipMemcpyAsync(nodes, m->nodes, (T > 1 ? T - 1 : 1) * sizeof(Node), hipMemcpyDeviceToHost, s));
    if (key && T) CLAPGPU_HIP(hipMemcpyAsync(key, m->skey, T * sizeof(uint2), hipMemcpyDeviceToHost, s));
    if (tri && T) CLAPGPU_HIP(hipMemcpyAsync(tri, m->stri, 9 * T * sizeof(double), hipMemcpyDeviceToHost, s));
    if (part_root && m->n_meshes)
        CLAPGPU_HIP(hipMemcpyAsync(part_root, m->part_root, (size_t)m->n_meshes * 4, hipMemcpyDeviceToHost, s));
    CLAPGPU_HIP(hipStreamSynchronize(s));
    return CLAPGPU_OK;
}
