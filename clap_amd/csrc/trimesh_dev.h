// trimesh_dev.h -- the mesh set's BVH as kernels read it: the node layout, the device view of the set (filled by
// trimesh.hip's trimesh_set alone) and the one walk of the tree.  The mesh ray pass (ray_trimesh.hip) walks it with a pruned
// slab test, the mesh contacts (mesh_contacts.hip) and the capsule sweep against meshes (contacts.hip, slide.hip) with a box query.
//
// Tree (built by trimesh.hip): one BVH2 over every triangle of every mesh.  A node is 64 B: both children's boxes
// (float, min xyz / max xyz, rounded outward from the fp64 triangles so that a box never excludes a point of a triangle
// it holds) and both links (bit 31: a leaf = one triangle in leaf order).  The height is at most 62 (see
// clapgpu_trimesh_status).  The walk's stack is in LDS, [TM_STACK entries][WAVE lanes] of u32 (16 KiB per wavefront): a
// register array indexed by a per-lane stack pointer would live in scratch memory, and the deep trees of degenerate
// meshes need all 64.
#pragma once
#include "common.h"

struct clapgpu_trimesh;

namespace clapgpu {

constexpr uint32_t TM_LEAF = 0x80000000u;                  // a child link with bit 31: one triangle in leaf order
constexpr int TM_STACK = 64;                               // the tree is at most 62 edges high (clapgpu_trimesh_status)

struct alignas(16) Node {
    float box[12];                                      // child 0: min xyz, max xyz; child 1: the same
    uint32_t child[2];
    uint32_t pad[2];
};
static_assert(sizeof(Node) == 64, "one node, one 64-byte sector");

struct MeshSet {
    const Node *nodes;
    const double *tri;                                  // [T][9] in leaf order
    const uint2 *key;                                   // [T]: (static, triangle of its mesh) in leaf order
    const int32_t *static_mesh;                         // [n_statics]: the static's mesh or -1
    uint32_t n_tris, n_statics;
};
MeshSet trimesh_set(const clapgpu_trimesh *m);          // trimesh.hip

// The walk: enter(box, key) says whether a child's box (min xyz, max xyz) is to be entered and gives the key that orders
// two inner children (the lower first, the left on a tie); leaf(slot) visits a leaf whose box is entered.  Both children
// are tested before either leaf is visited.  stk: this lane's column of a [TM_STACK][WAVE] LDS stack.
template <typename E, typename F>
__device__ __forceinline__ void bvh_walk(const MeshSet &m, uint32_t *stk, E &&enter, F &&leaf)
{
    if (m.n_tris == 0) return;
    uint32_t node = 0;
    int sp = 0;
    for (;;) {
        const float4 *np = reinterpret_cast<const float4 *>(m.nodes + node);
        const float4 f0 = np[0], f1 = np[1], f2 = np[2];
        const uint4 c = reinterpret_cast<const uint4 *>(np)[3];
        const float bl[6] = { f0.x, f0.y, f0.z, f0.w, f1.x, f1.y }, br[6] = { f1.z, f1.w, f2.x, f2.y, f2.z, f2.w };
        double tl, tr;
        bool hl = enter(bl, tl), hr = enter(br, tr);
        if (hl && (c.x & TM_LEAF)) { leaf(c.x & ~TM_LEAF); hl = false; }
        if (hr && (c.y & TM_LEAF) && c.y != c.x) leaf(c.y & ~TM_LEAF);           // (a one-leaf root holds it twice)
        if (hr && (c.y & TM_LEAF)) hr = false;
        if (hl && hr) {
            const bool lfirst = tl <= tr;
            if (sp < TM_STACK) stk[sp++ * WAVE] = lfirst ? c.y : c.x;
            node = lfirst ? c.x : c.y;
        } else if (hl) {
            node = c.x;
        } else if (hr) {
            node = c.y;
        } else {
            if (sp == 0) break;
            node = stk[--sp * WAVE];
        }
    }
}

// closed overlap of a float box (min xyz, max xyz) with the query box
__device__ __forceinline__ bool box_overlap(const float *b, const double (&lo)[3], const double (&hi)[3])
{
    return (double)b[0] <= hi[0] && (double)b[3] >= lo[0] && (double)b[1] <= hi[1] && (double)b[4] >= lo[1] &&
           (double)b[2] <= hi[2] && (double)b[5] >= lo[2];
}

// the box query: every leaf slot whose box meets [lo, hi], the left child first
template <typename F>
__device__ __forceinline__ void box_walk(const MeshSet &m, const double (&lo)[3], const double (&hi)[3], uint32_t *stk, F &&leaf)
{
    bvh_walk(m, stk, [&](const float *b, double &key) { key = 0.0; return box_overlap(b, lo, hi); }, leaf);
}

} // namespace clapgpu
