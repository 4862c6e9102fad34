// trimesh_dev.h -- the mesh set's BVH as the kernels outside trimesh.hip read it: the node layout, a device view of
// the set, and the walk of a box query (the mesh contacts and the capsule sweep against meshes, contacts.hip).
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
uint32_t trimesh_n_statics(const clapgpu_trimesh *m);

// closed overlap of a float box (min xyz, max xyz) with the query box
__device__ __forceinline__ bool box_overlap(const float *b, const double (&lo)[3], const double (&hi)[3])
{
    return (double)b[0] <= hi[0] && (double)b[3] >= lo[0] && (double)b[1] <= hi[1] && (double)b[4] >= lo[1] &&
           (double)b[2] <= hi[2] && (double)b[5] >= lo[2];
}

// every leaf slot whose box meets [lo, hi] (in no particular order); stk: this lane's column of a [TM_STACK][WAVE] LDS
// stack (a register array indexed by a per-lane stack pointer would live in scratch)
template <typename F>
__device__ __forceinline__ void box_walk(const MeshSet &m, const double (&lo)[3], const double (&hi)[3], uint32_t *stk, F &&leaf)
{
    if (m.n_tris == 0) return;
    uint32_t node = 0;
    int sp = 0;
    for (;;) {
        const float4 *np = reinterpret_cast<const float4 *>(m.nodes + node);
        const float4 f0 = np[0], f1 = np[1], f2 = np[2];
        const uint4 c = reinterpret_cast<const uint4 *>(np)[3];
        const float bl[6] = { f0.x, f0.y, f0.z, f0.w, f1.x, f1.y }, br[6] = { f1.z, f1.w, f2.x, f2.y, f2.z, f2.w };
        bool hl = box_overlap(bl, lo, hi), hr = box_overlap(br, lo, hi);
        if (hl && (c.x & TM_LEAF)) { leaf(c.x & ~TM_LEAF); hl = false; }
        if (hr && (c.y & TM_LEAF) && c.y != c.x) leaf(c.y & ~TM_LEAF);           // (a one-leaf root holds it twice)
        if (hr && (c.y & TM_LEAF)) hr = false;
        if (hl && hr) {
            if (sp < TM_STACK) stk[sp++ * WAVE] = c.y;
            node = c.x;
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

} // namespace clapgpu
