// mesh_contacts.hip -- contacts of bodies against static triangle meshes, for gfx950: near_callback for the (body,
// static) pairs whose static owns a mesh -- the triangles under the body's box, the rule of tricontact_dev.h,
// MAX_CONTACTS, canonical order; 160-byte records.
//
//   k_mesh_contacts_count   a pair's kept records, summed per wavefront
//   k_mesh_contacts_scan    the wavefronts' offsets and the total
//   k_mesh_contacts_write   the records, and the (pair, triangle) each came from
//
// Built without SimplifyCFG's common-code sinking: see phd::collide (phys_dev.h).
// fp64 throughout, no FMA contraction.
#include <string.h>
#include "common.h"
#include "phys_dev.h"
#include "geoms_dev.h"
#include "trimesh_dev.h"
#include "tricontact_dev.h"
#include "sweep_dev.h"
#include "contact_record_dev.h"

namespace clapgpu {

// One lane per (body, static) pair, one wavefront per workgroup (the LDS below is per lane: [entry][lane] columns).  A
// pair's records are kept in LDS as the 16 best by (deeper first, then lower triangle index) -- a pair keeps at most 16
// contacts, so no record beyond those can be kept -- and the kept ones are that order's longest prefix whose contacts
// fit in 16.  Both passes compute the same selection; the first counts, the scan places, the second writes.
constexpr int MC = WAVE;
constexpr int MC_KEEP = 16;                                              // MAX_CONTACTS, physics.c:150

struct MeshLds {
    uint32_t stk[TM_STACK * MC];
    double dep[MC_KEEP * MC];                                            // a record's depth: the deeper of its contacts
    uint32_t tri[MC_KEEP * MC];                                          // triangle of the mesh
    uint32_t slot[MC_KEEP * MC];                                         // leaf slot | (nc - 1) << 31
};

struct PairSel { uint32_t body, stat, kept, found; double a[3], b[3], r; };

// pair p's selection into the lane's LDS columns; false: the pair has no mesh contacts to look for
__device__ __forceinline__ bool select_mesh_records(const GeomsK &A, const GeomsK &B, const MeshSet &M, const uint2 *pairs,
                                                    uint32_t p, uint32_t np, MeshLds &L, int lane, PairSel &s)
{
    s.kept = s.found = 0;
    if (p >= np) return false;
    const uint2 pr = pairs[p];
    s.body = pr.x; s.stat = pr.y;
    if (pr.x >= A.n || pr.y >= B.n || mesh_of(M, pr.y) < 0) return false;
    phd::Geom g;
    load_geom(A, pr.x, g);
    if (!phd::geom_segment(g, s.a, s.b)) return false;                   // boxes: no triangle collider here
    s.r = g.radius;
    double lo[3], hi[3];
    segment_box(s.a, s.b, s.r, lo, hi);
    uint32_t n = 0, found = 0;
    box_walk(M, lo, hi, L.stk + lane, [&](uint32_t slot) {
        const uint2 kt = M.key[slot];
        if (kt.x != pr.y) return;                                        // another mesh's leaf
        phd::CGeom c0, c1;
        const int nc = phd::collide_segment_triangle(s.a, s.b, s.r, M.tri + 9 * (size_t)slot, c0, c1);
        if (nc <= 0) return;
        found++;
        const double d = nc > 1 && c1.depth > c0.depth ? c1.depth : c0.depth;
        auto before = [&](int k) {                                       // the new record goes before entry k
            const double dk = L.dep[k * MC + lane];
            return d > dk || (d == dk && kt.y < L.tri[k * MC + lane]);
        };
        if (n == MC_KEEP && !before(MC_KEEP - 1)) return;
        int k = n < MC_KEEP ? (int)n : MC_KEEP;
        while (k > 0 && before(k - 1)) {
            if (k < MC_KEEP) {
                L.dep[k * MC + lane] = L.dep[(k - 1) * MC + lane];
                L.tri[k * MC + lane] = L.tri[(k - 1) * MC + lane];
                L.slot[k * MC + lane] = L.slot[(k - 1) * MC + lane];
            }
            k--;
        }
        L.dep[k * MC + lane] = d;
        L.tri[k * MC + lane] = kt.y;
        L.slot[k * MC + lane] = slot | ((uint32_t)(nc - 1) << 31);
        if (n < MC_KEEP) n++;
    });
    uint32_t used = 0, kept = 0;
    for (; kept < n; kept++) {
        const uint32_t nc = (L.slot[kept * MC + lane] >> 31) + 1;
        if (used + nc > (uint32_t)MC_KEEP) break;
        used += nc;
    }
    s.kept = kept;
    s.found = found;
    return true;
}

__global__ __launch_bounds__(MC)
void k_mesh_contacts_count(GeomsK A, GeomsK B, MeshSet M, const uint2 *pairs, const uint32_t *pair_total, uint32_t capacity,
                           uint32_t *wsum, uint32_t *capped)
{
    __shared__ MeshLds L;
    const int lane = lane_id();
    const uint32_t np = clamped(pair_total, capacity);
    PairSel s;
    select_mesh_records(A, B, M, pairs, blockIdx.x * MC + lane, np, L, lane, s);
    uint32_t kept = s.kept, cap = s.found > s.kept ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) { kept += __shfl_xor(kept, o); cap += __shfl_xor(cap, o); }
    if (lane == 0) {
        wsum[blockIdx.x] = kept;
        if (cap && capped) atomicAdd(capped, cap);
    }
}

// one workgroup: the exclusive scan of the wavefronts' record counts in place, and the total
constexpr int MS = 1024;
__global__ __launch_bounds__(MS)
void k_mesh_contacts_scan(const uint32_t *pair_total, uint32_t capacity, uint32_t *wsum, uint32_t *total)
{
    __shared__ uint32_t part[MS / WAVE];
    const uint32_t np = clamped(pair_total, capacity);
    const uint32_t nw = (np + MC - 1) / MC, per = (nw + MS - 1) / MS;
    const uint32_t b0 = threadIdx.x * per, b1 = b0 + per < nw ? b0 + per : nw;
    uint32_t sum = 0;
    for (uint32_t i = b0; i < b1; i++) sum += wsum[i];
    const int lane = lane_id(), wv = threadIdx.x / WAVE;
    const uint32_t incl = wave_prefix_sum(sum);
    if (lane == WAVE - 1) part[wv] = incl;
    __syncthreads();
    uint32_t off = incl - sum;
    for (int k = 0; k < wv; k++) off += part[k];
    for (uint32_t i = b0; i < b1; i++) { const uint32_t c = wsum[i]; wsum[i] = off; off += c; }
    if (threadIdx.x == MS - 1) {
        uint32_t t = 0;
        for (int k = 0; k < MS / WAVE; k++) t += part[k];
        if (total) *total = t;
    }
}

__global__ __launch_bounds__(MC)
void k_mesh_contacts_write(GeomsK A, GeomsK B, MeshSet M, const uint2 *pairs, const uint32_t *pair_total, uint32_t capacity,
                           const uint32_t *wsum, uint32_t out_capacity, clapgpu_contact2 *out, uint32_t *mesh_ref,
                           uint32_t *body_flags)
{
    __shared__ MeshLds L;
    const int lane = lane_id();
    const uint32_t np = clamped(pair_total, capacity);
    if (blockIdx.x * MC >= np) return;                                   // wave-uniform
    const uint32_t p = blockIdx.x * MC + lane;
    PairSel s;
    select_mesh_records(A, B, M, pairs, p, np, L, lane, s);
    uint32_t incl = s.kept;                                              // wave_prefix_sum (common.h) restated: calling it moves this kernel's code
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint32_t u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    const uint32_t base = wsum[blockIdx.x] + incl - s.kept;
    if (s.kept == 0) return;
    const double *m1 = (A.material && B.material) ? A.material + 5 * (size_t)s.body : nullptr;
    const double *m2 = (A.material && B.material) ? B.material + 5 * (size_t)s.stat : nullptr;
    for (uint32_t k = 0; k < s.kept; k++) {
        const uint32_t t = L.tri[k * MC + lane];
        uint32_t rank = 0;                                               // ascending triangle index within the pair
        for (uint32_t j = 0; j < s.kept; j++) rank += L.tri[j * MC + lane] < t ? 1u : 0u;
        const uint32_t o = base + rank;
        if (o >= out_capacity) continue;
        const uint32_t slot = L.slot[k * MC + lane] & 0x7fffffffu;
        phd::CGeom c0, c1;
        memset(&c0, 0, sizeof(c0));
        memset(&c1, 0, sizeof(c1));
        const int nc = phd::collide_segment_triangle(s.a, s.b, s.r, M.tri + 9 * (size_t)slot, c0, c1);
        clapgpu_contact2 c;
        memset(&c, 0, sizeof(c));
        record_points(c, nc > 1, c0, c1);
        contact_surface(c, m1, m2);
        c.nc = (uint32_t)nc;
        out[o] = c;
        mesh_ref[2 * (size_t)o] = p;
        mesh_ref[2 * (size_t)o + 1] = t;
    }
    // mark_has_joint (contact_record_dev.h) restated: calling it turns this kernel's last branch around
    if (body_flags && !(body_flags[s.body] & CLAPGPU_BODY_HAS_JOINT)) body_flags[s.body] |= CLAPGPU_BODY_HAS_JOINT;
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" int clapgpu_contacts_meshes(void *stream, const clapgpu_geoms *bodies, const clapgpu_geoms *statics,
                                       const clapgpu_trimesh *meshes, const uint32_t *static_pairs,
                                       const uint32_t *static_pair_total, uint32_t static_capacity, uint32_t *scratch,
                                       uint32_t capacity, clapgpu_contact2 *contacts, uint32_t *mesh_ref,
                                       uint32_t *contact_total, uint32_t *capped_pairs, uint32_t *body_flags)
{
    if (!bodies || !statics || !meshes || !static_pair_total || (static_capacity && (!static_pairs || !scratch)) ||
        (capacity && (!contacts || !mesh_ref)))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (reinterpret_cast<uintptr_t>(contacts) & 15u) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (trimesh_set(meshes).n_statics != statics->n) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    hipStream_t s = as_stream(stream);
    if (contact_total) CLAPGPU_HIP(hipMemsetAsync(contact_total, 0, sizeof(uint32_t), s));
    if (capped_pairs) CLAPGPU_HIP(hipMemsetAsync(capped_pairs, 0, sizeof(uint32_t), s));
    if (static_capacity == 0 || bodies->n == 0 || statics->n == 0) return CLAPGPU_OK;
    const MeshSet M = trimesh_set(meshes);
    const uint32_t waves = (static_capacity + MC - 1) / MC;
    const uint2 *pairs = reinterpret_cast<const uint2 *>(static_pairs);
    hipLaunchKernelGGL(k_mesh_contacts_count, dim3(waves), dim3(MC), 0, s, geoms_k(bodies), geoms_k(statics), M, pairs,
                       static_pair_total, static_capacity, scratch, capped_pairs);
    CLAPGPU_LAUNCH_CHECK("k_mesh_contacts_count");
    hipLaunchKernelGGL(k_mesh_contacts_scan, dim3(1), dim3(MS), 0, s, static_pair_total, static_capacity, scratch, contact_total);
    CLAPGPU_LAUNCH_CHECK("k_mesh_contacts_scan");
    hipLaunchKernelGGL(k_mesh_contacts_write, dim3(waves), dim3(MC), 0, s, geoms_k(bodies), geoms_k(statics), M, pairs,
                       static_pair_total, static_capacity, scratch, capacity, contacts, mesh_ref, body_flags);
    CLAPGPU_LAUNCH_CHECK("k_mesh_contacts_write");
    return CLAPGPU_OK;
}
