// sweep_dev.h -- phys_body_sweep_capsule's march (physics.c:559-670) for one probe on one wavefront, shared by
// contacts.hip (k_sweep_capsules: the candidates are a list of the host's) and slide.hip (the candidates are gathered
// on the device, and the probe is a mover's running position).  Include it after phys_dev.h, geoms_dev.h,
// trimesh_dev.h and tricontact_dev.h; a translation unit that uses it is built with -mllvm
// -simplifycfg-sink-common=false (why: the comment on phd::collide, phys_dev.h; which: the Makefile).
#pragma once
#include <string.h>
#include "common.h"
#include "phys_dev.h"
#include "geoms_dev.h"
#include "trimesh_dev.h"
#include "tricontact_dev.h"

namespace clapgpu {

// the probe's box for a BVH query: the segment's box grown by the radius, and by a relative margin so that a triangle
// touching the geom (depth 0) is never left out by the rounding of the box
__device__ __forceinline__ void segment_box(const double (&a)[3], const double (&b)[3], double r, double (&lo)[3], double (&hi)[3])
{
    for (int i = 0; i < 3; i++) {
        const double l = fmin(a[i], b[i]) - r, h = fmax(a[i], b[i]) + r;
        const double pad = (fabs(l) + fabs(h) + r) * 0x1p-40;
        lo[i] = l - pad;
        hi[i] = h + pad;
    }
}

// the mesh of static `id`, or -1
__device__ __forceinline__ int32_t mesh_of(const MeshSet &M, uint32_t id)
{
    return (M.static_mesh && id < M.n_statics) ? M.static_mesh[id] : -1;
}

// the LDS a wavefront marches with when MESH: the walk's stack and the 16 lowest touching triangles of a lane's candidate
struct SweepLds { uint32_t *stk, *ltri, *lslot; };

// The march of `probe` (body `self` of A, at the position the sweep starts from) along `delta` (|delta| = delta_len, not
// below 1e-6f) against candidates 0 .. n_cand: cand_at(k) is an index into B or, with bit 31 set, into A; an index past
// the set is no candidate.  The candidates of a step are spread over the lanes.  MESH: a candidate static that owns a
// mesh collides with that mesh's triangles under the probe's box instead of its own collider, its contacts in ascending
// triangle index (the 16 lowest touching triangles kept in LDS: no more can be taken).  touched(body): called by the
// lane that found contacts with that body of A.  Every lane returns the same best_frac / best_normal / best_hit.
template <bool MESH, typename C, typename T>
__device__ __forceinline__ void sweep_march(const GeomsK &A, const GeomsK &B, const MeshSet &M, phd::Geom &probe, uint32_t self,
                                            const float (&delta)[3], float delta_len, uint32_t n_cand, C &&cand_at,
                                            const SweepLds &L, T &&touched, float &best_frac, float (&best_normal)[3],
                                            int32_t &best_hit)
{
    const int lane = lane_id();
    uint32_t *stk = L.stk, *ltri = L.ltri, *lslot = L.lslot;
    const double gp[3] = { probe.pos[0], probe.pos[1], probe.pos[2] };
    const float k = 1.0f / delta_len;
    const float dir[3] = { delta[0] * k, delta[1] * k, delta[2] * k };
    int nsteps = (int)ceilf((float)(delta_len / (probe.radius * 0.5f)));
    if (nsteps < 2) nsteps = 2;
    const uint32_t c0 = 0, c1 = n_cand;
    for (int s = 1; s <= nsteps; s++) {
        const float t = (float)s / nsteps;
        probe.pos[0] = gp[0] + delta[0] * t;
        probe.pos[1] = gp[1] + delta[1] * t;
        probe.pos[2] = gp[2] + delta[2] * t;
        uint32_t taken = 0;                                              // contacts of this step so far (cap 16)
        // (frac, order) of the wave's best contact this step; order = position in the candidate sequence
        float step_frac = best_frac;
        uint32_t step_order = 0xffffffffu;
        float step_normal[3] = { 0, 0, 0 };
        int32_t step_hit = -1;
        for (uint32_t base = c0; base < c1 && taken < 16; base += WAVE) {
            const uint32_t kk = base + lane;
            int nc = 0;
            phd::CGeom cg0, cg1;                                          // (two locals, not an array: nothing indexes them)
            memset(&cg0, 0, sizeof(cg0));
            memset(&cg1, 0, sizeof(cg1));
            bool is_body = false;
            uint32_t id = 0;
            uint32_t n_mesh = 0;                                          // MESH: touching triangles listed
            double sa[3], sb[3];                                          // MESH: the probe's segment
            if (kk < c1) {
                const uint32_t cv = cand_at(kk);
                is_body = (cv >> 31) != 0;
                id = cv & 0x7fffffffu;
                if (MESH && !is_body && id < B.n && mesh_of(M, id) >= 0) {
                    if (phd::geom_segment(probe, sa, sb)) {
                        double lo[3], hi[3];
                        segment_box(sa, sb, probe.radius, lo, hi);
                        uint32_t total = 0;
                        box_walk(M, lo, hi, stk + lane, [&](uint32_t slot) {
                            const uint2 kt = M.key[slot];
                            if (kt.x != id) return;
                            phd::CGeom t0, t1;
                            const int n = phd::collide_segment_triangle(sa, sb, probe.radius, M.tri + 9 * (size_t)slot, t0, t1);
                            if (n <= 0) return;
                            total += (uint32_t)n;
                            // the 16 lowest triangle indices, ascending
                            if (n_mesh == 16 && ltri[15 * WAVE + lane] < kt.y) return;
                            int k = n_mesh < 16 ? (int)n_mesh : 16;
                            while (k > 0 && ltri[(k - 1) * WAVE + lane] > kt.y) {
                                if (k < 16) { ltri[k * WAVE + lane] = ltri[(k - 1) * WAVE + lane]; lslot[k * WAVE + lane] = lslot[(k - 1) * WAVE + lane]; }
                                k--;
                            }
                            ltri[k * WAVE + lane] = kt.y;
                            lslot[k * WAVE + lane] = slot | ((uint32_t)(n - 1) << 31);
                            if (n_mesh < 16) n_mesh++;
                        });
                        nc = (int)total;
                    }
                } else if (!(is_body && id == self) && id < (is_body ? A.n : B.n)) {
                    phd::Geom other;
                    load_geom(is_body ? A : B, id, other);
                    nc = phd::collide(probe, other, cg0, cg1);
                    if (nc < 0) nc = 0;
                    if (is_body && nc > 0) touched(id);
                }
            }
            // ordinal of this lane's first contact among the step's contacts
            const uint32_t incl = wave_prefix_sum((uint32_t)nc);
            const uint32_t first = taken + incl - (uint32_t)nc;
            auto take = [&](const phd::CGeom &g, uint32_t i) {
                if (first + i >= 16) return;
                const float cn[3] = { (float)g.normal[0], (float)g.normal[1], (float)g.normal[2] };
                const float ndot = dir[0] * cn[0] + dir[1] * cn[1] + dir[2] * cn[2];
                if (ndot > -0.1f) return;
                const float backup = (float)(g.depth / -ndot);
                const float step_dist = t * delta_len;
                float safe_dist = step_dist - backup;
                if (safe_dist < 0) safe_dist = 0;
                const float frac = safe_dist / delta_len;
                const uint32_t order = first + i;
                if (frac < step_frac) {                                   // within a lane: contacts in order, strict <
                    step_frac = frac; step_order = order;
                    step_normal[0] = cn[0]; step_normal[1] = cn[1]; step_normal[2] = cn[2];
                    step_hit = is_body ? (int32_t)id : -2 - (int32_t)id;
                }
            };
            if (MESH && n_mesh) {                                         // the mesh's contacts in triangle order
                uint32_t i = 0;
                for (uint32_t k = 0; k < n_mesh && first + i < 16; k++) {
                    const uint32_t slot = lslot[k * WAVE + lane] & 0x7fffffffu;
                    phd::CGeom t0, t1;
                    const int n = phd::collide_segment_triangle(sa, sb, probe.radius, M.tri + 9 * (size_t)slot, t0, t1);
                    if (n > 0) take(t0, i);
                    if (n > 1) take(t1, i + 1);
                    i += (uint32_t)(n > 0 ? n : 0);
                }
            } else {
                if (nc > 0) take(cg0, 0);
                if (nc > 1) take(cg1, 1);
            }
            taken += __shfl(incl, WAVE - 1);
        }
        // the sequential loop keeps the FIRST contact (in order) among those with the smallest frac below best_frac
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float of = __shfl_xor(step_frac, o);
            const uint32_t oo = __shfl_xor(step_order, o);
            const float n0 = __shfl_xor(step_normal[0], o), n1 = __shfl_xor(step_normal[1], o), n2 = __shfl_xor(step_normal[2], o);
            const int32_t oh = __shfl_xor(step_hit, o);
            if (of < step_frac || (of == step_frac && oo < step_order)) {
                step_frac = of; step_order = oo; step_normal[0] = n0; step_normal[1] = n1; step_normal[2] = n2; step_hit = oh;
            }
        }
        if (step_order != 0xffffffffu) {
            best_frac = step_frac;
            best_normal[0] = step_normal[0]; best_normal[1] = step_normal[1]; best_normal[2] = step_normal[2];
            best_hit = step_hit;
        }
        if (best_frac < t) break;
    }
    probe.pos[0] = gp[0]; probe.pos[1] = gp[1]; probe.pos[2] = gp[2];
}

} // namespace clapgpu
