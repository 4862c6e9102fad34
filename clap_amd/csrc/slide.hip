// slide.hip -- the capsule sweep fed by the broadphase grid, and the characters' sweep-and-slide, for gfx950:
//
//   k_sweep_grid     phys_body_sweep_capsule (physics.c:559-670) with the candidates gathered on the device: one
//                    wavefront per sweep gathers them into LDS, then marches (sweep_dev.h: the march k_sweep_capsules runs)
//   k_slide_clear / k_slide_mark   count the listings of every body of a slide batch (a body listed twice moves nothing)
//   k_slide_decide   character_apply_velocity's ENTITY3D_HAS_PHYSICS branch (character.c:254-310) for a batch of movers:
//                    up to two character_sweep_delta calls (character.c:193-243) of up to three sweeps each, the mover's
//                    running position in registers; writes no pose
//   (bodies.hip's k_slide_apply then moves the bodies, through the geom writer of the step)
//
// The candidate list of a sweep is canonical: every static, then every body, in ascending index, whose AABB meets the
// probe's swept box (the union of its AABB at the start and at start + delta, closed overlap, grown by a relative 2^-40
// against the rounding of the boxes).  Two facts make every gather below give the same bits:
//   1. Contacts are taken in candidate order, 16 a step, and a candidate that does not touch the probe contributes none:
//      any superset of the list in the same relative order gives the same frac, normal and hit.  A gather may hold more
//      than the box asks for, never less.
//   2. A static's word is its index and a body's is its index with bit 31 set, so ascending words ARE the canonical
//      order: the grid gather, which meets the candidates in cell order, sorts the words and drops repeats (a static is
//      registered in every block it reaches).
// Gathers: the scan of every geom (bp == NULL, or the fallbacks of the ray cast: an indexed box larger than a cell, boxes
// binned again since the index, or a swept box over more cells than a scan tests geoms per lane), or the swept box's cell
// range, its blocks' statics and the large list, visited through grid_query_dev.h, which says why they hold every geom
// whose box meets the swept box.  Both keep the words that pass the box test, so they keep the same list.  A list longer
// than SLIDE_CAND words does not fit the wavefront's LDS: that sweep tests every geom's box at every step instead (same
// order, same bits, scan time).
// fp64 colliders, float sweep arithmetic as the reference writes it, no FMA contraction.
#include <string.h>
#include <stdlib.h>
#include "common.h"
#include "phys_dev.h"
#include "geoms_dev.h"
#include "grid_query_dev.h"
#include "trimesh_dev.h"
#include "tricontact_dev.h"
#include "sweep_dev.h"

namespace clapgpu {

constexpr int SB = 256;
constexpr uint32_t SLIDE_CAND = 512;                    // candidate words a wavefront keeps in LDS (a power of two)
constexpr uint32_t CAND_NONE = 0xffffffffu;             // body 0x7fffffff: past every set, no candidate
constexpr uint32_t STAGE_MULTI = 0x80u, STAGE_SHIFT = 8;   // k_slide_decide -> k_slide_apply, in flags[k]: see clapgpu_bodies_slide_apply

struct SlideScene {
    GeomsK bodies, statics;
    const double *body_aabb;            // [bodies.n][6], or NULL: every body is a candidate
    MeshSet M;
    bool grid;
    BpGridView g;
};

__device__ __forceinline__ void swept_box(const double (&bb)[6], const float (&delta)[3], double (&lo)[3], double (&hi)[3])
{
    for (int a = 0; a < 3; a++) {
        const double d = (double)delta[a];
        const double l = fmin(bb[2 * a], bb[2 * a] + d), h = fmax(bb[2 * a + 1], bb[2 * a + 1] + d);
        const double pad = (fabs(l) + fabs(h)) * 0x1p-40;
        lo[a] = l - pad;
        hi[a] = h + pad;
    }
}

__device__ __forceinline__ bool box_meets(const double *bb, const double (&lo)[3], const double (&hi)[3])
{
    return bb[0] <= hi[0] && bb[1] >= lo[0] && bb[2] <= hi[1] && bb[3] >= lo[1] && bb[4] <= hi[2] && bb[5] >= lo[2];
}

// static s against the swept box; other: it is an OTHER static without a mesh (CLAPGPU_SLIDE_UNRESOLVED)
__device__ __forceinline__ bool static_meets(const SlideScene &k, uint32_t s, const double (&lo)[3], const double (&hi)[3], bool &other)
{
    if (s >= k.statics.n) return false;
    if (k.statics.aabb && !box_meets(k.statics.aabb + 6 * (size_t)s, lo, hi)) return false;   // no box known: anywhere
    if (k.statics.kind && k.statics.kind[s] == CLAPGPU_GEOM_OTHER && mesh_of(k.M, s) < 0) other = true;
    return true;
}

__device__ __forceinline__ bool body_meets(const SlideScene &k, uint32_t i, uint32_t self, const double (&lo)[3], const double (&hi)[3])
{
    if (i >= k.bodies.n || i == self) return false;
    return !k.body_aabb || box_meets(k.body_aabb + 6 * (size_t)i, lo, hi);
}

// the wave appends the words of the lanes with `pred`, in lane order; count runs on past SLIDE_CAND (nothing is written)
__device__ __forceinline__ void append(uint32_t *list, uint32_t &count, bool pred, uint32_t word)
{
    const uint64_t m = __ballot(pred);
    const uint32_t at = count + (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull));
    if (pred && at < SLIDE_CAND) list[at] = word;
    count += (uint32_t)__popcll(m);
}

// the scan of every geom: the canonical list as it comes
__device__ __forceinline__ void gather_all(const SlideScene &k, uint32_t self, const double (&lo)[3], const double (&hi)[3],
                                           uint32_t *list, uint32_t &count, bool &other)
{
    const int lane = lane_id();
    count = 0;
    other = false;
    for (uint32_t base = 0; base < k.statics.n; base += WAVE)
        append(list, count, static_meets(k, base + lane, lo, hi, other), base + lane);
    for (uint32_t base = 0; base < k.bodies.n; base += WAVE)
        append(list, count, body_meets(k, base + lane, self, lo, hi), 0x80000000u | (base + lane));
}

// the swept box's cells, their blocks' statics and the large statics; false: more lookups than a scan tests geoms per lane.
// LEVELED (g.levels > 1): the swept box's cells of every level and the blocks of the statics' level; the limit holds the
// lookups of all levels together, so a large mover among small bodies scans
template <bool LEVELED>
__device__ bool gather_grid(const SlideScene &k, uint32_t self, const double (&lo)[3], const double (&hi)[3],
                            uint32_t *list, uint32_t &count, bool &other)
{
    const BpGridView &g = k.g;
    const uint32_t levels = grid_levels<LEVELED>(g);
    count = 0;
    other = false;
    double c = g.cell, lookups = grid_lookups(g, grid_range(c, lo, hi), grid_level_statics<LEVELED>(g, 0));
    for (uint32_t L = 1; L < levels; L++) { c *= 2.0; lookups += grid_lookups(g, grid_range(c, lo, hi), grid_level_statics<LEVELED>(g, L)); }
    if (!(lookups <= 64.0 + (double)(k.bodies.n + k.statics.n) / 64.0)) return false;
    auto take = [&](bool valid, bool is_static, uint32_t i) {
        const bool pred = valid && (is_static ? static_meets(k, i, lo, hi, other) : body_meets(k, i, self, lo, hi));
        append(list, count, pred, is_static ? i : 0x80000000u | i);
    };
    grid_visit_large<LEVELED>(g, take);
    c = g.cell;
    for (uint32_t L = 0; L < levels; L++, c *= 2.0)
        grid_visit<LEVELED>(g, L, grid_level_statics<LEVELED>(g, L), grid_range(c, lo, hi), nullptr, take);
    return true;
}

// ascending words without repeats, in place: a bitonic sort of the wavefront's LDS list, then a compaction
__device__ __forceinline__ void sort_unique(uint32_t *list, uint32_t &count)
{
    const int lane = lane_id();
    uint32_t n2 = WAVE;
    while (n2 < count) n2 <<= 1;
    for (uint32_t i = count + lane; i < n2; i += WAVE) list[i] = CAND_NONE;
    wave_lds_fence();
    for (uint32_t kk = 2; kk <= n2; kk <<= 1)
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            for (uint32_t t = lane; t < n2 / 2; t += WAVE) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint32_t a = list[i], b = list[l];
                const bool up = (i & kk) == 0;
                if ((a > b) == up) { list[i] = b; list[l] = a; }
            }
            wave_lds_fence();
        }
    uint32_t out = 0, last = CAND_NONE;                                      // no word is CAND_NONE
    for (uint32_t base = 0; base < count; base += WAVE) {
        const uint32_t i = base + lane;
        const uint32_t v = i < count ? list[i] : CAND_NONE;
        uint32_t prev = __shfl_up(v, 1);
        if (lane == 0) prev = last;
        last = __shfl(v, WAVE - 1);
        wave_lds_fence();                                                    // every read of the chunk before its writes
        append(list, out, i < count && v != prev, v);
        wave_lds_fence();
    }
    count = out;
}

// One sweep of `probe` (body `self`, at the position it starts from, its box there `bb`) along delta, |delta| =
// delta_len >= 1e-6f and finite: gather, then march.  list: SLIDE_CAND words of this wavefront's LDS.  Returns
// CLAPGPU_SLIDE_UNRESOLVED or 0; frac / normal / hit as phys_body_sweep_capsule leaves them.  LEVELED: k.g is a leveled
// index (the host picks the kernel by it, so a one-level index and the scan run the code they ran).
template <bool MESH, bool LEVELED, typename T>
__device__ __forceinline__ uint32_t sweep_once(const SlideScene &k, phd::Geom &probe, const double (&bb)[6], uint32_t self,
                                               const float (&delta)[3], float delta_len, uint32_t *list, const SweepLds &L,
                                               T &&touched, float &frac, float (&normal)[3], int32_t &hit)
{
    double lo[3], hi[3];
    swept_box(bb, delta, lo, hi);
    uint32_t count = 0;
    bool other = false;
    // the grid, unless: no index; the index may not be used (grid_usable); or too many cells
    const bool grid = k.grid && grid_usable(k.g);
    wave_lds_fence();                                                        // the list's last readers are done
    if (grid && gather_grid<LEVELED>(k, self, lo, hi, list, count, other)) {
        if (count <= SLIDE_CAND) {
            wave_lds_fence();
            sort_unique(list, count);
        }
    } else {
        gather_all(k, self, lo, hi, list, count, other);
    }
    wave_lds_fence();
    frac = 1.0f; normal[0] = 0.f; normal[1] = 1.f; normal[2] = 0.f;
    hit = -1;
    // a list that does not fit: every geom's box at every step, in the same order
    const bool fits = count <= SLIDE_CAND;
    const uint32_t ns = k.statics.n;
    sweep_march<MESH>(k.bodies, k.statics, k.M, probe, self, delta, delta_len, fits ? count : ns + k.bodies.n,
                      [&](uint32_t c) {
                          if (fits) return list[c];
                          bool o = false;
                          if (c < ns) return static_meets(k, c, lo, hi, o) ? c : CAND_NONE;
                          return body_meets(k, c - ns, self, lo, hi) ? (0x80000000u | (c - ns)) : CAND_NONE;
                      }, L, touched, frac, normal, hit);
    return __ballot(other) ? CLAPGPU_SLIDE_UNRESOLVED : 0u;
}

__device__ __forceinline__ bool finite3(const float (&v)[3]) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

// vec3_len (linmath.h:40-51)
__device__ __forceinline__ float vec3_len(const float (&v)[3])
{
    float p = 0.f;
    for (int i = 0; i < 3; i++) p += v[i] * v[i];
    return sqrtf(p);
}

template <bool MESH, bool LEVELED>
__global__ __launch_bounds__(SB)
void k_sweep_grid(SlideScene k, uint32_t n_sweeps, const uint32_t *sweep_body, const float *delta_in, float *frac_out,
                  float *normal_out, int32_t *hit_out, uint32_t *flags)
{
    constexpr uint32_t SW = MESH ? 1 : SB / WAVE;                         // sweeps per workgroup
    __shared__ uint32_t stk[MESH ? TM_STACK * WAVE : 1], ltri[MESH ? 16 * WAVE : 1], lslot[MESH ? 16 * WAVE : 1];
    __shared__ uint32_t lists[SW][SLIDE_CAND];
    const int lane = lane_id();
    const uint32_t sw = blockIdx.x * SW + threadIdx.x / WAVE;
    if (sw >= n_sweeps) return;
    const uint32_t self = sweep_body[sw];
    const float delta[3] = { delta_in[3 * (size_t)sw], delta_in[3 * (size_t)sw + 1], delta_in[3 * (size_t)sw + 2] };
    float frac = 1.0f, normal[3] = { 0.f, 1.f, 0.f };
    int32_t hit = -1;
    uint32_t f = 0;
    if (self >= k.bodies.n || !finite3(delta)) {
        f = CLAPGPU_SLIDE_INVALID;
    } else {
        const float delta_len = vec3_len(delta);
        if (!isfinite(delta_len)) {
            f = CLAPGPU_SLIDE_INVALID;
        } else if (!(delta_len < 1e-6f)) {
            phd::Geom probe;
            load_geom(k.bodies, self, probe);
            double bb[6];
            if (k.body_aabb)
                for (int a = 0; a < 6; a++) bb[a] = k.body_aabb[6 * (size_t)self + a];
            else
                phd::geom_aabb(probe.pos, probe.radius, probe.length, probe.axis, bb);
            const SweepLds lds = { stk, ltri, lslot };
            f = sweep_once<MESH, LEVELED>(k, probe, bb, self, delta, delta_len, lists[threadIdx.x / WAVE], lds, [](uint32_t) {}, frac,
                                 normal, hit);
        }
    }
    if (lane == 0) {
        frac_out[sw] = frac;
        normal_out[3 * (size_t)sw] = normal[0];
        normal_out[3 * (size_t)sw + 1] = normal[1];
        normal_out[3 * (size_t)sw + 2] = normal[2];
        hit_out[sw] = hit;
        if (flags) flags[sw] = f;
    }
}

// ------------------------------------------------------------------------------------------------- the slide
struct SlideK {
    uint32_t n;
    const uint32_t *body;
    float *velocity;
    const uint8_t *airborne;
    float *first_frac;
    int32_t *push_hit;
    uint32_t *flags;
};

// scratch[body]: bit 0 = the decide launch moved it, bits 1.. = its listings.  Cleared by a launch of its own, so that a
// captured graph holds kernel nodes only
__global__ __launch_bounds__(SB)
void k_slide_clear(uint32_t n_bodies, uint32_t *scratch)
{
    const uint32_t i = blockIdx.x * SB + threadIdx.x;
    if (i < n_bodies) scratch[i] = 0;
}

__global__ __launch_bounds__(SB)
void k_slide_mark(uint32_t n, const uint32_t *body, uint32_t n_bodies, uint32_t *scratch)
{
    const uint32_t j = blockIdx.x * SB + threadIdx.x;
    if (j < n && body[j] < n_bodies) atomicAdd(&scratch[body[j]], 2u);
}

// dt: the clamped frame delta.  stash[body][3]: where the mover ends, for the apply launch (the body's lvel, which that
// launch zeroes).  Nothing any sweep reads is written here: every mover sees the others where they were before the call.
template <bool MESH, bool LEVELED>
__global__ __launch_bounds__(SB)
void k_slide_decide(SlideScene k, SlideK s, double dt, uint32_t *scratch, double *stash)
{
    constexpr uint32_t SW = MESH ? 1 : SB / WAVE;
    __shared__ uint32_t stk[MESH ? TM_STACK * WAVE : 1], ltri[MESH ? 16 * WAVE : 1], lslot[MESH ? 16 * WAVE : 1];
    __shared__ uint32_t lists[SW][SLIDE_CAND];
    const int lane = lane_id();
    const uint32_t j = blockIdx.x * SW + threadIdx.x / WAVE;
    if (j >= s.n) return;
    const uint32_t self = s.body[j];
    float first[2] = { 1.0f, 1.0f };
    int32_t push[6] = { -1, -1, -1, -1, -1, -1 };
    float vel[3] = { s.velocity[3 * (size_t)j], s.velocity[3 * (size_t)j + 1], s.velocity[3 * (size_t)j + 2] };
    const bool air = s.airborne[j] != 0;
    // the deltas of the one or two character_sweep_delta calls (character.c:267-307)
    const bool falling = air && !(vel[1] > 0);
    float d0[3], d1[3] = { 0.f, 0.f, 0.f };
    if (falling) {
        d0[0] = 0.f; d0[1] = (float)((double)vel[1] * dt); d0[2] = 0.f;
        d1[0] = (float)((double)vel[0] * dt); d1[2] = (float)((double)vel[2] * dt);
    } else {
        const float dtf = (float)dt;                                          // vec3_scale takes a float
        for (int a = 0; a < 3; a++) d0[a] = vel[a] * dtf;
    }
    uint32_t f = 0;
    if (self >= k.bodies.n || (scratch[self] >> 1) != 1u || !finite3(d0) || !finite3(d1) || !isfinite(vec3_len(d0)) ||
        !isfinite(vec3_len(d1)))
        f = CLAPGPU_SLIDE_INVALID;
    uint32_t t_id = CAND_NONE;                                               // this lane's touched mover of the batch
    bool t_multi = false;
    double p[3] = { 0, 0, 0 }, p0[3] = { 0, 0, 0 };
    if (!f) {
        phd::Geom probe;
        load_geom(k.bodies, self, probe);
        for (int a = 0; a < 3; a++) p[a] = p0[a] = probe.pos[a];
        const SweepLds lds = { stk, ltri, lslot };
        const int ncalls = falling ? 2 : 1;
        int c = 0, iter = 0;
        float delta[3] = { d0[0], d0[1], d0[2] }, call_first = 1.0f;
        while (c < ncalls) {                                                  // character_sweep_delta, one sweep a trip
            const float min_normal_y = (falling && c == 0) ? 0.5f : -1.0f;
            const bool stop_on_block = !(falling && c == 0);
            bool done = true;
            const float len = vec3_len(delta);
            if (!(len < 1e-6f) && isfinite(len)) {                            // character.c:200
                double bb[6];
                for (int a = 0; a < 3; a++) probe.pos[a] = p[a];
                phd::geom_aabb(p, probe.radius, probe.length, probe.axis, bb);
                float frac, normal[3];
                int32_t hit;
                f |= sweep_once<MESH, LEVELED>(k, probe, bb, self, delta, len, lists[threadIdx.x / WAVE], lds,
                                      [&](uint32_t id) {
                                          if ((scratch[id] >> 1) != 1u) return;      // no mover of this batch
                                          if (t_id == CAND_NONE) t_id = id;
                                          else if (t_id != id) t_multi = true;
                                      }, frac, normal, hit);
                if (frac < 1.0f && normal[1] < min_normal_y) frac = 1.0f;     // :213
                if (iter == 0) call_first = frac;
                if (frac < 1.0f && hit >= 0) {                                // :220, phys_body_push's body
                    const int at = c * 3 + iter;
                    for (int q = 0; q < 6; q++) if (q == at) push[q] = hit;
                }
                if (frac > 0) {                                               // :223-227, phys_body_move
                    for (int a = 0; a < 3; a++) { const float step = delta[a] * frac; p[a] = p[a] + (double)step; }
                }
                done = frac >= 1.0f || (frac <= 0.0f && stop_on_block);        // :229-232
                if (!done) {                                                  // :235-239
                    float remaining[3];
                    for (int a = 0; a < 3; a++) remaining[a] = delta[a] * (1.0f - frac);
                    float dot = 0.f;
                    for (int a = 0; a < 3; a++) dot += normal[a] * remaining[a];
                    for (int a = 0; a < 3; a++) { const float along = normal[a] * dot; delta[a] = remaining[a] - along; }
                    if (++iter == 3) done = true;
                }
            }
            if (done) {
                if (c == 0) first[0] = call_first; else first[1] = call_first;
                c++; iter = 0; call_first = 1.0f;
                delta[0] = d1[0]; delta[1] = d1[1]; delta[2] = d1[2];
            }
        }
    }
    if (f) {                                                                  // moves nothing, keeps its velocity
        if (lane == 0) {
            s.first_frac[2 * (size_t)j] = 1.0f; s.first_frac[2 * (size_t)j + 1] = 1.0f;
            for (int q = 0; q < 6; q++) s.push_hit[6 * (size_t)j + q] = -1;
            s.flags[j] = f;
        }
        return;
    }
    // the movers of this batch that gave the probe a contact: one is handed to the apply launch, more than one is not
    // looked into (flagged whether they moved or not)
    const uint64_t any = __ballot(t_id != CAND_NONE);
    uint32_t stage = 0;
    if (any) {
        const uint32_t x = __shfl(t_id, __builtin_ctzll(any));
        const bool multi = __ballot(t_multi || (t_id != CAND_NONE && t_id != x)) != 0 || x + 1 >= (1u << (32 - STAGE_SHIFT));
        stage = multi ? STAGE_MULTI : (x + 1) << STAGE_SHIFT;
    }
    if (lane == 0) {
        s.first_frac[2 * (size_t)j] = first[0]; s.first_frac[2 * (size_t)j + 1] = first[1];
        for (int q = 0; q < 6; q++) s.push_hit[6 * (size_t)j + q] = push[q];
        if (air && first[0] < 1.0f) s.velocity[3 * (size_t)j + 1] = 0.f;       // :283-284, :299-300
        s.flags[j] = stage;
        for (int a = 0; a < 3; a++) stash[3 * (size_t)self + a] = p[a];
        if (p[0] != p0[0] || p[1] != p0[1] || p[2] != p0[2]) atomicOr(&scratch[self], 1u);
    }
}

} // namespace clapgpu

using namespace clapgpu;

// the scene both entry points read; bp: NULL or an index over (b->n, b->aabb) created with statics->n statics
static int slide_scene(SlideScene &k, clapgpu_bp *bp, const clapgpu_bodies *b, const clapgpu_geoms *statics,
                       const clapgpu_trimesh *meshes)
{
    if (!b || !statics || !b->pos || !b->quat || !b->radius) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    clapgpu_geoms g;
    if (!body_geoms(b, &g)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (b->n >= 0x7fffffffu || statics->n >= 0x7fffffffu) return CLAPGPU_ERR_TOO_LARGE;     // bit 31 of a candidate word
    if (bp && !b->aabb) return CLAPGPU_ERR_INVALID_ARGUMENTS;                // an index is over the bodies' own boxes
    memset(&k, 0, sizeof(k));
    const int rc = scene_grid(bp, b->n, b->aabb, statics->n, meshes, &k.g, &k.grid);
    if (rc) return rc;
    k.bodies = geoms_k(&g); k.statics = geoms_k(statics);
    k.body_aabb = b->aabb;
    if (meshes) k.M = trimesh_set(meshes);
    // statics without boxes are candidates wherever they are: only the scan of every geom holds them all
    if (statics->n && !statics->aabb) k.grid = false;
    return CLAPGPU_OK;
}

extern "C" int clapgpu_sweep_capsules_grid(void *stream, clapgpu_bp *bp, const clapgpu_bodies *b, const clapgpu_geoms *statics,
                                           const clapgpu_trimesh *meshes, uint32_t n_sweeps, const uint32_t *sweep_body,
                                           const float *delta, float *frac, float *normal, int32_t *hit, uint32_t *flags)
{
    SlideScene k;
    int rc = slide_scene(k, bp, b, statics, meshes);
    if (rc) return rc;
    if (n_sweeps && (!sweep_body || !delta || !frac || !normal || !hit)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (n_sweeps == 0) return CLAPGPU_OK;
    hipStream_t s = as_stream(stream);
    const bool leveled = k.grid && k.g.levels > 1;     // instantiations of their own: the others keep their code and registers
    if (meshes)
        hipLaunchKernelGGL((leveled ? k_sweep_grid<true, true> : k_sweep_grid<true, false>), dim3(n_sweeps), dim3(WAVE), 0, s, k, n_sweeps,
                           sweep_body, delta, frac, normal, hit, flags);
    else
        hipLaunchKernelGGL((leveled ? k_sweep_grid<false, true> : k_sweep_grid<false, false>), dim3((n_sweeps + SB / WAVE - 1) / (SB / WAVE)),
                           dim3(SB), 0, s, k, n_sweeps, sweep_body, delta, frac, normal, hit, flags);
    CLAPGPU_LAUNCH_CHECK("k_sweep_grid");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_characters_slide(void *stream, clapgpu_bp *bp, const clapgpu_bodies *b, const clapgpu_geoms *statics,
                                        const clapgpu_trimesh *meshes, double dt_sec, const clapgpu_slide *sl, uint32_t *scratch)
{
    SlideScene k;
    int rc = slide_scene(k, bp, b, statics, meshes);
    if (rc) return rc;
    rc = check_bodies(b);
    if (rc) return rc;
    if (!sl) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (sl->n && (!sl->body || !sl->velocity || !sl->airborne || !sl->first_frac || !sl->push_hit || !sl->flags || !scratch))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (sl->n == 0) return CLAPGPU_OK;
    if (dt_sec < 1e-6) return CLAPGPU_OK;                                    // character.c:259-260: nothing at all
    if (dt_sec > 1.0 / 30.0) dt_sec = 1.0 / 30.0;                            // :262-263
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_slide_clear, dim3((b->n + SB - 1) / SB), dim3(SB), 0, s, b->n, scratch);
    CLAPGPU_LAUNCH_CHECK("k_slide_clear");
    hipLaunchKernelGGL(k_slide_mark, dim3((sl->n + SB - 1) / SB), dim3(SB), 0, s, sl->n, sl->body, b->n, scratch);
    CLAPGPU_LAUNCH_CHECK("k_slide_mark");
    SlideK sk;
    sk.n = sl->n; sk.body = sl->body; sk.velocity = sl->velocity; sk.airborne = sl->airborne; sk.first_frac = sl->first_frac;
    sk.push_hit = sl->push_hit; sk.flags = sl->flags;
    const bool leveled = k.grid && k.g.levels > 1;
    if (meshes)
        hipLaunchKernelGGL((leveled ? k_slide_decide<true, true> : k_slide_decide<true, false>), dim3(sl->n), dim3(WAVE), 0, s, k, sk,
                           dt_sec, scratch, b->lvel);
    else
        hipLaunchKernelGGL((leveled ? k_slide_decide<false, true> : k_slide_decide<false, false>), dim3((sl->n + SB / WAVE - 1) / (SB / WAVE)),
                           dim3(SB), 0, s, k, sk, dt_sec, scratch, b->lvel);
    CLAPGPU_LAUNCH_CHECK("k_slide_decide");
    rc = clapgpu_bodies_slide_apply(stream, b, sl->n, sl->body, sl->flags, scratch);
    if (rc) return rc;
    if (bp) return clapgpu_bp_invalidate(stream, bp);                        // the moved boxes: the index is stale
    return CLAPGPU_OK;
}
