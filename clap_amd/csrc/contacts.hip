// contacts.hip -- the geom narrowphase of the world step and the capsule sweep over candidate lists, for gfx950:
//
//   k_contacts_geoms        near_callback's dCollide + phys_contact_surface (physics.c:399-449, 291-330) for candidate
//                           pairs of any two colliders, 160-byte records; one list of pairs a launch
//   k_contacts_geoms_both   both lists of a step (bodies x bodies, bodies x statics) in one launch, the totals through
//                           one ticket word
//   k_sweep_capsules<MESH>  phys_body_sweep_capsule (physics.c:559-670), one wavefront per sweep (the march: sweep_dev.h,
//                           which slide.hip runs too); true: candidates that own a mesh of the mesh set collide through
//                           its triangles (tricontact_dev.h).  It stays in this file: in a translation unit of its own
//                           both instantiations compile to other code, and <true> was 1 % slower
//                           (profiles/contacts_split/README.md)
//
// Built without SimplifyCFG's common-code sinking: see phd::collide (phys_dev.h).
// fp64 throughout, no FMA contraction.  ODE is an absent submodule of the reference: PARITY UNPINNED.
#include <string.h>
#include <stdlib.h>
#include "common.h"
#include "phys_dev.h"
#include "geoms_dev.h"
#include "bp_grid.h"
#include "trimesh_dev.h"
#include "tricontact_dev.h"
#include "sweep_dev.h"
#include "contact_record_dev.h"

namespace clapgpu {

constexpr int PB = 256;

// GeomsK, load_geom, geoms_k: geoms_dev.h (shared with the ray cast); contact_surface, record_points, mark_has_joint,
// clamped: contact_record_dev.h

// one candidate pair -> its record; true if the pair produced contacts (or is flagged deep)
__device__ __forceinline__ bool contact_of_pair(const GeomsK &A, const GeomsK &B, const uint2 pr, clapgpu_contact2 &c,
                                                uint32_t *flags_a, uint32_t *flags_b)
{
    bool counted = false;
    if (pr.x < A.n && pr.y < B.n) {
        phd::Geom ga, gb;
        load_geom(A, pr.x, ga);
        load_geom(B, pr.y, gb);
        phd::CGeom c0, c1;
        memset(&c0, 0, sizeof(c0));
        memset(&c1, 0, sizeof(c1));
        const int nc = phd::collide(ga, gb, c0, c1);
        if (nc < 0) {
            c.nc = CLAPGPU_CONTACT_DEEP;
            counted = true;
        } else if (nc > 0) {
            record_points(c, nc > 1, c0, c1);
            contact_surface(c, (A.material && B.material) ? A.material + 5 * (size_t)pr.x : nullptr,
                            (A.material && B.material) ? B.material + 5 * (size_t)pr.y : nullptr);
            c.nc = (uint32_t)nc;
            counted = true;
            mark_has_joint(flags_a, pr.x);
            mark_has_joint(flags_b, pr.y);
        }
    }
    return counted;
}

// 64 consecutive pairs of one list on one wavefront: each lane's 160-byte record goes through a wave-private LDS tile
// (rows padded to 176 bytes: the 16-byte writes of eight neighbouring lanes then fall on all 32 banks) and leaves as ten
// 1 KiB stores -- written per lane, ten 16-byte pieces at a 160-byte stride touched 64 cache lines per instruction.
constexpr int CONTACT_ROW = 11;                                          // uint4 per staged record (10 used)
__device__ __forceinline__ void store_chunk(const clapgpu_contact2 &c, clapgpu_contact2 *out, uint32_t p0, uint32_t np, uint4 *tile)
{
    static_assert(sizeof(clapgpu_contact2) == 160, "ten 16-byte pieces");
    const int lane = lane_id();
    uint4 v[10];
    memcpy(v, &c, sizeof(c));
#pragma unroll
    for (int k = 0; k < 10; k++) tile[lane * CONTACT_ROW + k] = v[k];
    wave_lds_fence();
    const uint32_t pieces = (np - p0 < (uint32_t)WAVE ? np - p0 : (uint32_t)WAVE) * 10u;
    uint4 *o = reinterpret_cast<uint4 *>(out + p0);
#pragma unroll
    for (int k = 0; k < 10; k++) {
        const uint32_t idx = (uint32_t)(k * WAVE + lane);
        if (idx < pieces) o[idx] = tile[(idx / 10u) * CONTACT_ROW + idx % 10u];
    }
    wave_lds_fence();
}

__device__ __forceinline__ uint32_t contacts_chunk(const GeomsK &A, const GeomsK &B, const uint2 *pairs, uint32_t p0, uint32_t np,
                                                    clapgpu_contact2 *out, uint32_t *flags_a, uint32_t *flags_b, uint4 *tile)
{
    const uint32_t p = p0 + lane_id();
    clapgpu_contact2 c;
    memset(&c, 0, sizeof(c));
    uint32_t counted = 0;
    if (p < np) counted = contact_of_pair(A, B, pairs[p], c, flags_a, flags_b);
    store_chunk(c, out, p0, np, tile);
    return counted;
}

// ---- the one-launch form's loop: a wavefront takes several chunks, and a chunk's inputs are asked for while the chunk
// before it is still being worked on (the chain per chunk is pair -> two geoms + two flag words -> arithmetic -> record;
// measured: a wavefront of the one-chunk-per-wavefront kernel lives ~17 us, two thirds of it waiting, and the kernel is
// two such rounds).  The next chunk's PAIR is requested before this chunk's arithmetic; the flag words come with the geoms.
// (The next chunk's geoms as well, under this chunk's stores: 224 VGPRs and 152 bytes of scratch -- not kept.)
struct PairInputs { uint2 pr; bool live; phd::Geom ga, gb; uint32_t fa, fb; };

__device__ __forceinline__ void load_pair_inputs(const GeomsK &A, const GeomsK &B, uint2 pr, bool in_range, uint32_t *flags_a,
                                                 uint32_t *flags_b, PairInputs &in)
{
    in.pr = pr;
    in.live = in_range && pr.x < A.n && pr.y < B.n;
    in.fa = in.fb = CLAPGPU_BODY_HAS_JOINT;
    if (in.live) {
        load_geom(A, pr.x, in.ga);
        load_geom(B, pr.y, in.gb);
        // the flag words early: every writer of this launch sets the same bit and nothing else changes the words
        if (flags_a) in.fa = flags_a[pr.x];
        if (flags_b) in.fb = flags_b[pr.y];
    }
}

__device__ __forceinline__ uint32_t contact_from_inputs(const GeomsK &A, const GeomsK &B, const PairInputs &in, clapgpu_contact2 &c,
                                                        uint32_t *flags_a, uint32_t *flags_b)
{
    if (!in.live) return 0;
    phd::CGeom c0, c1;
    memset(&c0, 0, sizeof(c0));
    memset(&c1, 0, sizeof(c1));
    const int nc = phd::collide(in.ga, in.gb, c0, c1);
    if (nc < 0) { c.nc = CLAPGPU_CONTACT_DEEP; return 1; }
    if (nc == 0) return 0;
    record_points(c, nc > 1, c0, c1);
    contact_surface(c, (A.material && B.material) ? A.material + 5 * (size_t)in.pr.x : nullptr,
                    (A.material && B.material) ? B.material + 5 * (size_t)in.pr.y : nullptr);
    c.nc = (uint32_t)nc;
    // mark_has_joint (contact_record_dev.h) from the words load_pair_inputs asked for early
    if (flags_a && !(in.fa & CLAPGPU_BODY_HAS_JOINT)) flags_a[in.pr.x] = in.fa | CLAPGPU_BODY_HAS_JOINT;
    if (flags_b && !(in.fb & CLAPGPU_BODY_HAS_JOINT)) flags_b[in.pr.y] = in.fb | CLAPGPU_BODY_HAS_JOINT;
    return 1;
}

__device__ __forceinline__ uint32_t chunk_from_pair(const GeomsK &A, const GeomsK &B, uint2 pr, bool in_range, uint32_t p0, uint32_t np,
                                                     clapgpu_contact2 *out, uint32_t *flags_a, uint32_t *flags_b, uint4 *tile)
{
    PairInputs in;
    load_pair_inputs(A, B, pr, in_range, flags_a, flags_b, in);
    clapgpu_contact2 c;
    memset(&c, 0, sizeof(c));
    const uint32_t counted = contact_from_inputs(A, B, in, c, flags_a, flags_b);
    store_chunk(c, out, p0, np, tile);
    return counted;
}

__global__ __launch_bounds__(PB)
void k_contacts_geoms(GeomsK A, GeomsK B, const uint2 *pairs, const uint32_t *pair_total, uint32_t capacity,
                      clapgpu_contact2 *out, uint32_t *contact_total, uint32_t *flags_a, uint32_t *flags_b)
{
    __shared__ uint32_t block_hits;
    __shared__ uint4 tile[PB / WAVE][WAVE * CONTACT_ROW];
    if (threadIdx.x == 0) block_hits = 0;
    __syncthreads();
    const uint32_t np = clamped(pair_total, capacity);
    uint32_t mine = 0;
    const uint32_t wave = threadIdx.x / WAVE;
    for (uint32_t p0 = blockIdx.x * PB + wave * WAVE; p0 < np; p0 += gridDim.x * PB)      // wave-uniform
        mine += contacts_chunk(A, B, pairs, p0, np, out, flags_a, flags_b, tile[wave]);
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if (lane_id() == 0 && mine) atomicAdd(&block_hits, mine);
    __syncthreads();
    if (threadIdx.x == 0 && block_hits && contact_total) atomicAdd(contact_total, block_hits);
}

// near_callback over BOTH lists of a step (bodies x bodies, bodies x statics: physics.c:751-753) in one launch, and
// without a cleared counter in front of it: a workgroup adds (1, its static count, its body count) to ONE 64-bit word with one
// atomic; the workgroup that finds every other ticket already taken holds the totals in what came back, stores them and
// leaves the word at zero for the next launch.  Two launches and two counter fills were 62 us of a frame for 47 us of work.
#ifndef CONTACTS_BOTH_WAVES
#define CONTACTS_BOTH_WAVES 2                                            // wavefronts a SIMD (174 VGPRs, nothing spilled; 3 = 168 VGPRs + 24 B of scratch: 0.3 us faster)
#endif
__global__ __launch_bounds__(PB) __attribute__((amdgpu_waves_per_eu(CONTACTS_BOTH_WAVES, CONTACTS_BOTH_WAVES)))
void k_contacts_geoms_both(GeomsK A, GeomsK B, const uint2 *pairs, const uint32_t *pair_total, uint32_t capacity,
                           clapgpu_contact2 *out, uint32_t *contact_total, const uint2 *spairs, const uint32_t *spair_total,
                           uint32_t scapacity, clapgpu_contact2 *sout, uint32_t *scontact_total, uint32_t *flags,
                           unsigned long long *word)
{
    __shared__ uint32_t block_hits[2];
    __shared__ uint4 tile[PB / WAVE][WAVE * CONTACT_ROW];
    if (threadIdx.x < 2) block_hits[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t nb = clamped(pair_total, capacity), ns = spair_total ? clamped(spair_total, scapacity) : 0u;
    uint32_t mine_b = 0, mine_s = 0;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));   // in an SGPR: what is selected by chunk is scalar
    const uint32_t cb = (nb + WAVE - 1) / WAVE, cs = (ns + WAVE - 1) / WAVE;   // 64-pair chunks: the bodies' list, then the statics'
    const int lane = lane_id();
    const uint32_t stride = gridDim.x * (PB / WAVE);
    // the pair a lane takes from chunk `c` (wave-uniform choice of list: the bodies', then the statics')
    auto pair_of = [&](uint32_t c, uint2 &pr) {
        const uint2 *list = c < cb ? pairs : spairs;
        const uint32_t p = (c < cb ? c : c - cb) * WAVE + lane, n = c < cb ? nb : ns;
        pr = make_uint2(0, 0);
        if (p < n) pr = list[p];
        return p < n;
    };
    uint32_t ch = blockIdx.x * (PB / WAVE) + wave;
    uint2 pr = make_uint2(0, 0);
    bool pin = ch < cb + cs && pair_of(ch, pr);
    while (ch < cb + cs) {
        const uint2 cur_pr = pr;
        const bool cur_in = pin;
        const uint32_t next = ch + stride;
        if (next < cb + cs) pin = pair_of(next, pr);                     // the next chunk's pair: under this chunk's geoms and arithmetic
        if (ch < cb) mine_b += chunk_from_pair(A, A, cur_pr, cur_in, ch * WAVE, nb, out, flags, flags, tile[wave]);
        else mine_s += chunk_from_pair(A, B, cur_pr, cur_in, (ch - cb) * WAVE, ns, sout, flags, nullptr, tile[wave]);
        ch = next;
    }
    for (int o = 32; o > 0; o >>= 1) { mine_b += __shfl_xor(mine_b, o); mine_s += __shfl_xor(mine_s, o); }
    if (lane_id() == 0) {
        if (mine_b) atomicAdd(&block_hits[0], mine_b);
        if (mine_s) atomicAdd(&block_hits[1], mine_s);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long add = (1ull << 48) | ((unsigned long long)block_hits[1] << 24) | block_hits[0];
        const unsigned long long old = atomicAdd(word, add);
        if ((uint32_t)(old >> 48) == gridDim.x - 1) {                   // the last ticket: `old` holds everybody else's counts
            if (contact_total) *contact_total = (uint32_t)(old & 0xffffffu) + block_hits[0];
            if (scontact_total) *scontact_total = (uint32_t)((old >> 24) & 0xffffffu) + block_hits[1];
            *word = 0;                                                   // ready for the next launch (stream order)
        }
    }
}

// segment_box, mesh_of, sweep_march: sweep_dev.h (shared with the slide)

// phys_body_sweep_capsule: one wavefront per sweep, the candidates of a step spread over the lanes (sweep_march).  MESH:
// one wavefront per workgroup for the LDS stack
template <bool MESH>
__global__ __launch_bounds__(PB)
void k_sweep_capsules(GeomsK A, GeomsK B, MeshSet M, uint32_t n_sweeps, const uint32_t *sweep_body, const float *delta_in,
                      const uint32_t *cand_first, const uint32_t *cand, float *frac_out, float *normal_out, int32_t *hit_out)
{
    constexpr uint32_t SW = MESH ? 1 : PB / WAVE;                         // sweeps per workgroup
    __shared__ uint32_t stk[MESH ? TM_STACK * WAVE : 1], ltri[MESH ? 16 * WAVE : 1], lslot[MESH ? 16 * WAVE : 1];
    const int lane = lane_id();
    const uint32_t sw = blockIdx.x * SW + threadIdx.x / WAVE;
    if (sw >= n_sweeps) return;
    const uint32_t self = sweep_body[sw];
    const float delta[3] = { delta_in[3 * (size_t)sw], delta_in[3 * (size_t)sw + 1], delta_in[3 * (size_t)sw + 2] };
    const float delta_len = sqrtf(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]);
    float best_frac = 1.0f, best_normal[3] = { 0.f, 1.f, 0.f };
    int32_t best_hit = -1;
    if (!(delta_len < 1e-6f) && self < A.n) {
        phd::Geom probe;
        load_geom(A, self, probe);
        const uint32_t c0 = cand_first[sw], c1 = cand_first[sw + 1];
        const SweepLds lds = { stk, ltri, lslot };
        sweep_march<MESH>(A, B, M, probe, self, delta, delta_len, c1 > c0 ? c1 - c0 : 0u,
                          [&](uint32_t k) { return cand[c0 + k]; }, lds, [](uint32_t) {}, best_frac, best_normal, best_hit);
    }
    if (lane == 0) {
        frac_out[sw] = best_frac;
        normal_out[3 * (size_t)sw] = best_normal[0];
        normal_out[3 * (size_t)sw + 1] = best_normal[1];
        normal_out[3 * (size_t)sw + 2] = best_normal[2];
        hit_out[sw] = best_hit;
    }
}

} // namespace clapgpu

using namespace clapgpu;

// workgroups of PB threads of `kernel` that fit the current device at once (`cached`: per kernel and thread, asked once per device).
// CLAPGPU_CONTACTS_GRID, read at every call, overrides it: the A/B knob, and how the tests make every wavefront walk many chunks
struct Resident { int dev = -1; uint32_t groups = 0; };
static uint32_t resident_workgroups(const void *kernel, Resident *cached)
{
    const char *g = getenv("CLAPGPU_CONTACTS_GRID");
    if (g && atoi(g) > 0) return (uint32_t)atoi(g);
    int per_cu = 0, cus = 0, dev = 0;
    if (current_device_cus(&dev, &cus) != CLAPGPU_OK) return 2048;
    if (cached->dev != dev) {
        const bool ok = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, PB, 0) == hipSuccess;
        cached->groups = ok ? (uint32_t)(per_cu > 0 ? per_cu : 1) * (uint32_t)(cus > 0 ? cus : 1) : 2048u;
        cached->dev = dev;                                               // last: a matching dev means groups is set
    }
    return cached->groups;
}

extern "C" int clapgpu_contacts_geoms(void *stream, const clapgpu_geoms *A, const clapgpu_geoms *B, const uint32_t *pairs,
                                      const uint32_t *pair_total, uint32_t capacity, clapgpu_contact2 *contacts,
                                      uint32_t *contact_total, uint32_t *body_flags_a, uint32_t *body_flags_b)
{
    if (!A || !B || !pair_total || (capacity && (!pairs || !contacts)))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (reinterpret_cast<uintptr_t>(contacts) & 15u)                    // the records leave as 16-byte pieces (contacts_chunk)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    hipStream_t s = as_stream(stream);
    if (contact_total)
        CLAPGPU_HIP(hipMemsetAsync(contact_total, 0, sizeof(uint32_t), s));
    if (capacity == 0 || A->n == 0 || B->n == 0)
        return CLAPGPU_OK;
    const uint32_t blocks = (capacity + PB - 1) / PB;
    static thread_local Resident cached;                                 // (see clapgpu_contacts_geoms_both)
    const uint32_t resident = resident_workgroups(reinterpret_cast<const void *>(k_contacts_geoms), &cached);
    hipLaunchKernelGGL(k_contacts_geoms, dim3(blocks < resident ? blocks : resident), dim3(PB), 0, s, geoms_k(A), geoms_k(B),
                       reinterpret_cast<const uint2 *>(pairs), pair_total, capacity, contacts, contact_total, body_flags_a,
                       body_flags_b);
    CLAPGPU_LAUNCH_CHECK("k_contacts_geoms");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_contacts_geoms_both(void *stream, clapgpu_bp *bp, const clapgpu_geoms *bodies, const clapgpu_geoms *statics,
                                           const uint32_t *pairs, const uint32_t *pair_total, uint32_t capacity,
                                           clapgpu_contact2 *contacts, uint32_t *contact_total,
                                           const uint32_t *static_pairs, const uint32_t *static_pair_total, uint32_t static_capacity,
                                           clapgpu_contact2 *static_contacts, uint32_t *static_contact_total, uint32_t *body_flags)
{
    if (!bp || !bodies || !statics || !pair_total || !static_pair_total || (capacity && (!pairs || !contacts)) ||
        (static_capacity && (!static_pairs || !static_contacts)))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if ((reinterpret_cast<uintptr_t>(contacts) | reinterpret_cast<uintptr_t>(static_contacts)) & 15u)   // 16-byte pieces
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (capacity >= (1u << 24) || static_capacity >= (1u << 24))         // the counts travel as 24-bit fields of one word
        return CLAPGPU_ERR_TOO_LARGE;
    hipStream_t s = as_stream(stream);
    if (bodies->n == 0 || (capacity == 0 && static_capacity == 0)) {
        if (contact_total) CLAPGPU_HIP(hipMemsetAsync(contact_total, 0, sizeof(uint32_t), s));
        if (static_contact_total) CLAPGPU_HIP(hipMemsetAsync(static_contact_total, 0, sizeof(uint32_t), s));
        return CLAPGPU_OK;
    }
    const uint32_t blocks = (capacity + static_capacity + PB - 1) / PB;
    // as many workgroups as are resident at once: a wavefront then walks its chunks with the next one's inputs in flight
    static thread_local Resident cached;
    const uint32_t resident = resident_workgroups(reinterpret_cast<const void *>(k_contacts_geoms_both), &cached);
    uint32_t grid = blocks < resident ? blocks : resident;
    // the tickets are the word's top 16 bits: with more than 2^16 workgroups none would see the last one (totals never
    // stored, the word never reset).  The grid-stride loop covers any list with fewer.
    if (grid > (1u << 16)) grid = 1u << 16;
    hipLaunchKernelGGL(k_contacts_geoms_both, dim3(grid), dim3(PB), 0, s, geoms_k(bodies), geoms_k(statics),
                       reinterpret_cast<const uint2 *>(pairs), pair_total, capacity, contacts, contact_total,
                       reinterpret_cast<const uint2 *>(static_pairs), static_pair_total, statics->n ? static_capacity : 0u,
                       static_contacts, static_contact_total, body_flags,
                       clapgpu_bp_contact_ticket(bp));
    CLAPGPU_LAUNCH_CHECK("k_contacts_geoms_both");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_sweep_capsules(void *stream, const clapgpu_geoms *A, const clapgpu_geoms *B,
                                      const clapgpu_trimesh *meshes, uint32_t n_sweeps, const uint32_t *sweep_body,
                                      const float *delta, const uint32_t *cand_first, const uint32_t *cand, float *frac,
                                      float *normal, int32_t *hit)
{
    if (!A || !B || (n_sweeps && (!sweep_body || !delta || !cand_first || !frac || !normal || !hit)))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (meshes && trimesh_set(meshes).n_statics != B->n) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (n_sweeps == 0) return CLAPGPU_OK;
    MeshSet M;
    memset(&M, 0, sizeof(M));
    if (meshes) {
        M = trimesh_set(meshes);
        hipLaunchKernelGGL(k_sweep_capsules<true>, dim3(n_sweeps), dim3(WAVE), 0, as_stream(stream), geoms_k(A), geoms_k(B), M,
                           n_sweeps, sweep_body, delta, cand_first, cand, frac, normal, hit);
    } else {
        hipLaunchKernelGGL(k_sweep_capsules<false>, dim3((n_sweeps + PB / WAVE - 1) / (PB / WAVE)), dim3(PB), 0, as_stream(stream),
                           geoms_k(A), geoms_k(B), M, n_sweeps, sweep_body, delta, cand_first, cand, frac, normal, hit);
    }
    CLAPGPU_LAUNCH_CHECK("k_sweep_capsules");
    return CLAPGPU_OK;
}
