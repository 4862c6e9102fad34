// contacts.hip -- narrowphase contact records and the capsule sweep, for gfx950 (a translation unit of its own so that
// it alone is built with -mllvm -simplifycfg-sink-common=false, see the Makefile).
//
//   k_contacts_geoms[_both]  near_callback's dCollide + phys_contact_surface (physics.c:399-449, 291-330)
//   k_contacts<BOX>          the same for sphere bodies against each other / against static boxes: 104-byte records
//   k_sweep_capsules         phys_body_sweep_capsule (physics.c:559-670), one wavefront per sweep; <true>: candidates
//                            that own a mesh of the mesh set collide through its triangles (tricontact_dev.h)
//   k_mesh_contacts_count / _scan / _write   near_callback for (body, static) pairs whose static owns a mesh: the
//                            triangles under the body's box, the rule of tricontact_dev.h, MAX_CONTACTS, canonical order
//
// Why the flag: phd::collide() writes its (up to two) contacts through CGeom references.  After inlining, LLVM's
// SimplifyCFG sinks the "same" stores of different call sites into one block that stores through a SELECTED pointer
// (c0 or c1), which keeps both contacts addressable: 56 bytes (contacts) / 128 bytes (sweep) of scratch per lane, and
// scratch is HBM traffic on gfx950.  Without the sinking SROA turns them into registers (private segment 0, +6 VGPRs).
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

namespace clapgpu {

constexpr int PB = 256;

// ================================================================================== narrowphase
// GeomsK, load_geom, geoms_k: geoms_dev.h (shared with the ray cast)

// phys_contact_surface (physics.c:291-330) for the two colliders' parameter rows (NULL: defaults), into either record
// type; nc is the caller's
template <typename Rec>
__device__ __forceinline__ void contact_surface(Rec &c, const double *m1, const double *m2)
{
    double bounce = 0, bounce_vel = 0, mu = 0, soft_erp = 0.05, soft_cfm = 0.01;   // physics.c:293-294
    if (m1 && m2) {
        bounce = fmax(m1[0], m2[0]);
        bounce_vel = (m1[1] + m2[1]) * 0.5;
        mu = sqrt(m1[2] * m2[2]);
        if (m1[3] > 0 && m2[3] > 0) soft_erp = fmin(m1[3], m2[3]);
        else if (m1[3] > 0) soft_erp = m1[3];
        else if (m2[3] > 0) soft_erp = m2[3];
        if (m1[4] > 0 && m2[4] > 0) soft_cfm = fmax(m1[4], m2[4]);
        else if (m1[4] > 0) soft_cfm = m1[4];
        else if (m2[4] > 0) soft_cfm = m2[4];
    }
    c.mode = CLAPGPU_CONTACT_SOFT_CFM | CLAPGPU_CONTACT_SOFT_ERP | (bounce > 0 ? CLAPGPU_CONTACT_BOUNCE : 0);
    c.mu = mu; c.bounce = bounce; c.bounce_vel = bounce_vel; c.soft_erp = soft_erp; c.soft_cfm = soft_cfm;
}

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
            for (int a = 0; a < 3; a++) { c.pos[a] = c0.pos[a]; c.normal[a] = c0.normal[a]; }
            c.depth = c0.depth;
            if (nc > 1) {
                for (int a = 0; a < 3; a++) { c.pos2[a] = c1.pos[a]; c.normal2[a] = c1.normal[a]; }
                c.depth2 = c1.depth;
            }
            contact_surface(c, (A.material && B.material) ? A.material + 5 * (size_t)pr.x : nullptr,
                            (A.material && B.material) ? B.material + 5 * (size_t)pr.y : nullptr);
            c.nc = (uint32_t)nc;
            counted = true;
            // plain read-modify-write: every writer of this launch sets the same bit and nothing else changes the word
            if (flags_a && !(flags_a[pr.x] & CLAPGPU_BODY_HAS_JOINT)) flags_a[pr.x] |= CLAPGPU_BODY_HAS_JOINT;
            if (flags_b && !(flags_b[pr.y] & CLAPGPU_BODY_HAS_JOINT)) flags_b[pr.y] |= CLAPGPU_BODY_HAS_JOINT;
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
    for (int a = 0; a < 3; a++) { c.pos[a] = c0.pos[a]; c.normal[a] = c0.normal[a]; }
    c.depth = c0.depth;
    if (nc > 1) {
        for (int a = 0; a < 3; a++) { c.pos2[a] = c1.pos[a]; c.normal2[a] = c1.normal[a]; }
        c.depth2 = c1.depth;
    }
    contact_surface(c, (A.material && B.material) ? A.material + 5 * (size_t)in.pr.x : nullptr,
                    (A.material && B.material) ? B.material + 5 * (size_t)in.pr.y : nullptr);
    c.nc = (uint32_t)nc;
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
    uint32_t np = *pair_total;
    if (np > capacity) np = capacity;
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
    uint32_t nb = *pair_total, ns = spair_total ? *spair_total : 0u;
    if (nb > capacity) nb = capacity;
    if (ns > scapacity) ns = scapacity;
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

// ---- sphere bodies, 104-byte records: near_callback's dCollide + phys_contact_surface (see include/clapgpu.h), one lane
// per candidate pair, IEEE fp64 (sqrt, divide), no contraction.  BOX = false: (body, body) sphere pairs; BOX = true: (body,
// static box) pairs, `other` = static_aabb, `other_material` = the static colliders' parameter rows.
template <bool BOX>
__global__ __launch_bounds__(PB)
void k_contacts(const double *pos, const double *radius, uint32_t n_bodies, const double *other, uint32_t n_other,
                const uint2 *pairs, const uint32_t *pair_total, uint32_t capacity, const double *material,
                const double *other_material, clapgpu_contact *out, uint32_t *contact_total)
{
    __shared__ __attribute__((aligned(16))) double recs[PB / WAVE][WAVE * 13];
    static_assert(sizeof(clapgpu_contact) == 13 * sizeof(double), "contact record layout");
    const uint32_t n_pairs = *pair_total < capacity ? *pair_total : capacity;
    const int lane = lane_id();
    uint32_t found = 0;
    // the pair count is only known on the device: a fixed grid strides over the pairs (a grid sized for
    // the capacity spends 50 us launching empty workgroups)
    for (uint32_t k = blockIdx.x * PB + threadIdx.x; k - lane < n_pairs; k += gridDim.x * PB) {
    double *rec = recs[threadIdx.x / WAVE];
    bool touch = false;
    if (k < n_pairs) {
        const uint2 pr = pairs[k];
        clapgpu_contact c;
        memset(&c, 0, sizeof(c));
        if (pr.x < n_bodies && pr.y < (BOX ? n_other : n_bodies)) {
            const double *p1 = pos + 3 * (size_t)pr.x;
            const double c1[3] = { p1[0], p1[1], p1[2] };
            phd::CGeom g;
            const double *m1 = nullptr, *m2 = nullptr;
            if (BOX) {
                const double *o = other + 6 * (size_t)pr.y;
                const double bb[6] = { o[0], o[1], o[2], o[3], o[4], o[5] };
                touch = phd::collide_sphere_box(c1, radius[pr.x], bb, g) != 0;
                if (material && other_material) { m1 = material + 5 * (size_t)pr.x; m2 = other_material + 5 * (size_t)pr.y; }
            } else {
                const double *o = pos + 3 * (size_t)pr.y;
                const double c2[3] = { o[0], o[1], o[2] };
                touch = phd::collide_spheres(c1, radius[pr.x], c2, radius[pr.y], g) != 0;
                if (material) { m1 = material + 5 * (size_t)pr.x; m2 = material + 5 * (size_t)pr.y; }
            }
            if (touch || BOX) {                                              // collide_sphere_box leaves zeros without a contact
                for (int a = 0; a < 3; a++) { c.pos[a] = g.pos[a]; c.normal[a] = g.normal[a]; }
                c.depth = g.depth;
            }
            if (touch) {
                contact_surface(c, m1, m2);
                c.nc = 1;
            }
        }
        // the 104-byte records of a wave are contiguous in memory: stage them in LDS and write the run as
        // 16-byte pieces (a record per lane straight to memory is 13 scattered 8-byte stores per lane)
        memcpy(rec + (size_t)lane * 13, &c, sizeof(c));
    }
    wave_lds_fence();
    {
        const uint32_t wave_first = k - lane;                       // first pair of this wave
        const uint32_t n_here = wave_first < n_pairs ? (n_pairs - wave_first < WAVE ? n_pairs - wave_first : WAVE) : 0;
        const uint32_t n16 = n_here * (uint32_t)(sizeof(clapgpu_contact) / 8) / 2;      // 16-byte pieces (104 * 64 % 16 == 0 only for even counts)
        const double2 *src = reinterpret_cast<const double2 *>(rec);
        double2 *dst = reinterpret_cast<double2 *>(out + wave_first);
        if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
            for (uint32_t q = lane; q < n16; q += WAVE) dst[q] = src[q];
            if ((n_here & 1) && lane == 0)                          // odd count: the last 8 bytes
                reinterpret_cast<double *>(out + wave_first)[n_here * 13 - 1] = rec[n_here * 13 - 1];
        } else {
            for (uint32_t q = lane; q < n_here * 13; q += WAVE)
                reinterpret_cast<double *>(out + wave_first)[q] = rec[q];
        }
    }
    found += (uint32_t)__popcll(__ballot(touch));
    wave_lds_fence();                                               // the staging tile is reused by the next trip
    }
    // one global atomic per workgroup: same-address atomics serialise at ~12 ns each (4096 of them were
    // 50 us of this kernel)
    __shared__ uint32_t block_found;
    if (threadIdx.x == 0) block_found = 0;
    __syncthreads();
    if (lane == 0 && found) atomicAdd(&block_found, found);
    __syncthreads();
    if (contact_total && threadIdx.x == 0 && block_found)
        atomicAdd(contact_total, block_found);
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


// ================================================================================== contacts against meshes
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
    uint32_t np = *pair_total;
    if (np > capacity) np = capacity;
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
    uint32_t np = *pair_total;
    if (np > capacity) np = capacity;
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
    uint32_t np = *pair_total;
    if (np > capacity) np = capacity;
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
        for (int i = 0; i < 3; i++) { c.pos[i] = c0.pos[i]; c.normal[i] = c0.normal[i]; }
        c.depth = c0.depth;
        if (nc > 1) {
            for (int i = 0; i < 3; i++) { c.pos2[i] = c1.pos[i]; c.normal2[i] = c1.normal[i]; }
            c.depth2 = c1.depth;
        }
        contact_surface(c, m1, m2);
        c.nc = (uint32_t)nc;
        out[o] = c;
        mesh_ref[2 * (size_t)o] = p;
        mesh_ref[2 * (size_t)o + 1] = t;
    }
    // plain read-modify-write: every writer of this launch sets the same bit and nothing else changes the word
    if (body_flags && !(body_flags[s.body] & CLAPGPU_BODY_HAS_JOINT)) body_flags[s.body] |= CLAPGPU_BODY_HAS_JOINT;
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

extern "C" int clapgpu_contacts_spheres(void *stream, const clapgpu_bodies *b, const uint32_t *pairs,
                                        const uint32_t *pair_total, uint32_t capacity, const double *material,
                                        clapgpu_contact *contacts, uint32_t *contact_total)
{
    int rc = check_bodies(b);
    if (rc) return rc;
    if (!pair_total || (capacity && (!pairs || !contacts)))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    hipStream_t s = as_stream(stream);
    if (contact_total)
        CLAPGPU_HIP(hipMemsetAsync(contact_total, 0, sizeof(uint32_t), s));
    if (capacity == 0 || b->n == 0)
        return CLAPGPU_OK;
    // the pair count lives on the device: launch for the capacity, lanes past the count retire at once
    const uint32_t blocks = (capacity + PB - 1) / PB;
    hipLaunchKernelGGL(k_contacts<false>, dim3(blocks < 512 ? blocks : 512), dim3(PB), 0, s,
                       b->pos, b->radius, b->n, nullptr, 0u, reinterpret_cast<const uint2 *>(pairs), pair_total, capacity,
                       material, nullptr, contacts, contact_total);
    CLAPGPU_LAUNCH_CHECK("k_contacts<spheres>");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_contacts_sphere_box(void *stream, const clapgpu_bodies *b, uint32_t n_static,
                                           const double *static_aabb, const uint32_t *pairs, const uint32_t *pair_total,
                                           uint32_t capacity, const double *material, const double *static_material,
                                           clapgpu_contact *contacts, uint32_t *contact_total)
{
    int rc = check_bodies(b);
    if (rc) return rc;
    if (!pair_total || (n_static && !static_aabb) || (capacity && (!pairs || !contacts)))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    hipStream_t s = as_stream(stream);
    if (contact_total)
        CLAPGPU_HIP(hipMemsetAsync(contact_total, 0, sizeof(uint32_t), s));
    if (capacity == 0 || b->n == 0 || n_static == 0)
        return CLAPGPU_OK;
    const uint32_t blocks = (capacity + PB - 1) / PB;
    hipLaunchKernelGGL(k_contacts<true>, dim3(blocks < 512 ? blocks : 512), dim3(PB), 0, s,
                       b->pos, b->radius, b->n, static_aabb, n_static, reinterpret_cast<const uint2 *>(pairs), pair_total,
                       capacity, material, static_material, contacts, contact_total);
    CLAPGPU_LAUNCH_CHECK("k_contacts<sphere_box>");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_sweep_capsules_meshes(void *stream, const clapgpu_geoms *A, const clapgpu_geoms *B,
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

extern "C" int clapgpu_sweep_capsules(void *stream, const clapgpu_geoms *A, const clapgpu_geoms *B, uint32_t n_sweeps,
                                      const uint32_t *sweep_body, const float *delta, const uint32_t *cand_first,
                                      const uint32_t *cand, float *frac, float *normal, int32_t *hit)
{
    return clapgpu_sweep_capsules_meshes(stream, A, B, nullptr, n_sweeps, sweep_body, delta, cand_first, cand, frac, normal, hit);
}

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
