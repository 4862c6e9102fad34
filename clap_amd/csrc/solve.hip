// solve.hip -- contact response for gfx950: dWorldQuickStep's constraint stage for contact joints, one SOR solve per
// island, islands in parallel; a small island on one lane, a large one level by level on a workgroup.
//
// near_callback leaves penetration to "contact joints and ERP" (physics.c:433-438); the records of the three contact
// lists become quickstep's rows (dxJointContact::getInfo2 of ODE 0.16 as physics.c:291-330 configures it) and are
// relaxed by its SOR iteration, with the row order FIXED to the canonical order of the lists instead of ODE's random
// reordering.  ODE is absent from the reference: the rule is the project's own, stated in include/clapgpu.h, restated in
// tests/solveref.py and held to bit equality -- PARITY UNPINNED.
//   k_solve_count   a fixed number of workgroups, each over one contiguous chunk of the record slots (static list, mesh
//                   list, body list, by capacity): the rows of its chunk into sums[workgroup]; the same launch zeroes
//                   a[], touched[], last_level[], row_level[] and fills the keys with the key that sorts last
//   k_solve_rows    the same walk again, now with the prefix of sums[]: every active contact writes its rows' constants
//                   (J, iMJ, rhs, Ad, cfm / h, lo, hi), its bodies (row_bodies: a dropped row keeps them), lambda = 0
//                   and the key (island << 32) | ordinal
//   (rocPRIM radix sort of the keys inside the caller's scratch: the keys are distinct)
//   k_solve_sweep   one lane per sorted key; the lane at the head of an island's run walks it through all sweeps, or,
//                   when the run has wide_rows rows or more, appends (start, length) to the wide list and leaves.
//                   lambda and a live in global scratch, each lane touching only its own island's words
//   k_solve_sweep_wide (solve_wide.hip; not launched when wide_rows is 0) a fixed grid of workgroups over the wide list
//   k_solve_apply   one lane per body: lvel += h a_lin, avel += h a_ang
// Islands are disjoint in the bodies they write and statics have no state: no atomic on a double and no hand-over
// between workgroups inside a launch; launches hand over at kernel boundaries.  The row total is known on the device
// only: the launches read it and apply nothing when it exceeds rows_capacity.
// The sweep is sequential only between rows that share a body (as a body's run is in push.hip): the lane path pays every
// row of its island as a dependent update, the wide path every LEVEL (solve_wide.hip); both run relax_row
// (solve_dev.h), stated once.
// fp64, no FMA contraction (the Makefile builds with -ffp-contract=off); every sum in the order of the header.
#include <rocprim/device/device_radix_sort.hpp>
#include "common.h"
#include "phys_dev.h"
#include "solve_dev.h"

namespace clapgpu {

constexpr uint32_t SOLVE_BLOCKS_MAX = 1024;             // workgroups of the two counting walks (sums[] is this long)
constexpr uint32_t SOLVE_WIDE_ROWS_DEFAULT = 64;        // clapgpu_solver_defaults' wide_rows: the measured crossover (profiles/solve)

struct SolveLists {
    uint32_t n;                                         // bodies
    uint32_t static_slots, mesh_slots, body_slots;      // slots of each list in the walk (its capacity, 0: absent)
    uint32_t static_pair_capacity;                      // what mesh_ref[k][0] is checked against
    const uint32_t *island, *bflags;
    const uint2 *static_pairs; const uint32_t *static_pair_total; const clapgpu_contact2 *static_contacts;
    const clapgpu_contact2 *mesh_contacts; const uint2 *mesh_ref; const uint32_t *mesh_contact_total;
    const uint2 *pairs; const uint32_t *pair_total; const clapgpu_contact2 *contacts;
};

struct SolveK {
    const double *pos, *quat, *lvel, *avel, *mass, *inertia, *facc;
    double g[3], h, sor_w, cfm;
};

struct SolveBody { double pos[3], v[3], w[3], invM, fext[3], invI[12]; };

__device__ __forceinline__ uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }

// The record of slot s and its bodies; false: the slot holds no active record.
__device__ __forceinline__ bool slot_record(const SolveLists &L, uint64_t s, const clapgpu_contact2 *&rec, uint32_t &b1, uint32_t &b2)
{
    b2 = NONE;
    if (s < L.static_slots) {
        if (s >= min_u32(*L.static_pair_total, L.static_slots)) return false;
        rec = L.static_contacts + s;
        b1 = L.static_pairs[s].x;
    } else if ((s -= L.static_slots) < L.mesh_slots) {
        if (s >= min_u32(*L.mesh_contact_total, L.mesh_slots)) return false;
        const uint32_t ref = L.mesh_ref[s].x;
        if (ref >= min_u32(*L.static_pair_total, L.static_pair_capacity)) return false;
        rec = L.mesh_contacts + s;
        b1 = L.static_pairs[ref].x;
    } else {
        s -= L.mesh_slots;
        if (s >= min_u32(*L.pair_total, L.body_slots)) return false;
        rec = L.contacts + s;
        const uint2 pr = L.pairs[s];
        b1 = pr.x; b2 = pr.y;
        if (b2 >= L.n || b2 == b1) return false;
    }
    if (b1 >= L.n) return false;
    if (L.bflags[b1] & CLAPGPU_BODY_DISABLED) return false;                 // active: body 1 enabled after the island pass
    return L.island[b1] < L.n;
}

// contacts of a record (0, 1, 2) and rows of each (1, or 3 with friction)
__device__ __forceinline__ uint32_t record_rows(const clapgpu_contact2 *rec, uint32_t &nc, uint32_t &per)
{
    nc = min_u32(rec->nc & ~CLAPGPU_CONTACT_DEEP, 2u);
    per = rec->mu > 0 ? 3u : 1u;
    return nc * per;
}

__device__ __forceinline__ uint32_t slot_rows(const SolveLists &L, uint64_t s)
{
    const clapgpu_contact2 *rec;
    uint32_t b1, b2, nc, per;
    return slot_record(L, s, rec, b1, b2) ? record_rows(rec, nc, per) : 0u;
}

// sum of v over the workgroup, in every thread.  lds: SB / WAVE words; all SB threads call it
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *lds)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();                                                        // the words may still be read from a call before
    if (lane_id() == 0) lds[threadIdx.x / WAVE] = v;
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (int k = 0; k < SB / WAVE; k++) t += lds[k];
    return t;
}

// launch 1: the rows of every chunk, and the fills
__global__ __launch_bounds__(SB)
void k_solve_count(SolveLists L, uint64_t slots, uint64_t chunk, uint32_t rows_capacity, uint32_t *sums, uint64_t *keys,
                   double *a, uint32_t *touched, uint32_t *last_level, uint32_t *ctl, uint32_t *row_level, uint32_t *wide_total)
{
    __shared__ uint32_t lds[SB / WAVE];
    const uint64_t lanes = (uint64_t)gridDim.x * SB, lane = (uint64_t)blockIdx.x * SB + threadIdx.x;
    for (uint64_t i = lane; i < L.n; i += lanes) {
#pragma unroll
        for (int k = 0; k < 6; k++) a[6 * i + k] = 0.0;
        touched[i] = 0;
        last_level[i] = 0;
    }
    if (lane == 0) {                                                        // no wide island yet
        ctl[1] = 0;
        if (wide_total) *wide_total = 0;
    }
    if (row_level)
        for (uint64_t i = lane; i < rows_capacity; i += lanes) row_level[i] = 0;
    const uint64_t last = (uint64_t)L.n << 32 | NONE;                       // island n: sorts behind every row
    for (uint64_t i = lane; i < rows_capacity; i += lanes) keys[i] = last;
    const uint64_t begin = blockIdx.x * chunk, end = begin + chunk < slots ? begin + chunk : slots;
    uint32_t c = 0;
    for (uint64_t s = begin + threadIdx.x; s < end; s += SB) c += slot_rows(L, s);
    c = block_sum(c, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = c;
}

__device__ __forceinline__ void load_body(const SolveK &k, const uint32_t *bflags, uint32_t i, SolveBody &B)
{
    const uint32_t fl = bflags[i];
    const bool kin = fl & CLAPGPU_BODY_KINEMATIC;
    const double m = k.mass[i];
    B.invM = kin ? 0.0 : 1.0 / m;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        B.pos[j] = k.pos[3 * (size_t)i + j];
        B.v[j] = k.lvel[3 * (size_t)i + j];
        B.w[j] = k.avel[3 * (size_t)i + j];
        B.fext[j] = (k.facc ? k.facc[3 * (size_t)i + j] : 0.0) + ((fl & CLAPGPU_BODY_NO_GRAVITY) ? 0.0 : m * k.g[j]);
    }
    if (k.inertia && !kin) {
        const double q[4] = { k.quat[4 * (size_t)i], k.quat[4 * (size_t)i + 1], k.quat[4 * (size_t)i + 2], k.quat[4 * (size_t)i + 3] };
        const double inv[3] = { 1.0 / k.inertia[3 * (size_t)i], 1.0 / k.inertia[3 * (size_t)i + 1], 1.0 / k.inertia[3 * (size_t)i + 2] };
        double R[12];
        phd::q_to_R(q, R);
        phd::world_tensor(R, inv, B.invI);
    } else {
#pragma unroll
        for (int j = 0; j < 12; j++) B.invI[j] = 0.0;
    }
}

// dPlaneSpace
__device__ __forceinline__ void plane_space(const double (&n)[3], double (&p)[3], double (&q)[3])
{
    if (fabs(n[2]) > M_SQRT1_2) {
        const double a = n[1] * n[1] + n[2] * n[2];
        const double k = 1.0 / sqrt(a);
        p[0] = 0.0; p[1] = -n[2] * k; p[2] = n[1] * k;
        q[0] = a * k; q[1] = -n[0] * p[2]; q[2] = n[0] * p[1];
    } else {
        const double a = n[0] * n[0] + n[1] * n[1];
        const double k = 1.0 / sqrt(a);
        p[0] = -n[1] * k; p[1] = n[0] * k; p[2] = 0.0;
        q[0] = -n[2] * p[1]; q[1] = n[2] * p[0]; q[2] = a * k;
    }
}

// J of a row along dir: (dir, r1 x dir, -dir, -(r2 x dir)); without body 2 its half is zero and never read
__device__ __forceinline__ void row_jacobian(const double (&dir)[3], const double (&r1)[3], const double (&r2)[3], bool two,
                                             double (&J)[12])
{
    J[0] = dir[0]; J[1] = dir[1]; J[2] = dir[2];
    J[3] = r1[1] * dir[2] - r1[2] * dir[1];
    J[4] = r1[2] * dir[0] - r1[0] * dir[2];
    J[5] = r1[0] * dir[1] - r1[1] * dir[0];
    if (two) {
        J[6] = -dir[0]; J[7] = -dir[1]; J[8] = -dir[2];
        J[9] = -(r2[1] * dir[2] - r2[2] * dir[1]);
        J[10] = -(r2[2] * dir[0] - r2[0] * dir[2]);
        J[11] = -(r2[0] * dir[1] - r2[1] * dir[0]);
    } else {
#pragma unroll
        for (int k = 6; k < 12; k++) J[k] = 0.0;
    }
}

// J . (v1, w1, v2, w2), left to right
__device__ __forceinline__ double row_velocity(const double (&J)[12], const SolveBody &B1, const SolveBody &B2, bool two)
{
    double s = J[0] * B1.v[0];
    s += J[1] * B1.v[1]; s += J[2] * B1.v[2];
    s += J[3] * B1.w[0]; s += J[4] * B1.w[1]; s += J[5] * B1.w[2];
    if (two) {
        s += J[6] * B2.v[0]; s += J[7] * B2.v[1]; s += J[8] * B2.v[2];
        s += J[9] * B2.w[0]; s += J[10] * B2.w[1]; s += J[11] * B2.w[2];
    }
    return s;
}

// the constants of one row
__device__ __forceinline__ void write_row(SolveRow *out, const SolveK &k, const double (&J)[12], const SolveBody &B1,
                                          const SolveBody &B2, bool two, uint32_t b1, uint32_t b2, double c, double cfm,
                                          double lo, double hi)
{
    const double h = k.h;
    double iMJ[12], t[3];
    const double j1a[3] = { J[3], J[4], J[5] }, j2a[3] = { J[9], J[10], J[11] };
    iMJ[0] = B1.invM * J[0]; iMJ[1] = B1.invM * J[1]; iMJ[2] = B1.invM * J[2];
    phd::mul331(t, B1.invI, j1a);
    iMJ[3] = t[0]; iMJ[4] = t[1]; iMJ[5] = t[2];
    if (two) {
        iMJ[6] = B2.invM * J[6]; iMJ[7] = B2.invM * J[7]; iMJ[8] = B2.invM * J[8];
        phd::mul331(t, B2.invI, j2a);
        iMJ[9] = t[0]; iMJ[10] = t[1]; iMJ[11] = t[2];
    } else {
#pragma unroll
        for (int j = 6; j < 12; j++) iMJ[j] = 0.0;
    }
    double s = J[0] * (B1.v[0] / h + B1.invM * B1.fext[0]);
    s += J[1] * (B1.v[1] / h + B1.invM * B1.fext[1]);
    s += J[2] * (B1.v[2] / h + B1.invM * B1.fext[2]);
    s += J[3] * (B1.w[0] / h); s += J[4] * (B1.w[1] / h); s += J[5] * (B1.w[2] / h);
    if (two) {
        s += J[6] * (B2.v[0] / h + B2.invM * B2.fext[0]);
        s += J[7] * (B2.v[1] / h + B2.invM * B2.fext[1]);
        s += J[8] * (B2.v[2] / h + B2.invM * B2.fext[2]);
        s += J[9] * (B2.w[0] / h); s += J[10] * (B2.w[1] / h); s += J[11] * (B2.w[2] / h);
    }
    const double rhs = c / h - s;
    const double cfmh = cfm / h;
    double d = iMJ[0] * J[0];
#pragma unroll
    for (int j = 1; j < 6; j++) d += iMJ[j] * J[j];
    if (two) {
#pragma unroll
        for (int j = 6; j < 12; j++) d += iMJ[j] * J[j];
    }
    d += cfmh;
#pragma unroll
    for (int j = 0; j < 12; j++) { out->J[j] = J[j]; out->iMJ[j] = iMJ[j]; }
    out->rhs = rhs; out->Ad = k.sor_w / d; out->cfmh = cfmh; out->lo = lo; out->hi = hi;
    out->b1 = d == 0.0 ? NONE : b1;
    out->b2 = two ? b2 : NONE;
}

// launch 2: the rows.  ctl[0] = the row total
__global__ __launch_bounds__(SB)
void k_solve_rows(SolveLists L, SolveK k, uint64_t slots, uint64_t chunk, uint32_t rows_capacity, const uint32_t *sums,
                  uint32_t *ctl, uint64_t *keys, SolveRow *rows, uint2 *row_bodies, double *lam, uint32_t *touched, uint64_t *row_key,
                  uint32_t *rows_total, uint32_t *status)
{
    __shared__ uint32_t lds[SB / WAVE];
    uint32_t before = 0, all = 0;
    for (uint32_t j = threadIdx.x; j < gridDim.x; j += SB) {
        const uint32_t v = sums[j];
        all += v;
        if (j < blockIdx.x) before += v;
    }
    const uint32_t total = block_sum(all, lds);
    uint32_t base = block_sum(before, lds);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl[0] = total;
        if (rows_total) *rows_total = total;
        if (status && total > rows_capacity) *status |= 1u;
    }
    if (total > rows_capacity) return;                                      // nothing is written, nothing will be applied
    const uint64_t begin = blockIdx.x * chunk, end = begin + chunk < slots ? begin + chunk : slots;
    for (uint64_t tile = begin; tile < end; tile += SB) {                   // the same trip count for the whole workgroup
        const uint64_t s = tile + threadIdx.x;
        const clapgpu_contact2 *rec = nullptr;
        uint32_t b1 = NONE, b2 = NONE, nc = 0, per = 0, c = 0;
        if (s < end && slot_record(L, s, rec, b1, b2)) c = record_rows(rec, nc, per);
        uint32_t tile_total;
        uint32_t r = base + block_prefix(c, lds, tile_total);
        base += tile_total;
        if (c == 0) continue;
        const bool two = b2 != NONE;
        SolveBody B1, B2;
        load_body(k, L.bflags, b1, B1);
        load_body(k, L.bflags, two ? b2 : b1, B2);
        __hip_atomic_store(touched + b1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // every writer writes 1
        if (two) __hip_atomic_store(touched + b2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t isl = (uint64_t)L.island[b1] << 32;
        const double mu = rec->mu, erp_h = rec->soft_erp / k.h, soft_cfm = rec->soft_cfm;
        const double bounce = rec->bounce, bounce_vel = rec->bounce_vel;
        const bool bouncy = rec->mode & CLAPGPU_CONTACT_BOUNCE;
#pragma unroll
        for (uint32_t j = 0; j < 2; j++) {
            if (j >= nc || (uint64_t)r + per > rows_capacity) break;      // (the second test cannot hold: total fits)
            const double *cp = j ? rec->pos2 : rec->pos, *cn = j ? rec->normal2 : rec->normal;
            const double depth = j ? rec->depth2 : rec->depth;
            const double n[3] = { cn[0], cn[1], cn[2] };
            const double r1[3] = { cp[0] - B1.pos[0], cp[1] - B1.pos[1], cp[2] - B1.pos[2] };
            const double r2[3] = { cp[0] - B2.pos[0], cp[1] - B2.pos[1], cp[2] - B2.pos[2] };
            double J[12];
            row_jacobian(n, r1, r2, two, J);
            double c0 = erp_h * depth;
            if (bouncy) {
                const double out = row_velocity(J, B1, B2, two);
                if (bounce_vel >= 0 && -out > bounce_vel) {
                    const double newc = -bounce * out;
                    if (newc > c0) c0 = newc;
                }
            }
            write_row(rows + r, k, J, B1, B2, two, b1, b2, c0, soft_cfm, 0.0, INFINITY);
            if (per == 3) {
                double t1[3], t2[3];
                plane_space(n, t1, t2);
                row_jacobian(t1, r1, r2, two, J);
                write_row(rows + r + 1, k, J, B1, B2, two, b1, b2, 0.0, k.cfm, -mu, mu);
                row_jacobian(t2, r1, r2, two, J);
                write_row(rows + r + 2, k, J, B1, B2, two, b1, b2, 0.0, k.cfm, -mu, mu);
            }
            for (uint32_t q = 0; q < per; q++) {
                const uint64_t key = isl | (r + q);
                keys[r + q] = key;
                row_bodies[r + q] = make_uint2(b1, b2);
                lam[r + q] = 0.0;
                if (row_key) row_key[r + q] = key;
            }
            r += per;
        }
    }
}

// launch 4: the sweeps.  The head of an island's run of sorted keys walks the run `iterations` times -- or hands a run of
// wide_rows rows or more (wide_rows != 0) to the wide sweep: (start, length) into wide_list[ctl[1]++], in any order
__global__ __launch_bounds__(SB)
void k_solve_sweep(uint32_t n, uint32_t rows_capacity, uint32_t iterations, uint32_t wide_rows, uint32_t *ctl,
                   const uint64_t *keys, const SolveRow *__restrict__ rows, double *lam, double *a, uint2 *wide_list)
{
    const uint32_t i = blockIdx.x * SB + threadIdx.x;
    if (i >= rows_capacity || ctl[0] > rows_capacity) return;
    const uint32_t t = (uint32_t)(keys[i] >> 32);
    if (t >= n) return;                                                     // the unused keys sort last
    if (i > 0 && (uint32_t)(keys[i - 1] >> 32) == t) return;                // not the head of its island's run
    const uint64_t far = (uint64_t)i + wide_rows - 1;                       // the run is sorted: wide when it reaches this far
    if (wide_rows && far < rows_capacity && (uint32_t)(keys[far] >> 32) == t) {
        uint32_t in = (uint32_t)far, out = rows_capacity;                   // keys[in] is the island's, keys[out] (or the end) is not
        while (out - in > 1) {
            const uint32_t mid = in + (out - in) / 2;
            if ((uint32_t)(keys[mid] >> 32) == t) in = mid;
            else out = mid;
        }
        const uint32_t at = atomicAdd(ctl + 1, 1u);
        if (at < rows_capacity) wide_list[at] = make_uint2(i, out - i);     // (it is: an island has a row)
        return;
    }
    for (uint32_t it = 0; it < iterations; it++) {
        for (uint32_t j = i; j < rows_capacity; j++) {
            const uint64_t key = keys[j];
            if ((uint32_t)(key >> 32) != t) break;
            const uint32_t r = (uint32_t)key;
            relax_row(rows, r, lam, a);
        }
    }
}

// launch 5: the velocities of the bodies the rows named
__global__ __launch_bounds__(SB)
void k_solve_apply(uint32_t n, uint32_t rows_capacity, double h, const uint32_t *ctl, const uint32_t *bflags,
                   const uint32_t *touched, const double *a, double *lvel, double *avel)
{
    const uint32_t i = blockIdx.x * SB + threadIdx.x;
    if (i >= n || ctl[0] > rows_capacity || !touched[i]) return;
    if (bflags[i] & (CLAPGPU_BODY_DISABLED | CLAPGPU_BODY_KINEMATIC)) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        lvel[3 * (size_t)i + k] += h * a[6 * (size_t)i + k];
        avel[3 * (size_t)i + k] += h * a[6 * (size_t)i + 3 + k];
    }
}

// the scratch: ctl [64] (0: the row total, 1: the wide islands) | sums [SOLVE_BLOCKS_MAX] | a [n][6] | touched [n] |
// keys [rows] | keys [rows] | rows [rows] | lambda [rows] | the sort's work space, sized for every key bit | the wide
// sweep's: row_bodies [rows][2] | list [rows][2] (every island may be wide: wide_rows == 1) | last_level [n] | level
// [rows] | cursor [rows] | order [rows]
struct SolveLayout {
    size_t ctl, sums, a, touched, keys0, keys1, rows, lam, sort, sort_bytes, row_bodies, wide_list, last_level, level, cursor,
           order, total;
};

static hipError_t solve_layout(uint32_t n, uint32_t rows_capacity, hipStream_t s, SolveLayout &l)
{
    Carve c;
    l.ctl = c.take(64 * sizeof(uint32_t));
    l.sums = c.take(SOLVE_BLOCKS_MAX * sizeof(uint32_t));
    l.a = c.take((size_t)n * 6 * sizeof(double));
    l.touched = c.take((size_t)n * sizeof(uint32_t));
    l.keys0 = c.take((size_t)rows_capacity * sizeof(uint64_t));
    l.keys1 = c.take((size_t)rows_capacity * sizeof(uint64_t));
    l.rows = c.take((size_t)rows_capacity * sizeof(SolveRow));
    l.lam = c.take((size_t)rows_capacity * sizeof(double));
    l.sort_bytes = 0;
    if (rows_capacity) {
        rocprim::double_buffer<uint64_t> none(nullptr, nullptr);
        const hipError_t err = rocprim::radix_sort_keys(nullptr, l.sort_bytes, none, (size_t)rows_capacity, 0, 64, s);
        if (err != hipSuccess) return err;
    }
    l.sort = c.take(l.sort_bytes);
    l.row_bodies = c.take((size_t)rows_capacity * sizeof(uint2));
    l.wide_list = c.take((size_t)rows_capacity * sizeof(uint2));
    l.last_level = c.take((size_t)n * sizeof(uint32_t));
    l.level = c.take((size_t)rows_capacity * sizeof(uint32_t));
    l.cursor = c.take((size_t)rows_capacity * sizeof(uint32_t));
    l.order = c.take((size_t)rows_capacity * sizeof(uint32_t));
    l.total = c.bytes();
    return hipSuccess;
}

} // namespace clapgpu

using namespace clapgpu;

static_assert(sizeof(SolveRow) == 240, "SolveRow");

extern "C" void clapgpu_solver_defaults(clapgpu_solver *s)
{
    if (!s) return;
    s->iterations = 20;                                 // dWorldSetQuickStepNumIterations' default
    s->wide_rows = SOLVE_WIDE_ROWS_DEFAULT;
    s->sor_w = 1.3;                                     // dWorldSetQuickStepW's default
    s->cfm = 1e-10;                                     // dWorldSetCFM's default under dDOUBLE
}

extern "C" size_t clapgpu_bodies_solve_scratch_bytes(uint32_t n, uint32_t rows_capacity)
{
    if (n == 0) return 0;
    SolveLayout l;
    if (solve_layout(n, rows_capacity, nullptr, l) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return l.total;
}

extern "C" int clapgpu_bodies_solve(void *stream, const clapgpu_bodies *b, const clapgpu_world *w, const clapgpu_solver *sv,
                                    double h, const uint32_t *island,
                                    const uint32_t *static_pairs, const uint32_t *static_pair_total, uint32_t static_capacity,
                                    const clapgpu_contact2 *static_contacts,
                                    const clapgpu_contact2 *mesh_contacts, const uint32_t *mesh_ref,
                                    const uint32_t *mesh_contact_total, uint32_t mesh_capacity,
                                    const uint32_t *pairs, const uint32_t *pair_total, uint32_t capacity,
                                    const clapgpu_contact2 *contacts,
                                    uint32_t rows_capacity, void *scratch, double *row_lambda, uint64_t *row_key,
                                    uint32_t *rows_total, uint32_t *status, uint32_t *row_level, uint32_t *wide_total)
{
    int rc = check_bodies(b);
    if (rc) return rc;
    if (!w || !sv) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    const uint32_t n = b->n;
    if (n == 0) return CLAPGPU_OK;
    // a list is there when it has pairs, a counter, records and a capacity; the mesh list needs the static pairs
    const bool have_sp = static_pairs && static_pair_total && static_capacity;
    const bool have_static = have_sp && static_contacts;
    const bool have_mesh = mesh_contacts && mesh_ref && mesh_contact_total && mesh_capacity;
    const bool have_body = pairs && pair_total && contacts && capacity;
    if (have_mesh && !have_sp) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!island || !scratch || (reinterpret_cast<uintptr_t>(scratch) & 255u)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if ((reinterpret_cast<uintptr_t>(pairs) & 7u) || (reinterpret_cast<uintptr_t>(static_pairs) & 7u) ||
        (reinterpret_cast<uintptr_t>(mesh_ref) & 7u) || (reinterpret_cast<uintptr_t>(contacts) & 15u) ||
        (reinterpret_cast<uintptr_t>(static_contacts) & 15u) || (reinterpret_cast<uintptr_t>(mesh_contacts) & 15u) ||
        (reinterpret_cast<uintptr_t>(row_lambda) & 7u) || (reinterpret_cast<uintptr_t>(row_key) & 7u) ||
        (reinterpret_cast<uintptr_t>(island) & 3u) || (reinterpret_cast<uintptr_t>(rows_total) & 3u) ||
        (reinterpret_cast<uintptr_t>(status) & 3u) || (reinterpret_cast<uintptr_t>(row_level) & 3u) ||
        (reinterpret_cast<uintptr_t>(wide_total) & 3u))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    hipStream_t s = as_stream(stream);

    SolveLists L;
    L.n = n;
    L.static_slots = have_static ? static_capacity : 0;
    L.mesh_slots = have_mesh ? mesh_capacity : 0;
    L.body_slots = have_body ? capacity : 0;
    L.static_pair_capacity = have_sp ? static_capacity : 0;
    L.island = island; L.bflags = b->bflags;
    L.static_pairs = reinterpret_cast<const uint2 *>(static_pairs); L.static_pair_total = static_pair_total;
    L.static_contacts = static_contacts;
    L.mesh_contacts = mesh_contacts; L.mesh_ref = reinterpret_cast<const uint2 *>(mesh_ref);
    L.mesh_contact_total = mesh_contact_total;
    L.pairs = reinterpret_cast<const uint2 *>(pairs); L.pair_total = pair_total; L.contacts = contacts;
    const uint64_t slots = (uint64_t)L.static_slots + L.mesh_slots + L.body_slots;
    if (slots > 0xffffffffull / 6) return CLAPGPU_ERR_TOO_LARGE;            // six rows a record: the total stays inside 32 bits
    if (slots == 0) {                                                       // no list: no rows, nothing changes
        if (rows_total) CLAPGPU_HIP(hipMemsetAsync(rows_total, 0, sizeof(uint32_t), s));
        if (wide_total) CLAPGPU_HIP(hipMemsetAsync(wide_total, 0, sizeof(uint32_t), s));
        if (row_level && rows_capacity) CLAPGPU_HIP(hipMemsetAsync(row_level, 0, (size_t)rows_capacity * sizeof(uint32_t), s));
        return CLAPGPU_OK;
    }
    SolveLayout l;
    CLAPGPU_HIP(solve_layout(n, rows_capacity, s, l));
    uint8_t *base = static_cast<uint8_t *>(scratch);
    uint32_t *ctl = reinterpret_cast<uint32_t *>(base + l.ctl), *sums = reinterpret_cast<uint32_t *>(base + l.sums);
    double *a = reinterpret_cast<double *>(base + l.a);
    uint32_t *touched = reinterpret_cast<uint32_t *>(base + l.touched);
    rocprim::double_buffer<uint64_t> keys(reinterpret_cast<uint64_t *>(base + l.keys0), reinterpret_cast<uint64_t *>(base + l.keys1));
    SolveRow *rows = reinterpret_cast<SolveRow *>(base + l.rows);
    double *lam = row_lambda ? row_lambda : reinterpret_cast<double *>(base + l.lam);
    uint2 *row_bodies = reinterpret_cast<uint2 *>(base + l.row_bodies);
    SolveWide wide;
    wide.row_bodies = row_bodies;
    wide.list = reinterpret_cast<uint2 *>(base + l.wide_list);
    wide.last_level = reinterpret_cast<uint32_t *>(base + l.last_level);
    wide.level = reinterpret_cast<uint32_t *>(base + l.level);
    wide.cursor = reinterpret_cast<uint32_t *>(base + l.cursor);
    wide.order = reinterpret_cast<uint32_t *>(base + l.order);

    SolveK k;
    k.pos = b->pos; k.quat = b->quat; k.lvel = b->lvel; k.avel = b->avel; k.mass = b->mass; k.inertia = b->inertia;
    k.facc = b->facc;
    k.g[0] = w->gravity[0]; k.g[1] = w->gravity[1]; k.g[2] = w->gravity[2];
    k.h = h; k.sor_w = sv->sor_w; k.cfm = sv->cfm;

    const uint64_t tiles = (slots + SB - 1) / SB;
    const uint32_t blocks = tiles < SOLVE_BLOCKS_MAX ? (uint32_t)tiles : SOLVE_BLOCKS_MAX;
    const uint64_t chunk = ((tiles + blocks - 1) / blocks) * SB;            // whole tiles per workgroup
    hipLaunchKernelGGL(k_solve_count, dim3(blocks), dim3(SB), 0, s, L, slots, chunk, rows_capacity, sums, keys.current(), a,
                       touched, wide.last_level, ctl, row_level, wide_total);
    CLAPGPU_LAUNCH_CHECK("k_solve_count");
    hipLaunchKernelGGL(k_solve_rows, dim3(blocks), dim3(SB), 0, s, L, k, slots, chunk, rows_capacity, sums, ctl, keys.current(),
                       rows, row_bodies, lam, touched, row_key, rows_total, status);
    CLAPGPU_LAUNCH_CHECK("k_solve_rows");
    if (rows_capacity == 0) return CLAPGPU_OK;                              // any row at all is one too many: status says so
    CLAPGPU_HIP(rocprim::radix_sort_keys(base + l.sort, l.sort_bytes, keys, (size_t)rows_capacity, 0, 32 + bits_of(n), s));
    hipLaunchKernelGGL(k_solve_sweep, dim3((rows_capacity + SB - 1) / SB), dim3(SB), 0, s, n, rows_capacity, sv->iterations,
                       sv->wide_rows, ctl, keys.current(), rows, lam, a, wide.list);
    CLAPGPU_LAUNCH_CHECK("k_solve_sweep");
    if (sv->wide_rows)                                                      // 0: never, and not a launch more than before
        CLAPGPU_HIP(solve_sweep_wide(s, rows_capacity, sv->iterations, ctl, keys.current(), rows, wide, lam, a, row_level,
                                     wide_total));
    hipLaunchKernelGGL(k_solve_apply, dim3((n + SB - 1) / SB), dim3(SB), 0, s, n, rows_capacity, h, ctl, b->bflags, touched, a,
                       b->lvel, b->avel);
    CLAPGPU_LAUNCH_CHECK("k_solve_apply");
    return CLAPGPU_OK;
}
