// contacts_spheres.hip -- the sphere-only narrowphase, for gfx950: near_callback's dCollide + phys_contact_surface
// (physics.c:399-449, 291-330) for sphere bodies against each other and against static boxes, 104-byte records.
//
//   k_contacts<BOX>   false: (body, body) sphere pairs; true: (body, static box) pairs
//
// fp64 throughout, no FMA contraction.  ODE is an absent submodule of the reference: PARITY UNPINNED.
#include <string.h>
#include "common.h"
#include "phys_dev.h"
#include "contact_record_dev.h"

namespace clapgpu {

constexpr int PB = 256;

// near_callback's dCollide + phys_contact_surface for sphere bodies (see include/clapgpu.h), one lane per candidate
// pair, IEEE fp64 (sqrt, divide), no contraction.  BOX = false: (body, body) sphere pairs; BOX = true: (body,
// static box) pairs, `other` = static_aabb, `other_material` = the static colliders' parameter rows.
template <bool BOX>
__global__ __launch_bounds__(PB)
void k_contacts(const double *pos, const double *radius, uint32_t n_bodies, const double *other, uint32_t n_other,
                const uint2 *pairs, const uint32_t *pair_total, uint32_t capacity, const double *material,
                const double *other_material, clapgpu_contact *out, uint32_t *contact_total)
{
    __shared__ __attribute__((aligned(16))) double recs[PB / WAVE][WAVE * 13];
    static_assert(sizeof(clapgpu_contact) == 13 * sizeof(double), "contact record layout");
    const uint32_t n_pairs = clamped(pair_total, capacity);
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

} // namespace clapgpu

using namespace clapgpu;

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
