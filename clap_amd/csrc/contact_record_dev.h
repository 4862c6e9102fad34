// contact_record_dev.h -- what every contact kernel writes into a record once a collider has answered: the surface
// parameters (phys_contact_surface), the one or two contact points, the HAS_JOINT mark of the bodies that touch, and the
// pair count a kernel may read.  Used by contacts.hip, contacts_spheres.hip and mesh_contacts.hip; include it after
// phys_dev.h.
#pragma once
#include "common.h"
#include "phys_dev.h"

namespace clapgpu {

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

// a collider's contacts into a 160-byte record: c0, and c1 when there is a second one.  `second` is the caller's nc > 1
// as a bool: an int tested here changes the compare k_contacts_geoms[_both] are built with
__device__ __forceinline__ void record_points(clapgpu_contact2 &c, bool second, const phd::CGeom &c0, const phd::CGeom &c1)
{
    for (int a = 0; a < 3; a++) { c.pos[a] = c0.pos[a]; c.normal[a] = c0.normal[a]; }
    c.depth = c0.depth;
    if (second) {
        for (int a = 0; a < 3; a++) { c.pos2[a] = c1.pos[a]; c.normal2[a] = c1.normal[a]; }
        c.depth2 = c1.depth;
    }
}

// body i has a contact.  Plain read-modify-write: every writer of a launch sets the same bit and nothing else changes the word
__device__ __forceinline__ void mark_has_joint(uint32_t *flags, uint32_t i)
{
    if (flags && !(flags[i] & CLAPGPU_BODY_HAS_JOINT)) flags[i] |= CLAPGPU_BODY_HAS_JOINT;
}

// the pairs of a list a kernel may read: the device's count, never past what the list holds
__device__ __forceinline__ uint32_t clamped(const uint32_t *pair_total, uint32_t capacity)
{
    const uint32_t n = *pair_total;
    return n > capacity ? capacity : n;
}

} // namespace clapgpu
