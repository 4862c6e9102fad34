// geoms_dev.h -- a clapgpu_geoms set as the narrowphase kernels read it (contacts.hip, rays.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "clapgpu.h"
#include "phys_dev.h"

namespace clapgpu {

struct GeomsK {
    uint32_t n;
    const double *pos, *axis, *radius, *length, *aabb, *material;
    const uint8_t *kind;
    const double *rec;               // [n][8] (pos, axis, radius, length): only for sets without kind / aabb
};

__device__ __forceinline__ void load_geom(const GeomsK &g, uint32_t i, phd::Geom &o)
{
    if (g.rec) {                                                 // spheres and capsules: the whole geom in one 64-byte record
        const double2 *r = reinterpret_cast<const double2 *>(g.rec + 8 * (size_t)i);
        const double2 a = r[0], b = r[1], c = r[2], d = r[3];
        o.pos[0] = a.x; o.pos[1] = a.y; o.pos[2] = b.x;
        o.axis[0] = b.y; o.axis[1] = c.x; o.axis[2] = c.y;
        o.radius = d.x; o.length = d.y;
        o.kind = d.y != 0.0 ? CLAPGPU_GEOM_CAPSULE : CLAPGPU_GEOM_SPHERE;
        for (int k = 0; k < 6; k++) o.aabb[k] = 0.0;
        return;
    }
    o.kind = g.kind ? g.kind[i] : ((g.length && g.length[i] != 0.0) ? CLAPGPU_GEOM_CAPSULE : CLAPGPU_GEOM_SPHERE);
    for (int a = 0; a < 3; a++) {
        o.pos[a] = g.pos ? g.pos[3 * (size_t)i + a] : 0.0;
        o.axis[a] = g.axis ? g.axis[3 * (size_t)i + a] : 0.0;
    }
    o.radius = g.radius ? g.radius[i] : 0.0;
    o.length = g.length ? g.length[i] : 0.0;
    for (int a = 0; a < 6; a++) o.aabb[a] = (g.aabb && o.kind == CLAPGPU_GEOM_BOX) ? g.aabb[6 * (size_t)i + a] : 0.0;
}

} // namespace clapgpu

static inline clapgpu::GeomsK geoms_k(const clapgpu_geoms *g)
{
    clapgpu::GeomsK k;
    k.n = g->n; k.pos = g->pos; k.axis = g->axis; k.radius = g->radius; k.length = g->length; k.aabb = g->aabb;
    k.material = g->material; k.kind = g->kind;
    // the one-sector records stand in for (pos, axis, radius, length) of sphere / capsule sets only
    k.rec = (g->records && !g->kind && !g->aabb && !(reinterpret_cast<uintptr_t>(g->records) & 15u)) ? g->records : nullptr;
    return k;
}

