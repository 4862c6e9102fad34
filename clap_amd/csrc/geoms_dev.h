// geoms_dev.h -- a clapgpu_geoms set as the narrowphase kernels read it (contacts.hip, mesh_contacts.hip,
// rays.hip, slide.hip), and the host's checks of the scene a device query reads: the bodies' geoms, the mesh set and the
// broadphase index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "clapgpu.h"
#include "phys_dev.h"
#include "bp_grid.h"
#include "trimesh_dev.h"

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

// ---- the scene checks the device queries share (rays.hip's cast_scene, slide.hip)
// the bodies' geoms, as PhysWorld.body_geoms; false: capsules need their axis
static inline bool body_geoms(const clapgpu_bodies *b, clapgpu_geoms *g)
{
    memset(g, 0, sizeof(*g));
    g->n = b->n; g->pos = b->pos; g->axis = b->axis; g->radius = b->radius; g->length = b->length; g->records = b->geom_records;
    return !b->length || b->axis || b->geom_records;
}

// The index of a scene's query.  meshes (or NULL) must be built for n_static statics.  bp == NULL: *grid = false.
// Otherwise bp must be indexed over exactly (n, aabb) (aabb == NULL: any n boxes) and created with n_static statics:
// *v is its view and *grid = true.  A leveled bp (clapgpu_bp_create_levels) whose index is switched off
// (clapgpu_bp_leveled_index; as created) has no index the queries can read: *grid = false, the scan they take for
// bp == NULL.  Switched on it is held to the same rule as a one-level object.
static inline int scene_grid(const clapgpu_bp *bp, uint32_t n, const double *aabb, uint32_t n_static, const clapgpu_trimesh *meshes,
                             clapgpu::BpGridView *v, bool *grid)
{
    *grid = false;
    if (meshes && clapgpu::trimesh_set(meshes).n_statics != n_static) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!bp || clapgpu_bp_scans(bp)) return CLAPGPU_OK;
    if (!clapgpu_bp_grid_view(bp, n, aabb, v) || v->n_static != n_static) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    *grid = true;
    return CLAPGPU_OK;
}

