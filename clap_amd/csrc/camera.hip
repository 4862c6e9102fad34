// camera.hip -- the camera controller on the device, for gfx950: camera_update (core/camera.c:208-246) for a camera that
// follows a control entity, as ONE launch that a frame graph can hold.
//
//   k_camera_calc   camera_target, the pull-in loop (four rays from the target to the near-plane corners of the orbiting
//                   camera; the orbit shortens until none is blocked) and the final transform_orbit; the pose goes into
//                   slot 0 of the view block's source, where clapgpu_views_calc picks it up
//
// One workgroup of four wavefronts.  Wavefront w owns corner ray w and casts it with the wave-cooperative cast<> of
// k_ray_cast (ray_cast_dev.h): the same scan or grid walk, the same colliders, the same tie rule.  Given a mesh set it
// then merges the triangles of the meshed statics by k_ray_trimesh's walk and test (trimesh_dev.h, ray_tri_dev.h) on one
// lane -- these are four rays, not a batch, so the other 63 idle for the few leaves a ray reaches.  The four answers meet
// in LDS behind one barrier; a second one keeps the next iteration's answers off them.  Every lane of every wavefront
// keeps the camera's own O(100 flop) arithmetic (lm_dev.h's camera_update, the statement the host twins share): all
// 256 lanes run the same operations on the same values, so the loop's trip count is uniform without a broadcast.
// Where the time goes: each iteration is a dependent chain of one cast (tens of us through a scan of 10^5 geoms, a few
// through the grid) -- what it replaces is the same chain plus a launch, a synchronisation and a download per iteration.
#include "common.h"
#include "lm_dev.h"
#include "views_dev.h"
#include "ray_cast_dev.h"
#include "ray_tri_dev.h"

namespace clapgpu {

constexpr int CB = 4 * WAVE;                            // a wavefront per corner ray

static_assert(lmd::CAMERA_IS_CHARACTER == CLAPGPU_CAMERA_IS_CHARACTER && lmd::CAMERA_HAS_HEAD_JOINT == CLAPGPU_CAMERA_HAS_HEAD_JOINT &&
              lmd::CAMERA_UNRESOLVED == CLAPGPU_CAMERA_UNRESOLVED && lmd::CAMERA_CAPPED == CLAPGPU_CAMERA_CAPPED &&
              lmd::CAMERA_ITER_MAX == CLAPGPU_CAMERA_ITER_MAX, "lm_dev.h restates the header's camera constants");

struct CameraEntK {                                     // what camera_target reads of the frame's entities
    uint32_t n, n_models;
    const float4 *pos_scale;
    const int32_t *model;
    const float4 *model_table;
    const float *center;
};

template <bool LEVELED>
__global__ __launch_bounds__(CB)
void k_camera_calc(CastK k, MeshSet m, bool meshes, clapgpu_camera *cam, CameraEntK e, const float *joint_pos,
                   clapgpu_views_source *src)
{
    // the walk's stack: [TM_STACK][WAVE] as bvh_walk strides it; the four walkers (lane 0 of each wavefront) take columns 0 .. 3
    __shared__ uint32_t stk[TM_STACK * WAVE];
    __shared__ double s_depth[4];
    __shared__ uint32_t s_hit[4], s_flags[4];
    const int lane = lane_id();
    const uint32_t w = threadIdx.x / WAVE;

    if (cam->moved == 0) {                               // camera.c:222: nothing but these two
        if (threadIdx.x == 0) { cam->status = 0; cam->iterations = 0; }
        return;
    }
    const uint32_t flags = cam->flags, ctl = cam->ctl_entity;
    if (ctl >= e.n || ((flags & CLAPGPU_CAMERA_HAS_HEAD_JOINT) && !joint_pos)) {
        if (threadIdx.x == 0) { cam->status = CLAPGPU_CAMERA_INVALID; cam->iterations = 0; }
        return;
    }
    const float quat[4] = { cam->quat[0], cam->quat[1], cam->quat[2], cam->quat[3] };
    const float near_plane = cam->near_plane, far_plane = cam->far_plane, aspect = cam->aspect;
    const int32_t skip = cam->ctl_skip;

    // ---- camera_target
    const float4 ps = e.pos_scale[ctl];
    const int32_t mraw = e.model[ctl];
    const int32_t mi = (uint32_t)mraw < e.n_models ? mraw : 0;                // as the LOD pick reads the table (visible.hip)
    const float4 blo = e.model_table[2 * mi], bhi = e.model_table[2 * mi + 1];
    const float pos_scale[4] = { ps.x, ps.y, ps.z, ps.w }, lo[3] = { blo.x, blo.y, blo.z }, hi[3] = { bhi.x, bhi.y, bhi.z };
    const float center[3] = { e.center[3 * (size_t)ctl], e.center[3 * (size_t)ctl + 1], e.center[3 * (size_t)ctl + 2] };
    float head[3] = { 0.f, 0.f, 0.f };
    if (flags & CLAPGPU_CAMERA_HAS_HEAD_JOINT) {
        const float *j = joint_pos + 4 * (size_t)cam->head_joint;
        head[0] = j[0]; head[1] = j[1]; head[2] = j[2];
    }
    lmd::CameraResult o;
    lmd::camera_target(o.target, o.dist, flags, pos_scale, lo, hi, center, head, far_plane);

    // ---- the loop: one iteration's four rays, a wavefront each
    const uint32_t skip_key = skip_key_of(skip);
    auto cast4 = [&](const double (&ray)[4][8], bool (&hit)[4], double (&depth)[4]) -> uint32_t {
        double in[8];
#pragma unroll
        for (int c = 0; c < 8; c++) in[c] = w == 0 ? ray[0][c] : w == 1 ? ray[1][c] : w == 2 ? ray[2][c] : ray[3][c];
        Ray r;
        uint32_t f = CLAPGPU_RAY_INVALID, key = KEY_NONE;
        double d = 0.0;
        if (make_ray(in, r)) {                           // (uniform in the wavefront: every lane holds the same ray)
            Best b;
            f = cast<LEVELED>(k, r, skip_key, b);
            key = b.key; d = b.depth;
            if (meshes && lane == 0) {                   // k_ray_trimesh's merge (ray_trimesh.hip), for this one ray
                MeshBest mb;
                mb.key = b.key;
                mb.t = b.key == KEY_NONE ? r.len : b.depth;
                mb.tri = 0;
                mb.slot = NO_SLOT;
                Shear q;
                shear_of(r, q);
                bvh_walk(m, stk + w,
                         [&](const float *box, double &tn) { return box_hit(r, q, box, mb.t, tn); },
                         [&](uint32_t slot) { test_tri(m, r, q, slot, skip_key, mb); });
                key = mb.key; d = mb.t;
                f = unresolved(b.other, r.len, mb.key, mb.t);
            }
        }
        if (lane == 0) { s_hit[w] = key != KEY_NONE ? 1u : 0u; s_depth[w] = d; s_flags[w] = f; }
        __syncthreads();
        uint32_t st = 0;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            hit[c] = s_hit[c] != 0;
            depth[c] = s_depth[c];
            if (s_flags[c] & CLAPGPU_RAY_UNRESOLVED) st |= CLAPGPU_CAMERA_UNRESOLVED;
        }
        __syncthreads();                                 // the next iteration's answers stay off these until all have read
        return st;
    };
    lmd::camera_update(o, quat, near_plane, aspect, skip != -1, cast4);

    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) { cam->pos[a] = o.pos[a]; cam->target[a] = o.target[a]; }
        cam->dist = o.dist;
        cam->updated = o.updated;
        if (o.iterations)
#pragma unroll
            for (int c = 0; c < 4; c++)
#pragma unroll
                for (int a = 0; a < 4; a++) cam->corner[c][a] = o.corner[c][a];
        cam->iterations = o.iterations;
        cam->status = o.status;
        clapgpu_view_source &s0 = src->slot[0];          // FROM_POSE: clapgpu_views_calc builds the view from these
#pragma unroll
        for (int a = 0; a < 3; a++) s0.pos[a] = o.pos[a];
#pragma unroll
        for (int a = 0; a < 4; a++) s0.quat[a] = quat[a];
    }
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" int clapgpu_camera_calc(void *stream, clapgpu_camera *cam, const clapgpu_entities *e, const float *joint_pos,
                                   clapgpu_bp *bp, const clapgpu_geoms *bodies, const clapgpu_geoms *statics,
                                   const clapgpu_trimesh *meshes, clapgpu_views_source *source)
{
    if (!view_block_ok(cam) || !view_block_ok(source) || !e || !bodies || !statics) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!e->pos_scale || !e->model || !e->model_table || !e->center) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    CastK k;
    const int rc = cast_scene(k, bp, bodies, nullptr, statics, meshes);
    if (rc) return rc;
    MeshSet m;
    memset(&m, 0, sizeof(m));
    if (meshes) m = trimesh_set(meshes);
    CameraEntK ek;
    ek.n = e->n; ek.n_models = e->n_models;
    ek.pos_scale = reinterpret_cast<const float4 *>(e->pos_scale);
    ek.model = e->model;
    ek.model_table = reinterpret_cast<const float4 *>(e->model_table);
    ek.center = e->center;
    hipLaunchKernelGGL(leveled(k) ? k_camera_calc<true> : k_camera_calc<false>, dim3(1), dim3(CB), 0, as_stream(stream), k, m,
                       meshes != nullptr, cam, ek, joint_pos, source);
    CLAPGPU_LAUNCH_CHECK("k_camera_calc");
    return CLAPGPU_OK;
}
