// runtime.hip -- device binding, memory helpers and the O(1)-per-frame host math
// (view matrix, projection, frustum planes/corners) of libclapgpu.
#include <string.h>
#include <stdlib.h>
#include <math.h>
#include <string>
#include <atomic>
#include "common.h"
#include "lm_dev.h"
#include "views_dev.h"
#include "draw_dev.h"

#ifdef CLAPGPU_EXPERIMENT               // an A/B or sensitivity build (common.h): never loadable as the product
#define ABI_EXPERIMENT_BIT 0x80000000u
#else
#define ABI_EXPERIMENT_BIT 0u
#endif

namespace clapgpu {

static thread_local std::string g_last_error;

int hip_fail(hipError_t err, const char *what)
{
    g_last_error = std::string(what) + ": " + hipGetErrorString(err);
    (void)hipGetLastError();                       // clear the sticky launch error
    if (err == hipErrorOutOfMemory)
        return CLAPGPU_ERR_NOMEM;
    if (err == hipErrorInvalidValue || err == hipErrorInvalidDevicePointer)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    return CLAPGPU_ERR_UNKNOWN;
}

void set_last_error(const char *what) { g_last_error = what; }

// clapgpu_test_fail_after(): < 0 = off; otherwise the number of launch checks that still pass.  Read by every launch
// check on any thread (the bindings' workers, a frame thread): atomic, and armed only in a process that asked for the
// hook in its environment -- a stray call in a shipping process must not turn a healthy device into permanent host
// fallback.
static std::atomic<int> g_fail_after{-1};

hipError_t launch_error()
{
    const hipError_t e = hipGetLastError();
    int left = g_fail_after.load(std::memory_order_relaxed);
    if (left < 0 || e != hipSuccess) return e;
    while (left > 0)
        if (g_fail_after.compare_exchange_weak(left, left - 1, std::memory_order_relaxed)) return e;
    return left == 0 ? hipErrorLaunchFailure : e;                // injected: the kernel itself ran
}

int current_device_cus(int *dev, int *n_cus)
{
    static thread_local struct { int dev, n_cus; } cache = { -1, 0 };
    CLAPGPU_HIP(hipGetDevice(dev));
    if (cache.dev != *dev) {
        CLAPGPU_HIP(hipDeviceGetAttribute(&cache.n_cus, hipDeviceAttributeMultiprocessorCount, *dev));
        cache.dev = *dev;
    }
    *n_cus = cache.n_cus;
    return CLAPGPU_OK;
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" void clapgpu_test_fail_after(int launches)
{
    static const bool armed = getenv("CLAPGPU_TEST_HOOKS") != nullptr;   // tests/test_dropin.py, oracle/ref/dropin.c `fail` set it
    if (armed || launches < 0) g_fail_after.store(launches, std::memory_order_relaxed);
}

extern "C" uint32_t clapgpu_abi_version(void) { return CLAPGPU_ABI_VERSION | ABI_EXPERIMENT_BIT; }

extern "C" const char *clapgpu_last_error(void) { return g_last_error.c_str(); }

extern "C" int clapgpu_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

extern "C" int clapgpu_init(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        g_last_error = "no HIP device";
        return CLAPGPU_ERR_INIT_FAILED;
    }
    if (device < 0 || device >= n)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    CLAPGPU_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    CLAPGPU_HIP(hipGetDeviceProperties(&prop, device));
    if (!strstr(prop.gcnArchName, "gfx950")) {     // the code object holds gfx950 ISA only
        g_last_error = std::string("device is ") + prop.gcnArchName + ", libclapgpu is built for gfx950";
        return CLAPGPU_ERR_NOT_SUPPORTED;
    }
    return CLAPGPU_OK;
}

extern "C" int clapgpu_malloc(void **dev, size_t bytes)
{
    if (!dev) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    CLAPGPU_HIP(hipMalloc(dev, bytes ? bytes : 1));
    return CLAPGPU_OK;
}

extern "C" int clapgpu_free(void *dev)
{
    CLAPGPU_HIP(hipFree(dev));
    return CLAPGPU_OK;
}

extern "C" int clapgpu_host_malloc(void **host, size_t bytes)
{
    if (!host) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    CLAPGPU_HIP(hipHostMalloc(host, bytes ? bytes : 1, hipHostMallocDefault));
    return CLAPGPU_OK;
}

// Page-locked host memory the device can address (zero-copy): *dev_alias is the pointer kernels use.  Coherent
// (fine-grained): a kernel's stores are visible to the host once the kernel has completed, no copy, no cache flush call.
extern "C" int clapgpu_host_malloc_mapped(void **host, void **dev_alias, size_t bytes)
{
    if (!host || !dev_alias) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    CLAPGPU_HIP(hipHostMalloc(host, bytes ? bytes : 1, hipHostMallocMapped | hipHostMallocCoherent));
    const hipError_t e = hipHostGetDevicePointer(dev_alias, *host, 0);
    if (e != hipSuccess) {
        (void)hipHostFree(*host);
        *host = nullptr;
        return hip_fail(e, "hipHostGetDevicePointer");
    }
    return CLAPGPU_OK;
}

extern "C" int clapgpu_wait_word(const volatile uint32_t *word, uint32_t value, void *stream)
{
    if (!word) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    for (uint32_t spins = 0;; spins++) {
        if (*word == value) return CLAPGPU_OK;
        __builtin_ia32_pause();
        if ((spins & 0xffffu) == 0xffffu) {                      // ~ every millisecond: is anything still running?
            const hipError_t e = hipStreamQuery(as_stream(stream));
            if (e == hipSuccess) {
                if (*word == value) return CLAPGPU_OK;
                g_last_error = "clapgpu_wait_word: the stream drained without the word being stored";
                return CLAPGPU_ERR_UNKNOWN;
            }
            if (e != hipErrorNotReady) return hip_fail(e, "hipStreamQuery");
        }
    }
}

extern "C" int clapgpu_host_free(void *host)
{
    CLAPGPU_HIP(hipHostFree(host));
    return CLAPGPU_OK;
}

extern "C" int clapgpu_memcpy_h2d(void *dev, const void *host, size_t bytes, void *stream)
{
    CLAPGPU_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, as_stream(stream)));
    return CLAPGPU_OK;
}

extern "C" int clapgpu_memcpy_d2h(void *host, const void *dev, size_t bytes, void *stream)
{
    CLAPGPU_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, as_stream(stream)));
    return CLAPGPU_OK;
}

extern "C" int clapgpu_memset(void *dev, int value, size_t bytes, void *stream)
{
    CLAPGPU_HIP(hipMemsetAsync(dev, value, bytes, as_stream(stream)));
    return CLAPGPU_OK;
}

extern "C" int clapgpu_stream_sync(void *stream)
{
    CLAPGPU_HIP(hipStreamSynchronize(as_stream(stream)));
    return CLAPGPU_OK;
}

// ---------------------------------------------------------------------------
// Host-side per-frame constants.  Same arithmetic as the kernels (lm_dev.h).
// ---------------------------------------------------------------------------

// transform.c:132-138 (lmd::view_matrix: the statement k_views_calc shares)
extern "C" void clapgpu_view_matrix(const float pos[3], const float quat[4], float view_mx[16])
{
    float t[16];
    const float p[3] = { pos[0], pos[1], pos[2] }, q[4] = { quat[0], quat[1], quat[2], quat[3] };
    lmd::view_matrix(t, p, q);
    memcpy(view_mx, t, sizeof(t));
}

// linmath.h:611-651 / 959-987: the kernels' own arithmetic for host callers (the scene loader's bind = invert(invmx),
// model.c:532; a skin's root pose, gltf.c:1246-1252)
extern "C" void clapgpu_mat4_invert(const float m[16], float out[16])
{
    float a[16], t[16];
    memcpy(a, m, sizeof(a));
    lmd::invert(t, a);
    memcpy(out, t, sizeof(t));
}

extern "C" void clapgpu_mat4_from_quat(const float quat_xyzw[4], float out[16])
{
    float t[16];
    lmd::from_quat(t, quat_xyzw[0], quat_xyzw[1], quat_xyzw[2], quat_xyzw[3]);
    memcpy(out, t, sizeof(t));
}

// linmath.h:709-734 (NDC z in [-1,1]) / 753-776 (NDC z in [0,1])
extern "C" void clapgpu_perspective(float fov, float aspect, float n, float f,
                                    int ndc_z_zero_one, float proj_mx[16])
{
    const float a = (float)(1.0 / tan((double)(fov / 2.f)));
    memset(proj_mx, 0, 16 * sizeof(float));
    proj_mx[0] = a / aspect;
    proj_mx[5] = a;
    proj_mx[11] = -1.f;
    if (ndc_z_zero_one) {
        proj_mx[10] = -(f / (f - n));
        proj_mx[14] = -((f * n) / (f - n));
    } else {
        proj_mx[10] = -((f + n) / (f - n));
        proj_mx[14] = -((2.f * f * n) / (f - n));
    }
}

// light.c:462-471, 385-410 (lmd::light_from_entity, spot_carrier_applies, spot_view_slot_ok: the statements
// k_lights_update shares), the carriers in list order: what the kernel's winners leave
extern "C" void clapgpu_lights_update_host(const clapgpu_entities *e, uint32_t mode, const clapgpu_spots *s,
                                           const clapgpu_lights *lights, clapgpu_views_source *source)
{
    if (spots_check(e, s, lights, source) || s->n == 0 || lights->nr_lights == 0) return;
    for (uint32_t k = 0; s->carrier_view_slot && k < s->n; k++)
        if (s->carrier_view_slot[k] && !spot_view_slot_ok(s->carrier_view_slot[k], source)) {
            *s->status = CLAPGPU_SPOTS_INVALID;
            return;
        }
    *s->status = 0;
    for (uint32_t k = 0; k < s->n; k++) {
        const int32_t l = s->carrier_light[k];
        const uint32_t ent = s->carrier_entity[k];
        if (!spot_carrier_applies(l, ent, lights->nr_lights, e->n, lights->active, e->flags, mode)) continue;
        const bool spot = lmd::light_is_spotlight(lights->is_dir[l], s->cutoff[l]);
        const float *ps = e->pos_scale + 4 * ent, *q = e->rot + 4 * ent, *o = s->carrier_off + 3 * k;
        const float pos[3] = { ps[0], ps[1], ps[2] }, rot[4] = { q[0], q[1], q[2], q[3] }, off[3] = { o[0], o[1], o[2] };
        float lpos[3], dir[3] = { 0.f, 0.f, 0.f };
        lmd::light_from_entity(lpos, dir, pos, off, rot, spot);
        memcpy(lights->pos + 3 * l, lpos, sizeof(lpos));
        if (!spot) continue;
        memcpy(s->dir + 3 * l, dir, sizeof(dir));
        const uint32_t vs = s->carrier_view_slot ? s->carrier_view_slot[k] : 0u;
        if (vs) {                                                    // the bits, NaNs included
            memcpy(source->slot[vs].pos, ps, 3 * sizeof(float));
            memcpy(source->slot[vs].quat, q, 4 * sizeof(float));
        }
    }
}

// model.c:784-1050 (draw_dev.h: the statements the kernels of draw.hip share), txmodel by txmodel, entity by entity
extern "C" void clapgpu_draw_records_host(const clapgpu_entities *e, const uint64_t *vis_mask, const int32_t *lod,
                                          const clapgpu_draw_order *o, const clapgpu_draw_inputs *inputs,
                                          const clapgpu_draw_pass *pass, clapgpu_draw_record *records, uint32_t capacity,
                                          uint32_t *count, uint32_t *group_first, uint32_t *status)
{
    if (draw_check(e, vis_mask, o, pass, records, capacity, count, group_first, status)) return;
    *count = 0;
    *status = 0;
    for (uint32_t g = 0; g <= o->n_groups; g++) group_first[g] = 0;
    if (o->n_order == 0 || e->n == 0) return;
    bool bad = o->group_start[0] != 0u || o->group_start[o->n_groups] != o->n_order;
    for (uint32_t g = 0; g < o->n_groups && !bad; g++) bad = o->group_start[g] > o->group_start[g + 1];
    for (uint32_t r = 0; r < o->n_order && !bad; r++) bad = o->order[r] >= e->n;
    if (bad) { *status = CLAPGPU_DRAW_INVALID; return; }
    clapgpu_draw_inputs in;
    memset(&in, 0, sizeof(in));
    if (inputs) in = *inputs;
    uint32_t total = 0;
    for (uint32_t g = 0; g < o->n_groups; g++) {
        group_first[g] = total;
        if (draw_group_skipped(o->group_flags[g], pass->flags)) continue;
        uint32_t nr_characters = 0;
        for (uint32_t r = o->group_start[g]; r < o->group_start[g + 1]; r++) {
            const uint32_t i = o->order[r];
            if (!draw_entity_drawn(vis_mask, e->flags, i)) continue;
            if (draw_counts_character(in.draw_flags ? in.draw_flags[i] : 0u, pass->mq_nr_characters)) nr_characters++;
            if (total < capacity) {
                clapgpu_draw_record *rec = records + total;
                const DrawTail t = draw_tail(in, *pass, lod, i, g, nr_characters);
                memcpy(rec->mx, e->mx + 16 * (size_t)i, 64);
                memcpy(rec->inv_mx, e->inv_mx + 16 * (size_t)i, 64);
                if (in.color) memcpy(rec->color, in.color + 4 * (size_t)i, 16);
                else memset(rec->color, 0, 16);
                memcpy(&rec->bloom_intensity, t.w, sizeof(t.w));
            }
            total++;
        }
    }
    group_first[o->n_groups] = total;
    *count = total;
    if (total > capacity) *status = CLAPGPU_DRAW_CAPPED;
}

// light.c:404-408, view.c:178-193: fov = cutoff * zoom (1.0f), aspect = (float)1 / (float)1, planes 0.1f and 200.0f
extern "C" void clapgpu_spot_persp(float cutoff, int ndc_z_zero_one, float proj[16])
{
    clapgpu_perspective(cutoff * 1.0f, 1.0f / 1.0f, 0.1f, 200.0f, ndc_z_zero_one, proj);
}

// view.c:248-289 (lmd::frustum_calc: the statement k_views_calc shares)
extern "C" void clapgpu_frustum_calc(const float view_mx[16], const float proj_mx[16],
                                     int ndc_z_zero_one, clapgpu_frustum *out)
{
    static_assert(sizeof(lmd::Frustum) == sizeof(clapgpu_frustum), "frustum layout");
    float v[16], p[16], mvp[16];
    memcpy(v, view_mx, sizeof(v));
    memcpy(p, proj_mx, sizeof(p));
    lmd::Frustum f;
    lmd::frustum_calc(f, mvp, v, p, ndc_z_zero_one != 0);
    memcpy(out, &f, sizeof(f));
}

// camera.c:174-206, 68-91, 101-116, 226-242 (lmd::camera_*: the statements k_camera_calc shares)
extern "C" void clapgpu_camera_target(uint32_t flags, const float pos_scale[4], const float lo[3], const float hi[3],
                                      const float center[3], const float head[3], float far_plane, float target[3], float *dist)
{
    float ps[4], l[3], h[3], c[3], hd[3] = { 0.f, 0.f, 0.f }, t[3], d;
    memcpy(ps, pos_scale, sizeof(ps)); memcpy(l, lo, sizeof(l)); memcpy(h, hi, sizeof(h)); memcpy(c, center, sizeof(c));
    if (head && (flags & CLAPGPU_CAMERA_HAS_HEAD_JOINT)) memcpy(hd, head, sizeof(hd));
    lmd::camera_target(t, d, flags, ps, l, h, c, hd, far_plane);
    memcpy(target, t, sizeof(t));
    *dist = d;
}

extern "C" void clapgpu_camera_rays(const float quat[4], const float target[3], float dist, float near_plane, float aspect,
                                    float corner[16], double ray[32])
{
    float q[4], t[3], cn[4][4];
    double r[4][8];
    memcpy(q, quat, sizeof(q)); memcpy(t, target, sizeof(t));
    lmd::camera_rays(cn, r, q, t, dist, near_plane, aspect);
    memcpy(corner, cn, sizeof(cn));
    memcpy(ray, r, sizeof(r));
}

extern "C" int clapgpu_camera_decide(float dist, const int32_t hit[4], const double depth[4], const double ray[32],
                                     double *min_scale, double *next_dist)
{
    bool h[4];
    double d[4], r[4][8], ms, next = 0.0;
    for (int k = 0; k < 4; k++) { h[k] = hit[k] != 0; d[k] = depth[k]; }
    memcpy(r, ray, sizeof(r));
    const bool good = lmd::camera_decide(ms, next, dist, h, d, r);
    *min_scale = ms;
    if (!good) *next_dist = next;
    return good ? 1 : 0;
}

extern "C" void clapgpu_camera_update_host(clapgpu_camera *cam, void *cast_fn, void *user)
{
    const clapgpu_camera_cast_fn cast = reinterpret_cast<clapgpu_camera_cast_fn>(cast_fn);
    if (cam->moved == 0) { cam->status = 0; cam->iterations = 0; return; }
    lmd::CameraResult o;
    memcpy(o.target, cam->target, sizeof(o.target));
    o.dist = cam->dist;
    float q[4];
    memcpy(q, cam->quat, sizeof(q));
    auto cast4 = [&](const double (&ray)[4][8], bool (&hit)[4], double (&depth)[4]) -> uint32_t {
        int32_t h[4] = { 0, 0, 0, 0 };
        const uint32_t f = cast(user, &ray[0][0], h, depth);
        for (int k = 0; k < 4; k++) hit[k] = h[k] != 0;
        return (f & CLAPGPU_RAY_UNRESOLVED) ? CLAPGPU_CAMERA_UNRESOLVED : 0u;
    };
    lmd::camera_update(o, q, cam->near_plane, cam->aspect, cam->ctl_skip != -1, cast4);
    memcpy(cam->pos, o.pos, sizeof(o.pos));
    memcpy(cam->target, o.target, sizeof(o.target));
    cam->dist = o.dist;
    cam->updated = o.updated;
    if (o.iterations) memcpy(cam->corner, o.corner, sizeof(o.corner));
    cam->iterations = o.iterations;
    cam->status = o.status;
}
