// pose_pack.hip -- a model's animations as k_pose reads them: the key-major pools of pose_pack.h, built once per model
// ON THE HOST (clapgpu_animations_pack), with what the reference's slerp derives from each key pair by the host's libm.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "common.h"
#include "pose_pack.h"

using namespace clapgpu;

extern "C" size_t clapgpu_animations_packed_bytes(uint32_t n_anims, uint32_t max_keys, uint32_t nr_joints)
{
    if (!n_anims || !max_keys || !pose_joints_ok(nr_joints)) return 0;
    return PosePack::of(n_anims, max_keys, nr_joints).total_bytes();
}

// interp.h:91-118 up to the point where the frame's blend factor enters, for the key pair (a, b): the host's float and
// double arithmetic and the host's libm, as the reference runs it
static RotConst rot_const(const float *a, const float *b)
{
    RotConst rc;
    float dot = 0.f;                                             // quat_inner_product (linmath.h:915-922)
    for (int i = 0; i < 4; i++)
        dot += b[i] * a[i];
    bool flip = false;
    if (dot < 0.0) { dot = -dot; flip = true; }
    if (dot > 0.9995) {                                          // quat_interp: nothing to precompute
        rc.theta0 = -1.0f;
        rc.inv_sin0 = 0.0;
    } else {
        const float theta_0 = (float)acos((double)dot);         // C's acos(float) is the double function (in C++ it would be acosf)
        const float sin_theta_0 = (float)sin((double)theta_0);
        rc.theta0 = theta_0;
        rc.inv_sin0 = 1.0 / (double)sin_theta_0;
    }
    uint32_t bits;
    memcpy(&bits, &dot, 4);
    bits = (bits & 0x7fffffffu) | (flip ? 0x80000000u : 0u);
    memcpy(&rc.dot_flip, &bits, 4);
    return rc;
}

// The model as fetched: its channel records ([anim][joint][path] of (time offset, data offset, keys, -)), then as much
// of the two pools as the records address
namespace {
struct PackSource {
    std::vector<uint32_t> tab;
    std::vector<float> times, data;
    size_t n_times = 0, n_data = 0;
    bool missing = false;                                        // some (joint, path) has no channel
};
}

// No channel longer than max_keys, none that reads past its pool; sizes the pools' fetch
static int pack_check_bounds(const clapgpu_animations *an, uint32_t max_keys, PackSource &src)
{
    for (size_t q = 0; q < src.tab.size() / 4; q++) {
        const uint32_t t_off = src.tab[4 * q], d_off = src.tab[4 * q + 1], nr = src.tab[4 * q + 2];
        if ((int32_t)nr <= 0) { src.missing = true; continue; }
        if (nr > max_keys)
            return CLAPGPU_ERR_INVALID_ARGUMENTS;                 // max_keys is not the longest channel
        const uint32_t stride = (q % 3) == 1 ? 4u : 3u;
        if ((size_t)t_off + nr > src.n_times) src.n_times = (size_t)t_off + nr;
        if ((size_t)d_off + (size_t)nr * stride > src.n_data) src.n_data = (size_t)d_off + (size_t)nr * stride;
    }
    if ((an->n_times && src.n_times > an->n_times) || (an->n_data && src.n_data > an->n_data))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;                     // a channel record that reads past its pool
    return CLAPGPU_OK;
}

// The kernel's bracket search counts the keys below the time (lo = #{t[k] < time}); that is channel_time_to_idx
// (model.c:1266-1288) for strictly increasing key times and for nothing else: the reference's cursor-dependent scan
// gives other pairs on equal or descending times.  Such an asset is refused here, once, not mis-posed every frame.
static int pack_check_key_times(const PackSource &src, size_t J)
{
    for (size_t q = 0; q < src.tab.size() / 4; q++) {
        const uint32_t nr = src.tab[4 * q + 2];
        if ((int32_t)nr <= 1) continue;
        const float *t = src.times.data() + src.tab[4 * q];
        for (uint32_t k = 0; k + 1 < nr; k++)
            if (!(t[k] < t[k + 1])) {
                char msg[160];
                snprintf(msg, sizeof(msg), "clapgpu_animations_pack: key times of animation %zu joint %zu path %zu are not strictly increasing at key %u",
                         q / (3 * J), (q / 3) % J, q % 3, k);
                set_last_error(msg);
                return CLAPGPU_ERR_INVALID_ARGUMENTS;
            }
    }
    return CLAPGPU_OK;
}

// The image of `packed` (pose_pack.h) from a checked source: host arithmetic only
static std::vector<unsigned char> pack_build(const PosePack &lay, uint32_t J, const PackSource &src)
{
    const uint32_t L = lay.lanes, kp = lay.kp, kk = lay.k;
    std::vector<unsigned char> img(lay.total_bytes(), 0);
    float *o_times = reinterpret_cast<float *>(img.data());
    uint32_t *o_nr = reinterpret_cast<uint32_t *>(img.data() + lay.counts_offset());
    float *o_vals = reinterpret_cast<float *>(img.data() + lay.vals_offset());
    RotConst *o_rc = reinterpret_cast<RotConst *>(img.data() + lay.rc_offset());
    for (uint32_t a = 0; a < lay.n_anims; a++)
        for (uint32_t p = 0; p < 3; p++)
            for (uint32_t lane = 0; lane < L; lane++) {
                const uint32_t j = lane < J ? lane : J - 1;
                const uint32_t *e = &src.tab[(((size_t)a * J + j) * 3 + p) * 4];
                const uint32_t nr = (int32_t)e[2] > 0 ? e[2] : 0u;
                const uint32_t stride = p == 1 ? 4u : 3u;
                const float *t = src.times.data() + e[0], *d = src.data.data() + e[1];
                o_nr[a * lay.counts_stride() + p * L + lane] = nr;
                float *ot = o_times + a * lay.times_stride() + (size_t)p * kp * L + lane;
                for (uint32_t k = 0; k < kp; k++)
                    ot[(size_t)k * L] = k < nr ? t[k] : INFINITY;
                float *ov = o_vals + (a * lay.vals_stride() + (size_t)p * kk * L + lane) * 4;
                for (uint32_t k = 0; k < nr; k++) {
                    float *v = ov + (size_t)k * L * 4;
                    v[0] = d[stride * k]; v[1] = d[stride * k + 1]; v[2] = d[stride * k + 2];
                    v[3] = p == 1 ? d[stride * k + 3] : 0.f;
                }
                if (p == 1)                                       // interval k = the key pair (k, k + 1), the last one wraps to key 0
                    for (uint32_t k = 0; k < nr; k++)
                        o_rc[a * lay.rc_stride() + (size_t)k * L + lane] = rot_const(d + 4 * k, d + 4 * (k + 1 < nr ? k + 1 : 0));
            }
    return img;
}

extern "C" int clapgpu_animations_pack(void *stream, const clapgpu_animations *an, uint32_t nr_joints, uint32_t max_keys,
                                       void *packed, uint32_t *packed_layout)
{
    if (!an || !packed || !packed_layout || !an->chan_table || !an->times || !an->data || !an->n_anims || !max_keys)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!pose_joints_ok(nr_joints) || an->n_anims > 0xffffu)
        return CLAPGPU_ERR_TOO_LARGE;
    if ((reinterpret_cast<uintptr_t>(packed) & 15u) != 0)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    const PosePack lay = PosePack::of(an->n_anims, max_keys, nr_joints);
    hipStream_t s = as_stream(stream);

    // fetch and validate: the records, then the pools they address
    PackSource src;
    src.tab.resize((size_t)an->n_anims * nr_joints * 3 * 4);
    CLAPGPU_HIP(hipMemcpyAsync(src.tab.data(), an->chan_table, src.tab.size() * 4, hipMemcpyDeviceToHost, s));
    CLAPGPU_HIP(hipStreamSynchronize(s));
    if (int rc = pack_check_bounds(an, max_keys, src)) return rc;
    src.times.resize(src.n_times ? src.n_times : 1);
    src.data.resize(src.n_data ? src.n_data : 1);
    if (src.n_times) CLAPGPU_HIP(hipMemcpyAsync(src.times.data(), an->times, src.n_times * 4, hipMemcpyDeviceToHost, s));
    if (src.n_data) CLAPGPU_HIP(hipMemcpyAsync(src.data.data(), an->data, src.n_data * 4, hipMemcpyDeviceToHost, s));
    CLAPGPU_HIP(hipStreamSynchronize(s));
    if (int rc = pack_check_key_times(src, nr_joints)) return rc;

    const std::vector<unsigned char> img = pack_build(lay, nr_joints, src);
    CLAPGPU_HIP(hipMemcpyAsync(packed, img.data(), img.size(), hipMemcpyHostToDevice, s));
    CLAPGPU_HIP(hipStreamSynchronize(s));
    *packed_layout = lay.layout_word(src.missing);
    return CLAPGPU_OK;
}
