// pose_pack.h -- the layout of a model's packed animation pools, for the host that builds them (pose_pack.hip) and the
// code that binds and reads them (pose.hip).  The layout's arithmetic is written here and nowhere else.
//
// `packed`, L = the joints rounded up to whole wavefronts (64, 128, 192, 256), kp = a power of two above the longest channel:
//   times  [n_anims][3][kp][L] f32 (+INF past a channel's last key) | key counts [n_anims][3][L] u32 |
//   (16-byte aligned) values [n_anims][3][k][L] float4 | rotation interval constants [n_anims][k][L] RotConst
// Key-major: key k of (path, joint j) sits at row k, column j.  Columns past the last joint repeat the last joint's
// channels, as the loop's clamped joint index does.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace clapgpu {

// What quat_slerp (interp.h:91-118) computes from the key pair (a, b) of one rotation interval alone, made by the host
// with the host's libm (clapgpu_animations_pack):
//   theta0        (float)acos((double)dot), dot = |quat_inner_product(a, b)|; -1 where dot > 0.9995 (quat_interp)
//   dot_flip      dot, its sign bit set where the inner product was negative (the reference then negates b)
//   inv_sin0      1.0 / (double)(float)sin((double)theta0)
struct RotConst { float theta0, dot_flip; double inv_sin0; };
static_assert(sizeof(RotConst) == 16, "one 16-byte load per lane");

// clapgpu_animations.packed_layout: L / 64 | POSE_LAYOUT_MISSING | POSE_LAYOUT_TAG | n_anims << 16
constexpr uint32_t POSE_LAYOUT_TAG = 0x100u;       // the pools are clapgpu_animations_pack()'s
constexpr uint32_t POSE_LAYOUT_MISSING = 0x010u;   // some (joint, path) has no channel

constexpr int POSE_MAX_JOINTS = 256;               // four wavefronts; JOINTS_MAX is 200 (shader_constants.h:6)
constexpr bool pose_joints_ok(uint32_t nr_joints) { return nr_joints != 0 && nr_joints <= (uint32_t)POSE_MAX_JOINTS; }
constexpr uint32_t pose_lanes(uint32_t nr_joints) { return (nr_joints + 63) / 64 * 64; }

struct PosePack {
    uint32_t n_anims, k, kp, lanes;                // animations, value rows (= the longest channel), time rows, columns (L)

    static constexpr PosePack of(uint32_t n_anims, uint32_t max_keys, uint32_t nr_joints)
    {
        uint32_t kp = 2;
        while (kp <= max_keys) kp <<= 1;           // a power of two STRICTLY above the longest channel: the search's +INF row
        return PosePack{ n_anims, max_keys, kp, pose_lanes(nr_joints) };
    }
    // one animation's part of each pool, in the pool's elements
    constexpr size_t times_stride() const { return (size_t)3 * kp * lanes; }       // f32
    constexpr size_t counts_stride() const { return (size_t)3 * lanes; }           // u32
    constexpr size_t vals_stride() const { return (size_t)3 * k * lanes; }         // float4
    constexpr size_t rc_stride() const { return (size_t)k * lanes; }               // RotConst
    // the head: key times, then key counts -- what k_pose<.., TIMES_LDS = true> stages in LDS
    constexpr size_t time_floats() const { return n_anims * times_stride(); }
    constexpr size_t head_floats() const { return time_floats() + n_anims * counts_stride(); }
    // byte offsets into `packed`
    constexpr size_t counts_offset() const { return time_floats() * 4; }
    constexpr size_t vals_offset() const { return (head_floats() * 4 + 15) & ~(size_t)15; }
    constexpr size_t rc_offset() const { return vals_offset() + n_anims * vals_stride() * 16; }
    constexpr size_t total_bytes() const { return rc_offset() + n_anims * rc_stride() * sizeof(RotConst); }

    constexpr uint32_t layout_word(bool missing) const { return (lanes / 64) | (missing ? POSE_LAYOUT_MISSING : 0u) | POSE_LAYOUT_TAG | (n_anims << 16); }
    constexpr bool made(uint32_t layout_word) const          // by clapgpu_animations_pack() for this skeleton class and animation count
    {
        return (layout_word & POSE_LAYOUT_TAG) && (layout_word & 0xfu) * 64u == lanes && (layout_word >> 16) == n_anims;
    }
};

} // namespace clapgpu
