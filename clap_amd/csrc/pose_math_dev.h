// pose_math_dev.h -- the reference's scalar arithmetic of the pose path (interp.h, linmath.h), for k_pose and k_joint_pos_world.
//
// Numerics (round 4): every operation of the path is the reference's operation, in the reference's
// order, with the reference's roundings -- pose.hip is compiled without FMA contraction like the
// rest of the library:
//   * key fraction: the fp32 quotient, correctly rounded (the compiler's IEEE division sequence);
//   * lerp (interp.h:25-29): (float)((double)a * (1.0 - (double)f) + (double)(b * f)) in fp64 on the device;
//   * slerp (interp.h:91-118): theta_0 = (float)acos(dot) and sin(theta_0) depend on the KEY PAIR alone, so
//     clapgpu_animations_pack() evaluates them once per model ON THE HOST with the host's libm -- the very
//     calls the reference makes -- and stores them per key interval; sin(theta) and cos(theta) of the frame
//     are fp64 polynomials on [0, pi/2].  MEASURED against glibc (tools/pose_exact_probe.c, round 5): (float)sin(theta)
//     is glibc's for EVERY float theta of [0, pi/2] (all 1 070 141 404 of them: exact by exhaustion); _rfac =
//     (float)(cos(theta) - u) cancels as fac -> 1 and rounds one float ulp differently in 27 of 10^10 slerps with fac
//     uniform in [0, 1] (the polynomial's cos differs from glibc's in its last fp64 bits for 0.32 % of the arguments):
//     at 3.2 M slerps a frame, one weight of one quaternion one ulp off every ~115 frames;
//     the two quotients by sin(theta_0) are fp64 products with its stored reciprocal, rounded to float: the fp32
//     quotient exactly (a quotient of two floats keeps 2^-49 away from every rounding boundary, the product errs by 2^-52);
//   * hierarchy: global[j] = ((global[parent] * T) * R) * S, evaluated level by level in THAT association
//     (model.c:1363-1383), then * invmx (model.c:1389), * bind's translation column, e->mx * (model.c:1392-1400).
// T / R / S, the palette and the joint positions therefore EQUAL the reference's, bit for bit, except where that one
// subtraction flips (2.7e-9 of the slerps): 0 of 3.2 M joints differ at BASELINE configs[2] in the tests' frames
// (tests/test_pose_skin_gpu.py, tools/pose_exact_check.py), and so do the skinned vertices.
// (Signed zeros included: the "0.f +" that opens mat4x4_mul's sums and turns a -0 sum into +0 is the zero addend of the
// v_pk_fma_f32 that forms the first product -- comb4<true>.)
#pragma once
#include "common.h"

namespace clapgpu {

typedef float v2f __attribute__((ext_vector_type(2)));

// interp.h:25-29 linf_interp: a * (1.0 - blend) + b * blend with float a, b, blend -- the first product and the sum in
// double, b * blend a float product.  g = 1.0 - (double)blend.
__device__ __forceinline__ float lerp_ref(float a, float b, float blend, double g)
{
    const float bf = b * blend;
    const double t = (double)a * g;
    return (float)(t + (double)bf);
}

// sin and cos of x in [0, pi/2] in fp64: Taylor to x^21 / x^22 (|error| < 2 ulp of the double; rounded to float the
// results equal glibc's in 2 * 10^8 of 2 * 10^8 samples).  No range reduction: theta = fac * acos(dot), fac in [0, 1], dot >= 0.
// fma(a, b, c) with the coefficient c taken from an SGPR pair.  (Left to itself the compiler keeps the polynomials' 19
// coefficients in 38 VGPRs for the life of the kernel and copies one with v_mov_b64 in front of every v_fmac_f64.)
__device__ __forceinline__ double fma_coef(double a, double b, double c_uniform)
{
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c_uniform));
    return r;
}
// fma(c0, z, c1) with both coefficients from SGPR pairs (one scalar operand per VALU instruction: c0 goes through a move)
__device__ __forceinline__ double fma_coef2(double c0_uniform, double z, double c1_uniform)
{
    double r;
    asm("v_mov_b64 %0, %2\n\tv_fma_f64 %0, %0, %1, %3" : "=&v"(r) : "v"(z), "s"(c0_uniform), "s"(c1_uniform));
    return r;
}
__device__ __forceinline__ void sincos_halfpi(double x, double &sn, double &cs)
{
    const double z = x * x;
    double ps = fma_coef2(-1.9572941063391263e-20, z, 8.2206352466243295e-18);          // -1/21!, 1/19!
    ps = fma_coef(ps, z, -2.8114572543455206e-15);
    ps = fma_coef(ps, z, 7.6471637318198164e-13);
    ps = fma_coef(ps, z, -1.6059043836821613e-10);
    ps = fma_coef(ps, z, 2.5052108385441720e-08);
    ps = fma_coef(ps, z, -2.7557319223985893e-06);
    ps = fma_coef(ps, z, 1.9841269841269841e-04);
    ps = fma_coef(ps, z, -8.3333333333333332e-03);
    ps = fma_coef(ps, z, 1.6666666666666666e-01);
    sn = __builtin_fma(-(x * z), ps, x);
    double pc = fma_coef2(-8.8967913924505741e-22, z, 4.1103176233121648e-19);           // -1/22!, 1/20!
    pc = fma_coef(pc, z, -1.5619206968586225e-16);
    pc = fma_coef(pc, z, 4.7794773323873853e-14);
    pc = fma_coef(pc, z, -1.1470745597729725e-11);
    pc = fma_coef(pc, z, 2.0876756987868100e-09);
    pc = fma_coef(pc, z, -2.7557319223985888e-07);
    pc = fma_coef(pc, z, 2.4801587301587302e-05);
    pc = fma_coef(pc, z, -1.3888888888888889e-03);
    pc = fma_coef(pc, z, 4.1666666666666664e-02);
    pc = __builtin_fma(pc, z, -0.5);
    cs = __builtin_fma(z, pc, 1.0);
}
__device__ __forceinline__ void slerp_ref(float (&res)[4], const float (&a)[4], const float (&b_in)[4], float fac, const uint4 rcw)
{
    const float theta0 = __uint_as_float(rcw.x);
    const uint32_t flip = rcw.y & 0x80000000u;                   // dot < 0: b = -b, dot = -dot
    const float dot = __uint_as_float(rcw.y & 0x7fffffffu);
    float b[4];
#pragma unroll
    for (int i = 0; i < 4; i++) b[i] = __uint_as_float(__float_as_uint(b_in[i]) ^ flip);
    if (theta0 < 0.0f) {                                         // dot > 0.9995: quat_interp's '+' branch (its own dot is >= 0), vec4_norm
        const float rfac = 1.f - fac;
        float t[4];
#pragma unroll
        for (int i = 0; i < 4; i++) t[i] = rfac * a[i] + fac * b[i];
        float p = t[0] * t[0];                                   // vec4_mul_inner: p = 0; p += b[i] * a[i]
        p += t[1] * t[1];
        p += t[2] * t[2];
        p += t[3] * t[3];
        const float len = sqrtf(p);                                // correctly rounded (__fsqrt_rn is the bare v_sqrt_f32: 1 ulp)
        // vec4_norm's k = 1.0 / len is a DOUBLE quotient rounded to float.  (A Newton / Markstein reciprocal in fp32 ties at
        // len = 1 - 2^-24, the length rounding gives nearly-unit quaternions half of the time, and rounds it to even.)
        const float k = (float)(1.0 / (double)len);
#pragma unroll
        for (int i = 0; i < 4; i++) res[i] = t[i] * k;
        return;
    }
    const float theta = fac * theta0;
    double sd, cd;
    sincos_halfpi((double)theta, sd, cd);
    const float sin_theta = (float)sd;
    const double inv_sin0 = __hiloint2double((int)rcw.w, (int)rcw.z);
    const float u = (float)((double)(dot * sin_theta) * inv_sin0);        // dot * sin_theta / sin_theta_0 in fp32
    const float rf = (float)(cd - (double)u);                             // cos(theta) is a double in the reference
    const float f = (float)((double)sin_theta * inv_sin0);
#pragma unroll
    for (int i = 0; i < 4; i++) res[i] = a[i] * rf + b[i] * f;             // quat_scale, quat_scale, quat_add
}

// One matrix column as two register pairs; out = ((A0 x + A1 y) + A2 z) + A3 w is mat4x4_mul's / mat4x4_mul_vec4_post's
// sum for one column (linmath.h:506-516, 297-305), with separately rounded products and sums: 4 v_pk_mul_f32 (or one
// v_pk_fma_f32 with a zero addend and 3 v_pk_mul_f32) + 3 v_pk_add_f32 per pair of rows.
struct Col { v2f lo, hi; };
__device__ __forceinline__ Col col_of(const float4 v) { Col r; r.lo = v2f{v.x, v.y}; r.hi = v2f{v.z, v.w}; return r; }
__device__ __forceinline__ float4 f4_of(const Col r) { return make_float4(r.lo.x, r.lo.y, r.hi.x, r.hi.y); }
// ZERO_FIRST: mat4x4_mul's "t = 0.f; t += ..." (linmath.h:506-516) -- the add that turns a -0 first product into +0, so that
// a sum of zeros comes out +0 as the reference's does; mat4x4_mul_vec4_post (linmath.h:297-305) has no such add.
template <bool ZERO_FIRST>
__device__ __forceinline__ Col comb4(const Col A0, const Col A1, const Col A2, const Col A3, float x, float y, float z, float w)
{
    Col o;
    if (ZERO_FIRST) {                                            // fma(a, x, +0) = round(a * x) with -0 turned into +0: "0.f + a * x" in one v_pk_fma_f32
        o.lo = __builtin_elementwise_fma(A0.lo, v2f{ x, x }, v2f{ 0.f, 0.f });
        o.hi = __builtin_elementwise_fma(A0.hi, v2f{ x, x }, v2f{ 0.f, 0.f });
    } else {
        o.lo = A0.lo * x; o.hi = A0.hi * x;
    }
    o.lo = o.lo + A1.lo * y; o.hi = o.hi + A1.hi * y;
    o.lo = o.lo + A2.lo * z; o.hi = o.hi + A2.hi * z;
    o.lo = o.lo + A3.lo * w; o.hi = o.hi + A3.hi * w;
    return o;
}

} // namespace clapgpu
