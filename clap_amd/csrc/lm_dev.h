// lm_dev.h -- fp32 matrix arithmetic for the gfx950 kernels, in the operation
// ORDER of the reference's x86-64 scalar path (core/linmath.h), so that world
// matrices, AABBs and therefore cull decisions come out bit-identical.
//
// Build rule: -ffp-contract=off (hipcc defaults to fast contraction).  The
// reference's x86 path has no FMA; a fused a*b+c changes the last bit of mx,
// which moves AABBs, which flips cull results at frustum edges.
//
// mat4 = float[16] column-major, (col c,row r) at [4c+r].  Everything is
// fully unrolled with compile-time indices so matrices live in VGPRs.
#pragma once
#include <hip/hip_runtime.h>

#define LMD __host__ __device__ __forceinline__
#define E_(m, c, r) ((m)[4 * (c) + (r)])

namespace lmd {

// linmath.h:506-516: out[c][r] = ((0 + a[0][r] b[c][0]) + a[1][r] b[c][1]) + ...
LMD void mul(float (&out)[16], const float (&a)[16], const float (&b)[16])
{
    float t[16];
#pragma unroll
    for (int c = 0; c < 4; c++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 4; k++)
                s += E_(a, k, r) * E_(b, c, k);
            E_(t, c, r) = s;
        }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = t[i];
}

// linmath.h:959-987 with a=w b=x c=y d=z
LMD void from_quat(float (&m)[16], float qx, float qy, float qz, float qw)
{
    float a = qw, b = qx, c = qy, d = qz;
    float a2 = a * a, b2 = b * b, c2 = c * c, d2 = d * d;

    E_(m, 0, 0) = a2 + b2 - c2 - d2;
    E_(m, 0, 1) = 2.f * (b * c + a * d);
    E_(m, 0, 2) = 2.f * (b * d - a * c);
    E_(m, 0, 3) = 0.f;
    E_(m, 1, 0) = 2.f * (b * c - a * d);
    E_(m, 1, 1) = a2 - b2 + c2 - d2;
    E_(m, 1, 2) = 2.f * (c * d + a * b);
    E_(m, 1, 3) = 0.f;
    E_(m, 2, 0) = 2.f * (b * d + a * c);
    E_(m, 2, 1) = 2.f * (c * d - a * b);
    E_(m, 2, 2) = a2 - b2 - c2 + d2;
    E_(m, 2, 3) = 0.f;
    E_(m, 3, 0) = 0.f;
    E_(m, 3, 1) = 0.f;
    E_(m, 3, 2) = 0.f;
    E_(m, 3, 3) = 1.f;
}

LMD void identity(float (&m)[16])
{
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] = (i % 5 == 0) ? 1.f : 0.f;
}

// linmath.h:525-534: M[3][i] += dot4(row_i(M), (x,y,z,0)), dot4 = (((0 + r0 x) + r1 y) + r2 z) + r3*0
LMD void translate_in_place(float (&m)[16], float x, float y, float z)
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        float p = 0.f;
        p += x * E_(m, 0, i);
        p += y * E_(m, 1, i);
        p += z * E_(m, 2, i);
        p += 0.f * E_(m, 3, i);
        E_(m, 3, i) += p;
    }
}

// linmath.h:448-457
LMD void scale_aniso(float (&m)[16], float x, float y, float z)
{
#pragma unroll
    for (int r = 0; r < 4; r++) {
        E_(m, 0, r) = E_(m, 0, r) * x;
        E_(m, 1, r) = E_(m, 1, r) * y;
        E_(m, 2, r) = E_(m, 2, r) * z;
    }
}

// model.c:1618-1622 / 1670-1675: I -> translate_in_place(pos) -> (* R(quat)) -> scale_aniso(s,s,s)
LMD void trs(float (&m)[16], float px, float py, float pz, float s,
             float qx, float qy, float qz, float qw)
{
    float r[16];
    identity(m);
    translate_in_place(m, px, py, pz);
    from_quat(r, qx, qy, qz, qw);
    mul(m, m, r);
    scale_aniso(m, s, s, s);
}

// linmath.h:611-651
LMD void invert(float (&t)[16], const float (&m)[16])
{
    float s0 = E_(m,0,0)*E_(m,1,1) - E_(m,1,0)*E_(m,0,1);
    float s1 = E_(m,0,0)*E_(m,1,2) - E_(m,1,0)*E_(m,0,2);
    float s2 = E_(m,0,0)*E_(m,1,3) - E_(m,1,0)*E_(m,0,3);
    float s3 = E_(m,0,1)*E_(m,1,2) - E_(m,1,1)*E_(m,0,2);
    float s4 = E_(m,0,1)*E_(m,1,3) - E_(m,1,1)*E_(m,0,3);
    float s5 = E_(m,0,2)*E_(m,1,3) - E_(m,1,2)*E_(m,0,3);

    float c0 = E_(m,2,0)*E_(m,3,1) - E_(m,3,0)*E_(m,2,1);
    float c1 = E_(m,2,0)*E_(m,3,2) - E_(m,3,0)*E_(m,2,2);
    float c2 = E_(m,2,0)*E_(m,3,3) - E_(m,3,0)*E_(m,2,3);
    float c3 = E_(m,2,1)*E_(m,3,2) - E_(m,3,1)*E_(m,2,2);
    float c4 = E_(m,2,1)*E_(m,3,3) - E_(m,3,1)*E_(m,2,3);
    float c5 = E_(m,2,2)*E_(m,3,3) - E_(m,3,2)*E_(m,2,3);

    float idet = 1.0f / (s0*c5 - s1*c4 + s2*c3 + s3*c2 - s4*c1 + s5*c0);

    E_(t,0,0) = ( E_(m,1,1)*c5 - E_(m,1,2)*c4 + E_(m,1,3)*c3) * idet;
    E_(t,0,1) = (-E_(m,0,1)*c5 + E_(m,0,2)*c4 - E_(m,0,3)*c3) * idet;
    E_(t,0,2) = ( E_(m,3,1)*s5 - E_(m,3,2)*s4 + E_(m,3,3)*s3) * idet;
    E_(t,0,3) = (-E_(m,2,1)*s5 + E_(m,2,2)*s4 - E_(m,2,3)*s3) * idet;

    E_(t,1,0) = (-E_(m,1,0)*c5 + E_(m,1,2)*c2 - E_(m,1,3)*c1) * idet;
    E_(t,1,1) = ( E_(m,0,0)*c5 - E_(m,0,2)*c2 + E_(m,0,3)*c1) * idet;
    E_(t,1,2) = (-E_(m,3,0)*s5 + E_(m,3,2)*s2 - E_(m,3,3)*s1) * idet;
    E_(t,1,3) = ( E_(m,2,0)*s5 - E_(m,2,2)*s2 + E_(m,2,3)*s1) * idet;

    E_(t,2,0) = ( E_(m,1,0)*c4 - E_(m,1,1)*c2 + E_(m,1,3)*c0) * idet;
    E_(t,2,1) = (-E_(m,0,0)*c4 + E_(m,0,1)*c2 - E_(m,0,3)*c0) * idet;
    E_(t,2,2) = ( E_(m,3,0)*s4 - E_(m,3,1)*s2 + E_(m,3,3)*s0) * idet;
    E_(t,2,3) = (-E_(m,2,0)*s4 + E_(m,2,1)*s2 - E_(m,2,3)*s0) * idet;

    E_(t,3,0) = (-E_(m,1,0)*c3 + E_(m,1,1)*c1 - E_(m,1,2)*c0) * idet;
    E_(t,3,1) = ( E_(m,0,0)*c3 - E_(m,0,1)*c1 + E_(m,0,2)*c0) * idet;
    E_(t,3,2) = (-E_(m,3,0)*s3 + E_(m,3,1)*s1 - E_(m,3,2)*s0) * idet;
    E_(t,3,3) = ( E_(m,2,0)*s3 - E_(m,2,1)*s1 + E_(m,2,2)*s0) * idet;
}

// linmath.h:297-305 with v = (x,y,z,w): ((m0 x + m1 y) + m2 z) + m3 w, rows 0..2 only
LMD void mul_point3(float &ox, float &oy, float &oz, const float (&m)[16],
                    float x, float y, float z, float w)
{
    float t0 = E_(m,0,0) * x + E_(m,1,0) * y + E_(m,2,0) * z;  t0 += E_(m,3,0) * w;
    float t1 = E_(m,0,1) * x + E_(m,1,1) * y + E_(m,2,1) * z;  t1 += E_(m,3,1) * w;
    float t2 = E_(m,0,2) * x + E_(m,1,2) * y + E_(m,2,2) * z;  t2 += E_(m,3,2) * w;
    ox = t0; oy = t1; oz = t2;
}

LMD void mul_vec4(float (&o)[4], const float (&m)[16], const float (&v)[4])
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        float t = E_(m,0,i) * v[0] + E_(m,1,i) * v[1] + E_(m,2,i) * v[2];
        t += E_(m,3,i) * v[3];
        o[i] = t;
    }
}

// util.h:188-201: ternary min / max (kept literal for NaN ordering)
LMD float tmin(float a, float b) { return a < b ? a : b; }
LMD float tmax(float a, float b) { return a > b ? a : b; }

// util.h:104-109 aabb_center: three separate operations
LMD void box_center(float (&ctr)[3], const float (&bb)[6])
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float d = bb[3 + k] - bb[k];
        d = d * 0.5f;
        ctr[k] = d + bb[k];
    }
}

// model.c:1200-1234 (corner order 1207-1216): all eight corners through mul_point3 and a compare-and-keep chain
LMD void world_box_literal(float (&bb)[6], const float (&m)[16],
                           float lx, float ly, float lz, float hx, float hy, float hz)
{
    bb[0] = bb[1] = bb[2] = INFINITY;
    bb[3] = bb[4] = bb[5] = -INFINITY;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        float x = (i & 4) ? hx : lx;
        float y = (i & 1) ? hy : ly;
        float z = (i & 2) ? hz : lz;
        float vx, vy, vz;
        mul_point3(vx, vy, vz, m, x, y, z, 1.0f);
        bb[0] = tmin(vx, bb[0]);  bb[3] = tmax(vx, bb[3]);
        bb[1] = tmin(vy, bb[1]);  bb[4] = tmax(vy, bb[4]);
        bb[2] = tmin(vz, bb[2]);  bb[5] = tmax(vz, bb[5]);
    }
}

LMD void world_aabb_literal(float (&bb)[6], float (&ctr)[3], const float (&m)[16],
                            float lx, float ly, float lz, float hx, float hy, float hz)
{
    world_box_literal(bb, m, lx, ly, lz, hx, hy, hz);
    box_center(ctr, bb);
}

// The finiteness of many values in one register: v * 0 is +-0 for a finite v and NaN for an infinity or a NaN, and a sum
// keeps a NaN, so `acc` is +-0 while every value fed to it was finite (fabsf(v) <= FLT_MAX) and NaN after the first that
// was not.  Each value is tested on its own (fmaxf over the magnitudes would drop a NaN) at one instruction a value; as a
// chain of compares the compiler assembled a bit mask, four instructions a value.  An explicit fma: -ffp-contract=off
// is about a * b + c written apart.
LMD float nan_unless_finite(float acc, float v) { return __builtin_fmaf(v, 0.0f, acc); }

// The same box from its two extreme corners per axis instead of all eight.  A corner's world coordinate a is the fp32
// chain ((m0a x + m1a y) + m2a z) + m3a 1 (mul_point3).  Rounding is monotone, so the chain is non-decreasing in each of
// its three products: the largest of the eight values is the chain over max(m0a lx, m0a hx), max(m1a ly, m1a hy),
// max(m2a lz, m2a hz), the smallest the chain over the three minima -- the operations and operands of one of the eight
// corners, hence its bits.  Which of two equal values the literal chain keeps shows only in the sign of a zero, and a
// zero result can be -0 only where the translation term m3a is -0 (exact cancellation gives +0, and +-0 + +0 is +0).
// A non-finite product or translation breaks monotonicity (inf - inf).  Returns false, with bb unspecified, for those
// two cases: the caller takes the literal chain then.
LMD bool world_box_extremes(float (&bb)[6], const float (&m)[16],
                            float lx, float ly, float lz, float hx, float hy, float hz)
{
    float finite = 0.0f;
    uint32_t not_neg0 = 0xffffffffu;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float ax = E_(m,0,a) * lx, bx = E_(m,0,a) * hx;
        const float ay = E_(m,1,a) * ly, by = E_(m,1,a) * hy;
        const float az = E_(m,2,a) * lz, bz = E_(m,2,a) * hz;
        const float d = E_(m,3,a) * 1.0f;
        // (one chain for the three axes: a chain each cost k_entities_tiles<true> a wavefront per SIMD in registers)
        finite = nan_unless_finite(nan_unless_finite(finite, ax), bx);
        finite = nan_unless_finite(nan_unless_finite(finite, ay), by);
        finite = nan_unless_finite(nan_unless_finite(finite, az), bz);
        finite = nan_unless_finite(finite, d);
        const uint32_t d_flipped = __builtin_bit_cast(uint32_t, d) ^ 0x80000000u;      // 0 for -0.0 alone
        not_neg0 = d_flipped < not_neg0 ? d_flipped : not_neg0;
        float h = fmaxf(ax, bx) + fmaxf(ay, by);  h = h + fmaxf(az, bz);  h = h + d;
        float l = fminf(ax, bx) + fminf(ay, by);  l = l + fminf(az, bz);  l = l + d;
        bb[a] = l;  bb[3 + a] = h;
    }
    return finite == 0.0f && not_neg0 != 0u;
}

// entity3d_aabb_update: world box and centre, bit for bit world_aabb_literal's.  The fallback branch holds arithmetic
// only -- no load, no store: entities.hip's straight-line row counts its memory operations.
LMD void world_aabb(float (&bb)[6], float (&ctr)[3], const float (&m)[16],
                    float lx, float ly, float lz, float hx, float hy, float hz)
{
    if (!world_box_extremes(bb, m, lx, ly, lz, hx, hy, hz))
        world_box_literal(bb, m, lx, ly, lz, hx, hy, hz);
    box_center(ctr, bb);
}

struct Frustum {
    float planes[6][4];
    float corners[8][4];
};

// view.c:296-337.  dot4 order: (((0 + x px) + y py) + z pz) + 1 pw, compared `< 0.0`.
LMD bool aabb_in_frustum(const Frustum &f, const float (&bb)[6])
{
#pragma unroll
    for (int i = 0; i < 6; i++) {
        int r = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            float x = (k & 1) ? bb[3] : bb[0];
            float y = (k & 2) ? bb[4] : bb[1];
            float z = (k & 4) ? bb[5] : bb[2];
            float p = 0.f;
            p += x * f.planes[i][0];
            p += y * f.planes[i][1];
            p += z * f.planes[i][2];
            p += 1.0f * f.planes[i][3];
            r += (p < 0.0f) ? 1 : 0;
        }
        if (r == 8)
            return false;
    }
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        int r = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) r += (f.corners[i][ax] > bb[3 + ax]) ? 1 : 0;
        if (r == 8) return false;
        r = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) r += (f.corners[i][ax] < bb[ax]) ? 1 : 0;
        if (r == 8) return false;
    }
    return true;
}

// Kernel-side frustum: the reference's planes/corners plus per-axis extremes of the 8
// frustum corners, precomputed on the host (make_frustum_k in entities_args.h).
struct FrustumK {
    Frustum  f;
    float    cmin[3];      // min_i corners[i][ax], NaN if any is NaN
    float    cmax[3];      // max_i corners[i][ax], NaN if any is NaN
    uint32_t finite;       // every plane component is finite
};

// Same decisions as aabb_in_frustum with ~1/8 of the arithmetic:
//  * plane i rejects iff all 8 corner dots are < 0 iff the LARGEST dot is < 0.  Each dot is the
//    fp32 chain (((0 + x px) + y py) + z pz) + pw; rounding is monotone, so the chain is
//    non-decreasing in every product and the largest value is reached at the corner that takes
//    max[a] where the plane component is >= 0 and min[a] otherwise -- the same fp32 operations
//    on the same operands, hence the same bits.  With a non-finite box or plane (0 * inf = NaN
//    breaks monotonicity) the literal 8-corner test is used.
//  * "all 8 frustum corners beyond the box on axis a" compares the per-axis extreme only.
LMD bool aabb_in_frustum_fast(const FrustumK &k, const float (&bb)[6])
{
    bool box_finite = true;
#pragma unroll
    for (int a = 0; a < 6; a++) box_finite = box_finite && (fabsf(bb[a]) <= 3.402823466e+38f);
    if (!(k.finite && box_finite))
        return aabb_in_frustum(k.f, bb);
#pragma unroll
    for (int i = 0; i < 6; i++) {
        // (fmin/fmax: a stored box with max < min is still handled exactly)
        const float x = (k.f.planes[i][0] >= 0.f) ? fmaxf(bb[0], bb[3]) : fminf(bb[0], bb[3]);
        const float y = (k.f.planes[i][1] >= 0.f) ? fmaxf(bb[1], bb[4]) : fminf(bb[1], bb[4]);
        const float z = (k.f.planes[i][2] >= 0.f) ? fmaxf(bb[2], bb[5]) : fminf(bb[2], bb[5]);
        float p = 0.f;
        p += x * k.f.planes[i][0];
        p += y * k.f.planes[i][1];
        p += z * k.f.planes[i][2];
        p += 1.0f * k.f.planes[i][3];
        if (p < 0.0f)
            return false;
    }
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        if (k.cmin[ax] > bb[3 + ax]) return false;
        if (k.cmax[ax] < bb[ax]) return false;
    }
    return true;
}

// ---- libm cbrtf for the LOD pick (visible.hip) and the camera (below) ----
// glibc 2.35 sysdeps/ieee754/flt-32/s_cbrtf.c restated (the reference calls libm cbrtf(),
// model.c:1263): the float is rescaled by frexpf, a quadratic start and one Halley step run in
// double, ldexpf rescales.  Bit-identical to libm on every one of 3.0e8 floats probed over the
// whole normal range, which is what makes the integer LOD exact.
LMD float cbrtf_glibc(float x)
{
    int xe;
    const float xm = frexpf(fabsf(x), &xe);
    if (xe == 0 && (x == 0.0f || x != x || isinf(x)))
        return x + x;
    const float u = (float)(0.492659620528969547 + (0.697570460207922770 - 0.191502161678719066 * (double)xm) * (double)xm);
    const float t2 = u * u * u;
    const int r = xe % 3;
    const double f = r == -2 ? 1.0 / 1.5874010519681994748 : r == -1 ? 1.0 / 1.2599210498948731648
                   : r == 0 ? 1.0 : r == 1 ? 1.2599210498948731648 : 1.5874010519681994748;
    const float ym = (float)((double)u * ((double)t2 + 2.0 * (double)xm) / (2.0 * (double)t2 + (double)xm) * f);
    return ldexpf(x > 0.0f ? ym : -ym, xe / 3);
}

// ---- a view: the O(1)-per-frame arithmetic of the host entry points (runtime.hip) and of k_views_calc (views.hip) ----
// Stated once, here, for both machines.  What an invalid operation leaves in a NaN's sign and payload is the machine's
// (x86: 0xffc00000, gfx950: 0x7fc00000) and nothing reads it: whatever these functions store goes through one_nan.
LMD float one_nan(float v) { return v != v ? __builtin_nanf("") : v; }

// transform.c:132-138: I * R(quat), transpose the 3x3, translate_in_place(-pos)
LMD void view_matrix(float (&out)[16], const float (&pos)[3], const float (&quat)[4])
{
    float m[16], r[16], t[16];
    identity(m);
    from_quat(r, quat[0], quat[1], quat[2], quat[3]);
    mul(m, m, r);
#pragma unroll
    for (int i = 0; i < 16; i++) t[i] = m[i];
#pragma unroll
    for (int c = 0; c < 3; c++)                      // linmath.h:408-416
#pragma unroll
        for (int rr = 0; rr < 3; rr++)
            t[4 * c + rr] = m[4 * rr + c];
    // The negated position reaches translate_in_place as a value, not as a negation the device compiler can move: it
    // turns 0 + (-x) m0 + (-y) m1 into (-(x m0)) - y m1, without the +0 that makes a zero sum +0 (a camera at the origin
    // came out with -0 in the translation).  The host compiler does not; the barrier costs nothing.
    float npos[3] = { -pos[0], -pos[1], -pos[2] };
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(npos[0]), "+v"(npos[1]), "+v"(npos[2]));
#endif
    translate_in_place(t, npos[0], npos[1], npos[2]);
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = one_nan(t[i]);
}

// view.c:248-289: mvp = proj * view, the planes and the corners
LMD void frustum_calc(Frustum &out, float (&mvp)[16], const float (&v)[16], const float (&p)[16], bool ndc_z_zero_one)
{
    float inv[16];
    mul(mvp, p, v);
    invert(inv, mvp);
    // planes = row3(mvp) +/- row{0,1,2}(mvp)  (view.c:271,275-280 via the transpose)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float r0 = mvp[4 * k + 0], r1 = mvp[4 * k + 1], r2 = mvp[4 * k + 2], r3 = mvp[4 * k + 3];
        out.planes[0][k] = one_nan(r3 + r0);
        out.planes[1][k] = one_nan(r3 - r0);
        out.planes[2][k] = one_nan(r3 + r1);
        out.planes[3][k] = one_nan(r3 - r1);
        out.planes[4][k] = one_nan(r3 + r2);
        out.planes[5][k] = one_nan(r3 - r2);
    }
    const float zn = ndc_z_zero_one ? 0.f : -1.f;   // view.c:252-265
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const float sx = (i == 0 || i == 3 || i == 4 || i == 7) ? -1.f : 1.f;
        const float sy = ((i & 3) < 2) ? -1.f : 1.f;
        const float c[4] = { sx, sy, i < 4 ? zn : 1.f, 1.f };
        float q[4];
        mul_vec4(q, inv, c);
        const float s = 1.f / q[3];
#pragma unroll
        for (int k = 0; k < 4; k++)
            out.corners[i][k] = one_nan(q[k] * s);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) mvp[i] = one_nan(mvp[i]);
}

// The cull's constants of a frustum (FrustumK above): per-axis extremes of the corners (NaN if any corner is NaN, so the
// comparison is false exactly when the reference's count cannot reach 8) and "every plane component is finite".
LMD void frustum_constants(FrustumK &k)
{
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        float lo = __builtin_inff(), hi = -__builtin_inff();
        bool nan = false;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const float c = k.f.corners[i][ax];
            nan = nan || (c != c);
            lo = c < lo ? c : lo;
            hi = c > hi ? c : hi;
        }
        k.cmin[ax] = nan ? __builtin_nanf("") : lo;
        k.cmax[ax] = nan ? __builtin_nanf("") : hi;
    }
    k.finite = 1;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (!(__builtin_fabsf(k.f.planes[i][c]) <= 3.402823466e+38f))
                k.finite = 0;
}

// ---- the camera controller: camera_update (core/camera.c:51-117, 174-246) over transform_orbit (transform.c:109-123) ----
// Stated once, here, for k_camera_calc (camera.hip) and for the host's clapgpu_camera_* (runtime.hip): fp32 and fp64
// where the reference has them, its order of operations, and whatever is stored goes through one_nan.  The rule is in
// include/clapgpu.h ("The camera controller on the device").
constexpr uint32_t CAMERA_IS_CHARACTER = 1u, CAMERA_HAS_HEAD_JOINT = 2u;          // CLAPGPU_CAMERA_* (flags)
constexpr uint32_t CAMERA_UNRESOLVED = 1u, CAMERA_CAPPED = 2u;                    // CLAPGPU_CAMERA_* (status)
constexpr uint32_t CAMERA_ITER_MAX = 16384u;

// linmath.h:939-958: t = 2 cross(q.xyz, v); r = (v + q.w t) + cross(q.xyz, t)
LMD void quat_mul_vec3(float (&r)[3], const float (&q)[4], const float (&v)[3])
{
    float t[3], u[3];
    t[0] = q[1] * v[2] - q[2] * v[1];
    t[1] = q[2] * v[0] - q[0] * v[2];
    t[2] = q[0] * v[1] - q[1] * v[0];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = t[i] * 2.f;
    u[0] = q[1] * t[2] - q[2] * t[1];
    u[1] = q[2] * t[0] - q[0] * t[2];
    u[2] = q[0] * t[1] - q[1] * t[0];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = t[i] * q[3];
#pragma unroll
    for (int i = 0; i < 3; i++) r[i] = v[i] + t[i];
#pragma unroll
    for (int i = 0; i < 3; i++) r[i] = r[i] + u[i];
}

// transform.c:116-123: pos = rotate((0, 0, len)) + target
LMD void orbit(float (&pos)[3], const float (&quat)[4], const float (&target)[3], float len)
{
    const float start[3] = { 0.f, 0.f, len };
    float r[3];
    quat_mul_vec3(r, quat, start);
#pragma unroll
    for (int i = 0; i < 3; i++) pos[i] = one_nan(r[i] + target[i]);
}

// camera.c:174-206.  pos_scale / lo / hi / center: the control entity's position and scale, its MODEL box
// (model_table) and its world centre; head: its head joint's world position (read when HAS_HEAD_JOINT)
LMD void camera_target(float (&target)[3], float &dist, uint32_t flags, const float (&pos_scale)[4], const float (&lo)[3],
                       const float (&hi)[3], const float (&center)[3], const float (&head)[3], float far_plane)
{
    const float s = pos_scale[3];                    // entity3d_aabb_X / Y / Z (model.c:1185-1198, 433-447)
    const float X = fabsf(hi[0] - lo[0]) * s, Y = fabsf(hi[1] - lo[1]) * s, Z = fabsf(hi[2] - lo[2]) * s;
    float height;
    if (flags & CAMERA_IS_CHARACTER) {
        height = Y;
        if (flags & CAMERA_HAS_HEAD_JOINT) {
            target[0] = head[0] + 0.0f;
            target[1] = head[1] + height * 0.2f;
            target[2] = head[2] + 0.0f;
        } else {
            target[0] = pos_scale[0];
            target[1] = pos_scale[1] + height * 0.75f;
            target[2] = pos_scale[2];
        }
    } else {
        target[0] = center[0]; target[1] = center[1]; target[2] = center[2];
        height = Y / 2.0f;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) target[i] = one_nan(target[i]);
    const float dist_cap = fmaxf(10.0f, cbrtf_glibc(X * Y * Z));               // entity3d_aabb_avg_edge, model.c:1261-1264
    dist = one_nan(fminf(height * 3.0f, fminf(dist_cap, far_plane - 10.0f)));
}

// camera.c:68-91 and 56-57: the orbiting camera's four near-plane corners and the rays to them as clapgpu_ray_cast takes
// them (start, direction, length, pad)
LMD void camera_rays(float (&corner)[4][4], double (&ray)[4][8], const float (&quat)[4], const float (&target)[3], float dist,
                     float near_plane, float aspect)
{
    const float w = near_plane, h = near_plane / aspect;
    float pos[3], m[16], inv[16];
    orbit(pos, quat, target, dist);
    view_matrix(m, pos, quat);
    invert(inv, m);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float r[4] = { (k & 1) ? -w : w, (k & 2) ? -h : h, 0.0f, 1.0f };
#pragma unroll
        for (int j = 0; j < 4; j++) {                // mat4x4_mul_vec4, linmath.h:308-316
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < 4; i++) t += E_(inv, i, j) * r[i];
            corner[k][j] = one_nan(t);
        }
        float dir[3], p = 0.f;
#pragma unroll
        for (int i = 0; i < 3; i++) dir[i] = one_nan(corner[k][i] - target[i]);
#pragma unroll
        for (int i = 0; i < 3; i++) p += dir[i] * dir[i];
#pragma unroll
        for (int i = 0; i < 3; i++) { ray[k][i] = (double)target[i]; ray[k][3 + i] = (double)dir[i]; }
        ray[k][6] = (double)one_nan(sqrtf(p));       // distance, camera.c:57
        ray[k][7] = 0.0;
    }
}

// camera.c:101-116: true = the position is good; false: next = the distance to try
LMD bool camera_decide(double &min_scale, double &next, float dist, const bool (&hit)[4], const double (&depth)[4],
                       const double (&ray)[4][8])
{
    min_scale = 1.0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (hit[k]) min_scale = fmin(min_scale, depth[k] / ray[k][6]);
    if (min_scale < 0.99) {
        next = (double)dist * min_scale;
        return false;
    }
    return true;
}

struct CameraResult {
    float pos[3], dist, target[3];
    float corner[4][4];
    uint32_t updated, iterations, status;
};

// camera.c:226-242 behind camera_target (target and dist of `o` are its).  cast(ray, hit, depth) casts the four rays and
// returns CAMERA_UNRESOLVED or 0; it is not called when the control entity has no physics (phys_ray_cast returns NULL,
// physics.c:536).  o.corner is written when o.iterations > 0.
// The loop ends on every input: a continuing iteration multiplies a finite dist by less than 0.99 and the loop stops at
// or below 0.1, at most ln(3.4e39) / -ln(0.99) ~ 9 040 iterations from the largest float; a NaN dist fails `> 0.1`; an
// infinite one gives non-finite corners, whose rays are invalid and miss, so min_scale stays 1.  CAMERA_ITER_MAX can
// therefore never bind; it is there so that no arithmetic argument stands between a kernel and its end.
template <typename Cast>
LMD void camera_update(CameraResult &o, const float (&quat)[4], float near_plane, float aspect, bool has_physics, Cast &&cast)
{
    const float cdist = o.dist;
    double dist = cdist, next = 0.0, min_scale;
    o.iterations = 0;
    o.status = 0;
    while (dist > 0.1) {
        if (o.iterations == CAMERA_ITER_MAX) { o.status |= CAMERA_CAPPED; break; }
        o.iterations++;
        double ray[4][8], depth[4] = { 0.0, 0.0, 0.0, 0.0 };
        bool hit[4] = { false, false, false, false };
        camera_rays(o.corner, ray, quat, o.target, (float)dist, near_plane, aspect);
        if (has_physics) o.status |= cast(ray, hit, depth);
        if (camera_decide(min_scale, next, (float)dist, hit, depth, ray)) break;
        dist = next;
    }
    o.updated = (double)cdist != dist ? 1u : 0u;     // camera.c:238
    o.dist = one_nan((float)dist);
    orbit(o.pos, quat, o.target, o.dist);
}

// ---- the shadow cascades: scene_camera_calc behind camera_update (scene.c:1021-1046) over view_update_from_frustum
// (view.c:129-163, 195-246) ----
// Stated once, here, for k_cascades_calc (cascades.hip) and for the host's clapgpu_cascades_* beside it.  The rule is in
// include/clapgpu.h ("The shadow cascades on the device").  Intermediate NaNs keep the machine's sign and payload: no
// comparison reads them, and whatever is stored goes through one_nan.
constexpr uint32_t CASCADES_Z_REVERSE = 1u, CASCADES_NDC_Z_ZERO_ONE = 2u, CASCADES_NEAR_BACKUP_FROM_BV = 4u;   // CLAPGPU_CASCADES_*

// linmath.h:40-47: p = 0; p += b[i] * a[i]
LMD float inner3(const float (&a)[3], const float (&b)[3])
{
    float p = 0.f;
#pragma unroll
    for (int i = 0; i < 3; i++) p += b[i] * a[i];
    return p;
}

// linmath.h:58-62: k = 1.0 / len in double, rounded to float (r may be v)
LMD void norm3(float (&r)[3], const float (&v)[3])
{
    const float k = (float)(1.0 / (double)sqrtf(inner3(v, v)));
#pragma unroll
    for (int i = 0; i < 3; i++) r[i] = v[i] * k;
}

// linmath.h:63-69: a NaN length is "true"
LMD void norm3_safe(float (&r)[3], const float (&v)[3])
{
    if (sqrtf(inner3(v, v)) != 0.f) {
        norm3(r, v);
    } else {
#pragma unroll
        for (int i = 0; i < 3; i++) r[i] = v[i];
    }
}

// linmath.h:250-255
LMD void cross3(float (&r)[3], const float (&a)[3], const float (&b)[3])
{
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}

// linmath.h:777-817.  The negated forward vector and eye reach the matrix and translate_in_place as values (the barrier
// of view_matrix, for its reason: a sum that loses its leading +0 turns a zero translation into -0)
LMD void look_at(float (&m)[16], const float (&eye)[3], const float (&center)[3], const float (&up)[3])
{
    float f[3], s[3], t[3];
#pragma unroll
    for (int i = 0; i < 3; i++) f[i] = center[i] - eye[i];
    norm3(f, f);
    cross3(s, f, up);
    norm3(s, s);
    cross3(t, s, f);
    float nf[3] = { -f[0], -f[1], -f[2] }, ne[3] = { -eye[0], -eye[1], -eye[2] };
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(nf[0]), "+v"(nf[1]), "+v"(nf[2]), "+v"(ne[0]), "+v"(ne[1]), "+v"(ne[2]));
#endif
#pragma unroll
    for (int c = 0; c < 3; c++) {
        E_(m, c, 0) = s[c];
        E_(m, c, 1) = t[c];
        E_(m, c, 2) = nf[c];
        E_(m, c, 3) = 0.f;
    }
    E_(m, 3, 0) = 0.f; E_(m, 3, 1) = 0.f; E_(m, 3, 2) = 0.f; E_(m, 3, 3) = 1.f;
    translate_in_place(m, ne[0], ne[1], ne[2]);
}

// linmath.h:819-833 with up = (0, 1, 0): the literal inner product (inf * 0 is NaN, and NaN > 0.999f is false)
LMD void look_at_safe(float (&m)[16], const float (&eye)[3], const float (&center)[3])
{
    const float up[3] = { 0.f, 1.f, 0.f }, other[3] = { 0.f, 0.f, -1.f };
    float fw[3];
#pragma unroll
    for (int i = 0; i < 3; i++) fw[i] = center[i] - eye[i];
    norm3(fw, fw);
    const float dp = fabsf(inner3(fw, up));
    if (dp > 0.999f) look_at(m, eye, center, other);
    else look_at(m, eye, center, up);
}

// linmath.h:692-707 (NDC z in [-1, 1]) / 736-751 (NDC z in [0, 1])
LMD void ortho(float (&M)[16], float l, float r, float b, float t, float n, float f, bool ndc_z_zero_one)
{
#pragma unroll
    for (int i = 0; i < 16; i++) M[i] = 0.f;
    E_(M, 0, 0) = 2.f / (r - l);
    E_(M, 1, 1) = 2.f / (t - b);
    E_(M, 2, 2) = ndc_z_zero_one ? -1.f / (f - n) : -2.f / (f - n);
    E_(M, 3, 0) = -(r + l) / (r - l);
    E_(M, 3, 1) = -(t + b) / (t - b);
    E_(M, 3, 2) = ndc_z_zero_one ? -(n) / (f - n) : -(f + n) / (f - n);
    E_(M, 3, 3) = 1.f;
}

// util.c:59-78 over eight vec4 corners (a stride of four floats): (x, y, z, 1) of each, through xlate when given
// (mat4x4_mul_vec4_post, then * (1.0f / w)), folded from +-INFINITY by min(v, cur) / max(v, cur)
LMD void corners_box(float (&bb)[6], const float (&corners)[8][4], const float (*xlate)[16])
{
    bb[0] = bb[1] = bb[2] = INFINITY;
    bb[3] = bb[4] = bb[5] = -INFINITY;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        float v[4] = { corners[i][0], corners[i][1], corners[i][2], 1.0f };
        if (xlate) {
            float q[4];
            mul_vec4(q, *xlate, v);
            const float s = 1.0f / q[3];
#pragma unroll
            for (int j = 0; j < 3; j++) v[j] = q[j] * s;
        }
#pragma unroll
        for (int j = 0; j < 3; j++) {
            bb[j] = tmin(v[j], bb[j]);
            bb[3 + j] = tmax(v[j], bb[3 + j]);
        }
    }
}

// scene.c:1030-1037 for the bounding volume `env`: its MODEL box and scale (entity3d_aabb_X / Y / Z as camera_target).
// interp.h:25-29: a * (1.0 - blend) + b * blend -- the complement, the first product and the sum are double, b * blend is
// a float product
LMD float near_backup(const float (&light_dir)[3], const float (&lo)[3], const float (&hi)[3], float scale)
{
    const float X = fabsf(hi[0] - lo[0]) * scale, Y = fabsf(hi[1] - lo[1]) * scale, Z = fabsf(hi[2] - lo[2]) * scale;
    const float ex[3] = { 1.f, 0.f, 0.f }, ey[3] = { 0.f, 1.f, 0.f };
    float d[3];
    norm3_safe(d, light_dir);
    const float blend = fabsf(inner3(d, ex));
    const float xz_mix = (float)((double)Z * (1.0 - (double)blend) + (double)(X * blend));
    const float ycos = fmaxf(fabsf(inner3(d, ey)), 0.2f);
    const float q = xz_mix / ycos, edge = cbrtf_glibc(X * Y * Z);
    return one_nan(q < edge ? q : edge);
}

// view.c:195-228: the light's view fitted to eight frustum corners
LMD void cascade_fit(float (&view)[16], float (&inv_view)[16], const float (&corners)[8][4], const float (&light_dir)[3],
                     float near_backup)
{
    float world[6], ctr[3], dir[3], eye[3], m[16], light[6];
    corners_box(world, corners, nullptr);
    box_center(ctr, world);
    ctr[1] = world[1];
    const float target[3] = { -light_dir[0], -light_dir[1], -light_dir[2] };      // view.c:242
    norm3_safe(dir, target);
    near_backup = fmaxf(near_backup, 1.0f);
#pragma unroll
    for (int i = 0; i < 3; i++) dir[i] = dir[i] * near_backup;
#pragma unroll
    for (int i = 0; i < 3; i++) eye[i] = dir[i] + ctr[i];
    look_at_safe(m, eye, ctr);
    corners_box(light, corners, &m);
    const float len = fabsf(light[2] - light[5]);
    const float k = (near_backup + len) / near_backup;
#pragma unroll
    for (int i = 0; i < 3; i++) dir[i] = dir[i] * k;
#pragma unroll
    for (int i = 0; i < 3; i++) eye[i] = dir[i] + ctr[i];
    look_at_safe(m, eye, ctr);
    invert(inv_view, m);
#pragma unroll
    for (int i = 0; i < 16; i++) { view[i] = one_nan(m[i]); inv_view[i] = one_nan(inv_view[i]); }
}

// view.c:129-146 (far_factor is 1.0): the cascade's orthographic projection over the camera sub-frustum in light space
LMD void cascade_projection(float (&proj)[16], float (&inv_proj)[16], float (&mvp)[16], float &far_plane,
                            const float (&view)[16], const float (&corners)[8][4], uint32_t flags)
{
    float bb[6];
    corners_box(bb, corners, &view);
    const float near_plane = 0.1f, far = -bb[2] * 1.0f;
    const bool z01 = (flags & CASCADES_NDC_Z_ZERO_ONE) != 0;
    if (flags & CASCADES_Z_REVERSE) ortho(proj, bb[0], bb[3], bb[1], bb[4], far, near_plane, z01);
    else ortho(proj, bb[0], bb[3], bb[1], bb[4], near_plane, far, z01);
    invert(inv_proj, proj);
    mul(mvp, proj, view);
    far_plane = one_nan(far);
#pragma unroll
    for (int i = 0; i < 16; i++) { proj[i] = one_nan(proj[i]); inv_proj[i] = one_nan(inv_proj[i]); mvp[i] = one_nan(mvp[i]); }
}

// ---- a tracked light: light_update_from_entity (core/light.c:385-422) ----
// Stated once, here, for k_lights_update (lights.hip) and for the host's clapgpu_lights_update_host (runtime.hip).  The
// rule is in include/clapgpu.h ("Spotlights on the device").
// light.c:516-522: the cutoff is compared as a double; a NaN cutoff is no spotlight
LMD bool light_is_spotlight(int32_t is_dir, float cutoff) { return is_dir && (double)cutoff > 0.0; }

// light.c:391-393: pos + light_off (the sum clapgpu_lights_from_entities stores); light.c:398-400, 508-514, spotlights
// only: dir = (0,0,0) - rotate((0,0,1)) -- vec3_sub from a zero vector, so a -0 of the rotation becomes +0
LMD void light_from_entity(float (&lpos)[3], float (&dir)[3], const float (&pos)[3], const float (&off)[3],
                           const float (&rot)[4], bool spot)
{
#pragma unroll
    for (int i = 0; i < 3; i++) lpos[i] = pos[i] + off[i];
    if (!spot) return;
    const float fwd[3] = { 0.f, 0.f, 1.f };
    float r[3];
    quat_mul_vec3(r, rot, fwd);
#pragma unroll
    for (int i = 0; i < 3; i++) dir[i] = one_nan(0.0f - r[i]);
}

} // namespace lmd
