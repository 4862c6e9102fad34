// bodies.hip -- capsule / sphere bodies for gfx950: the integrator, the geoms it writes, and the glue of phys_step()
// around them.
//
// What phys_step() (physics.c:773-787) does per fixed substep through ODE, for bodies without constraint rows:
//   k_bodies_step     dWorldQuickStep's body stage (quickstep.cpp stage 0 + dxStepBody + auto-disable), fused with
//                     the moved geom's axis / AABB (dxCapsule::computeAABB)                      HBM-bound, 1 lane / body
//                     <true>: ... and with the next broadphase's bin pass (bp_grid.h)
//                     <.., true>: ... with the force accumulator (dxBody::facc) and kinematic bodies; the gravity-only
//                     instantiations are what ran before the accumulator existed, instruction for instruction
//   k_bodies_aabb     the geoms alone
//   k_ground_apply    phys_body_ground_collide's moves (the rays and the decision: rays.hip, ray_trimesh.hip)
//   k_slide_apply     character_apply_velocity's moves (the sweeps and the decision: slide.hip)
//   k_phys_body_update, k_bodies_rotate_from_entities   body pose -> entity SoA (physics.c:789-812) and back
//                     (physics.c:136-145)
// and on the host: the fixed-step schedule, world defaults, and the masses and capsule geoms phys_body_new gives a body.
// The broadphase is broadphase.hip, the narrowphase and the sweep contacts.hip (spheres only: contacts_spheres.hip;
// against meshes: mesh_contacts.hip).
// fp64 throughout (the reference builds ODE with dDOUBLE, physics.h:5-9), no FMA contraction.
// ODE is an absent submodule of the reference: PARITY UNPINNED (oracle/physics.c, oracle/physics2.c state what is restated).
#include <string.h>
#include <stdlib.h>
#include "common.h"
#include "phys_dev.h"
#include "bp_grid.h"

namespace clapgpu {

constexpr int PB = 256;

struct BodiesK {
    uint32_t n, samples;
    double *pos, *quat, *lvel, *avel;
    const double *mass, *radius;
    uint32_t *bflags;
    int32_t *adis_steps_left;
    double *adis_time_left;
    const double *length, *inertia;
    double Roff[12];
    double *aabb, *axis, *adis_samples;
    uint32_t *adis_counter;
    double *geom_records;
};

__device__ __forceinline__ void write_geom(const BodiesK &b, uint32_t i, const double (&p)[3], const double (&q)[4],
                                           double (*bb_out)[6] = nullptr)
{
    if (!b.aabb && !b.axis && !b.geom_records) return;
    double R[12], axis[3], bb[6];
    phd::q_to_R(q, R);
    phd::capsule_axis(R, b.Roff, axis);
    const double lz = b.length ? b.length[i] : 0.0;
    phd::geom_aabb(p, b.radius[i], lz, axis, bb);
    if (b.geom_records) {                                        // the narrowphase's view of this geom, one 64-byte sector
        double2 *r = reinterpret_cast<double2 *>(b.geom_records + 8 * (size_t)i);
        r[0] = make_double2(p[0], p[1]); r[1] = make_double2(p[2], axis[0]);
        r[2] = make_double2(axis[1], axis[2]); r[3] = make_double2(b.radius[i], lz);
    }
    if (b.axis) { double *a = b.axis + 3 * (size_t)i; a[0] = axis[0]; a[1] = axis[1]; a[2] = axis[2]; }
    if (b.aabb) {
        double2 *o = reinterpret_cast<double2 *>(b.aabb + 6 * (size_t)i);
        o[0] = make_double2(bb[0], bb[1]); o[1] = make_double2(bb[2], bb[3]); o[2] = make_double2(bb[4], bb[5]);
    }
    if (bb_out)
#pragma unroll
        for (int a = 0; a < 6; a++) (*bb_out)[a] = bb[a];
}

// a body the step leaves alone keeps its stored box: binned from there
__device__ __forceinline__ void bin_stored(const BinK &bin, const BodiesK &b, uint32_t i)
{
    const double2 *p = reinterpret_cast<const double2 *>(b.aabb + 6 * (size_t)i);
    const double2 x = p[0], y = p[1], z = p[2];
    const double bb[6] = { x.x, x.y, y.x, y.y, z.x, z.y };
    bin_body(bin, i, bb);
}

__global__ __launch_bounds__(PB)
void k_bodies_aabb(BodiesK b)
{
    const uint32_t i = blockIdx.x * PB + threadIdx.x;
    if (i >= b.n) return;
    const double p[3] = { b.pos[3 * (size_t)i], b.pos[3 * (size_t)i + 1], b.pos[3 * (size_t)i + 2] };
    const double q[4] = { b.quat[4 * (size_t)i], b.quat[4 * (size_t)i + 1], b.quat[4 * (size_t)i + 2], b.quat[4 * (size_t)i + 3] };
    write_geom(b, i, p, q);
}

// facc: [n][3], read by the FORCES instantiations alone (a trailing argument: the others keep their argument layout)
template <bool BIN, bool FORCES = false>
__global__ __launch_bounds__(PB)
void k_bodies_step(BodiesK b, clapgpu_world w, double h, BinK bin, double *facc)
{
    const uint32_t i = blockIdx.x * PB + threadIdx.x;
    if (BIN && i == 0) bin.ctrl[CTRL_EPOCH] = bin.ctrl[CTRL_EPOCH] + 1;   // what k_bp_bin's first thread does
    if (i >= b.n) return;
    uint32_t fl = b.bflags[i];
    if (fl & CLAPGPU_BODY_DISABLED) { if (BIN) bin_stored(bin, b, i); return; }
    double *pp = b.pos + 3 * (size_t)i, *qp = b.quat + 4 * (size_t)i, *vp = b.lvel + 3 * (size_t)i, *op = b.avel + 3 * (size_t)i;
    double v[3] = { vp[0], vp[1], vp[2] }, om[3] = { op[0], op[1], op[2] };

    // dInternalHandleAutoDisabling: enabled bodies with the flag that hold a joint.  The same statements as auto_disable()
    // of adis_dev.h, which k_islands_seed runs ahead of the island pass; written out here because calling that function
    // moved this kernel over 128 VGPRs and out of the parent's timing spread (profiles/islands/README.md).  Change both.
    if ((fl & CLAPGPU_BODY_AUTO_DISABLE) && (fl & CLAPGPU_BODY_HAS_JOINT)) {
        bool idle = false;
        double al[3], aa[3];
        const uint32_t S = b.samples > 1 ? b.samples : 1;
        if (S == 1) {
            for (int a = 0; a < 3; a++) { al[a] = v[a]; aa[a] = om[a]; }
            idle = true;
        } else {
            double *ring = b.adis_samples + (size_t)i * S * 6;
            uint32_t c = b.adis_counter[i] & 0x7fffffffu, ready = b.adis_counter[i] >> 31;
            for (int a = 0; a < 3; a++) { ring[6 * (size_t)c + a] = v[a]; ring[6 * (size_t)c + 3 + a] = om[a]; }
            if (++c >= S) { c = 0; ready = 1; }
            b.adis_counter[i] = c | ready << 31;
            if (ready) {
                idle = true;
                for (int a = 0; a < 3; a++) { al[a] = ring[a]; aa[a] = ring[3 + a]; }
                for (uint32_t s = 1; s < S; s++)
                    for (int a = 0; a < 3; a++) { al[a] += ring[6 * (size_t)s + a]; aa[a] += ring[6 * (size_t)s + 3 + a]; }
                const double r1 = 1.0 / (double)S;
                for (int a = 0; a < 3; a++) { al[a] *= r1; aa[a] *= r1; }
            }
        }
        if (idle) {
            if (al[0] * al[0] + al[1] * al[1] + al[2] * al[2] > w.adis_linear_threshold_sq) idle = false;
            else if (aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2] > w.adis_angular_threshold_sq) idle = false;
        }
        int32_t sl = b.adis_steps_left[i];
        double tl = b.adis_time_left[i];
        if (idle) { sl--; tl -= h; } else { sl = w.adis_steps; tl = w.adis_time; }
        b.adis_steps_left[i] = sl;
        b.adis_time_left[i] = tl;
        if (sl <= 0 && tl <= 0) {
            b.bflags[i] = (fl | CLAPGPU_BODY_DISABLED) & ~CLAPGPU_BODY_HAS_JOINT;
            vp[0] = vp[1] = vp[2] = 0;
            op[0] = op[1] = op[2] = 0;
            if (BIN) bin_stored(bin, b, i);
            return;
        }
    }
    if (fl & CLAPGPU_BODY_HAS_JOINT)
        b.bflags[i] = fl & ~CLAPGPU_BODY_HAS_JOINT;                   // dJointGroupEmpty after the step

    const bool kin = FORCES && (fl & CLAPGPU_BODY_KINEMATIC);           // dBodySetKinematic: invMass 0, invI 0
    double q[4] = { qp[0], qp[1], qp[2], qp[3] };
    double tacc[3] = { 0, 0, 0 }, invIw[12];
    const bool have_inertia = b.inertia != nullptr;
    if (have_inertia) {
        const double Ib[3] = { b.inertia[3 * (size_t)i], b.inertia[3 * (size_t)i + 1], b.inertia[3 * (size_t)i + 2] };
        const double invIb[3] = { 1.0 / Ib[0], 1.0 / Ib[1], 1.0 / Ib[2] };
        double R[12];
        phd::q_to_R(q, R);
        phd::world_tensor(R, invIb, invIw);
        if (FORCES && kin)
            for (int k = 0; k < 12; k++) invIw[k] = 0;                  // the product below is still formed
        if (fl & CLAPGPU_BODY_GYROSCOPIC) {                             // implicit gyroscopic torque (quickstep.cpp stage 0)
            double Iw[12], L[3], Itild[12], itInv[12];
            phd::world_tensor(R, Ib, Iw);
            phd::mul331(L, Iw, om);
            for (int k = 0; k < 12; k++) Itild[k] = 0;
            Itild[1] = L[2]; Itild[2] = -L[1];                          // dSetCrossMatrixMinus
            Itild[4] = -L[2]; Itild[6] = L[0];
            Itild[8] = L[1]; Itild[9] = -L[0];
            for (int k = 0; k < 12; k++) Itild[k] = Itild[k] * h + Iw[k];
            const double rh = 1.0 / h;
            L[0] *= rh; L[1] *= rh; L[2] *= rh;
            if (phd::invert3(itInv, Itild)) {
                double T[12], tau0[3];
                for (int r = 0; r < 3; r++) {
                    for (int c = 0; c < 3; c++)
                        T[4 * r + c] = Iw[4 * r] * itInv[c] + Iw[4 * r + 1] * itInv[4 + c] + Iw[4 * r + 2] * itInv[8 + c];
                    T[4 * r + 3] = 0;
                }
                T[0] -= 1; T[5] -= 1; T[10] -= 1;
                phd::mul331(tau0, T, L);
                tacc[0] += tau0[0]; tacc[1] += tau0[1]; tacc[2] += tau0[2];
            }
        }
    }
    const double m = b.mass[i];
    const double k = h * ((FORCES && kin) ? 0.0 : 1.0 / m);
    const bool grav = !(fl & CLAPGPU_BODY_NO_GRAVITY);
    if (FORCES) {
        double *fp = facc + 3 * (size_t)i;
        for (int j = 0; j < 3; j++)
            v[j] += k * (fp[j] + (grav ? m * w.gravity[j] : 0.0));     // facc += m * g, then lvel += (h * invMass) * facc
        fp[0] = fp[1] = fp[2] = 0;
    } else {
        for (int j = 0; j < 3; j++)
            v[j] += k * (grav ? m * w.gravity[j] : 0.0);
    }
    if (have_inertia) {
        double d[3];
        tacc[0] *= h; tacc[1] *= h; tacc[2] *= h;
        phd::mul331(d, invIw, tacc);
        om[0] += d[0]; om[1] += d[1]; om[2] += d[2];
        op[0] = om[0]; op[1] = om[1]; op[2] = om[2];
    }
    double p[3] = { pp[0], pp[1], pp[2] };
    for (int j = 0; j < 3; j++) p[j] += h * v[j];                      // dxStepBody
    pp[0] = p[0]; pp[1] = p[1]; pp[2] = p[2];
    const double d0 = 0.5 * (-om[0] * q[1] - om[1] * q[2] - om[2] * q[3]);   // dWtoDQ
    const double d1 = 0.5 * ( om[0] * q[0] + om[1] * q[3] - om[2] * q[2]);
    const double d2 = 0.5 * (-om[0] * q[3] + om[1] * q[0] + om[2] * q[1]);
    const double d3 = 0.5 * ( om[0] * q[2] - om[1] * q[1] + om[2] * q[0]);
    q[0] += h * d0; q[1] += h * d1; q[2] += h * d2; q[3] += h * d3;
    double l = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];   // dNormalize4
    if (l > 0) {
        l = 1.0 / sqrt(l);
        q[0] *= l; q[1] *= l; q[2] *= l; q[3] *= l;
    } else {
        q[0] = 1; q[1] = q[2] = q[3] = 0;
    }
    qp[0] = q[0]; qp[1] = q[1]; qp[2] = q[2]; qp[3] = q[3];
    if (w.linear_damping != 0.0) {
        const double speed2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        if (speed2 > w.linear_damping_threshold_sq) {
            const double s = 1 - w.linear_damping;
            v[0] *= s; v[1] *= s; v[2] *= s;
        }
    }
    vp[0] = v[0]; vp[1] = v[1]; vp[2] = v[2];
    if (BIN) {
        double bb[6];
        write_geom(b, i, p, q, &bb);
        bin_body(bin, i, bb);
    } else
        write_geom(b, i, p, q);
}

// clapgpu_bodies_ground_collide's second launch (rays.hip and ray_trimesh.hip cast, this moves): phys_body_move of every
// body whose ray said so, through a vec3 (float), then the geom as clapgpu_bodies_aabb writes it.  A ray whose hit body
// moved here is flagged: it saw that body where it was before the call.
__global__ __launch_bounds__(PB)
void k_ground_apply(BodiesK b, const double *yoffset, uint32_t n, const uint32_t *body, const double *ray_off,
                    const uint8_t *grounded, uint8_t *grounded_out, const double *dist, const int32_t *hit, uint32_t *flags,
                    const uint32_t *moved)
{
    const uint32_t j = blockIdx.x * PB + threadIdx.x;
    if (j >= n) return;
    const uint32_t f = flags[j];
    const int32_t h = hit[j];
    const uint32_t i = body[j];
    if (i >= b.n) return;                                                   // flagged invalid by the ray launch
    if ((moved[i] >> 1) > 1) {                                              // listed twice: none of its rays moves it
        flags[j] = f | CLAPGPU_RAY_INVALID;
        grounded_out[j] = 0;
        return;
    }
    if (f || h == -1) return;                                               // invalid, unresolved or a miss: nothing moves
    double roff;
    const double ray_len = phd::ground_ray_len(ray_off[j], yoffset[i], roff);
    float dy;
    bool mv;
    phd::ground_branch(dist[j], ray_len, grounded[j] != 0, dy, mv);
    if (h >= 0 && (uint32_t)h < b.n && (moved[h] & 1u) && (moved[h] >> 1) == 1) flags[j] = f | CLAPGPU_RAY_MOVED_TARGET;
    if (!mv) return;
    const float d[3] = { 0.0f, dy, 0.0f };
    double *pp = b.pos + 3 * (size_t)i;
    const double p[3] = { pp[0] + d[0], pp[1] + d[1], pp[2] + d[2] };     // dBodySetPosition(pos + delta)
    pp[0] = p[0]; pp[1] = p[1]; pp[2] = p[2];
    const double q[4] = { b.quat[4 * (size_t)i], b.quat[4 * (size_t)i + 1], b.quat[4 * (size_t)i + 2], b.quat[4 * (size_t)i + 3] };
    write_geom(b, i, p, q);
}

// clapgpu_characters_slide's last launch (slide.hip sweeps and decides, this moves): the mover's final position, which
// the decide launch left in its lvel, becomes its pos (dBodySetPosition), lvel becomes 0 (phys_body_set_velocity,
// character.c:310), then the geom as clapgpu_bodies_aabb writes it.  flags[j] comes in as the decide launch's: an
// INVALID or UNRESOLVED mover stays; else bits 8.. hold one mover of the batch that gave this mover's probe a contact
// (index + 1) and bit 7 says there were several: CLAPGPU_SLIDE_MOVED_TARGET when that one moved (moved[] bit 0), or
// outright when there were several.
__global__ __launch_bounds__(PB)
void k_slide_apply(BodiesK b, uint32_t n, const uint32_t *body, uint32_t *flags, const uint32_t *moved)
{
    const uint32_t j = blockIdx.x * PB + threadIdx.x;
    if (j >= n) return;
    const uint32_t f = flags[j];
    const uint32_t i = body[j];
    if (i >= b.n || (f & (CLAPGPU_SLIDE_INVALID | CLAPGPU_SLIDE_UNRESOLVED))) return;
    uint32_t out = 0;
    const uint32_t one = f >> 8;
    if ((f & 0x80u) || (one && one - 1 < b.n && (moved[one - 1] & 1u))) out = CLAPGPU_SLIDE_MOVED_TARGET;
    flags[j] = out;
    double *pp = b.pos + 3 * (size_t)i, *vp = b.lvel + 3 * (size_t)i;
    const double p[3] = { vp[0], vp[1], vp[2] };
    vp[0] = vp[1] = vp[2] = 0.0;
    pp[0] = p[0]; pp[1] = p[1]; pp[2] = p[2];
    const double q[4] = { b.quat[4 * (size_t)i], b.quat[4 * (size_t)i + 1], b.quat[4 * (size_t)i + 2], b.quat[4 * (size_t)i + 3] };
    write_geom(b, i, p, q);
}

// phys_body_update (physics.c:789-812): scatter body pose into the entity SoA, mark it dirty
__global__ __launch_bounds__(PB)
void k_phys_body_update(uint32_t n, const double *pos, const double *quat, const double *lvel,
                        const double *yoffset, const int32_t *body_entity, uint32_t n_entities,
                        float *pos_scale, float *rot, uint32_t *entity_flags, uint8_t *moving)
{
    const uint32_t i = blockIdx.x * PB + threadIdx.x;
    if (i >= n)
        return;
    const int32_t e = body_entity[i];
    const double *p = pos + 3 * (size_t)i, *q = quat + 4 * (size_t)i, *v = lvel + 3 * (size_t)i;
    if (e >= 0 && (uint32_t)e < n_entities) {
        pos_scale[4 * (size_t)e + 0] = (float)p[0];
        pos_scale[4 * (size_t)e + 1] = (float)(p[1] - yoffset[i]);
        pos_scale[4 * (size_t)e + 2] = (float)p[2];
        reinterpret_cast<float4 *>(rot)[e] = make_float4((float)q[1], (float)q[2], (float)q[3], (float)q[0]);
        atomicOr(&entity_flags[e], CLAPGPU_E_DIRTY);
    }
    if (moving)
        moving[i] = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) > 1e-3 ? 1 : 0;
}

// phys_body_rotate_xform (physics.c:136-145) for the linked entities that default_update rebuilt
__global__ __launch_bounds__(PB)
void k_bodies_rotate_from_entities(uint32_t n_links, const uint32_t *link_body, const uint32_t *link_entity,
                                   uint32_t n_bodies, uint32_t n_entities, uint32_t mode, const float4 *rot,
                                   const int32_t *parent, const uint32_t *flags, double *quat)
{
    const uint32_t k = blockIdx.x * PB + threadIdx.x;
    if (k >= n_links) return;
    const uint32_t b = link_body[k], e = link_entity[k];
    if (b >= n_bodies || e >= n_entities || parent[e] >= 0) return;
    if (!(mode & CLAPGPU_UPDATE_ALL_DIRTY) && !(flags[e] & CLAPGPU_E_DIRTY)) return;
    const float4 r = rot[e];
    double q[4] = { (double)r.w, (double)r.x, (double)r.y, (double)r.z };
    const double l = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);   // dNormalize4
    for (int a = 0; a < 4; a++) quat[4 * (size_t)b + a] = q[a] * l;
}

} // namespace clapgpu

using namespace clapgpu;

// ---------------------------------------------------------------------------------- host helpers
// physics.c:773-787 (host)
extern "C" int clapgpu_phys_step_schedule(double *time_acc, double dt)
{
    const double fixed_dt = 1.0 / 120.0;
    int steps = 0;
    const int max_steps = 5;
    *time_acc += dt;
    for (; *time_acc >= fixed_dt && steps < max_steps; *time_acc -= fixed_dt, steps++)
        ;
    if (steps == max_steps)
        *time_acc = 0.0;
    return steps;
}

extern "C" void clapgpu_world_defaults(clapgpu_world *w)
{
    memset(w, 0, sizeof(*w));
    w->gravity[1] = -9.8;                          // physics.c:1125
    w->linear_damping = 0.001;                     // physics.c:1129
    w->linear_damping_threshold_sq = 0.01 * 0.01;  // ODE default damping threshold
    w->adis_linear_threshold_sq = 0.05 * 0.05;     // physics.c:1040
    w->adis_angular_threshold_sq = 0.05 * 0.05;    // physics.c:1041
    w->adis_steps = 30;                            // physics.c:1042
    w->adis_time = 0.0;
}

static void h_q_from_axis_and_angle(double (&q)[4], double ax, double ay, double az, double angle)
{
    double l = ax * ax + ay * ay + az * az;
    if (l > 0.0) {
        angle *= 0.5;
        q[0] = cos(angle);
        l = sin(angle) * (1.0 / sqrt(l));
        q[1] = ax * l; q[2] = ay * l; q[3] = az * l;
    } else {
        q[0] = 1; q[1] = q[2] = q[3] = 0;
    }
}

extern "C" void clapgpu_geom_offset_rotation(double R[12])
{
    double q[4], M[12];
    h_q_from_axis_and_angle(q, 1.0, 1.0, 1.0, -M_PI * 2.0 / 3.0);
    phd::q_to_R(q, M);
    memcpy(R, M, sizeof(M));
}

extern "C" void clapgpu_mass_sphere_total(double total_mass, double radius, double I[3])
{
    const double m1 = (4.0 / 3.0) * M_PI * radius * radius * radius * 1.0;      // dMassSetSphere(m, 1.0, r)
    const double II = 0.4 * m1 * radius * radius;
    const double scale = total_mass / m1;                                        // dMassAdjust
    I[0] = I[1] = I[2] = II * scale;
}

extern "C" void clapgpu_mass_capsule_total(double total_mass, int direction, double a, double b, double I[3])
{
    if (direction < 1 || direction > 3) direction = 3;
    const double M1 = M_PI * a * a * b * 1.0;
    const double M2 = (4.0 / 3.0) * M_PI * a * a * a * 1.0;
    const double m = M1 + M2;
    const double Ia = M1 * (0.25 * a * a + (1.0 / 12.0) * b * b) + M2 * (0.4 * a * a + 0.375 * a * b + 0.25 * b * b);
    const double Ib = (M1 * 0.5 + M2 * 0.4) * a * a;
    const double scale = total_mass / m;
    I[0] = I[1] = I[2] = Ia;
    I[direction - 1] = Ib;
    I[0] *= scale; I[1] *= scale; I[2] *= scale;
}

// physics.c:814-873
extern "C" void clapgpu_capsule_geom(float X, float Y, float Z, double geom_radius, double geom_offset,
                                     float *radius, float *length, float *yoffset, int *direction, float *ray_off)
{
    float r = 0.f, len = 0.f, off = 0.f, ro = 0.f;
    float mx = Y > Z ? Y : Z;                                                   // max3 / xmax3 (util.h:203-209)
    if (X > mx) mx = X;
    int w = 0;
    if (mx == Y) w = 1; else if (mx == Z) w = 2;
    const int dir = w + 1;
    if (dir == 3) {
        r = geom_radius ? (float)geom_radius : X / 2;
        len = Z - r * 2;
        off = geom_offset ? (float)geom_offset : (Y - r * 2) / 2;
        ro = r;
    } else {
        float mn = Y < Z ? Y : Z;
        if (X < mn) mn = X;
        r = geom_radius ? (float)geom_radius : mn / 2;
        const float l = Y / 2 - r * 2;
        len = l > 0 ? l : 0;
        off = geom_offset ? (float)geom_offset : Y / 2;
        ro = r + len / 2;
    }
    *radius = r; *length = len; *yoffset = off; *direction = dir; *ray_off = ro;
}

// ---------------------------------------------------------------------------------- entry points
__attribute__((visibility("hidden"))) int clapgpu::check_bodies(const clapgpu_bodies *b)
{
    if (!b || !b->pos || !b->quat || !b->lvel || !b->avel || !b->mass || !b->radius || !b->bflags ||
        !b->adis_steps_left || !b->adis_time_left)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (b->adis_average_samples > 1 && (!b->adis_samples || !b->adis_counter))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    return CLAPGPU_OK;
}

static BodiesK bodies_k(const clapgpu_bodies *b)
{
    BodiesK k;
    k.n = b->n; k.samples = b->adis_average_samples;
    k.pos = b->pos; k.quat = b->quat; k.lvel = b->lvel; k.avel = b->avel;
    k.mass = b->mass; k.radius = b->radius; k.bflags = b->bflags;
    k.adis_steps_left = b->adis_steps_left; k.adis_time_left = b->adis_time_left;
    k.length = b->length; k.inertia = b->inertia;
    memcpy(k.Roff, b->geom_offset_R, sizeof(k.Roff));
    bool zero = true;
    for (int i = 0; i < 12; i++) zero &= k.Roff[i] == 0.0;
    if (zero) k.Roff[0] = k.Roff[5] = k.Roff[10] = 1.0;                          // unset = no offset rotation
    k.aabb = b->aabb; k.axis = b->axis; k.adis_samples = b->adis_samples; k.adis_counter = b->adis_counter;
    k.geom_records = (reinterpret_cast<uintptr_t>(b->geom_records) & 15u) ? nullptr : b->geom_records;
    return k;
}

extern "C" int clapgpu_bodies_aabb(void *stream, const clapgpu_bodies *b)
{
    int rc = check_bodies(b);
    if (rc) return rc;
    if (b->n == 0) return CLAPGPU_OK;
    hipLaunchKernelGGL(k_bodies_aabb, dim3((b->n + PB - 1) / PB), dim3(PB), 0, as_stream(stream), bodies_k(b));
    CLAPGPU_LAUNCH_CHECK("k_bodies_aabb");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_bodies_step(void *stream, const clapgpu_bodies *b, const clapgpu_world *w, double h)
{
    int rc = check_bodies(b);
    if (rc) return rc;
    if (!w) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (b->n == 0) return CLAPGPU_OK;
    const dim3 grid((b->n + PB - 1) / PB);
    if (b->facc)
        hipLaunchKernelGGL((k_bodies_step<false, true>), grid, dim3(PB), 0, as_stream(stream), bodies_k(b), *w, h, BinK{}, b->facc);
    else
        hipLaunchKernelGGL((k_bodies_step<false>), grid, dim3(PB), 0, as_stream(stream), bodies_k(b), *w, h, BinK{},
                           static_cast<double *>(nullptr));
    CLAPGPU_LAUNCH_CHECK("k_bodies_step");
    return CLAPGPU_OK;
}

// The step + the NEXT broadphase's bin pass in one launch (the bin pass reads nothing but the box the step has in
// registers, and its one atomic per body hides under the step's fp64 traffic): -1 launch and the boxes' re-read per substep.
extern "C" int clapgpu_bodies_step_prebin(void *stream, const clapgpu_bodies *b, const clapgpu_world *w, double h, clapgpu_bp *bp)
{
    int rc = check_bodies(b);
    if (rc) return rc;
    if (!w || !bp || !b->aabb) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    BinK bin;
    rc = clapgpu_bp_prebin(stream, bp, b->n, b->aabb, &bin);
    if (rc || b->n == 0) return rc;
    if (!bin.key) return clapgpu_bodies_step(stream, b, w, h);   // a leveled bp bins in its own collide: the plain step
    const dim3 grid((b->n + PB - 1) / PB);
    if (b->facc)
        hipLaunchKernelGGL((k_bodies_step<true, true>), grid, dim3(PB), 0, as_stream(stream), bodies_k(b), *w, h, bin, b->facc);
    else
        hipLaunchKernelGGL((k_bodies_step<true>), grid, dim3(PB), 0, as_stream(stream), bodies_k(b), *w, h, bin,
                           static_cast<double *>(nullptr));
    const hipError_t err = launch_error();
    if (err != hipSuccess) {                                     // nothing was binned
        (void)clapgpu_bp_invalidate(stream, bp);
        return hip_fail(err, "k_bodies_step<prebin>");
    }
    return CLAPGPU_OK;
}

// rays.hip's clapgpu_bodies_ground_collide: the moves
__attribute__((visibility("hidden"))) int clapgpu_bodies_ground_apply(void *stream, const clapgpu_bodies *b, uint32_t n,
                                                                      const uint32_t *body, const double *ray_off,
                                                                      const uint8_t *grounded, uint8_t *grounded_out,
                                                                      const double *dist, const int32_t *hit, uint32_t *flags,
                                                                      const uint32_t *moved)
{
    int rc = check_bodies(b);
    if (rc) return rc;
    if (n == 0) return CLAPGPU_OK;
    hipLaunchKernelGGL(k_ground_apply, dim3((n + PB - 1) / PB), dim3(PB), 0, as_stream(stream), bodies_k(b), b->yoffset, n, body,
                       ray_off, grounded, grounded_out, dist, hit, flags, moved);
    CLAPGPU_LAUNCH_CHECK("k_ground_apply");
    return CLAPGPU_OK;
}

// slide.hip's clapgpu_characters_slide: the moves
__attribute__((visibility("hidden"))) int clapgpu_bodies_slide_apply(void *stream, const clapgpu_bodies *b, uint32_t n,
                                                                     const uint32_t *body, uint32_t *flags, const uint32_t *moved)
{
    int rc = check_bodies(b);
    if (rc) return rc;
    if (n == 0) return CLAPGPU_OK;
    hipLaunchKernelGGL(k_slide_apply, dim3((n + PB - 1) / PB), dim3(PB), 0, as_stream(stream), bodies_k(b), n, body, flags, moved);
    CLAPGPU_LAUNCH_CHECK("k_slide_apply");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_phys_body_update(void *stream, const clapgpu_bodies *b, uint32_t n_entities, float *pos_scale,
                                        float *rot, uint32_t *entity_flags, uint8_t *moving)
{
    int rc = check_bodies(b);
    if (rc) return rc;
    if (!b->yoffset || !b->body_entity || !pos_scale || !rot || !entity_flags)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (b->n == 0) return CLAPGPU_OK;
    hipLaunchKernelGGL(k_phys_body_update, dim3((b->n + PB - 1) / PB), dim3(PB), 0,
                       as_stream(stream), b->n, b->pos, b->quat, b->lvel, b->yoffset, b->body_entity, n_entities,
                       pos_scale, rot, entity_flags, moving);
    CLAPGPU_LAUNCH_CHECK("k_phys_body_update");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_bodies_rotate_from_entities(void *stream, const clapgpu_bodies *b, const clapgpu_entities *e,
                                                   uint32_t mode, uint32_t n_links, const uint32_t *link_body,
                                                   const uint32_t *link_entity)
{
    int rc = check_bodies(b);
    if (rc) return rc;
    if (!e || !e->rot || !e->parent || !e->flags || (n_links && (!link_body || !link_entity)))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (n_links == 0 || b->n == 0)
        return CLAPGPU_OK;
    hipLaunchKernelGGL(k_bodies_rotate_from_entities, dim3((n_links + PB - 1) / PB), dim3(PB), 0,
                       as_stream(stream), n_links, link_body, link_entity, b->n, e->n, mode,
                       reinterpret_cast<const float4 *>(e->rot), e->parent, e->flags, b->quat);
    CLAPGPU_LAUNCH_CHECK("k_bodies_rotate_from_entities");
    return CLAPGPU_OK;
}
