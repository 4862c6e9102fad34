// move.hip -- character_move (character.c:450-537) for a batch of characters with a body, for gfx950: the stage of
// clap_frame() in front of phys_step (scene_characters_move, clap.c:589) as one call without a host round trip.
//
// Every physics call the function makes is a batched call of its own already: the ground ray (rays.hip, ray_trimesh.hip,
// bodies.hip's k_ground_apply), the sweep-and-slide (slide.hip, k_slide_apply) and the pushes (push.hip).  This file is
// what the host did between them:
//   k_move_begin    grounded[k] = !airborne[k], what phys_body_ground_collide is given (:454); also clears the per-body
//                   words of the ray stage, so that the whole call is kernel launches (a captured graph holds no
//                   memset node of this file's making)
//   k_move_decide   one lane per mover: airborne from the ray, the jump protection (:464), gravity (:477-484), the jump
//                   (character_jump, :428-448), the walking velocity out of the ground normal (:504-527), the state it
//                   asks character_set_state for, and whether character_apply_velocity runs; the mover's entry in the
//                   slide's list (its body, or 0xffffffff: the slide leaves that entry alone) and the velocity the push
//                   is given
//   k_move_finish   flags = the ray's | the slide's << 8 (the CLAPGPU_SLIDE_INVALID of a 0xffffffff entry dropped), and
//                   entity3d_rotate's hand-off to the entity SoA (:313)
// The host side issues the stages through move_slice (stages 1 to 5 over a contiguous slice of the movers, with or without
// the push) and move_finish (move_dev.h): clapgpu_characters_move runs them over all movers at once, order.hip's
// clapgpu_characters_move_ordered over one slice per conflict level.
// float arithmetic as character.c and linmath.h write it, no FMA contraction.  No collider is called here.
// ODE is absent from the reference: PARITY UNPINNED.  The rule is in include/clapgpu.h, restated in tests/moveref.py.
#include "common.h"
#include "move_dev.h"

namespace clapgpu {

constexpr int MB = 256;
constexpr uint32_t NO_BODY = 0xffffffffu;

struct MoveK {
    uint32_t n;
    const uint32_t *body;
    const float *motion;
    const uint8_t *state, *jump;
    const float *jump_params;
    float *velocity;
    const float *normal;
    uint8_t *airborne;
    uint8_t *request, *applied;
    float *first_frac;
    int32_t *push_hit;
    uint32_t *flags;                    // the ray's, as k_ground_apply left them
    const uint8_t *grounded_out;
    uint32_t *slide_body, *slide_flags;
    float *given;
};

__global__ __launch_bounds__(MB)
void k_move_begin(uint32_t n, const uint8_t *airborne, uint8_t *grounded, uint32_t n_words, uint32_t *words)
{
    const uint32_t k = blockIdx.x * MB + threadIdx.x;
    if (k < n) grounded[k] = airborne[k] ? 0 : 1;
    if (k < n_words) words[k] = 0;
}

// vec3_len (linmath.h:40-51)
__device__ __forceinline__ float len3(const float (&v)[3])
{
    float p = 0.f;
    for (int i = 0; i < 3; i++) p += v[i] * v[i];
    return sqrtf(p);
}

// vec3_mul_cross (linmath.h:250-255)
__device__ __forceinline__ void cross3(float (&r)[3], const float (&a)[3], const float (&b)[3])
{
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}

// vec3_norm (linmath.h:58-62): float k = 1.0 / vec3_len(v); vec3_scale(r, v, k)
__device__ __forceinline__ void norm3(float (&v)[3])
{
    const float k = (float)(1.0 / (double)len3(v));
    for (int i = 0; i < 3; i++) v[i] = v[i] * k;
}

// gravity_y: (float)w->gravity[1], what phys_body_get_gravity hands back; dt: the raw frame delta
__global__ __launch_bounds__(MB)
void k_move_decide(MoveK m, float gravity_y, double dt)
{
    const uint32_t k = blockIdx.x * MB + threadIdx.x;
    if (k >= m.n) return;
    float vel[3] = { m.velocity[3 * (size_t)k], m.velocity[3 * (size_t)k + 1], m.velocity[3 * (size_t)k + 2] };
    uint8_t request = CLAPGPU_CS_NONE;
    bool apply = false;
    if (!(m.flags[k] & (CLAPGPU_RAY_INVALID | CLAPGPU_RAY_UNRESOLVED))) {      // else the host redoes this mover
        const uint32_t st = m.state[k];
        bool air = m.grounded_out[k] == 0;                                     // :454
        if (st == CLAPGPU_CS_JUMPING && vel[1] > 0) air = true;                // :464
        if (air) {
            if (dt > 1e-6) {                                                   // :478-484
                vel[1] = (float)((double)vel[1] + (double)gravity_y * dt);
                apply = true;
            }
            request = CLAPGPU_CS_FALLING;
        } else {
            const float dx = m.motion[2 * (size_t)k], dz = m.motion[2 * (size_t)k + 1];
            const float motion[3] = { dx, 0.0f, dz };
            if (m.jump[k]) {                                                   // character_jump: airborne is 0 here
                const float fwd = m.jump_params[2 * (size_t)k], up = m.jump_params[2 * (size_t)k + 1];
                vel[0] = dx * fwd; vel[1] = up; vel[2] = dz * fwd;             // :443
                request = CLAPGPU_CS_JUMP_START;
                if (st == CLAPGPU_CS_MOVING) air = true;                       // :388
            } else if (len3(motion) != 0.0f) {                                 // :504
                const float newy[3] = { m.normal[3 * (size_t)k], m.normal[3 * (size_t)k + 1], m.normal[3 * (size_t)k + 2] };
                if ((double)len3(newy) > 0.0) {                                // :509
                    const float oldx[3] = { 1.0f, 0.0f, 0.0f };
                    float newx[3], newz[3];
                    cross3(newz, oldx, newy);
                    cross3(newx, newy, newz);
                    norm3(newx);
                    norm3(newz);
                    const float coef = st == CLAPGPU_CS_MOVING ? 1.0f : 0.3f;
                    const float sx = dx * coef, sz = dz * coef;
                    for (int i = 0; i < 3; i++) vel[i] = newx[i] * sx + newz[i] * sz;      // vec3_add_scaled, :526
                }
                request = CLAPGPU_CS_MOVING;
                apply = st >= CLAPGPU_CS_IDLE;                                 // character_set_state's early return, :319-326
            } else {
                request = CLAPGPU_CS_IDLE;                                     // :530-531
            }
        }
        m.airborne[k] = air ? 1 : 0;
        for (int i = 0; i < 3; i++) m.velocity[3 * (size_t)k + i] = vel[i];
    }
    m.request[k] = request;
    m.applied[k] = apply ? 1 : 0;
    m.first_frac[2 * (size_t)k] = 1.0f; m.first_frac[2 * (size_t)k + 1] = 1.0f;
    for (int q = 0; q < 6; q++) m.push_hit[6 * (size_t)k + q] = -1;
    m.slide_body[k] = apply ? m.body[k] : NO_BODY;
    m.slide_flags[k] = 0;
    for (int i = 0; i < 3; i++) m.given[3 * (size_t)k + i] = vel[i];
}

__global__ __launch_bounds__(MB)
void k_move_finish(uint32_t n, const uint32_t *slide_body, const uint32_t *slide_flags, uint32_t *flags, const uint8_t *applied,
                   const uint32_t *entity, const float4 *yaw_quat, uint32_t n_entities, float4 *rot, uint32_t *entity_flags)
{
    const uint32_t k = blockIdx.x * MB + threadIdx.x;
    if (k >= n) return;
    const uint32_t sf = slide_body[k] == NO_BODY ? 0u : slide_flags[k];
    flags[k] |= sf << 8;
    if (entity && applied[k]) {
        const uint32_t e = entity[k];
        if (e < n_entities) {
            rot[e] = yaw_quat[k];
            entity_flags[e] |= CLAPGPU_E_DIRTY;                                // one character per entity: no other writer
        }
    }
}

// the scratch, every part 256-byte aligned (Carve, common.h); the last is the push's own, by its own count
struct MoveScratch {
    size_t words, slide_body, slide_flags, given, dist, other, grounded, grounded_out, push, bytes;
};

static MoveScratch move_layout(uint32_t n_bodies, uint32_t n, size_t push_bytes)
{
    MoveScratch l;
    Carve c;
    l.words = c.take((size_t)(n_bodies ? n_bodies : 1) * sizeof(uint32_t));
    l.slide_body = c.take((size_t)n * sizeof(uint32_t));
    l.slide_flags = c.take((size_t)n * sizeof(uint32_t));
    l.given = c.take((size_t)n * 3 * sizeof(float));
    l.dist = c.take((size_t)n * sizeof(double));
    l.other = c.take((size_t)n * sizeof(double));
    l.grounded = c.take(n);
    l.grounded_out = c.take(n);
    l.push = c.take(push_bytes);
    l.bytes = c.bytes();
    return l;
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" size_t clapgpu_characters_move_scratch_bytes(uint32_t n_bodies, uint32_t n)
{
    const size_t push_bytes = clapgpu_bodies_push_scratch_bytes(n);
    if (!push_bytes) return 0;                                               // n == 0, n too large, or no device to ask
    return move_layout(n_bodies, n, push_bytes).bytes;
}

int clapgpu::move_check(clapgpu_bp *bp, const clapgpu_bodies *b, const clapgpu_world *w, const clapgpu_geoms *statics,
                        const clapgpu_entities *e, const clapgpu_move *m)
{
    if (!m || !b || !w || !statics) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    // what the three stages ask of the bodies, asked before anything is issued
    if (!b->pos || !b->quat || !b->lvel || !b->radius || !b->yoffset || !b->facc || !b->mass || !b->bflags ||
        !b->adis_steps_left || !b->adis_time_left || (bp && !b->aabb))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (m->n == 0) return CLAPGPU_OK;
    if (!m->body || !m->ray_off || !m->motion || !m->state || !m->jump || !m->jump_params || !m->velocity || !m->normal ||
        !m->airborne || !m->request || !m->applied || !m->collision || !m->first_frac || !m->push_hit || !m->flags)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!m->entity != !m->yaw_quat) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (m->entity && (!e || !e->rot || !e->flags || (reinterpret_cast<uintptr_t>(m->yaw_quat) & 15u)))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    return CLAPGPU_OK;
}

int clapgpu::move_parts(void *scratch, uint32_t n_bodies, uint32_t n, MoveParts *p)
{
    const size_t push_bytes = clapgpu_bodies_push_scratch_bytes(n);          // asks the sort, launches nothing
    if (!push_bytes) return n > (1u << 28) ? CLAPGPU_ERR_TOO_LARGE : CLAPGPU_ERR_UNKNOWN;
    const MoveScratch l = move_layout(n_bodies, n, push_bytes);
    uint8_t *base = static_cast<uint8_t *>(scratch);
    p->words = reinterpret_cast<uint32_t *>(base + l.words);
    p->slide_body = reinterpret_cast<uint32_t *>(base + l.slide_body);
    p->slide_flags = reinterpret_cast<uint32_t *>(base + l.slide_flags);
    p->given = reinterpret_cast<float *>(base + l.given);
    p->dist = reinterpret_cast<double *>(base + l.dist);
    p->other = reinterpret_cast<double *>(base + l.other);
    p->grounded = base + l.grounded;
    p->grounded_out = base + l.grounded_out;
    p->push = base + l.push;
    return CLAPGPU_OK;
}

int clapgpu::move_slice(void *stream, clapgpu_bp *bp, const clapgpu_bodies *b, const clapgpu_world *w, const clapgpu_geoms *statics,
                        const clapgpu_trimesh *meshes, double dt_sec, const clapgpu_move *m, uint32_t at, uint32_t n,
                        const MoveParts &p, bool push)
{
    const size_t o = at;
    uint32_t *slide_body = p.slide_body + o, *slide_flags = p.slide_flags + o;
    float *given = p.given + 3 * o;
    uint8_t *grounded = p.grounded + o, *grounded_out = p.grounded_out + o;
    uint32_t *words = p.words;
    hipStream_t s = as_stream(stream);
    const dim3 grid((n + MB - 1) / MB);
    int rc;
    // ---- phys_body_ground_collide(body, !ch->airborne), :454 ----
    if (bp && (rc = clapgpu_bp_index(stream, bp, b->n, b->aabb))) return rc;
    const uint32_t n_words = b->n ? b->n : 1, lanes = n > n_words ? n : n_words;
    hipLaunchKernelGGL(k_move_begin, dim3((lanes + MB - 1) / MB), dim3(MB), 0, s, n, m->airborne + o, grounded, n_words, words);
    CLAPGPU_LAUNCH_CHECK("k_move_begin");
    rc = clapgpu_bodies_ground_collide_on(stream, bp, b, statics, meshes, n, m->body + o, m->ray_off + o, grounded, grounded_out,
                                          m->normal + 3 * o, p.dist + o, m->collision + o, m->flags + o, words, p.other + o, true);
    if (rc) return rc;
    // ---- :464-532 ----
    MoveK k;
    k.n = n; k.body = m->body + o; k.motion = m->motion + 2 * o; k.state = m->state + o; k.jump = m->jump + o;
    k.jump_params = m->jump_params + 2 * o; k.velocity = m->velocity + 3 * o; k.normal = m->normal + 3 * o;
    k.airborne = m->airborne + o; k.request = m->request + o; k.applied = m->applied + o;
    k.first_frac = m->first_frac + 2 * o; k.push_hit = m->push_hit + 6 * o; k.flags = m->flags + o; k.grounded_out = grounded_out;
    k.slide_body = slide_body; k.slide_flags = slide_flags; k.given = given;
    hipLaunchKernelGGL(k_move_decide, grid, dim3(MB), 0, s, k, (float)w->gravity[1], dt_sec);
    CLAPGPU_LAUNCH_CHECK("k_move_decide");
    // ---- character_apply_velocity's physics branch and its phys_body_push calls; nothing below 1e-6 (:259-260) ----
    if (!(dt_sec < 1e-6)) {
        if (bp && (rc = clapgpu_bp_index(stream, bp, b->n, b->aabb))) return rc;      // the ground snaps moved boxes
        clapgpu_slide sl;
        sl.n = n; sl.body = slide_body; sl.velocity = m->velocity + 3 * o; sl.airborne = m->airborne + o;
        sl.first_frac = m->first_frac + 2 * o; sl.push_hit = m->push_hit + 6 * o; sl.flags = slide_flags;
        rc = clapgpu_characters_slide(stream, bp, b, statics, meshes, dt_sec, &sl, words);
        if (rc) return rc;
        if (push) {
            rc = clapgpu_bodies_push(stream, b, w, n, slide_body, given, m->push_hit + 6 * o, slide_flags, nullptr, p.push);
            if (rc) return rc;
        }
    }
    return CLAPGPU_OK;
}

int clapgpu::move_finish(void *stream, const clapgpu_entities *e, const clapgpu_move *m, const MoveParts &p)
{
    const uint32_t n = m->n;
    hipLaunchKernelGGL(k_move_finish, dim3((n + MB - 1) / MB), dim3(MB), 0, as_stream(stream), n, p.slide_body, p.slide_flags,
                       m->flags, m->applied, m->entity, reinterpret_cast<const float4 *>(m->yaw_quat), m->entity ? e->n : 0u,
                       m->entity ? reinterpret_cast<float4 *>(const_cast<float *>(e->rot)) : nullptr,
                       m->entity ? e->flags : nullptr);
    CLAPGPU_LAUNCH_CHECK("k_move_finish");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_characters_move(void *stream, clapgpu_bp *bp, const clapgpu_bodies *b, const clapgpu_world *w,
                                       const clapgpu_geoms *statics, const clapgpu_trimesh *meshes, const clapgpu_entities *e,
                                       double dt_sec, const clapgpu_move *m, void *scratch)
{
    int rc = move_check(bp, b, w, statics, e, m);
    if (rc) return rc;
    if (m->n == 0) return CLAPGPU_OK;
    if (!scratch || (reinterpret_cast<uintptr_t>(scratch) & 255u)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    MoveParts p;
    if ((rc = move_parts(scratch, b->n, m->n, &p))) return rc;
    if ((rc = move_slice(stream, bp, b, w, statics, meshes, dt_sec, m, 0, m->n, p, true))) return rc;
    return move_finish(stream, e, m, p);
}
