// aniq_dev.h -- the character state machine and its animation queue, stated once for the host and the device:
//   character_set_state                                  character.c:316-426
//   character_idle / _start_motion / _any_to_jump        character.c:86-121   (the end callbacks the engine installs)
//   animation_end / animation_next / animation_push_by_name / animated_update's tail      model.c:1443-1592
// on ONE character's state held in registers (aniq::Work).  state_step() and time_step() at the end load a Work, run
// set_state() or update() on it and store it back unless the step made the character the host's (Work::host): aniq.hip's
// kernels call them once per lane, a host program once per character.  tests/aniqref.py restates the same rule line by
// line with a queue of unlimited length.
//
// What the reference does by recursion is a call tree of bounded depth here, spelled out by the template level L:
//   set_state<0> -> push_clear<0> -> end callback -> set_state<1> -> push_clear<1> -> (no callback left to call)
//   next         -> end callback  -> set_state<1> / push_clear<1>
// A clearing push copies the current entry, empties the queue and calls the copy's callback (model.c:1530-1541), so a
// push made from inside that callback finds an empty queue; animation_next nulls the entry's callback before it calls it
// (model.c:1450), so a push made from inside THAT callback copies an entry without one.  push_clear<1> therefore never has
// a callback to call; should it meet one all the same, the character becomes the host's, like every other case the
// device does not decide.
//
// The queue is four entries of two words, indexed by selects (pick / put): no runtime subscript, no private memory.
// The joint cursors animation_start resets (model.c:1419-1422) have no device counterpart: pose.hip brackets a key
// time without a cursor.  sfx_state is the host's (CLAPGPU_ANIQ_STARTED tells it when to reset it).
#pragma once
#include <stdint.h>
#include "clapgpu.h"

#ifdef __HIPCC__
#define ANIQ_HD __host__ __device__ __forceinline__
#else
#define ANIQ_HD static inline
#endif

namespace aniq {

constexpr int MAXQ = (int)CLAPGPU_ANIQ_MAX;

struct Work {
    // the queue: w0 = animation | repeat << 16 | end << 24 (clapgpu_aniq_entry's first word), w1 = speed's bits
    // (named members, not arrays: nothing here may end up in private memory)
    uint32_t a0, a1, a2, a3, s0, s1, s2, s3;
    int32_t  len, cur;
    uint32_t cleared;
    double   ani_time;
    // struct character
    uint32_t state, airborne;
    float    vel_x, vel_y, vel_z, motion_x, motion_z, jump_forward, jump_upward;
    // the step
    const int32_t *name_anim;
    uint32_t n_anims;
    double   now;
    uint32_t events;
    bool     host;
};

ANIQ_HD uint32_t entry_word(uint32_t animation, bool repeat, uint32_t end)
{
    return (animation & 0xffffu) | (repeat ? 1u << 16 : 0u) | (end << 24);
}
ANIQ_HD uint32_t entry_animation(uint32_t w0) { return w0 & 0xffffu; }
ANIQ_HD bool     entry_repeat(uint32_t w0) { return ((w0 >> 16) & 0xffu) != 0; }
ANIQ_HD uint32_t entry_end(uint32_t w0) { return w0 >> 24; }

ANIQ_HD uint32_t pick(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, int32_t i)
{
    return i == 1 ? v1 : i == 2 ? v2 : i == 3 ? v3 : v0;
}
ANIQ_HD void put(uint32_t &v0, uint32_t &v1, uint32_t &v2, uint32_t &v3, int32_t i, uint32_t v)
{
    v0 = i == 0 ? v : v0;
    v1 = i == 1 ? v : v1;
    v2 = i == 2 ? v : v2;
    v3 = i == 3 ? v : v3;
}
// entry i's first word (animation, repeat, end) and its speed
ANIQ_HD uint32_t entry(const Work &w, int32_t i) { return pick(w.a0, w.a1, w.a2, w.a3, i); }
ANIQ_HD uint32_t entry_speed(const Work &w, int32_t i) { return pick(w.s0, w.s1, w.s2, w.s3, i); }
ANIQ_HD void set_entry(Work &w, int32_t i, uint32_t v) { put(w.a0, w.a1, w.a2, w.a3, i, v); }
ANIQ_HD void set_entry_speed(Work &w, int32_t i, uint32_t v) { put(w.s0, w.s1, w.s2, w.s3, i, v); }

// the conditions under which a call does not touch a character at all (include/clapgpu.h, "Host-owned characters")
ANIQ_HD bool host_owned_on_entry(const Work &w)
{
    if (w.len <= 0 || w.len > MAXQ || w.cur < 0 || w.cur >= w.len) return true;
    return entry_animation(w.a0) >= w.n_anims || (w.len > 1 && entry_animation(w.a1) >= w.n_anims) ||
           (w.len > 2 && entry_animation(w.a2) >= w.n_anims) || (w.len > 3 && entry_animation(w.a3) >= w.n_anims);
}

// animation_start (model.c:1406-1424): without animations nothing happens (:1413-1414)
ANIQ_HD void animation_start(Work &w)
{
    if (!w.n_anims) return;
    w.ani_time = w.now;                                                       // :1423
    w.events |= CLAPGPU_ANIQ_STARTED;
}

// ani_current (model.c:1436-1441): e->animation is an int compared with a size_t, so -1 is "none" too
ANIQ_HD bool has_current(const Work &w) { return w.cur >= 0 && w.cur < w.len; }

// animation_set_end_callback (model.c:1485-1494)
ANIQ_HD void set_end_callback(Work &w, uint32_t end)
{
    if (!w.len) return;
    const uint32_t last = entry(w, w.len - 1);
    set_entry(w, w.len - 1, (last & 0x00ffffffu) | (end << 24));
}

// the tail of animation_push_by_name (model.c:1543-1560)
ANIQ_HD bool push_tail(Work &w, uint32_t slot, bool clear, bool repeat)
{
    const int32_t id = w.name_anim[slot];                                     // animation_by_name, :1543
    if (id < 0) {
        if (clear) w.cur = -1;                                                // :1545-1546
        return false;
    }
    if ((uint32_t)id >= w.n_anims || id > 0xffff) { w.host = true; return false; }
    if (w.len >= MAXQ) {                                                      // darray_add of a fifth entry
        if (!w.host) w.events |= CLAPGPU_ANIQ_OVERFLOW;                       // reported when it is the first cause
        w.host = true;
        return false;
    }
    set_entry(w, w.len, entry_word((uint32_t)id, repeat, CLAPGPU_ANI_END_NONE));       // :1550-1552 (darray_add zeroes)
    set_entry_speed(w, w.len, 0x3f800000u);                                   // speed = 1.0, :1553
    w.len++;
    if (clear) {                                                              // :1554-1558
        animation_start(w);
        w.cur = 0;
        w.cleared = 1;
    }
    return true;
}

// animation_push_by_name(..., clear = false, ...): no callback can run
ANIQ_HD bool push_append(Work &w, uint32_t slot, bool repeat) { return push_tail(w, slot, false, repeat); }

template <int L> ANIQ_HD void set_state(Work &w, uint32_t request);
template <int L> ANIQ_HD void end_callback(Work &w, uint32_t end);

// animation_push_by_name(..., clear = true, ...) (model.c:1525-1561)
template <int L> ANIQ_HD bool push_clear(Work &w, uint32_t slot, bool repeat)
{
    const bool had = has_current(w);                                          // :1533
    const uint32_t copy = had ? entry(w, w.cur) : 0u;                          // :1534-1535
    w.len = 0;                                                                // darray_clearout, :1537
    if (had && entry_end(copy) != CLAPGPU_ANI_END_NONE) {                     // animation_end(&_qa), :1539-1540
        if constexpr (L == 0) end_callback<0>(w, entry_end(copy));
        else w.host = true;                                                   // (see the head of this file)
    }
    return push_tail(w, slot, true, repeat);
}

// what animation_end calls (model.c:1451): character.c:86-121
template <int L> ANIQ_HD void end_callback(Work &w, uint32_t end)
{
    if (end == CLAPGPU_ANI_END_IDLE) {                                        // character_idle, :86-92
        w.events |= CLAPGPU_ANIQ_CB_IDLE;
        w.state = CLAPGPU_CS_IDLE;                                            // CS_AWAKE == CS_IDLE
        push_clear<1>(w, CLAPGPU_ANI_IDLE, true);
    } else if (end == CLAPGPU_ANI_END_START_MOTION) {                         // character_start_motion, :94-99
        w.events |= CLAPGPU_ANIQ_CB_START_MOTION;
        w.state = CLAPGPU_CS_MOVING;
    } else if (end == CLAPGPU_ANI_END_ANY_TO_JUMP) {                          // character_any_to_jump, :103-121
        w.events |= CLAPGPU_ANIQ_CB_ANY_TO_JUMP;
        w.airborne = 1;
        w.vel_x = w.motion_x * w.jump_forward;                                // ch->motion, not this frame's input
        w.vel_y = w.jump_upward;
        w.vel_z = w.motion_z * w.jump_forward;
        set_state<1>(w, CLAPGPU_CS_JUMPING);
    } else {
        w.host = true;                                                        // CLAPGPU_ANI_END_HOST, or no code at all
    }
}

// character_set_state (character.c:316-426).  Each pass of the switch makes at most one clearing push (`first`), gives
// it an end callback when it found its name (`end`), and at most one appending push behind it (`second`); where the
// reference tests a push's return value a failure sends the pass to fail_fallback (`must`, `must_second`).  The
// conditions of a pass are read before its first push, as the reference's else-if chains read them.
template <int L> ANIQ_HD void set_state(Work &w, uint32_t request)
{
    if (request != CLAPGPU_CS_IDLE && w.state < CLAPGPU_CS_IDLE) {            // :319-326
        if (w.state == CLAPGPU_CS_START) {
            w.state = CLAPGPU_CS_WAKING;
            push_clear<L>(w, CLAPGPU_ANI_START_TO_IDLE, false);
            set_end_callback(w, CLAPGPU_ANI_END_IDLE);
        }
        return;
    }
    for (int pass = 0; pass < 2; pass++) {                                    // fail_fallback: the second pass is CS_IDLE
        int32_t first = -1, second = -1;
        bool first_repeat = false, must = false, must_second = false, fallback = false;
        uint32_t end = CLAPGPU_ANI_END_NONE;
        const uint32_t st = w.state;
        switch (request) {
        case CLAPGPU_CS_IDLE:                                                 // :330-346
            if (w.airborne) return;
            if (st == CLAPGPU_CS_MOVING) first = CLAPGPU_ANI_MOTION_STOP;
            else if (st == CLAPGPU_CS_JUMPING) first = CLAPGPU_ANI_JUMP_TO_IDLE;
            else if (st == CLAPGPU_CS_FALLING) first = CLAPGPU_ANI_FALL_TO_IDLE;
            else if (st <= CLAPGPU_CS_IDLE || st == CLAPGPU_CS_JUMP_START) return;
            second = CLAPGPU_ANI_IDLE;
            break;
        case CLAPGPU_CS_MOVING:                                               // :348-377 without :350-351 (the move's)
            if (st == CLAPGPU_CS_IDLE) {
                first = CLAPGPU_ANI_MOTION_START; must = true; end = CLAPGPU_ANI_END_START_MOTION;
            } else if ((st == CLAPGPU_CS_FALLING || st == CLAPGPU_CS_JUMPING) && !w.airborne) {
                first = CLAPGPU_ANI_JUMP_TO_MOTION; must = true;
            } else if (st == CLAPGPU_CS_JUMP_START) {
                fallback = true;
            } else if (st == CLAPGPU_CS_MOVING) {
                return;
            }
            second = CLAPGPU_ANI_MOTION; must_second = true;
            break;
        case CLAPGPU_CS_JUMP_START:                                           // :379-402
            if (st == CLAPGPU_CS_IDLE) {
                first = CLAPGPU_ANI_IDLE_TO_JUMP; must = true; end = CLAPGPU_ANI_END_ANY_TO_JUMP;
            } else if (st == CLAPGPU_CS_MOVING) {
                w.airborne = 1;                                               // :388
                first = CLAPGPU_ANI_MOTION_TO_JUMP; must = true; end = CLAPGPU_ANI_END_ANY_TO_JUMP;
            } else if (st == CLAPGPU_CS_JUMP_START || st == CLAPGPU_CS_JUMPING) {
                fallback = true;
            }
            break;
        case CLAPGPU_CS_JUMPING:                                              // :404-412
            if (st == CLAPGPU_CS_JUMP_START) { first = CLAPGPU_ANI_JUMP; first_repeat = true; must = true; }
            else fallback = true;
            break;
        case CLAPGPU_CS_FALLING:                                              // :414-420
            if (st == CLAPGPU_CS_JUMP_START || st == CLAPGPU_CS_JUMPING) return;
            first = CLAPGPU_ANI_FALL; first_repeat = true;
            break;
        default:                                                              // :422-424
            break;
        }
        if (!fallback && first >= 0) {
            const bool ok = push_clear<L>(w, (uint32_t)first, first_repeat);
            if (ok && end != CLAPGPU_ANI_END_NONE) set_end_callback(w, end);
            fallback = !ok && must;
        }
        if (!fallback && second >= 0) {
            const bool ok = push_append(w, (uint32_t)second, true);
            fallback = !ok && must_second;
        }
        if (!fallback) {
            w.state = request;
            return;
        }
        request = CLAPGPU_CS_IDLE;                                            // state = CS_IDLE; goto fail_fallback
    }
}

// animation_next (model.c:1454-1483) for a queue that is not empty, with cur >= 0
ANIQ_HD void next(Work &w)
{
    uint32_t qa = entry(w, w.cur);                                            // :1471
    if (!entry_repeat(qa)) {
        const uint32_t end = entry_end(qa);                                   // animation_end, :1443-1452
        if (end != CLAPGPU_ANI_END_NONE) {
            set_entry(w, w.cur, qa & 0x00ffffffu);                            // qa->end = NULL, before the call
            end_callback<0>(w, end);
        }
        if (w.cleared) {                                                      // :1474-1477
            w.cleared = 0;
            return;
        }
        if (w.len <= 0) { w.host = true; return; }                            // (cur + 1) % 0: the reference divides by zero
        w.cur = (w.cur + 1) % w.len;                                          // :1478
        w.events |= CLAPGPU_ANIQ_ADVANCED;
    }
    animation_start(w);                                                       // :1481-1482 (sfx_state: the host's)
}

// animated_update (model.c:1563-1592) behind its ani_current: the frame time the pose is given, then the advance
ANIQ_HD void update(Work &w, const float *time_end, uint32_t *pose_anim, float *frame_time)
{
    const uint32_t an = entry_animation(entry(w, w.cur));
    const float speed = __builtin_bit_cast(float, entry_speed(w, w.cur));
    const double ft = (w.now - w.ani_time) * (double)speed;                   // :1578
    *pose_anim = an;
    *frame_time = (float)ft;                                                  // channels_transform's float, :1582
    if (ft >= (double)time_end[an]) {                                         // :1590
        w.events |= CLAPGPU_ANIQ_ENDED;
        next(w);
    }
}

// ---- one character of a clapgpu_aniq: in and out of registers, and the two steps of the library ----
ANIQ_HD void load(Work &w, const clapgpu_aniq &q, uint32_t c, double now)
{
    const uint32_t *qp = static_cast<const uint32_t *>(__builtin_assume_aligned(q.queue, 16)) + 8 * (size_t)c;
    w.a0 = qp[0]; w.s0 = qp[1]; w.a1 = qp[2]; w.s1 = qp[3];
    w.a2 = qp[4]; w.s2 = qp[5]; w.a3 = qp[6]; w.s3 = qp[7];
    w.len = q.len[c];
    w.cur = q.cur[c];
    w.cleared = q.cleared[c];
    w.ani_time = q.ani_time[c];
    w.state = q.state[c];
    w.airborne = q.airborne[c];
    w.vel_x = q.velocity[3 * (size_t)c]; w.vel_y = q.velocity[3 * (size_t)c + 1]; w.vel_z = q.velocity[3 * (size_t)c + 2];
    w.motion_x = q.ch_motion[2 * (size_t)c];
    w.motion_z = q.ch_motion[2 * (size_t)c + 1];
    w.jump_forward = q.jump_params[2 * (size_t)c];
    w.jump_upward = q.jump_params[2 * (size_t)c + 1];
    w.name_anim = q.name_anim;
    w.n_anims = q.n_anims;
    w.now = now;
    w.events = 0;
    w.host = false;
}

// entries behind len are stored as zeros: what a committed character's queue holds is a function of its state alone
ANIQ_HD void store(const Work &w, const clapgpu_aniq &q, uint32_t c)
{
    uint32_t *qp = static_cast<uint32_t *>(__builtin_assume_aligned(q.queue, 16)) + 8 * (size_t)c;
    qp[0] = w.len > 0 ? w.a0 : 0u; qp[1] = w.len > 0 ? w.s0 : 0u; qp[2] = w.len > 1 ? w.a1 : 0u; qp[3] = w.len > 1 ? w.s1 : 0u;
    qp[4] = w.len > 2 ? w.a2 : 0u; qp[5] = w.len > 2 ? w.s2 : 0u; qp[6] = w.len > 3 ? w.a3 : 0u; qp[7] = w.len > 3 ? w.s3 : 0u;
    q.len[c] = (uint8_t)w.len;
    q.cur[c] = (int8_t)w.cur;
    q.cleared[c] = (uint8_t)w.cleared;
    q.ani_time[c] = w.ani_time;
    q.state[c] = (uint8_t)w.state;
    q.airborne[c] = (uint8_t)w.airborne;
    q.velocity[3 * (size_t)c] = w.vel_x; q.velocity[3 * (size_t)c + 1] = w.vel_y; q.velocity[3 * (size_t)c + 2] = w.vel_z;
    q.ch_motion[2 * (size_t)c] = w.motion_x;
    q.ch_motion[2 * (size_t)c + 1] = w.motion_z;
}

// the bits a host-owned character's step reports: what it did on the copy is not told
ANIQ_HD uint32_t step_events(const Work &w)
{
    return w.host ? CLAPGPU_ANIQ_HOST | (w.events & CLAPGPU_ANIQ_OVERFLOW) : w.events;
}

// clapgpu_characters_state for character c: request / motion are the clapgpu_move's, n_movers its n
ANIQ_HD void state_step(const clapgpu_aniq &q, uint32_t c, uint32_t n_movers, const uint8_t *request, const float *motion,
                        double now)
{
    const int32_t k = q.mover ? q.mover[c] : (int32_t)c;
    uint32_t req = CLAPGPU_CS_NONE;
    if (k >= 0 && (uint32_t)k < n_movers) req = request[k];
    if (req == CLAPGPU_CS_NONE) {
        q.events[c] = 0;
        return;
    }
    Work w;
    load(w, q, c, now);
    w.host = host_owned_on_entry(w);
    if (!w.host) {
        if (req == CLAPGPU_CS_JUMP_START || req == CLAPGPU_CS_MOVING || req == CLAPGPU_CS_IDLE) {      // character.c:499
            w.motion_x = motion[2 * (size_t)k];
            w.motion_z = motion[2 * (size_t)k + 1];
        }
        set_state<0>(w, req);
    }
    if (!w.host) store(w, q, c);
    q.events[c] = step_events(w) << CLAPGPU_ANIQ_STATE_SHIFT;
}

// clapgpu_animation_queue_time for character c
ANIQ_HD void time_step(const clapgpu_aniq &q, uint32_t c, double now)
{
    Work w;
    load(w, q, c, now);
    w.host = host_owned_on_entry(w);                                          // model.c:1570-1574: animation_next's idle push
    uint32_t pose_anim = 0;
    float frame_time = 0.f;
    if (!w.host) update(w, q.time_end, &pose_anim, &frame_time);
    if (!w.host) {
        store(w, q, c);
        q.pose_anim[c] = pose_anim;
        q.frame_time[c] = frame_time;
    }
    q.events[c] = (q.events[c] & (0xffu << CLAPGPU_ANIQ_STATE_SHIFT)) | step_events(w);
}

} // namespace aniq
