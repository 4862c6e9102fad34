// aniq.hip -- character states and animation queues on the device, for gfx950: the last host-only link between
// clapgpu_characters_move and clapgpu_pose_update.
//   k_characters_state   character_set_state(request) behind the move (character.c:316-426), one lane per character
//   k_aniq_time          animated_update's control flow (model.c:1563-1592) in place of k_animation_time: frame time,
//                        then animation_next with the end callbacks
// Both are one call of aniq_dev.h per lane (state_step / time_step): load one character's queue and struct character
// fields into registers, run the rule on that copy, store it back only when the step stayed the device's -- a host-owned
// character (include/clapgpu.h) keeps every byte, and its events word says so.  The header compiles for the host as
// well: tests/test_aniq.py runs the same two functions on the CPU against the restatement, tests/aniqref.py.
// No float arithmetic but one product per velocity component (character.c:115-119) and the clock's doubles; no FMA
// contraction (the Makefile's -ffp-contract=off).  No private memory: the queue is indexed by selects.
#include "common.h"
#include "aniq_dev.h"

namespace clapgpu {

constexpr int AQ = 256;

__global__ __launch_bounds__(AQ)
void k_characters_state(clapgpu_aniq q, uint32_t n_movers, const uint8_t *request, const float *motion, double now,
                        const double *now_dev)
{
    const uint32_t c = blockIdx.x * AQ + threadIdx.x;
    if (c >= q.n) return;
    if (now_dev) now = *now_dev;
    aniq::state_step(q, c, n_movers, request, motion, now);
}

__global__ __launch_bounds__(AQ)
void k_aniq_time(clapgpu_aniq q, double now, const double *now_dev)
{
    const uint32_t c = blockIdx.x * AQ + threadIdx.x;
    if (c >= q.n) return;
    if (now_dev) now = *now_dev;
    aniq::time_step(q, c, now);
}

static int aniq_check(const clapgpu_aniq *q, bool clock)
{
    if (!q) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (q->n == 0) return CLAPGPU_OK;
    if (!q->name_anim || !q->queue || !q->len || !q->cur || !q->cleared || !q->ani_time || !q->state || !q->airborne ||
        !q->velocity || !q->ch_motion || !q->jump_params || !q->events)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (reinterpret_cast<uintptr_t>(q->queue) & 15u) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (clock && (!q->pose_anim || !q->frame_time || (q->n_anims && !q->time_end))) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    return CLAPGPU_OK;
}

} // namespace clapgpu

using namespace clapgpu;

extern "C" int clapgpu_characters_state(void *stream, const clapgpu_aniq *q, const clapgpu_move *m, double now,
                                        const double *now_dev)
{
    if (!m) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    const int rc = aniq_check(q, false);
    if (rc) return rc;
    if (q->n == 0) return CLAPGPU_OK;
    if (m->n && (!m->request || !m->motion)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (!q->mover && q->n > m->n) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    hipLaunchKernelGGL(k_characters_state, dim3((q->n + AQ - 1) / AQ), dim3(AQ), 0, as_stream(stream), *q, m->n, m->request,
                       m->motion, now, now_dev);
    CLAPGPU_LAUNCH_CHECK("k_characters_state");
    return CLAPGPU_OK;
}

extern "C" int clapgpu_animation_queue_time(void *stream, const clapgpu_aniq *q, double now, const double *now_dev)
{
    const int rc = aniq_check(q, true);
    if (rc) return rc;
    if (q->n == 0) return CLAPGPU_OK;
    hipLaunchKernelGGL(k_aniq_time, dim3((q->n + AQ - 1) / AQ), dim3(AQ), 0, as_stream(stream), *q, now, now_dev);
    CLAPGPU_LAUNCH_CHECK("k_aniq_time");
    return CLAPGPU_OK;
}
