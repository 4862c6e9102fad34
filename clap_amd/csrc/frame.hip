// frame.hip -- one display frame of the batched path as ONE C call: the sequence clap_frame() runs
// (core/clap.c:551-665) -- scene_characters_move (clap.c:589: clapgpu_characters_move, when asked for) -> phys_step
// (clap.c:604: per fixed substep the two broadphase passes, near_callback's
// contact records, the island pass and the contact solve when asked for, the world step) -> scene_update -> mq_update with every entity's hook in list order
// (character_update in front of default_update: body read-back, rotation push to colliders, light hand-off, TRS
// rebuild, animated_update; particles_update) -> light grid -> render-pass glue (visible list, LOD pick).
// Nothing is read back.  Every part is optional (NULL).  The caller keeps the time base
// (clapgpu_phys_step_schedule) and passes the number of substeps.
// With f->aniq (ABI 46) the host is not needed between the move and the pose either: character_set_state follows the move
// (clapgpu_characters_state), and animated_update's clock is the queue clock (clapgpu_animation_queue_time: frame time,
// animation_next, the end callbacks), a launch of its own behind the character hooks -- character_update reads airborne
// before animated_update's callback can set it, so the fused k_characters_update_clock would race.  Chain B (below) is
// then forked behind that launch instead of at the head of the frame.
// With f->skin_select (ABI 48) the skinning follows the cull and the LOD as the reference's vertex shader does: chain B
// stops at the palette, and clapgpu_skin_drawn is the frame's last stage, behind the visible list and the LOD pick (and
// behind the join), over the frame's own mask planes and cur_lod.
// With f->views_source / f->views_state (ABI 49) nothing about a view is a kernel argument: clapgpu_views_calc is the
// frame's first launch, ahead of any fork, the entity update runs without its fused cull (the fused kernels take their
// frustum by value and are not touched: entities.hip) with clapgpu_entities_cull_views behind it over the boxes it stored,
// and particles, light grid and LOD pick read the block.  A captured frame then follows whatever the source holds.
// With f->camera (ABI 50) the camera controller runs in the reference's place in the frame, scene_cameras_calc behind
// scene_update (clap.c:614-616): the head clapgpu_views_calc stays (particles and the light grid see the camera the
// previous frame left, as the reference's do) and, behind the join, clapgpu_joint_pos_world and the light grid, come
// clapgpu_bp_index(camera_bp) when an index is asked for, clapgpu_camera_calc (camera.hip: camera_target, the pull-in rays
// against this frame's colliders, the orbit; it writes slot 0 of the source), a second clapgpu_views_calc, and only then
// the cull, which therefore moves from behind the update to here, the visible list, the LOD pick and skin_select.
// With f->cascades (ABI 51) the rest of scene_camera_calc (scene.c:1015-1046) follows the camera there, so the tail takes
// that shape whether or not f->camera is set: clapgpu_entities_bv_views (default_update's bounding-volume pick, when
// bv_result is given; ahead of the camera, whose previous position it reads from the head views_calc), the camera,
// clapgpu_cascades_calc (cascades.hip: the cascade sub-frusta, near_backup, the light's views; it writes the light's slot
// of the source), the second clapgpu_views_calc, the cull, the list, the LOD pick and skin_select.
// With f->spots (ABI 52) light_update (scene.c:1170, ahead of mq_update) runs where the reference has it: clapgpu_lights_update
// directly before the light hand-off, behind the body read-back and the character hooks, which set DIRTY, and ahead of the
// entity update, which clears it.  With a carrier_view_slot it writes a spot's pose into the source behind the head
// views_calc, so the tail takes the cascades frame's shape: the second views_calc and the cull behind the join.  With
// f->view_visible[v] the frame also compacts plane v of entities->views behind the main list: shadow pass v's list.
// With f->draw (ABI 53) the frame leaves what _models_render (model.c:742-1086) consumes: clapgpu_draw_records per pass.
// pipeline_render runs the shadow passes before the model pass (pipeline-builder.c:246-272) and they have no camera, so
// they draw with the cur_lod the last model pass left (model.c:975): the further views' records are issued behind the
// cull and AHEAD of the visible list and the LOD pick, the main pass's behind the pick; skin_select stays last.
//
// Round 4: the frame as THREE CHAINS (opt-in: CLAPGPU_FRAME_OVERLAP).  What the reference runs in list order has only these
// data dependences:
//   A  physics substeps -> character hooks -> body read-back / rotation push / light hand-off -> entity update
//      (a chain of ~12 launches at the launch floor and two dozen MB each: latency, HBM idle)
//   B  animation clock -> keyframes + palette (k_pose) -> skinning (k_skin): 1.3 GB of HBM traffic, no input from A but
//      ONE -- joint world positions are e->mx * mpos (model.c:1400) and e->mx is A's last product.  k_pose therefore
//      leaves the model-space mpos (model.c:1392-1397) in joint_pos[] and a 16-byte-per-joint pass behind the join
//      multiplies it by e->mx: the same two mat4x4_mul_vec4_post, bit for bit (clapgpu_joint_pos_world)
//   C  particles (needs the view matrix alone)
// A runs on the caller's stream, B and C on two helper streams forked from it by an event and joined by two; behind
// the join: joint positions, light grid (needs A's light hand-off), visible list + LOD (need A's boxes).  Fork / join
// by events is what stream capture records as graph edges, so FrameLoop.capture() captures the overlap as it is.
// MEASURED (profiles/r04_a/frame_overlap.md): the chains do run at the same time -- 368 of a frame's 596 us have two or
// more kernels in flight -- and the frame is no shorter: 0.64-0.65 ms against 0.62-0.63 ms on one stream.  The physics
// chain is not idle time waiting to be filled: its kernels are bound by atomics, LDS and dependent loads on the SAME
// CUs, and next to k_pose (whose persistent workgroups hold every CU's registers) or k_skin they run 2-10x longer
// (k_bp_scatter 10 -> 110 us, k_bp_emit 20 -> 142 us).  Lower stream priority for B / C, a k_pose of 8 instead of 12
// wavefronts per CU, and CU-masked helper streams (slower still) changed nothing.  The default therefore stays ONE
// stream in the reference's order; the overlapped form is kept behind the flag, bit-identical (tests/test_frame_gpu.py).
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "views_dev.h"
#include "geoms_dev.h"
#include "draw_dev.h"

using namespace clapgpu;

#define FR(x) do { int rc__ = (x); if (rc__) return rc__; } while (0)

namespace {
struct FrameStreams { int dev; hipStream_t b, c; hipEvent_t fork, join_b, join_c, fork_b; };
thread_local FrameStreams g_fs = { -1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };

int frame_streams(FrameStreams **out)
{
    int dev = 0;
    CLAPGPU_HIP(hipGetDevice(&dev));
    if (g_fs.dev != dev) {                                       // per thread and device, for the life of the process
        FrameStreams n = { dev, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
        hipError_t err = hipStreamCreateWithFlags(&n.b, hipStreamNonBlocking);
        if (err == hipSuccess) err = hipStreamCreateWithFlags(&n.c, hipStreamNonBlocking);
        if (err == hipSuccess) err = hipEventCreateWithFlags(&n.fork, hipEventDisableTiming);
        if (err == hipSuccess) err = hipEventCreateWithFlags(&n.join_b, hipEventDisableTiming);
        if (err == hipSuccess) err = hipEventCreateWithFlags(&n.join_c, hipEventDisableTiming);
        if (err == hipSuccess) err = hipEventCreateWithFlags(&n.fork_b, hipEventDisableTiming);
        if (err != hipSuccess) {                                 // nothing half-made is kept (or leaked)
            if (n.b) (void)hipStreamDestroy(n.b);
            if (n.c) (void)hipStreamDestroy(n.c);
            if (n.fork) (void)hipEventDestroy(n.fork);
            if (n.join_b) (void)hipEventDestroy(n.join_b);
            if (n.join_c) (void)hipEventDestroy(n.join_c);
            if (n.fork_b) (void)hipEventDestroy(n.fork_b);
            return hip_fail(err, "clapgpu_frame_issue: helper streams");
        }
        g_fs = n;
    }
    *out = &g_fs;
    return CLAPGPU_OK;
}
} // namespace

// Everything between the fork and the join of an overlapped frame.  Whatever it returns, the caller joins the helper
// streams before it returns itself: a failed launch in chain A must not leave the caller's stream unordered behind pose,
// skinning and particles work that is still writing (and, under stream capture, must not leave forked streams unjoined:
// EndCapture would fail and invalidate the capture).
static int frame_body(void *stream, const clapgpu_frame *f, double now, uint32_t substeps, bool overlap, FrameStreams *fs,
                      void *sb, void *sc, bool *b_forked, bool *joined);

extern "C" int clapgpu_frame_issue(void *stream, const clapgpu_frame *f, double now, uint32_t substeps)
{
    if (!f || !f->entities) return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if ((f->views_source != nullptr) != (f->views_state != nullptr) || (f->views_state && f->frustum) ||
        (f->views_state && (!view_block_ok(f->views_source) || !view_block_ok(f->views_state))))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (f->views_state && f->entities->views && f->entities->views->n > CLAPGPU_EXTRA_VIEWS_MAX)
        return CLAPGPU_ERR_INVALID_ARGUMENTS;
    if (f->camera && (!f->views_state || !view_block_ok(f->camera) || (f->camera_bp && !f->bodies)))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;                    // the camera writes the view block's source
    if (f->cascades && (!f->views_state || !view_block_ok(f->cascades) || !f->entities->views || f->entities->views->n < 1))
        return CLAPGPU_ERR_INVALID_ARGUMENTS;                    // the fit writes the light's slot of the source
    if (f->spots) {                                              // the tracked lights: slots to write, and a block for a spot's view
        if (!f->lights || (f->spots->carrier_view_slot && !f->views_state)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
        FR(spots_check(f->entities, f->spots, f->lights, f->views_source));
    }
    for (uint32_t v = 0; v < CLAPGPU_EXTRA_VIEWS_MAX; v++) {     // a shadow pass's list: a plane to compact, beside a main view
        if (!f->view_visible[v]) continue;
        const clapgpu_views *xv = f->entities->views;
        if (!(f->frustum || f->views_state) || !xv || v >= xv->n || !xv->vis_mask[v] || !f->view_visible_count[v] ||
            !f->visible_scratch)
            return CLAPGPU_ERR_INVALID_ARGUMENTS;
    }
    if (f->draw) {                                               // the passes' records: a main view, and what the call itself asks
        const clapgpu_frame_draw *d = f->draw;
        const clapgpu_entities *e = f->entities;
        if (!(f->frustum || f->views_state) || !d->order || !d->scratch || (reinterpret_cast<uintptr_t>(d->scratch) & 255u) ||
            !e->vis_mask)
            return CLAPGPU_ERR_INVALID_ARGUMENTS;
        if ((reinterpret_cast<uintptr_t>(e->mx) | reinterpret_cast<uintptr_t>(e->inv_mx) |
             reinterpret_cast<uintptr_t>(d->inputs ? d->inputs->color : nullptr)) & 15u)
            return CLAPGPU_ERR_INVALID_ARGUMENTS;
        if (d->main.count)
            FR(draw_check(e, e->vis_mask, d->order, &d->main.pass, d->main.records, d->main.capacity, d->main.count,
                          d->main.group_first, d->main.status));
        for (uint32_t v = 0; v < CLAPGPU_EXTRA_VIEWS_MAX; v++) {
            const clapgpu_frame_draw_pass *p = &d->view[v];
            if (!p->count) continue;
            if (!e->views || v >= e->views->n || !e->views->vis_mask[v]) return CLAPGPU_ERR_INVALID_ARGUMENTS;
            FR(draw_check(e, e->views->vis_mask[v], d->order, &p->pass, p->records, p->capacity, p->count, p->group_first,
                          p->status));
        }
    }
    const bool animated = f->skeleton && f->animations && f->pose;
    const bool particles = f->particles && (f->view_mx || f->views_state);
    const bool overlap = (f->flags & CLAPGPU_FRAME_OVERLAP) && (animated || particles);
    if (f->aniq) {                                               // the queues drive the pose: asked before anything is issued
        if (!animated || f->pose->anim != f->aniq->pose_anim || f->pose->frame_time != f->aniq->frame_time ||
            f->pose->n_chars != f->aniq->n)
            return CLAPGPU_ERR_INVALID_ARGUMENTS;
    }
    if (f->skin_select) {                                        // skinning what is drawn: a palette and a cull to follow
        const clapgpu_entities *e = f->entities;
        if (!f->skin || !animated || !(f->frustum || f->views_state)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
        if (f->skin_select->n_planes == 0 && (!e->vis_mask || (e->views && e->views->n > CLAPGPU_EXTRA_VIEWS_MAX)))
            return CLAPGPU_ERR_INVALID_ARGUMENTS;
    }
    if (f->views_state)                                          // the views of this frame: ahead of every reader, on every chain
        FR(clapgpu_views_calc(stream, f->views_source, f->views_state, 1 + (f->entities->views ? f->entities->views->n : 0)));
    void *sb = stream, *sc = stream;                             // chains B and C: the caller's stream unless they overlap
    FrameStreams *fs = nullptr;
    bool b_forked = false;                                       // with aniq chain B is forked later, behind the queue clock
    if (overlap) {
        FR(frame_streams(&fs));
        CLAPGPU_HIP(hipEventRecord(fs->fork, as_stream(stream)));
        if (animated) sb = fs->b;
        if (animated && !f->aniq) {
            const hipError_t err = hipStreamWaitEvent(fs->b, fs->fork, 0);
            if (err != hipSuccess) return hip_fail(err, "clapgpu_frame_issue: fork");      // nothing forked yet
            b_forked = true;
        }
        if (particles) {
            const hipError_t err = hipStreamWaitEvent(fs->c, fs->fork, 0);
            if (err != hipSuccess) {
                if (b_forked) {                                  // b is forked already: join it before giving up
                    (void)hipEventRecord(fs->join_b, fs->b);
                    (void)hipStreamWaitEvent(as_stream(stream), fs->join_b, 0);
                }
                return hip_fail(err, "clapgpu_frame_issue: fork");
            }
            sc = fs->c;
        }
    }
    bool joined = false;
    const int rc = frame_body(stream, f, now, substeps, overlap, fs, sb, sc, &b_forked, &joined);
    if (overlap && !joined) {                                    // an early exit: the one join every path goes through
        if (b_forked) { (void)hipEventRecord(fs->join_b, fs->b); (void)hipStreamWaitEvent(as_stream(stream), fs->join_b, 0); }
        if (particles) { (void)hipEventRecord(fs->join_c, fs->c); (void)hipStreamWaitEvent(as_stream(stream), fs->join_c, 0); }
    }
    return rc;
}

static int frame_body(void *stream, const clapgpu_frame *f, double now, uint32_t substeps, bool overlap, FrameStreams *fs,
                      void *sb, void *sc, bool *b_forked, bool *joined)
{
    const clapgpu_entities *e = f->entities;
    const bool animated = f->skeleton && f->animations && f->pose;
    const bool particles = f->particles && (f->view_mx || f->views_state);
    const clapgpu_views_state *vs = f->views_state;             // NULL: the views are host values
    // joint positions need e->mx: with the chains apart k_pose stops at the model-space position
    clapgpu_pose_batch pose_b;
    bool finish_pos = false;
    if (animated) {
        pose_b = *f->pose;
        finish_pos = overlap && pose_b.joint_pos && !(pose_b.skip & CLAPGPU_POSE_SKIP_JOINT_POS);
        if (finish_pos) pose_b.skip |= CLAPGPU_POSE_JOINT_POS_MODEL;
    }

    // ---- chain B: animated_update -- clock, pose, palette; the vertex shader's skinning loop once per frame ----
    // one stream: the clock rides the character hooks' launch (two per-character passes over different state)
    // (not with aniq: character_update reads airborne, which animated_update's callback sets behind it)
    const bool clock_with_hooks = !overlap && animated && f->anim_clock && f->characters && !f->aniq;
    auto chain_b = [&]() -> int {
        if (!animated) return CLAPGPU_OK;
        if (f->anim_clock && !clock_with_hooks && !f->aniq) {
            if (f->now_dev) FR(clapgpu_animation_time_dev(sb, f->anim_clock, f->now_dev));
            else FR(clapgpu_animation_time(sb, f->anim_clock, now));
        }
        FR(clapgpu_pose_update(sb, f->skeleton, f->animations, &pose_b));
        if (f->skin && !f->skin_select)                              // with skin_select: the frame's last stage, below
            FR(clapgpu_skin(sb, f->skin));
        return CLAPGPU_OK;
    };
    // ---- chain C: particles_update hooks ----
    auto chain_c = [&]() -> int {
        if (particles && vs) FR(clapgpu_particles_update_views(sc, f->particles, vs));
        else if (particles) FR(clapgpu_particles_update(sc, f->particles, f->view_mx));
        return CLAPGPU_OK;
    };
    if (overlap) {                                               // issued first: their launches are in the queues while A's are made
        if (!f->aniq) FR(chain_b());
        FR(chain_c());
    }

    // ---- chain A.  scene_characters_move (clap.c:589): ground ray, velocity, slide and push of the movers ----
    if (f->move) {
        if (!f->bodies || !f->world || !f->static_geoms) return CLAPGPU_ERR_INVALID_ARGUMENTS;
        FR(clapgpu_characters_move(stream, f->bp, f->bodies, f->world, f->static_geoms, f->meshes, f->move->entity ? e : nullptr,
                                   f->move_dt_sec, f->move, f->move_scratch));
        if (f->aniq)                                             // character_move's character_set_state, on the device
            FR(clapgpu_characters_state(stream, f->aniq, f->move, now, f->now_dev));
    }
    // ---- phys_step: per substep broadphase x2, contacts, dWorldQuickStep's body stage (physics.c:746-771) ----
    if (f->bodies && f->world) {
        for (uint32_t s = 0; s < substeps; s++) {
            if (f->bp) {
                FR(clapgpu_bp_collide(stream, f->bp, f->bodies->n, f->bodies->aabb, f->pairs, f->pair_capacity, f->pair_total,
                                      f->static_pairs, f->static_pair_capacity, f->static_pair_total));
                if (f->body_geoms && f->contacts && f->static_geoms && f->static_contacts && f->static_pair_total &&
                    f->pair_capacity < (1u << 24) && f->static_pair_capacity < (1u << 24)) {
                    FR(clapgpu_contacts_geoms_both(stream, f->bp, f->body_geoms, f->static_geoms, f->pairs, f->pair_total,
                                                   f->pair_capacity, f->contacts, f->contact_total, f->static_pairs,
                                                   f->static_pair_total, f->static_pair_capacity, f->static_contacts,
                                                   f->static_contact_total, f->bodies->bflags));
                } else if (f->body_geoms && f->contacts) {
                    FR(clapgpu_contacts_geoms(stream, f->body_geoms, f->body_geoms, f->pairs, f->pair_total, f->pair_capacity,
                                              f->contacts, f->contact_total, f->bodies->bflags, f->bodies->bflags));
                    if (f->static_geoms && f->static_contacts && f->static_pair_total)
                        FR(clapgpu_contacts_geoms(stream, f->body_geoms, f->static_geoms, f->static_pairs, f->static_pair_total,
                                                  f->static_pair_capacity, f->static_contacts, f->static_contact_total,
                                                  f->bodies->bflags, nullptr));
                }
                if (f->meshes && f->body_geoms && f->static_geoms && f->static_pair_total)
                    FR(clapgpu_contacts_meshes(stream, f->body_geoms, f->static_geoms, f->meshes, f->static_pairs,
                                               f->static_pair_total, f->static_pair_capacity, f->mesh_scratch,
                                               f->mesh_contact_capacity, f->mesh_contacts, f->mesh_ref,
                                               f->mesh_contact_total, f->mesh_capped, f->bodies->bflags));
            }
            if (f->island_scratch) {                             // dxProcessIslands: behind every launch that sets HAS_JOINT
                if (!f->bp || !f->body_geoms || !f->contacts) return CLAPGPU_ERR_INVALID_ARGUMENTS;
                FR(clapgpu_bodies_islands(stream, f->bodies, f->world, 1.0 / 120.0, f->pairs, f->pair_total, f->pair_capacity,
                                          f->contacts, f->island_scratch, f->island, f->island_woken));
            }
            if (f->solve_scratch) {                              // the contact rows: between the island pass and the step
                if (!f->island_scratch || !f->island) return CLAPGPU_ERR_INVALID_ARGUMENTS;
                clapgpu_solver sv;
                if (f->solver) sv = *f->solver;
                else clapgpu_solver_defaults(&sv);
                const bool statics = f->static_pairs && f->static_pair_total && f->static_contacts && f->static_geoms;
                const bool meshes = statics && f->meshes && f->mesh_contacts && f->mesh_ref && f->mesh_contact_total;
                FR(clapgpu_bodies_solve(stream, f->bodies, f->world, &sv, 1.0 / 120.0, f->island,
                                        statics ? f->static_pairs : nullptr, statics ? f->static_pair_total : nullptr,
                                        statics ? f->static_pair_capacity : 0, statics ? f->static_contacts : nullptr,
                                        meshes ? f->mesh_contacts : nullptr, meshes ? f->mesh_ref : nullptr,
                                        meshes ? f->mesh_contact_total : nullptr, meshes ? f->mesh_contact_capacity : 0,
                                        f->pairs, f->pair_total, f->pair_capacity, f->contacts, f->solve_rows_capacity,
                                        f->solve_scratch, nullptr, nullptr, nullptr, f->solve_status, nullptr, nullptr));
            }
            if ((f->flags & CLAPGPU_FRAME_PREBIN) && f->bp && f->bodies->aabb)
                FR(clapgpu_bodies_step_prebin(stream, f->bodies, f->world, 1.0 / 120.0, f->bp));
            else
                FR(clapgpu_bodies_step(stream, f->bodies, f->world, 1.0 / 120.0));      // fixed_dt, physics.c:775
        }
    }
    // ---- character_update hooks (character.c:583-611) ----
    if (clock_with_hooks)
        FR(clapgpu_characters_update_clock(stream, f->characters, e, f->bodies, f->anim_clock, now, f->now_dev));
    else if (f->characters)
        FR(clapgpu_characters_update(stream, f->characters, e, f->bodies));
    // ---- animated_update's clock with the queues: behind the hooks, in list order; chain B starts here ----
    if (f->aniq) {
        FR(clapgpu_animation_queue_time(stream, f->aniq, now, f->now_dev));
        if (overlap) {
            CLAPGPU_HIP(hipEventRecord(fs->fork_b, as_stream(stream)));
            CLAPGPU_HIP(hipStreamWaitEvent(fs->b, fs->fork_b, 0));
            *b_forked = true;
            FR(chain_b());
        }
    }
    // ---- default_update: phys_body_update of dynamic bodies (model.c:1659-1665), rotation push (1680-1687),
    //      light hand-off (1689-1694) ----
    if (f->bodies) {
        FR(clapgpu_phys_body_update(stream, f->bodies, e->n, const_cast<float *>(e->pos_scale), const_cast<float *>(e->rot),
                                    e->flags, nullptr));
        if (f->n_body_links)
            FR(clapgpu_bodies_rotate_from_entities(stream, f->bodies, e, 0, f->n_body_links, f->link_body, f->link_entity));
    }
    if (f->spots)                                                // light_update (scene.c:1170): ahead of mq_update's hand-off
        FR(clapgpu_lights_update(stream, e, 0, f->spots, f->lights, const_cast<clapgpu_views_source *>(f->views_source)));
    if (f->lights && f->n_light_carriers)
        FR(clapgpu_lights_from_entities(stream, e, 0, f->n_light_carriers, f->carrier_entity, f->carrier_light, f->carrier_offset,
                                        f->lights));
    // ---- TRS -> mx -> inverse -> AABB (+ the main view's cull) ----
    if (f->tile_row_start)
        FR(clapgpu_entities_update_tiles(stream, e, f->tile_row_start, f->n_tiles, 0, f->frustum));
    else
        FR(clapgpu_entities_update(stream, e, f->level_start, f->n_levels, 0, f->frustum));
    // scene_cameras_calc on the device, or a spot's view written above (behind the head views_calc): the cull waits for it
    const bool late_views = f->camera || f->cascades || (f->spots && f->spots->carrier_view_slot);
    if (vs && !late_views)                                       // f->frustum is NULL: the update above did not cull
        FR(clapgpu_entities_cull_views(stream, e, vs));

    if (overlap) {                                               // join
        *joined = true;                                          // (a failure inside these four calls cannot be joined any better by the caller)
        if (*b_forked) { CLAPGPU_HIP(hipEventRecord(fs->join_b, fs->b)); CLAPGPU_HIP(hipStreamWaitEvent(as_stream(stream), fs->join_b, 0)); }
        if (particles) { CLAPGPU_HIP(hipEventRecord(fs->join_c, fs->c)); CLAPGPU_HIP(hipStreamWaitEvent(as_stream(stream), fs->join_c, 0)); }
        if (finish_pos) FR(clapgpu_joint_pos_world(stream, f->skeleton, f->pose));
    } else {
        FR(chain_b());
        FR(chain_c());
    }
    // ---- scene_update: light_grid_compute ----
    if (f->lights && f->light_tiles && vs)
        FR(clapgpu_light_grid_compute_views(stream, f->lights, vs, f->light_width, f->light_height, f->light_cell, f->light_tiles));
    else if (f->lights && f->light_tiles && f->view_mx && f->proj_mx)
        FR(clapgpu_light_grid_compute(stream, f->lights, f->view_mx, f->proj_mx, f->light_width, f->light_height, f->light_cell,
                                      f->light_tiles));
    // ---- scene_cameras_calc (clap.c:616): camera_update and the cascades on the device, this frame's views, and the cull
    //      they wait for.  The bounding-volume pick is default_update's: it sees the camera the previous frame left (the
    //      head views_calc's cam_pos) and runs ahead of the camera ----
    if (f->cascades && f->bv_result)
        FR(clapgpu_entities_bv_views(stream, e, vs, f->bv_has_ctl, f->bv_ctl_entity, f->bv_result, nullptr));
    if (f->camera) {
        clapgpu_geoms none, from_bodies;
        memset(&none, 0, sizeof(none));
        const clapgpu_geoms *bg = f->body_geoms;
        if (!bg && f->bodies) {
            if (!body_geoms(f->bodies, &from_bodies)) return CLAPGPU_ERR_INVALID_ARGUMENTS;
            bg = &from_bodies;
        }
        if (f->camera_bp) FR(clapgpu_bp_index(stream, f->camera_bp, f->bodies->n, f->bodies->aabb));
        FR(clapgpu_camera_calc(stream, f->camera, e, animated ? f->pose->joint_pos : nullptr, f->camera_bp, bg ? bg : &none,
                               f->static_geoms ? f->static_geoms : &none, f->meshes, const_cast<clapgpu_views_source *>(f->views_source)));
    }
    if (f->cascades)
        FR(clapgpu_cascades_calc(stream, f->cascades, const_cast<clapgpu_views_source *>(f->views_source), e, f->bv_result));
    if (late_views) {
        FR(clapgpu_views_calc(stream, f->views_source, f->views_state, 1 + (e->views ? e->views->n : 0)));
        FR(clapgpu_entities_cull_views(stream, e, vs));
    }
    // ---- the shadow passes' draw records: ahead of the model pass, with the LODs the last one left (model.c:975) ----
    if (f->draw)
        for (uint32_t v = 0; v < CLAPGPU_EXTRA_VIEWS_MAX; v++) {
            const clapgpu_frame_draw_pass *p = &f->draw->view[v];
            if (p->count)
                FR(clapgpu_draw_records(stream, e, e->views->vis_mask[v], f->cur_lod, f->draw->order, f->draw->inputs, &p->pass,
                                        p->records, p->capacity, p->count, p->group_first, p->status, f->draw->scratch));
        }
    // ---- render pass glue: ordered visible list + LOD pick ----
    if ((f->frustum || vs) && f->visible && f->visible_count && f->visible_scratch) {
        if (f->cur_lod && f->draw_lod && vs)
            FR(clapgpu_visible_compact_lod_views(stream, e, f->index_base, vs, f->force_lod, f->cur_lod, f->visible,
                                                 f->visible_count, f->draw_lod, f->visible_scratch));
        else if (f->cur_lod && f->draw_lod)                      // list + LODs in one launch
            FR(clapgpu_visible_compact_lod(stream, e, f->index_base, f->cam_pos, f->force_lod, f->cur_lod, f->visible,
                                           f->visible_count, f->draw_lod, f->visible_scratch));
        else
            FR(clapgpu_visible_compact(stream, e->vis_mask, e->vis_row_pop, e->n, f->index_base, f->visible, f->visible_count,
                                       f->visible_scratch));
    }
    // ---- the shadow passes' lists (_models_render with view = &light->view[0]): no camera, no LOD pick (model.c:975) ----
    for (uint32_t v = 0; v < CLAPGPU_EXTRA_VIEWS_MAX; v++)
        if (f->view_visible[v])
            FR(clapgpu_visible_compact(stream, e->views->vis_mask[v], e->views->vis_row_pop[v], e->n, f->index_base,
                                       f->view_visible[v], f->view_visible_count[v], f->visible_scratch));
    // ---- the model pass's draw records: behind the LOD pick (model.c:975-997), this frame's cur_lod ----
    if (f->draw && f->draw->main.count) {
        const clapgpu_frame_draw_pass *p = &f->draw->main;
        FR(clapgpu_draw_records(stream, e, e->vis_mask, f->cur_lod, f->draw->order, f->draw->inputs, &p->pass, p->records,
                                p->capacity, p->count, p->group_first, p->status, f->draw->scratch));
    }
    // ---- the vertex shader's skinning loop for what the passes draw, at the LOD just picked (model.c:959-997) ----
    if (f->skin_select) {
        clapgpu_skin_select sel = *f->skin_select;
        if (sel.n_planes == 0) {                                 // the frame's own planes: the main view's and the further views'
            const uint32_t nx = e->views ? e->views->n : 0;
            sel.planes[0] = e->vis_mask;
            for (uint32_t v = 0; v < nx; v++) sel.planes[1 + v] = e->views->vis_mask[v];
            sel.n_planes = 1 + nx;
            sel.n_entities = e->n;
        }
        if (!sel.cur_lod) sel.cur_lod = f->cur_lod;
        FR(clapgpu_skin_drawn(stream, f->skin, &sel));
    }
    return CLAPGPU_OK;
}
