"""One display frame of the batched path, in the reference's order.

``clap_frame()`` (core/clap.c:551-665) runs: ``phys_step`` (clap.c:604) -> ``scene_update`` ->
``mq_update`` with every entity's update hook in list order -- ``character_update`` (character.c:583)
in front of ``default_update`` (model.c:1649: body read-back, TRS rebuild, light hand-off, rotation
push to colliders, ``animated_update``), ``particles_update`` (particle.c:89) -> camera / light grid
-> render passes (frustum test, LOD pick per drawn entity; the vertex shader skins).  The sequence itself
lives in C: ``clapgpu_frame_issue`` (clap_amd/csrc/frame.hip) issues it as a fixed series of launches on one
stream from a ``clapgpu_frame`` descriptor; ``FrameLoop`` only gathers the descriptor from the harness objects,
keeps the host-side time base and captures / replays the call as a HIP graph.  Nothing is read back unless asked.
(A variant that forked the particle systems and one broadphase pass onto a side stream was measured in round 1:
no faster at BASELINE size, slower at testbed size; removed.)
"""
import numpy as np
import torch

from . import entities as ent_mod


class FrameLoop:
    def __init__(self, batch, cam, world=None, feed=None, body_links=None, lights=None, characters=None,
                 particles=None, contacts=False, pose_readers=("trs", "joint_pos"), prebin=False, islands=False, solve=False,
                 move=None, aniq=None, skin_select=None, views_dev=False, camera=None, camera_index=False, cascades=None,
                 bv_result=None, bv_ctl_entity=None, view_lists=False, draw=None):
        """batch: EntityBatch.  world: PhysWorld (dynamic bodies write their entities through
        body_entity; character bodies have body_entity = -1).  feed: CharacterFeed.  body_links:
        (link_body, link_entity) of characters / static colliders whose rotation follows the entity.
        lights: LightSet (with carriers).  characters: CharacterBatch (pose + skin).  particles:
        ParticleBatch.  pose_readers: which of the pose's host-visible by-products somebody reads this frame --
        "trs" (struct joint's translation / rotation / scale) and "joint_pos" (struct joint.pos: camera_target,
        camera.c:191-205); the draw path and the skinning consume joint_transforms alone (model.c:1020-1022), so a frame
        whose skinning runs on the device registers none and the pose writes 64 of its 120 bytes per joint
        (clapgpu_pose_batch.skip).  A model with (joint, path) pairs that have no channel keeps "trs": such a path's
        value lives there (model.c:1301).  islands: every substep wakes sleeping bodies by contact
        (clapgpu_bodies_islands between its contacts and its step; implies contacts).  solve: every substep's contacts
        act on the bodies (clapgpu_bodies_solve between the island pass and the step; implies islands).  move: a
        physics.CharacterMoves over `world`: character_move of those characters is the frame's first stage
        (clapgpu_characters_move, scene_characters_move of clap.c:589) with the frame's dt as its raw frame delta; the
        host updates its arrays (CharacterMoves.set) between frames and reads its outputs after them.  aniq: an
        animation.AnimationQueues over `characters`: character_set_state follows the move on the device
        (clapgpu_characters_state) and the queue clock (clapgpu_animation_queue_time) takes the place of the plain one,
        so the frame needs no host between the move and the pose; the host reads aniq's events afterwards.
        skin_select: True, or the keyword arguments of CharacterBatch.set_skin_select (entity, row, lod_lists; planes
        and cur_lod given there replace the frame's own): the frame skins what its passes draw -- clapgpu_skin_drawn as
        its last stage, over the batch's main plane and the planes of its further views at the LODs just picked, in place
        of clapgpu_skin.  None (the default): the plain call.  views_dev: the frame's views live in device memory (a
        views.ViewBlock; clapgpu_frame.views_source / views_state): set_camera writes the pose into pinned host memory
        and every frame copies it to the device ahead of its launches, the frame's first launch derives frustum,
        matrices and camera position from it (clapgpu_views_calc) and cull, light grid, particles and LOD pick read
        those, so neither set_camera nor a replayed graph needs a new descriptor.  Further views of the batch go into
        slots 1.. from the matrices given to EntityBatch.set_views(..., matrices=).  camera: a camera.CameraBlock (needs
        views_dev): the camera controller runs on the device in the reference's place in the frame
        (clapgpu_frame.camera: camera_target, the pull-in rays against `world`'s colliders, the orbit, then this frame's
        views and the cull), so a following camera needs no read-back and a replayed graph follows the control entity.
        The caller writes the block's inputs (CameraBlock.set + upload) whenever they change; the frame copies the view
        source only after set_camera, since slot 0's pose is now the device's.  camera_index: the rays go through an
        index of the world's broadphase grid built in the frame (clapgpu_frame.camera_bp) instead of scanning.
        cascades: a cascades.CascadesBlock (needs views_dev and a further view of the batch in the block's light_slot):
        the shadow light's views are fitted to the camera's cascade sub-frusta on the device behind the camera
        (clapgpu_frame.cascades), the light's main view goes into its slot of the view source and the shadow planes are
        culled against it, so the light follows the camera without a read-back, replayed graphs included.  The caller
        writes the block's inputs (CascadesBlock.set + upload) whenever they change.  From the first frame on the light's
        slot of the source is the device's: later copies of the source leave it out.  bv_result: a device int64 tensor
        of one key: the frame runs default_update's bounding-volume pick (clapgpu_entities_bv_views, with bv_ctl_entity
        as the control entity or None) ahead of the camera and the cascades read it when their block asks for
        near_backup from the volume.  A `lights` with tracked lights (LightSet.set_spots) makes the frame run light_update
        on the device ahead of the light hand-off (clapgpu_frame.spots); with view slots (needs views_dev) the
        spotlights' poses go into the view source and the shadow planes are culled against this frame's spot, replayed
        graphs included; the batch's further view in such a slot gives its projection (EntityBatch.set_views(None,
        matrices=[(any view matrix, lights.spot_persp(cutoff, z01), z01)])), and from the first frame on those slots of
        the source are the device's.  view_lists: the frame also
        writes the ordered list of every further view (clapgpu_frame.view_visible: batch.view_visible[v] /
        batch.view_visible_count[v]), the shadow passes' lists.  draw: a draw.FrameDraw: the frame also leaves every
        pass's draw records in render order (clapgpu_frame.draw) -- the further views' ahead of the LOD pick, with the
        LODs the previous frame left, the main pass's behind it."""
        self.draw = draw
        islands = islands or solve
        self.view_lists = view_lists
        self.move, self.move_dt = move, 0.0
        self.aniq = aniq
        self.skin_select = skin_select
        self.solve = solve
        self.batch, self.world, self.feed, self.lights = batch, world, feed, lights
        self.characters, self.particles = characters, particles
        self.body_links, self.contacts = body_links, contacts or islands
        self.islands = islands
        self.overlap = False        # CLAPGPU_FRAME_OVERLAP: a caller may set it (three chains on three streams, frame.hip)
        self.prebin = prebin        # CLAPGPU_FRAME_PREBIN: the step bins its boxes for the next frame's broadphase (nothing else writes them)
        self._desc = None
        self.views = None
        self.camera, self.camera_index = camera, camera_index
        self._views_dirty = True
        self.cascades, self.bv_result, self.bv_ctl_entity = cascades, bv_result, bv_ctl_entity
        self._light_slot_sent = False
        if cascades is not None and not views_dev:
            from . import _lib
            raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "FrameLoop", "cascades: the fit writes the view block (views_dev=True)")
        if camera is not None and not views_dev:
            from . import _lib
            raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "FrameLoop", "camera: the camera writes the view block (views_dev=True)")
        if views_dev:
            from .views import ViewBlock
            self.views = ViewBlock(batch.device)
        if characters is not None:
            missing = bool(characters.model.anim_desc.packed_layout & 0x010)        # POSE_LAYOUT_MISSING (pose_pack.h)
            characters.set_outputs(trs=("trs" in pose_readers) or missing, joint_pos="joint_pos" in pose_readers)
        self.set_camera(cam)

    def set_camera(self, cam):
        self.cam = cam
        if self.views is not None:                          # the source block: the descriptor does not change
            self.views.set_camera(0, cam)
            self._views_dirty = True
            return
        self.frustum, self.view_mx, self.proj_mx = ent_mod.view_calc_frustum(cam)
        self._desc = None                                   # frustum / matrices are part of the descriptor

    def _further_views(self):
        """Slots 1.. of the source block from the batch's further views (EntityBatch.set_views(..., matrices=))."""
        from . import _lib
        b = self.batch
        extra = getattr(b, "view_matrices", None) or []
        if len(getattr(b, "view_masks", [])) != len(extra):
            raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "FrameLoop",
                                    "views_dev: EntityBatch.set_views(..., matrices=) for every further view")
        spot_slots = self.lights.spot_view_slots() if self.lights is not None else []
        for v, (vm, pm, z01) in enumerate(extra):
            if 1 + v in spot_slots:                         # a spotlight's view: a pose slot, its pose the device's
                self.views.set_pose(1 + v, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), pm, ndc_z_zero_one=z01)
            else:
                self.views.set_matrices(1 + v, vm, pm, ndc_z_zero_one=z01)
        self._views_seen = getattr(b, "view_matrices", None)

    # ---- the clapgpu_frame descriptor ---------------------------------------------------
    def _build(self):
        import ctypes as C
        from . import _lib
        b, w = self.batch, self.world
        f = _lib.FrameDesc()
        keep = []                                           # ctypes objects the descriptor points into
        f.entities = C.pointer(b._desc)
        if b.tiled:
            f.tile_row_start, f.n_tiles = b.tile_row_start.data_ptr(), b.n_tiles
        else:
            f.level_start, f.n_levels = b.level_start.ctypes.data, b.n_levels
        if self.views is not None:
            self._further_views()
            f.views_source, f.views_state = self.views.source.data_ptr(), self.views.state.data_ptr()
        else:
            f.frustum = C.pointer(self.frustum)
        if w is not None:
            f.bodies, f.world, f.bp = C.pointer(w._desc), C.pointer(w.world), w._bp
            f.pairs, f.pair_capacity, f.pair_total = w.pairs.data_ptr(), w.capacity, w.pair_total.data_ptr()
            if w.n_static:
                f.static_pairs, f.static_pair_capacity = w.static_pairs.data_ptr(), w.static_capacity
                f.static_pair_total = w.static_pair_total.data_ptr()
            if self.contacts:
                w.alloc_contacts()
                g = w.body_geoms()
                keep.append(g)
                f.body_geoms = C.pointer(g)
                f.contacts, f.contact_total = w.contact2_buf.data_ptr(), w.contact2_total.data_ptr()
                if w.n_static:
                    sg = w.static_geoms()
                    keep.append(sg)
                    f.static_geoms = C.pointer(sg)
                    f.static_contacts = w.static_contact2_buf.data_ptr()
                    f.static_contact_total = w.static_contact2_total.data_ptr()
                    if w._meshes is not None:                   # contacts against the static meshes (clapgpu_contacts_meshes)
                        w.alloc_mesh_contacts()
                        f.meshes = w._meshes
                        f.mesh_contacts, f.mesh_ref = w.mesh_contact_buf.data_ptr(), w.mesh_ref.data_ptr()
                        f.mesh_contact_capacity = w.mesh_contact_capacity
                        f.mesh_contact_total, f.mesh_capped = w.mesh_contact_total.data_ptr(), w.mesh_capped.data_ptr()
                        f.mesh_scratch = w.mesh_scratch.data_ptr()
            if self.islands:
                w.alloc_islands()
                f.island_scratch, f.island = w.island_scratch.data_ptr(), w.island.data_ptr()
                f.island_woken = w.island_woken.data_ptr()
            if self.solve:
                w.alloc_solve()
                keep.append(w.solver)
                f.solver = C.pointer(w.solver)
                f.solve_scratch, f.solve_rows_capacity = w.solve_scratch.data_ptr(), w.solve_rows_capacity
                f.solve_status = w.solve_status.data_ptr()
            if self.move is not None:
                if w.facc is None or self.move.world is not w:
                    raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "FrameLoop",
                                            "move: a CharacterMoves over this world, and PhysWorld(forces=True)")
                if not f.static_geoms:                          # (alone they add no launch to the physics block)
                    sg = w.static_geoms()
                    keep.append(sg)
                    f.static_geoms = C.pointer(sg)
                if w._meshes is not None:
                    f.meshes = w._meshes
                f.move, f.move_scratch = C.pointer(self.move._desc), self.move.scratch.data_ptr()
            if self.camera is not None:                         # the rays' colliders (body geoms: the frame takes the bodies')
                if not f.static_geoms and w.n_static:
                    sg = w.static_geoms()
                    keep.append(sg)
                    f.static_geoms = C.pointer(sg)
                if w._meshes is not None:
                    f.meshes = w._meshes
                if self.camera_index:
                    f.camera_bp = w._bp
            if self.body_links is not None:
                lb, le = w.upload_links(*self.body_links)
                f.n_body_links, f.link_body, f.link_entity = len(self.body_links[0]), lb.data_ptr(), le.data_ptr()
        if self.camera is not None:
            f.camera = self.camera.dev.data_ptr()
        if self.cascades is not None:
            f.cascades = self.cascades.dev.data_ptr()
            if self.bv_result is not None:
                f.bv_result = self.bv_result.data_ptr()
                f.bv_has_ctl = 0 if self.bv_ctl_entity is None else 1
                f.bv_ctl_entity = 0 if self.bv_ctl_entity is None else int(self.bv_ctl_entity)
        if self.feed is not None:
            f.characters = C.pointer(self.feed._desc)
        if self.views is None:
            vm = np.ascontiguousarray(self.view_mx, np.float32)
            pm = np.ascontiguousarray(self.proj_mx, np.float32)
            keep += [vm, pm]
            f.view_mx = vm.ctypes.data_as(C.POINTER(C.c_float))
            f.proj_mx = pm.ctypes.data_as(C.POINTER(C.c_float))
        ls = self.lights
        if ls is not None:
            d = ls._desc()
            keep.append(d)
            f.lights = C.pointer(d)
            if ls._carriers and ls._carriers[0]:
                n, ce, cl, co = ls._carriers
                f.n_light_carriers, f.carrier_entity, f.carrier_light, f.carrier_offset = n, ce.data_ptr(), cl.data_ptr(), co.data_ptr()
            if ls._spots:
                if ls._spots[4] is not None and self.views is None:
                    raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "FrameLoop", "spot views: the update writes the view block (views_dev=True)")
                sp = ls._spots_desc()
                keep.append(sp)
                f.spots = C.pointer(sp)
            tiles = ls.alloc_tiles()
            if tiles is not None:
                f.light_width, f.light_height, f.light_cell, f.light_tiles = ls.width, ls.height, ls.cell, tiles.data_ptr()
        cb = self.characters
        if cb is not None:
            if cb._clock is None:
                cb.start_clock()
            f.anim_clock = C.pointer(cb._clock)
            f.skeleton, f.animations = C.pointer(cb.model.skel_desc), C.pointer(cb.model.anim_desc)
            f.pose = C.pointer(cb._pose_desc)
            if cb._skin_desc is not None:
                f.skin = C.pointer(cb._skin_desc)
        if self.skin_select is not None and self.skin_select is not False:
            if cb is None or cb._skin_desc is None:
                raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "FrameLoop", "skin_select: characters with a skinned mesh")
            kw = dict(self.skin_select) if isinstance(self.skin_select, dict) else {}
            kw.setdefault("planes", None)                       # n_planes 0: clapgpu_frame_issue supplies the batch's planes
            cb.set_skin_select(**kw)
            f.skin_select = C.pointer(cb._sel_desc)
        if self.aniq is not None:
            if cb is None or self.aniq.batch is not cb:
                raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "FrameLoop", "aniq: AnimationQueues(batch=characters)")
            f.aniq = C.pointer(self.aniq._desc)
        if self.particles is not None:
            f.particles = C.pointer(self.particles._desc)
        b.alloc_lod()
        f.index_base = 0
        f.visible, f.visible_count, f.visible_scratch = b.visible.data_ptr(), b.visible_count.data_ptr(), b.scratch.data_ptr()
        if self.views is None:
            f.cam_pos[:] = [float(v) for v in self.cam["cam_pos"]]
        if self.view_lists:                                     # the shadow passes' lists
            from ._dev import device_array
            nv = len(getattr(b, "view_masks", []))
            if getattr(b, "view_visible", None) is None or len(b.view_visible) != nv:
                b.view_visible = [device_array((max(b.n, 1),), torch.int32, b.device) for _ in range(nv)]
                b.view_visible_count = [device_array((1,), torch.int32, b.device) for _ in range(nv)]
            for v in range(nv):
                f.view_visible[v], f.view_visible_count[v] = b.view_visible[v].data_ptr(), b.view_visible_count[v].data_ptr()
        f.force_lod = b.force_lod.data_ptr() if b.force_lod is not None else None
        f.cur_lod, f.draw_lod = b.cur_lod.data_ptr(), b.draw_lod.data_ptr()
        if self.draw is not None:                               # every pass's draw records
            dd = self.draw.desc()
            keep.append(dd)
            f.draw = C.pointer(dd)
        self._desc, self._keep = f, keep
        return f

    def capture(self, dt=1.0 / 120.0, warmup_now=0.0):
        """Record one frame (with one physics substep) as a HIP graph.  Afterwards clap_frame_replay(now) costs one
        graph launch instead of ~35 kernel launches: what a testbed-sized scene, whose frame is launch latency, needs.
        With views_dev=True the graph follows the camera: set_camera() writes the pose into the pinned source block,
        clap_frame_replay copies it to the device ahead of the replay, and the graph's first node (clapgpu_views_calc)
        derives every view from it.  Without it the frustum, the matrices and the camera position are kernel arguments
        frozen in the graph: re-capture after a camera change."""
        self.clap_frame(warmup_now, dt)                      # everything allocated, lazily created state exists
        torch.cuda.synchronize()
        self._now_host = torch.zeros(1, dtype=torch.float64).pin_memory()
        self._graph = torch.cuda.CUDAGraph()
        saved = (None if self.world is None else self.world.time_acc.value)
        with torch.cuda.graph(self._graph):
            self._issue(None, steps=1)
        if self.world is not None:
            self.world.time_acc.value = saved

    def clap_frame_replay(self, now):
        self._now_host[0] = float(now)
        if self.characters is not None:
            self.characters.now_dev.copy_(self._now_host, non_blocking=True)
        if self.views is not None:
            self._upload_views()
        self._graph.replay()

    def _upload_views(self):
        """The source block's copy ahead of a frame.  With a camera on the device slot 0's pose is the device's from the
        first frame on: the copy is made only when the host changed the source (set_camera, set_views)."""
        changed = getattr(self.batch, "view_matrices", None) is not self._views_seen
        if changed:
            self._further_views()                            # set_views since the last frame
        if self.camera is None or self._views_dirty or changed:
            owned = set()                                    # slots that are the device's from the first frame on
            if self._light_slot_sent and not changed:
                if self.cascades is not None:
                    owned.add(int(self.cascades.host[0]["light_slot"]))
                if self.lights is not None:
                    owned.update(self.lights.spot_view_slots())
            if owned:
                from . import _lib
                words = _lib.VIEWS_SOURCE_BYTES // _lib.VIEW_SLOTS // 4
                first = None                                 # one copy per run of the host's slots
                for v in range(_lib.VIEW_SLOTS + 1):
                    if v < _lib.VIEW_SLOTS and v not in owned:
                        first = v if first is None else first
                    elif first is not None:
                        self.views.source[first * words:v * words].copy_(self.views.host[first * words:v * words], non_blocking=True)
                        first = None
            else:
                self.views.upload()
                self._light_slot_sent = True
            self._views_dirty = False

    def clap_frame(self, now, dt):
        steps = self.world.phys_step_begin(dt) if self.world is not None else 0
        self.move_dt = float(dt)                             # character_move's frame delta (clap_get_fps_delta)
        self._issue(now, steps)

    def _issue(self, now, steps):
        import ctypes as C
        from . import _lib
        f = self._desc or self._build()
        if self.lights is not None:
            self.lights._upload()                            # slot edits made on the host since the last frame
        # graph capture: the clock comes from a device double written before every replay
        f.now_dev = self.characters.now_dev.data_ptr() if (now is None and self.characters is not None) else None
        # CLAPGPU_FRAME_OVERLAP: three chains on three streams (frame.hip); CLAPGPU_FRAME_PREBIN
        f.flags = (1 if self.overlap else 0) | (2 if self.prebin else 0)
        f.move_dt_sec = self.move_dt
        if self.views is not None and now is not None:       # (under capture the copy is the replay's, not a graph node)
            self._upload_views()
        rc = _lib.lib().clapgpu_frame_issue(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(f),
                                            0.0 if now is None else float(now), int(steps))
        _lib.check(rc, "clapgpu_frame_issue")
