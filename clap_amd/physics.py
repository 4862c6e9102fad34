"""Host-side mirror of the reference's physics interface for capsule / sphere bodies without constraint rows.

``PhysWorld.phys_step(dt)`` follows phys_step() / __phys_step() (physics.c:746-787): the
fixed-step schedule runs on the host, each substep does the two broadphase calls and the ODE
world step on the GPU; ``phys_body_update`` is the body -> entity read-back of
physics.c:789-812.  ODE being absent from the reference tree, this block is parity-unpinned
(DESIGN.md).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._dev import device_array, ptr as _ptr, stream as _stream, upload
from .characters import CharacterMoves  # noqa: F401  (physics.CharacterMoves: the name callers know it by)

# a node of the static meshes' BVH as read_static_meshes returns it (trimesh_dev.h: 64 bytes)
NODE = np.dtype([("box", np.float32, (2, 6)), ("child", np.uint32, 2), ("pad", np.uint32, 2)])


class PhysWorld:
    def __init__(self, bodies, statics=None, pair_capacity=None, device="cuda:0", static_pair_capacity=None, geom_records=True,
                 forces=False, bp_levels=1, leveled_index=False):
        """bodies: dict from synth.sphere_bodies() / synth.capsule_bodies(); statics: float64 [ns, 6]
        (minx,maxx,miny,maxy,minz,maxz), host array: binned once by clapgpu_bp_create.  forces: give the bodies a force
        accumulator (clapgpu_bodies.facc, zeros or bodies["facc"]): the step consumes it, bodies_push adds to it.
        bp_levels > 1: a multi-level broadphase grid (clapgpu_bp_create_levels) whose level-0 cell is bodies["cell"], for
        bodies of mixed sizes: same pair lists; queries through it scan every geom unless leveled_index (bp_leveled_index)."""
        self.device = dev = torch.device(device)
        self.n = n = int(bodies["n"])
        t = lambda k, dt: upload(bodies[k], dt, dev)
        self.pos, self.quat = t("pos", np.float64), t("quat", np.float64)
        self.lvel, self.avel = t("lvel", np.float64), t("avel", np.float64)
        self.mass, self.radius, self.yoffset = t("mass", np.float64), t("radius", np.float64), t("yoffset", np.float64)
        self.bflags = t("bflags", np.uint32)
        self.adis_steps_left = t("adis_steps_left", np.int32)
        self.adis_time_left = t("adis_time_left", np.float64)
        self.body_entity = t("body_entity", np.int32)
        self.length = t("length", np.float64) if "length" in bodies else None
        self.inertia = t("inertia", np.float64) if "inertia" in bodies else None
        self.aabb, self.axis = self._out(n, (6,), torch.float64), self._out(n, (3,), torch.float64)
        self.cell = float(bodies["cell"])
        self.world = _lib.World()
        _lib.lib().clapgpu_world_defaults(C.byref(self.world))
        self.time_acc = C.c_double(0.0)
        samples = int(bodies.get("adis_average_samples", 1))
        self.adis_samples = self.adis_counter = None
        if samples > 1:
            self.adis_samples, self.adis_counter = self._out(n, (samples, 6), torch.float64), self._out(n, (), torch.int32)
        d = _lib.Bodies(n, samples, _ptr(self.pos), _ptr(self.quat), _ptr(self.lvel), _ptr(self.avel),
                        _ptr(self.mass), _ptr(self.radius), _ptr(self.yoffset), _ptr(self.bflags),
                        _ptr(self.adis_steps_left), _ptr(self.adis_time_left), _ptr(self.body_entity))
        d.length, d.inertia = _ptr(self.length), _ptr(self.inertia)
        _lib.lib().clapgpu_geom_offset_rotation(d.geom_offset_R)           # physics.c:974-978
        d.aabb, d.axis = _ptr(self.aabb), _ptr(self.axis)
        d.adis_samples, d.adis_counter = _ptr(self.adis_samples), _ptr(self.adis_counter)
        # the narrowphase's one-sector view of every body geom (clapgpu_bodies.geom_records), kept by the step / aabb kernels
        self.geom_records = self._out(n, (8,), torch.float64) if geom_records else None
        d.geom_records = _ptr(self.geom_records)
        self.facc = None
        self._desc = d
        if forces:
            self.enable_forces(bodies.get("facc"))
        self.capacity = int(pair_capacity if pair_capacity is not None else max(8 * n, 1024))
        self.static_capacity = int(static_pair_capacity if static_pair_capacity is not None else self.capacity)
        self.pairs = device_array((self.capacity, 2), torch.int32, dev)
        self.pair_total = device_array(1, torch.int32, dev)
        self.static_pairs = device_array((self.static_capacity, 2), torch.int32, dev)
        self.static_pair_total = device_array(1, torch.int32, dev)
        self.n_static = 0
        st = None
        if statics is not None and len(statics):
            st = np.ascontiguousarray(statics, np.float64)
            self.n_static = st.shape[0]
        self._statics_host = st
        self._bp = C.c_void_p()
        self.bp_levels = int(bp_levels)
        st_ptr = st.ctypes.data if st is not None else None
        if self.bp_levels > 1:
            _lib.check(_lib.lib().clapgpu_bp_create_levels(C.byref(self._bp), n, self.cell, self.bp_levels, self.n_static, st_ptr),
                       "clapgpu_bp_create_levels")
        else:
            _lib.check(_lib.lib().clapgpu_bp_create(C.byref(self._bp), n, self.cell, self.n_static, st_ptr), "clapgpu_bp_create")
        self.statics_ptr = _lib.lib().clapgpu_bp_static_aabb(self._bp)     # device copy owned by the broadphase object
        if leveled_index:
            self.bp_leveled_index(True)
        # what the methods below allocate on demand (the alloc_* methods) or keep from their last call
        self.material = self.static_material = None                        # set_materials / contacts_static, or assigned
        self._static_geoms = self._static_keep = None                      # static_geoms / set_static_geoms
        self._links_key = self._links = None                               # upload_links
        self.contact_buf = self.contact_total = self.static_contact_buf = self.static_contact_total = None
        self.contact2_buf = self.contact2_total = self.static_contact2_buf = self.static_contact2_total = None
        self.island_scratch = self.island = self.island_woken = None
        self.solver = self.solve_scratch = self.row_lambda = self.row_key = self.rows_total = self.solve_status = None
        self.row_level = self.wide_total = None
        self.solve_rows_capacity = self.mesh_contact_capacity = 0
        self.mesh_contact_buf = self.mesh_ref = self.mesh_contact_total = self.mesh_capped = self.mesh_scratch = None
        self._meshes_keep = None                                           # set_static_meshes (beside _meshes)
        self._slide_scratch = self._ground_scratch = self._push_scratch_buf = None
        self._sweep_keep = self._sweep_grid_keep = self._slide_keep = self._push_keep = None
        self._ray_keep = self._ground_keep = None
        # characters_order / characters_move_ordered: the second broadphase object (over reach boxes), its pair room
        self._order_bp, self._order_bp_n, self._order_capacity = None, 0, 0
        self._order_scratch = self._order_keep = None
        self.order_summary = (0, 0, 0, 0)                                  # the last characters_order's summary[4]
        self.bodies_aabb()

    def __del__(self):
        try:
            self._free_meshes()
        except Exception:
            pass
        for name in ("_bp", "_order_bp"):
            bp = getattr(self, name, None)
            setattr(self, name, None)
            if bp:
                try:
                    _lib.lib().clapgpu_bp_destroy(bp)
                except Exception:
                    pass

    def enable_forces(self, facc=None):
        """Give the bodies a force accumulator (clapgpu_bodies.facc; zeros, or facc [n, 3]): from now on the step is the
        force path -- it adds facc to gravity, honours BODY_KINEMATIC and clears what it consumed."""
        self.facc = self._out(self.n, (3,), torch.float64)
        if facc is not None and self.n:
            self.facc[:self.n] = upload(facc, np.float64, self.device, (-1, 3))
        self._desc.facc = _ptr(self.facc)

    def _out(self, n, tail_shape, dtype, fill=0):
        """A device array of n rows of tail_shape, every element `fill`; one row when n is 0, so that its address is
        never null (callers hand out [:n])."""
        return device_array((max(n, 1), *tail_shape), dtype, self.device, fill)

    def _grown(self, name, need):
        """The byte scratch kept in attribute `name`, allocated anew (zeroed, at least 256 bytes) only when it is missing
        or smaller than `need`."""
        have = vars(self)[name]
        if have is None or have.numel() < need:
            have = device_array(max(need, 256), torch.uint8, self.device)
            setattr(self, name, have)
        return have

    # ---- __phys_step pieces -----------------------------------------------------------
    def bp_invalidate(self):
        """Boxes a step pre-binned (world_step(prebin=True) / FrameLoop(prebin=True)) were rewritten by something else."""
        _lib.check(_lib.lib().clapgpu_bp_invalidate(_stream(), self._bp), "clapgpu_bp_invalidate")

    def bodies_aabb(self):
        """Geom axis + AABB of every body from its pose (after the host moved bodies; world_step keeps them current)."""
        self.bp_invalidate()
        _lib.check(_lib.lib().clapgpu_bodies_aabb(_stream(), C.byref(self._desc)), "clapgpu_bodies_aabb")

    def broadphase(self, side=None):
        """dSpaceCollide2(ground, bodies) + dSpaceCollide(bodies) (physics.c:751-753): both candidate pair lists,
        ascending, from one pass of four launches over the bodies' AABBs."""
        L = _lib.lib()
        _lib.check(L.clapgpu_bp_collide(_stream(), self._bp, self.n, _ptr(self.aabb), _ptr(self.pairs), self.capacity,
                                        _ptr(self.pair_total), _ptr(self.static_pairs) if self.n_static else None,
                                        self.static_capacity if self.n_static else 0,
                                        _ptr(self.static_pair_total) if self.n_static else None), "clapgpu_bp_collide")

    def broadphase_status(self):
        st = C.c_uint32(0)
        _lib.check(_lib.lib().clapgpu_bp_status(_stream(), self._bp, C.byref(st)), "clapgpu_bp_status")
        return st.value

    def body_geoms(self):
        return _lib.Geoms(self.n, 0, _ptr(self.pos), _ptr(self.axis), _ptr(self.radius), _ptr(self.length), 0, 0,
                          _ptr(self.material), _ptr(self.geom_records))

    def static_geoms(self):
        """The statics as axis-aligned boxes (their AABBs); static_geom_arrays overrides kind / pos / radius / ..."""
        sg = self._static_geoms
        if sg is None:
            kind = self._out(self.n_static, (), torch.uint8, _lib.GEOM_BOX)
            self._static_keep = dict(kind=kind)
            sg = self._static_geoms = _lib.Geoms(self.n_static, 0, 0, 0, 0, 0, _ptr(kind), self.statics_ptr, 0)
        sg.material = _ptr(self.static_material)
        return sg

    def set_static_geoms(self, kind, pos=None, axis=None, radius=None, length=None):
        """Narrowphase description of the statics (default: every static is its AABB as a box)."""
        dev = self.device
        keep = dict(kind=upload(kind, np.uint8, dev))
        for name, a in (("pos", pos), ("axis", axis), ("radius", radius), ("length", length)):
            keep[name] = None if a is None else upload(a, np.float64, dev)
        self._static_keep = keep
        self._static_geoms = _lib.Geoms(self.n_static, 0, _ptr(keep["pos"]), _ptr(keep["axis"]), _ptr(keep["radius"]),
                                        _ptr(keep["length"]), _ptr(keep["kind"]), self.statics_ptr,
                                        _ptr(self.static_material))

    def alloc_contacts(self):
        if self.contact2_buf is None:
            self.contact2_buf = device_array((self.capacity, 160), torch.uint8, self.device)
            self.contact2_total = device_array(1, torch.int32, self.device)
            self.static_contact2_buf = device_array((self.static_capacity if self.n_static else 1, 160), torch.uint8,
                                                    self.device)
            self.static_contact2_total = device_array(1, torch.int32, self.device)

    def alloc_islands(self):
        """The island pass's scratch and outputs (island [n], island_woken [1])."""
        have = self.island_scratch
        if self._grown("island_scratch", _lib.bodies_islands_scratch_bytes(self.n)) is not have:
            self.island = self._out(self.n, (), torch.int32)
            self.island_woken = device_array(1, torch.int32, self.device)

    def upload_links(self, link_body, link_entity):
        """Device copies of a (body, entity) link table, uploaded once per table."""
        key = (id(link_body), id(link_entity))
        if self._links_key != key:
            self._links_key = key
            self._links = (upload(link_body, np.uint32, self.device), upload(link_entity, np.uint32, self.device))
        return self._links

    def contacts_geoms(self, set_joint_flags=True):
        """near_callback on both candidate lists of the last broadphase(): 160-byte records (clapgpu_contact2)."""
        L = _lib.lib()
        self.alloc_contacts()
        g = self.body_geoms()
        fl = _ptr(self.bflags) if set_joint_flags else 0
        _lib.check(L.clapgpu_contacts_geoms(_stream(), C.byref(g), C.byref(g), _ptr(self.pairs), _ptr(self.pair_total),
                                            self.capacity, _ptr(self.contact2_buf), _ptr(self.contact2_total), fl, fl),
                   "clapgpu_contacts_geoms")
        if self.n_static:
            sg = self.static_geoms()
            _lib.check(L.clapgpu_contacts_geoms(_stream(), C.byref(g), C.byref(sg), _ptr(self.static_pairs),
                                                _ptr(self.static_pair_total), self.static_capacity,
                                                _ptr(self.static_contact2_buf), _ptr(self.static_contact2_total), fl, 0),
                       "clapgpu_contacts_geoms(static)")

    def contacts_geoms_both(self, set_joint_flags=True):
        """contacts_geoms() as ONE launch over both lists (clapgpu_contacts_geoms_both): needs statics."""
        L = _lib.lib()
        self.alloc_contacts()
        g, sg = self.body_geoms(), self.static_geoms()
        fl = _ptr(self.bflags) if set_joint_flags else 0
        _lib.check(L.clapgpu_contacts_geoms_both(_stream(), self._bp, C.byref(g), C.byref(sg), _ptr(self.pairs),
                                                 _ptr(self.pair_total), self.capacity, _ptr(self.contact2_buf),
                                                 _ptr(self.contact2_total), _ptr(self.static_pairs),
                                                 _ptr(self.static_pair_total), self.static_capacity,
                                                 _ptr(self.static_contact2_buf), _ptr(self.static_contact2_total), fl),
                   "clapgpu_contacts_geoms_both")

    def download_contacts2(self, dtype):
        torch.cuda.synchronize(self.device)
        npairs = min(int(self.pair_total.item()), self.capacity)
        out = dict(body=(self.contact2_buf[:npairs].cpu().numpy().view(dtype).reshape(-1), int(self.contact2_total.item())))
        if self.n_static:
            ns = min(int(self.static_pair_total.item()), self.static_capacity)
            out["static"] = (self.static_contact2_buf[:ns].cpu().numpy().view(dtype).reshape(-1),
                             int(self.static_contact2_total.item()))
        return out

    def sweep_capsules(self, sweep_body, delta, cand_first, cand, meshes=True):
        """phys_body_sweep_capsule for a batch (physics.c:559-670): returns (frac, normal[n,3], hit) device tensors.
        meshes: candidate statics that own a mesh collide through its triangles once set_static_meshes ran."""
        dev = self.device
        ns = len(sweep_body)
        sb, dl = upload(sweep_body, np.uint32, dev), upload(delta, np.float32, dev)
        cf, cd = upload(cand_first, np.uint32, dev), upload(cand, np.uint32, dev)
        frac, normal, hit = self._out(ns, (), torch.float32), self._out(ns, (3,), torch.float32), self._out(ns, (), torch.int32)
        g, sg = self.body_geoms(), self.static_geoms()
        _lib.check(_lib.lib().clapgpu_sweep_capsules(_stream(), C.byref(g), C.byref(sg), self._meshes if meshes else None,
                                                     ns, _ptr(sb), _ptr(dl), _ptr(cf), _ptr(cd), _ptr(frac), _ptr(normal),
                                                     _ptr(hit)), "clapgpu_sweep_capsules")
        self._sweep_keep = (sb, dl, cf, cd)
        return frac[:ns], normal[:ns], hit[:ns]

    def sweep_capsules_grid(self, sweep_body, delta, grid=True, meshes=True):
        """phys_body_sweep_capsule for a batch without candidate lists (clapgpu_sweep_capsules_grid): the candidates of a
        sweep are gathered on the device, through the last bp_index() (grid) or from every geom's box.  Returns device
        tensors (frac, normal [n, 3], hit, flags)."""
        dev = self.device
        ns = len(sweep_body)
        sb, dl = upload(sweep_body, np.uint32, dev), upload(delta, np.float32, dev, (-1, 3))
        frac, normal = self._out(ns, (), torch.float32), self._out(ns, (3,), torch.float32)
        hit, flags = self._out(ns, (), torch.int32), self._out(ns, (), torch.int32)
        sg = self.static_geoms()
        _lib.check(_lib.lib().clapgpu_sweep_capsules_grid(_stream(), self._bp if grid else None, C.byref(self._desc), C.byref(sg),
                                                          self._meshes if meshes else None, ns, _ptr(sb), _ptr(dl), _ptr(frac),
                                                          _ptr(normal), _ptr(hit), _ptr(flags)), "clapgpu_sweep_capsules_grid")
        self._sweep_grid_keep = (sb, dl)
        return frac[:ns], normal[:ns], hit[:ns], flags[:ns]

    def slide(self, bodies, velocity, airborne, dt_sec, grid=True, meshes=True):
        """character_apply_velocity's physics branch for the bodies listed (clapgpu_characters_slide): sweeps and slides
        them, zeroes their lvel and rewrites their geoms (a body listed twice is flagged SLIDE_INVALID and stays).
        Returns device tensors (velocity [n, 3] float32, first_frac [n, 2], push_hit [n, 6], flags [n])."""
        dev = self.device
        nb = len(bodies)
        body_d = upload(bodies, np.uint32, dev)
        vel = upload(velocity, np.float32, dev, (-1, 3)) if nb else self._out(0, (3,), torch.float32)
        air_d = upload(np.asarray(airborne) != 0, np.uint8, dev)
        first, push = self._out(nb, (2,), torch.float32, 1), self._out(nb, (6,), torch.int32, -1)
        flags = self._out(nb, (), torch.int32)
        if self._slide_scratch is None:                          # [n] words of the call's own
            self._slide_scratch = self._out(self.n, (), torch.int32)
        sg = self.static_geoms()
        s = _lib.Slide(nb, _ptr(body_d), _ptr(vel), _ptr(air_d), _ptr(first), _ptr(push), _ptr(flags))
        _lib.check(_lib.lib().clapgpu_characters_slide(_stream(), self._bp if grid else None, C.byref(self._desc), C.byref(sg),
                                                       self._meshes if meshes else None, float(dt_sec), C.byref(s),
                                                       _ptr(self._slide_scratch)), "clapgpu_characters_slide")
        self._slide_keep = (body_d, air_d, vel, first, push, flags)
        return vel[:nb], first[:nb], push[:nb], flags[:nb]

    def bodies_push(self, pusher, velocity, push_hit, flags=None, want_pushed=True):
        """phys_body_push for a slide batch (clapgpu_bodies_push): pusher [n] bodies, velocity [n, 3] float32 as the slide
        was GIVEN it, push_hit [n, 6] and flags [n] as the slide left them (host arrays or device tensors).  Adds the
        forces to facc in the reference's order and wakes the pushed bodies.  Returns pushed [self.n] (device), or None."""
        if self.facc is None:
            raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "bodies_push", "no force accumulator: PhysWorld(forces=True)")
        dev = self.device
        n = len(pusher)
        pu, ve, ph = upload(pusher, np.uint32, dev), upload(velocity, np.float32, dev), upload(push_hit, np.int32, dev)
        fl = None if flags is None else upload(flags, np.uint32, dev)
        pushed = self._out(self.n, (), torch.int32) if want_pushed else None
        scratch = self._grown("_push_scratch_buf", _lib.bodies_push_scratch_bytes(n) if n else 0)
        _lib.check(_lib.lib().clapgpu_bodies_push(_stream(), C.byref(self._desc), C.byref(self.world), n, _ptr(pu), _ptr(ve),
                                                  _ptr(ph), _ptr(fl), _ptr(pushed), _ptr(scratch)), "clapgpu_bodies_push")
        self._push_keep = (pu, ve, ph, fl, scratch)
        return None if pushed is None else pushed[:self.n]

    def slide_and_push(self, bodies, velocity, airborne, dt_sec, grid=True, meshes=True):
        """slide(), then the pushes of that batch (bodies_push) with the velocity the slide was given: the whole
        ENTITY3D_HAS_PHYSICS branch of character_apply_velocity.  Returns slide()'s tuple and pushed [self.n]."""
        given = upload(velocity, np.float32, self.device, (-1, 3))
        vel, first, push, flags = self.slide(bodies, velocity, airborne, dt_sec, grid=grid, meshes=meshes)
        body_d = self._slide_keep[0]
        nb = len(bodies)
        pushed = self.bodies_push(body_d[:nb], given[:nb] if nb else given, push, flags)
        return vel, first, push, flags, pushed

    def characters_move(self, moves, dt_sec, grid=True, meshes=True):
        """character_move for the movers of `moves` (a CharacterMoves over this world) as one call without a host round
        trip (clapgpu_characters_move): ground ray, the airborne / jump / walking decision, slide and push, and the
        rotation hand-off when `moves` has one.  dt_sec: the raw frame delta.  Returns moves.outputs(): device tensors."""
        if self.facc is None:
            raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "characters_move", "no force accumulator: PhysWorld(forces=True)")
        sg = self.static_geoms()
        e = C.byref(moves.entity_batch._desc) if moves.entity_batch is not None else None
        _lib.check(_lib.lib().clapgpu_characters_move(_stream(), self._bp if grid else None, C.byref(self._desc),
                                                      C.byref(self.world), C.byref(sg), self._meshes if meshes else None, e,
                                                      float(dt_sec), C.byref(moves._desc), _ptr(moves.scratch) if moves.n else None),
                   "clapgpu_characters_move")
        return moves.outputs()

    ORDER_BP_LEVELS = 16                                                   # CLAPGPU_BP_LEVELS_MAX: top cell = cell * 2^15

    def _order_bp_for(self, n):
        """The broadphase object the reach boxes of n movers are searched with: leveled (reach boxes are of mixed sizes:
        a body's box and what its velocity adds in a frame), no statics, level-0 cell = the bodies' cell.  Made on first
        use, and anew when n outgrows it or after a reach box was too large for it (its status bit is sticky).  At
        workload B (65 536 movers, 3.1 M pairs) it finds the pairs in a third of the time a one-level object of twice the
        bodies' cell takes (profiles/ordered_move/)."""
        if self._order_bp is None or self._order_bp_n < n:
            old, self._order_bp = self._order_bp, None
            if old:
                _lib.lib().clapgpu_bp_destroy(old)
            bp = C.c_void_p()
            _lib.check(_lib.lib().clapgpu_bp_create_levels(C.byref(bp), n, self.cell, self.ORDER_BP_LEVELS, 0, None),
                       "clapgpu_bp_create_levels(order)")
            self._order_bp, self._order_bp_n = bp, n
        return self._order_bp

    def _ordered(self, n, pair_capacity, where, call):
        """call(order_bp, capacity) -> rc, with room for the conflict pairs that doubles while they do not fit (a
        pair_capacity given is taken as it is); raises as _lib.check does."""
        cap = int(pair_capacity) if pair_capacity is not None else max(self._order_capacity, 8 * n, 1024)
        while True:
            bp = self._order_bp_for(n)
            rc = call(bp, cap)
            if rc != _lib.ERR_TOO_LARGE:
                break
            status = C.c_uint32(0)
            _lib.check(_lib.lib().clapgpu_bp_status(_stream(), bp, C.byref(status)), "clapgpu_bp_status")
            if status.value & 1:                                           # sticky: the next call makes another object
                self._order_bp = None
                _lib.lib().clapgpu_bp_destroy(bp)
                break
            if pair_capacity is not None or cap > n * (n - 1) // 2:        # every pair fits: the pairs are not the reason
                break
            cap *= 2
        if pair_capacity is None:
            self._order_capacity = cap
        _lib.check(rc, where)

    def characters_order(self, moves, dt_sec, pair_capacity=None):
        """The conflict levels of the movers of `moves` (clapgpu_characters_order): nothing moves.  Returns (reach [n, 6],
        level [n]: device tensors, n_levels, pair_total).  Synchronises.  pair_capacity: the room for the conflict pairs,
        taken as it is (by default it doubles until they fit)."""
        n = moves.n
        reach, level = self._out(n, (6,), torch.float64), self._out(n, (), torch.int32)
        summary = (C.c_uint32 * 4)()
        if n:
            def call(bp, cap):
                scratch = self._grown("_order_scratch", _lib.characters_order_scratch_bytes(n, cap))
                return _lib.lib().clapgpu_characters_order(_stream(), bp, C.byref(self._desc), C.byref(self.world),
                                                           float(dt_sec), C.byref(moves._desc), cap, _ptr(reach), _ptr(level),
                                                           summary, _ptr(scratch))
            try:
                self._ordered(n, pair_capacity, "clapgpu_characters_order", call)
            finally:                                                       # also of a call that refused: how many pairs
                self.order_summary = tuple(int(v) for v in summary)        # n_levels, pair_total, order_bp status, rounds
        self._order_keep = (reach, level)
        return reach[:n], level[:n], int(summary[0]), int(summary[1])

    def characters_move_ordered(self, moves, dt_sec, grid=True, meshes=True, pair_capacity=None):
        """characters_move for a crowd, in list order (clapgpu_characters_move_ordered): what characters_move gives when
        it is called once per mover in list order, the movers that cannot reach each other moved together.  Returns
        moves.outputs() with "level" [n] (device) and "n_levels".  Synchronises; pair_capacity as characters_order."""
        if self.facc is None:
            raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "characters_move_ordered", "no force accumulator: PhysWorld(forces=True)")
        n = moves.n
        level = self._out(n, (), torch.int32)
        n_levels = C.c_uint32(0)
        sg = self.static_geoms()
        e = C.byref(moves.entity_batch._desc) if moves.entity_batch is not None else None
        if n:
            def call(bp, cap):
                scratch = self._grown("_order_scratch", _lib.characters_move_ordered_scratch_bytes(self.n, n, cap))
                return _lib.lib().clapgpu_characters_move_ordered(
                    _stream(), self._bp if grid else None, bp, C.byref(self._desc), C.byref(self.world), C.byref(sg),
                    self._meshes if meshes else None, e, float(dt_sec), C.byref(moves._desc), cap, _ptr(level),
                    C.byref(n_levels), _ptr(scratch))
            self._ordered(n, pair_capacity, "clapgpu_characters_move_ordered", call)
        self._order_keep = (level,)
        out = moves.outputs()
        out["level"], out["n_levels"] = level[:n], int(n_levels.value)
        return out

    def islands(self, h, want_island=True, want_woken=True):
        """The island pass of dWorldQuickStep (clapgpu_bodies_islands) over the body-body pairs of the last broadphase()
        and the records of the last contacts_geoms(): the step's auto-disable bookkeeping, then every sleeping body in
        touch -- directly or through others -- with an awake one is enabled.  Run it between the contacts and
        world_step(h).  Returns device tensors (island [n]: the smallest body index of each body's component, woken [1]:
        the number of bodies enabled), None for what was not asked for."""
        self.alloc_contacts()
        self.alloc_islands()
        island = self.island if want_island else None
        woken = self.island_woken if want_woken else None
        _lib.check(_lib.lib().clapgpu_bodies_islands(_stream(), C.byref(self._desc), C.byref(self.world), h, _ptr(self.pairs),
                                                     _ptr(self.pair_total), self.capacity, _ptr(self.contact2_buf),
                                                     _ptr(self.island_scratch), _ptr(island), _ptr(woken)),
                   "clapgpu_bodies_islands")
        return (None if island is None else island[:self.n]), woken

    def alloc_solve(self, rows_capacity=None):
        """The solve's scratch, outputs and parameters (clapgpu_solver_defaults in self.solver).  rows_capacity: the most
        contact rows a substep may have (240 bytes of scratch each); by default 6 n + 1024."""
        cap = int(rows_capacity if rows_capacity is not None else self.solve_rows_capacity or 6 * self.n + 1024)
        if self.solve_scratch is None or self.solve_rows_capacity != cap:
            self.solve_rows_capacity = cap
            self.solve_scratch = None                  # another capacity: all of it anew, zeroed
            self._grown("solve_scratch", _lib.bodies_solve_scratch_bytes(self.n, cap))
            self.row_lambda, self.row_key = self._out(cap, (), torch.float64), self._out(cap, (), torch.int64)
            self.rows_total = device_array(1, torch.int32, self.device)
            self.solve_status = device_array(1, torch.int32, self.device)
            self.row_level = self._out(cap, (), torch.int32)
            self.wide_total = device_array(1, torch.int32, self.device)
        if self.solver is None:
            self.solver = _lib.Solver()
            _lib.lib().clapgpu_solver_defaults(C.byref(self.solver))

    def solve(self, h, want_lambda=False, rows_capacity=None, want_levels=False):
        """Contact response (clapgpu_bodies_solve): the rows of the last contacts_geoms[_both]() / contacts_meshes() lists,
        solved island by island with the islands of the last islands(); changes lvel / avel of the enabled bodies in
        contact.  Run it between islands() and world_step(h).  Returns device tensors (rows_total [1], status [1]; bit 0:
        the rows did not fit and nothing was applied; the caller clears it) and, with want_lambda, (row_lambda
        [rows_capacity], row_key [rows_capacity]) in canonical row order; with want_levels, behind those, (row_level
        [rows_capacity]: a row's level when a workgroup solved its island -- one of at least self.solver.wide_rows rows --
        and 0 when one lane did, wide_total [1]: the islands a workgroup solved)."""
        if self.island is None or self.contact2_buf is None:
            raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "solve", "no islands: call contacts_geoms and islands first")
        self.alloc_solve(rows_capacity)
        st = bool(self.n_static)
        mesh = st and self._meshes is not None and self.mesh_contact_buf is not None
        _lib.check(_lib.lib().clapgpu_bodies_solve(
            _stream(), C.byref(self._desc), C.byref(self.world), C.byref(self.solver), h, _ptr(self.island),
            _ptr(self.static_pairs) if st else None, _ptr(self.static_pair_total) if st else None,
            self.static_capacity if st else 0, _ptr(self.static_contact2_buf) if st else None,
            _ptr(self.mesh_contact_buf) if mesh else None, _ptr(self.mesh_ref) if mesh else None,
            _ptr(self.mesh_contact_total) if mesh else None, self.mesh_contact_capacity if mesh else 0,
            _ptr(self.pairs), _ptr(self.pair_total), self.capacity, _ptr(self.contact2_buf),
            self.solve_rows_capacity, _ptr(self.solve_scratch),
            _ptr(self.row_lambda) if want_lambda else None, _ptr(self.row_key) if want_lambda else None,
            _ptr(self.rows_total), _ptr(self.solve_status),
            _ptr(self.row_level) if want_levels else None, _ptr(self.wide_total) if want_levels else None),
            "clapgpu_bodies_solve")
        out = (self.rows_total, self.solve_status)
        if want_lambda:
            out += (self.row_lambda, self.row_key)
        if want_levels:
            out += (self.row_level, self.wide_total)
        return out

    def alloc_mesh_contacts(self, capacity=None):
        """The mesh contact list (clapgpu_contact2 records, mesh_ref [k][2]), its totals and scratch."""
        cap = int(capacity if capacity is not None else self.mesh_contact_capacity or
                  max(min(self.static_capacity, 16 * self.n), 1024))
        if self.mesh_contact_buf is None or self.mesh_contact_capacity != cap:
            dev = self.device
            self.mesh_contact_capacity = cap
            self.mesh_contact_buf, self.mesh_ref = self._out(cap, (160,), torch.uint8), self._out(cap, (2,), torch.int32)
            self.mesh_contact_total = device_array(1, torch.int32, dev)
            self.mesh_capped = device_array(1, torch.int32, dev)
            self.mesh_scratch = device_array(_lib.mesh_contact_scratch(self.static_capacity), torch.int32, dev)

    def contacts_meshes(self, set_joint_flags=True, capacity=None):
        """near_callback for the (body, static) pairs of the last broadphase() whose static owns a mesh of
        set_static_meshes (clapgpu_contacts_meshes): one record per touching (pair, triangle)."""
        if self._meshes is None:
            raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "contacts_meshes", "no mesh set: call set_static_meshes")
        self.alloc_mesh_contacts(capacity)
        g, sg = self.body_geoms(), self.static_geoms()
        _lib.check(_lib.lib().clapgpu_contacts_meshes(_stream(), C.byref(g), C.byref(sg), self._meshes, _ptr(self.static_pairs),
                                                      _ptr(self.static_pair_total), self.static_capacity,
                                                      _ptr(self.mesh_scratch), self.mesh_contact_capacity,
                                                      _ptr(self.mesh_contact_buf), _ptr(self.mesh_ref),
                                                      _ptr(self.mesh_contact_total), _ptr(self.mesh_capped),
                                                      _ptr(self.bflags) if set_joint_flags else None),
                   "clapgpu_contacts_meshes")

    def download_mesh_contacts(self, dtype):
        """(records [k] of dtype, mesh_ref [k, 2] (static pair index, triangle of the mesh), total, capped pairs); k is
        the written prefix: min(total, capacity)."""
        torch.cuda.synchronize(self.device)
        total = int(self.mesh_contact_total.item())
        k = min(total, self.mesh_contact_capacity)
        return (self.mesh_contact_buf[:k].cpu().numpy().view(dtype).reshape(-1),
                self.mesh_ref[:k].cpu().numpy().view(np.uint32), total, int(self.mesh_capped.item()))

    # ---- ray casts (physics.c:474-540, 695-744) ------------------------------------------
    def bp_index(self):
        """The broadphase grid of the bodies' CURRENT boxes (clapgpu_bp_index): what ray_cast(grid=True) looks up."""
        _lib.check(_lib.lib().clapgpu_bp_index(_stream(), self._bp, self.n, _ptr(self.aabb)), "clapgpu_bp_index")

    def bp_leveled_index(self, on):
        """Switch the index of a leveled broadphase object on or off (clapgpu_bp_leveled_index; off as created).  On:
        bp_index() builds an index over all levels and the queries read it; off: bp_index() launches nothing and they scan
        every geom.  Either way the index held is dropped: bp_index() again.  A one-level world: accepted, no effect."""
        _lib.check(_lib.lib().clapgpu_bp_leveled_index(self._bp, 1 if on else 0), "clapgpu_bp_leveled_index")

    def update_statics(self, aabb):
        """The statics moved (dGeomSetPosition on a geom without a body): their new boxes, float64 [n_static, 6] as at
        construction, a host array or a device tensor, registered again on the device (clapgpu_bp_statics_update).
        statics_ptr and every static geom description built on it keep their address and hold the new boxes.  Synchronises
        the stream; drops the index and a recorded prebin; a graph captured from frames of this world must be captured
        again.  Meshes are left to pose_static_meshes.  The order for a moving static that owns a mesh: update_statics
        (the box must hold the posed mesh), then pose_static_meshes (or, on a set in parts, pose_static_meshes_some with
        the moved meshes alone), then bp_index."""
        a = upload(aabb, np.float64, self.device, (-1, 6))
        if a.dtype != torch.float64 or a.dim() != 2 or tuple(a.shape) != (self.n_static, 6):
            raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "update_statics", f"float64 [{self.n_static}, 6] expected")
        _lib.check(_lib.lib().clapgpu_bp_statics_update(_stream(), self._bp, self.n_static, _ptr(a) if self.n_static else None),
                   "clapgpu_bp_statics_update")
        if self.n_static:
            self._statics_host = a.cpu().numpy()

    def bp_index_status(self):
        st = C.c_uint32(0)
        _lib.check(_lib.lib().clapgpu_bp_index_status(_stream(), self._bp, C.byref(st)), "clapgpu_bp_index_status")
        return st.value

    _meshes = None
    _meshes_shape = (0, 0)                                             # (meshes, triangles) of the set

    def set_static_meshes(self, static_index, vertices, indices, scale, pos, quat, parts=False):
        """The triangle meshes of trimesh statics (phys_geom_trimesh_new, physics.c:882-930): mesh m belongs to static
        static_index[m]; vertices[m] float [V, 3] in model space, indices[m] u16 [T, 3], scale[m] (entity->scale),
        pos[m] (entity position), quat[m] (entity rotation x, y, z, w).  From then on ray_cast and ground_collide
        intersect those statics through their triangles (clapgpu_trimesh_create).  parts: the set in parts
        (clapgpu_trimesh_create_parts), which answers the same bit for bit and takes pose_static_meshes_some; it pays where
        few of many meshes move per frame (profiles/trimesh_parts/README.md)."""
        dev = self.device
        m = len(static_index)
        vx = [np.asarray(v, np.float32).reshape(-1, 3) for v in vertices]
        ix = [np.asarray(i, np.uint16).reshape(-1, 3) for i in indices]
        vx_first = np.concatenate([[0], np.cumsum([len(v) for v in vx])]).astype(np.uint32)
        tri_first = np.concatenate([[0], np.cumsum([len(i) for i in ix])]).astype(np.uint32)
        keep = dict(static_index=upload(static_index, np.uint32, dev),
                    vx_first=upload(vx_first, np.uint32, dev), tri_first=upload(tri_first, np.uint32, dev),
                    vx=upload(np.concatenate(vx) if vx_first[-1] else np.zeros((1, 3)), np.float32, dev),
                    idx=upload(np.concatenate(ix) if tri_first[-1] else np.zeros((1, 3)), np.uint16, dev),
                    scale=upload(scale, np.float32, dev, (-1,)), pos=upload(pos, np.float64, dev, (-1, 3)),
                    quat=upload(quat, np.float32, dev, (-1, 4)))
        d = _lib.TrimeshDesc(m, self.n_static, *[(_ptr(keep[k]) if m else None) for k in
                                                  ("static_index", "vx_first", "tri_first", "vx", "idx", "scale", "pos", "quat")])
        out = C.c_void_p()
        name = "clapgpu_trimesh_create_parts" if parts else "clapgpu_trimesh_create"
        _lib.check(getattr(_lib.lib(), name)(_stream(), C.byref(out), C.byref(d)), name)
        self._free_meshes()
        self._meshes, self._meshes_keep = out, keep
        self._meshes_shape = (m, int(tri_first[-1]))

    def pose_static_meshes(self, pos, quat):
        """New poses of every mesh (entity position, rotation x, y, z, w): re-bake and rebuild (clapgpu_trimesh_pose)."""
        dev = self.device
        p, q = upload(pos, np.float64, dev, (-1, 3)), upload(quat, np.float32, dev, (-1, 4))
        _lib.check(_lib.lib().clapgpu_trimesh_pose(_stream(), self._meshes, _ptr(p), _ptr(q)), "clapgpu_trimesh_pose")
        torch.cuda.current_stream().synchronize()

    def pose_static_meshes_some(self, mesh, pos, quat):
        """New poses of the listed meshes of a set in parts (mesh [k] indices, pos [k, 3], quat [k, 4]; host arrays or
        device tensors): those meshes are baked and refit, the others untouched (clapgpu_trimesh_pose_meshes).  Does not
        synchronise."""
        dev = self.device
        i, p, q = upload(mesh, np.uint32, dev, (-1,)), upload(pos, np.float64, dev, (-1, 3)), upload(quat, np.float32, dev, (-1, 4))
        k = int(i.shape[0])
        if p.shape[0] != k or q.shape[0] != k:
            raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "pose_static_meshes_some", f"{k} meshes, {p.shape[0]} positions, "
                                    f"{q.shape[0]} rotations")
        _lib.check(_lib.lib().clapgpu_trimesh_pose_meshes(_stream(), self._meshes, k, _ptr(i) if k else None, _ptr(p) if k else None,
                                                          _ptr(q) if k else None), "clapgpu_trimesh_pose_meshes")

    def static_meshes_parts_status(self):
        """(in parts, top height, deepest part's height, sticky flags) of the mesh set (clapgpu_trimesh_parts_status)."""
        out = (C.c_uint32 * 4)()
        _lib.check(_lib.lib().clapgpu_trimesh_parts_status(_stream(), self._meshes, out), "clapgpu_trimesh_parts_status")
        return bool(out[0]), out[1], out[2], out[3]

    def read_static_meshes(self):
        """The set's image on the host (clapgpu_trimesh_read): dict of nodes (structured: box [2, 6] float32, child [2],
        pad [2] uint32), key [T, 2], tri [T, 9] in leaf order, and part_root [n_meshes] for a set in parts, else None."""
        n_meshes, T = self._meshes_shape
        nodes = np.zeros(max(T - 1, 1), NODE)
        key, tri = np.zeros((T, 2), np.uint32), np.zeros((T, 9), np.float64)
        root = np.zeros(n_meshes, np.uint32) if self.static_meshes_parts_status()[0] else None
        hp = lambda a: a.ctypes.data if a is not None and a.size else None
        _lib.check(_lib.lib().clapgpu_trimesh_read(_stream(), self._meshes, hp(nodes), hp(key), hp(tri), hp(root)),
                   "clapgpu_trimesh_read")
        return dict(nodes=nodes, key=key, tri=tri, part_root=root)

    def static_meshes_status(self):
        """(tree height, triangles) of the mesh set."""
        depth, ntri = C.c_uint32(0), C.c_uint32(0)
        _lib.check(_lib.lib().clapgpu_trimesh_status(_stream(), self._meshes, C.byref(depth), C.byref(ntri)),
                   "clapgpu_trimesh_status")
        return depth.value, ntri.value

    def _free_meshes(self):
        m, self._meshes = self._meshes, None
        if m:
            _lib.lib().clapgpu_trimesh_destroy(m)

    def ray_cast(self, start, dir, length, skip=None, grid=True, meshes=True):
        """__phys_ray_cast for a batch: start / dir [n, 3], length [n]; skip [n] (body i, -2 - s, -1).  grid: through the
        last bp_index().  meshes: through the static meshes once set_static_meshes ran.  Returns device tensors (dist [n]
        (NaN on a miss), hit [n], contact [n, 6], flags [n])."""
        dev = self.device
        start, dir = np.asarray(start, np.float64).reshape(-1, 3), np.asarray(dir, np.float64).reshape(-1, 3)
        nr = start.shape[0]
        ray = np.zeros((max(nr, 1), 8))
        ray[:nr, 0:3], ray[:nr, 3:6], ray[:nr, 6] = start, dir, np.broadcast_to(np.asarray(length, np.float64), (nr,))
        ray_d = upload(ray, np.float64, dev)
        skip_d = None if skip is None else upload(skip, np.int32, dev)
        nan = float("nan")
        dist, contact = self._out(nr, (), torch.float64, nan), self._out(nr, (6,), torch.float64, nan)
        hit, flags = self._out(nr, (), torch.int32), self._out(nr, (), torch.int32)
        g, sg = self.body_geoms(), self.static_geoms()
        _lib.check(_lib.lib().clapgpu_ray_cast(_stream(), self._bp if grid else None, C.byref(g), C.byref(sg),
                                               self._meshes if meshes else None, nr, _ptr(ray_d), _ptr(skip_d),
                                               _ptr(dist), _ptr(hit), _ptr(contact), _ptr(flags)),
                   "clapgpu_ray_cast")
        self._ray_keep = (ray_d, skip_d)
        return dist[:nr], hit[:nr], contact[:nr], flags[:nr]

    def ground_collide(self, bodies, ray_off, grounded, grid=True, meshes=True):
        """phys_body_ground_collide for the bodies listed: moves them onto the ground (a body listed twice is flagged
        CLAPGPU_RAY_INVALID and stays).  Returns device tensors (grounded_out [n] uint8, normal [n, 3] float32, dist [n],
        hit [n], flags [n])."""
        dev = self.device
        nb = len(bodies)
        body_d, off_d = upload(bodies, np.uint32, dev), upload(ray_off, np.float64, dev)
        gr_d = upload(np.asarray(grounded) != 0, np.uint8, dev)
        out, normal = self._out(nb, (), torch.uint8), self._out(nb, (3,), torch.float32)
        dist = self._out(nb, (), torch.float64, float("nan"))
        hit, flags = self._out(nb, (), torch.int32), self._out(nb, (), torch.int32)
        if self._ground_scratch is None:                         # [n] words of the call's own
            self._ground_scratch = self._out(self.n, (), torch.int32)
        sg = self.static_geoms()
        _lib.check(_lib.lib().clapgpu_bodies_ground_collide(_stream(), self._bp if grid else None, C.byref(self._desc),
                                                            C.byref(sg), self._meshes if meshes else None, nb,
                                                            _ptr(body_d), _ptr(off_d), _ptr(gr_d), _ptr(out),
                                                            _ptr(normal), _ptr(dist), _ptr(hit), _ptr(flags),
                                                            _ptr(self._ground_scratch)),
                   "clapgpu_bodies_ground_collide")
        self._ground_keep = (body_d, off_d, gr_d)
        return out[:nb], normal[:nb], dist[:nb], hit[:nb], flags[:nb]

    def rotate_from_entities(self, entity_batch, link_body, link_entity, all_dirty=False):
        """phys_body_rotate_xform for the (body, entity) links whose entity default_update is about to
        rebuild (model.c:1680-1687); run before entity_batch.mq_update."""
        lb, le = self.upload_links(link_body, link_entity)     # once per link table (also keeps graph capture clean)
        rc = _lib.lib().clapgpu_bodies_rotate_from_entities(_stream(), C.byref(self._desc), C.byref(entity_batch._desc),
                                                            _lib.UPDATE_ALL_DIRTY if all_dirty else 0, len(link_body),
                                                            _ptr(lb), _ptr(le))
        _lib.check(rc, "clapgpu_bodies_rotate_from_entities")

    def set_materials(self, material):
        """Per-body phys_body parameters (bounce, bounce_vel, mu, soft_erp, soft_cfm; physics.c:77-81)."""
        self.material = upload(material, np.float64, self.device)

    def contacts(self):
        """near_callback on the body x body candidate pairs of the last broadphase(): one contact record
        per pair (oracle.binding.CONTACT_DTYPE layout = clapgpu_contact) + the number of touching pairs."""
        if self.contact_buf is None:
            self.contact_buf = device_array((self.capacity, 104), torch.uint8, self.device)
            self.contact_total = device_array(1, torch.int32, self.device)
        _lib.check(_lib.lib().clapgpu_contacts_spheres(_stream(), C.byref(self._desc), _ptr(self.pairs),
                                                       _ptr(self.pair_total), self.capacity, _ptr(self.material),
                                                       _ptr(self.contact_buf), _ptr(self.contact_total)),
                   "clapgpu_contacts_spheres")

    def contacts_static(self, static_material=None):
        """near_callback on the (body, static box) candidate pairs of the last broadphase(): ODE's
        dCollideSphereBox + phys_contact_surface, one record per pair."""
        if self.static_contact_buf is None:
            self.static_contact_buf = device_array((self.static_capacity, 104), torch.uint8, self.device)
            self.static_contact_total = device_array(1, torch.int32, self.device)
        if static_material is not None:
            self.static_material = upload(static_material, np.float64, self.device)
        _lib.check(_lib.lib().clapgpu_contacts_sphere_box(_stream(), C.byref(self._desc), self.n_static,
                                                          self.statics_ptr, _ptr(self.static_pairs),
                                                          _ptr(self.static_pair_total), self.static_capacity,
                                                          _ptr(self.material), _ptr(self.static_material),
                                                          _ptr(self.static_contact_buf),
                                                          _ptr(self.static_contact_total)),
                   "clapgpu_contacts_sphere_box")

    def download_static_contacts(self, dtype):
        torch.cuda.synchronize(self.device)
        npairs = min(int(self.static_pair_total.item()), self.static_capacity)
        return (self.static_contact_buf[:npairs].cpu().numpy().view(dtype).reshape(-1),
                int(self.static_contact_total.item()))

    def download_contacts(self, dtype):
        torch.cuda.synchronize(self.device)
        npairs = min(int(self.pair_total.item()), self.capacity)
        return self.contact_buf[:npairs].cpu().numpy().view(dtype).reshape(-1), int(self.contact_total.item())

    def world_step(self, h, prebin=False):
        """quickstep's body stage; prebin: also the bin pass of the next broadphase() over the boxes it writes."""
        if prebin:
            _lib.check(_lib.lib().clapgpu_bodies_step_prebin(_stream(), C.byref(self._desc), C.byref(self.world), h, self._bp),
                       "clapgpu_bodies_step_prebin")
            return
        _lib.check(_lib.lib().clapgpu_bodies_step(_stream(), C.byref(self._desc), C.byref(self.world), h),
                   "clapgpu_bodies_step")

    def phys_step_begin(self, dt):
        """The schedule half of phys_step (physics.c:773-787): number of fixed substeps for this frame."""
        return _lib.lib().clapgpu_phys_step_schedule(C.byref(self.time_acc), dt)

    def phys_step(self, dt, broadphase=True, islands=False, solve=False):
        """phys_step(phys, dt): returns the number of fixed substeps taken.  islands: every substep also collides its
        pairs (contacts_geoms, mesh contacts when there are meshes) and wakes sleeping bodies by contact (islands()).
        solve: ... and its contacts act on the bodies (solve(), between the island pass and the step); implies islands."""
        steps = _lib.lib().clapgpu_phys_step_schedule(C.byref(self.time_acc), dt)
        islands = islands or solve
        if islands and not broadphase:
            raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "phys_step", "islands needs the broadphase's pairs")
        for _ in range(steps):
            if broadphase:
                self.broadphase()
            if islands:
                if self.n_static:
                    self.contacts_geoms_both()
                    if self._meshes is not None:
                        self.contacts_meshes()
                else:
                    self.contacts_geoms()
                self.islands(1.0 / 120.0)
                if solve:
                    self.solve(1.0 / 120.0)
            self.world_step(1.0 / 120.0)
        return steps

    def phys_body_update(self, entity_batch, moving=None):
        """phys_body_update for every body: entity TRS <- body pose, entities marked dirty."""
        _lib.check(_lib.lib().clapgpu_phys_body_update(_stream(), C.byref(self._desc), entity_batch.n,
                                                       _ptr(entity_batch.pos_scale),
                                                       _ptr(entity_batch.rot), _ptr(entity_batch.flags),
                                                       _ptr(moving)),
                   "clapgpu_phys_body_update")

    def download(self):
        torch.cuda.synchronize(self.device)
        npairs = int(self.pair_total.item())
        nst = int(self.static_pair_total.item())
        return dict(pos=self.pos.cpu().numpy(), quat=self.quat.cpu().numpy(), lvel=self.lvel.cpu().numpy(),
                    avel=self.avel.cpu().numpy(), aabb=self.aabb.cpu().numpy()[:self.n], axis=self.axis.cpu().numpy()[:self.n],
                    bflags=self.bflags.cpu().numpy().view(np.uint32),
                    adis_steps_left=self.adis_steps_left.cpu().numpy(), adis_time_left=self.adis_time_left.cpu().numpy(),
                    pair_total=npairs, pairs=self.pairs[:min(npairs, self.capacity)].cpu().numpy().view(np.uint32),
                    static_pair_total=nst,
                    static_pairs=self.static_pairs[:min(nst, self.static_capacity)].cpu().numpy().view(np.uint32))

    def integrate_algorithmic_bytes(self):
        return 232 * self.n

