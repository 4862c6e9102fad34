"""Host-side mirror of the reference's skeletal animation + skinning interface.

``SkinnedModel`` holds what ``model3d_add_skinning`` (model.c:524-538), ``animation_new`` /
``animation_add_channel`` (model.c:688-741) and ``model3d_make``'s vertex attributes set up
once; ``CharacterBatch.animated_update`` is the batched ``animated_update`` (model.c:1563-1592:
host time base -> channels_transform + one_joint_transform on the GPU) and
``CharacterBatch.skin`` the compute form of the skinning loop of shaders/model.vert:32-48.
``AnimationQueues`` holds what ``character_set_state`` and ``animation_next`` keep per character -- the state, the
queue of ``struct queued_animation``, ``e->animation``, ``ani_cleared``, ``ani_time`` -- for
``clapgpu_characters_state`` and ``clapgpu_animation_queue_time`` (the queue clock in place of the plain one).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._dev import device_array, ptr as _ptr, stream as _stream, upload


def joint_depths(parent):
    """Level of every joint under joint 0; -1 for joints the reference's recursion from joint 0
    (model.c:1583, 1402-1403) never reaches."""
    parent = np.asarray(parent, np.int64)
    J = parent.shape[0]
    depth = np.full(J, -1, np.int32)
    if J:
        depth[0] = 0
    changed = True
    while changed:
        changed = False
        for j in range(1, J):
            p = parent[j]
            if depth[j] < 0 and p >= 0 and depth[p] >= 0:
                depth[j] = depth[p] + 1
                changed = True
    return depth


def channel_table(anims, nr_joints):
    """chan_table[a][joint][path] = (time_off, data_off, nr, 0) into the pooled key times / values
    of all animations; the last listed channel of a (joint, path) wins (model.c:1348-1349)."""
    table = np.zeros((len(anims), nr_joints, 3, 4), np.uint32)
    times, data = [], []
    t_base = d_base = 0
    for ai, an in enumerate(anims):
        for c in range(int(an["n_channels"])):
            tgt, path, nr = int(an["ch_target"][c]), int(an["ch_path"][c]), int(an["ch_nr"][c])
            if tgt < nr_joints and path < 3 and nr > 0:
                table[ai, tgt, path] = (t_base + int(an["ch_time_off"][c]), d_base + int(an["ch_data_off"][c]), nr, 0)
        times.append(an["times"])
        data.append(an["data"])
        t_base += an["times"].shape[0]
        d_base += an["data"].shape[0]
    return dict(chan_table=table, times=np.concatenate(times).astype(np.float32),
                data=np.concatenate(data).astype(np.float32))


def skeleton_bind(invmx):
    """model3d_add_skinning's bind = mat4x4_invert(invmx) per joint (model.c:524-537), with the library's arithmetic."""
    inv = np.ascontiguousarray(invmx, np.float32).reshape(-1, 16)
    out = np.zeros_like(inv)
    L, fp = _lib.lib(), C.POINTER(C.c_float)
    for j in range(inv.shape[0]):
        L.clapgpu_mat4_invert(inv[j].ctypes.data_as(fp), out[j].ctypes.data_as(fp))
    return out


def skin_lod_lists(index_buffers, n_verts, capacity=None, total=0):
    """clapgpu_skin_lod_lists (include/clapgpu_scene.h; host only): the ascending distinct vertices each LOD's DT_USHORT
    index buffer references -> (rc, lod_first [n_lods], lod_count [n_lods], list [capacity], total).  A LOD that references
    every vertex gets SKIN_LOD_ALL and no entries.  capacity None: sized to fit.  total: entries already in a list these
    are appended to (lod_first counts from there; `list` holds the new ones from index `total` on)."""
    from . import snapshot
    L = snapshot.lib()
    bufs = [np.ascontiguousarray(b, np.uint16).reshape(-1) for b in index_buffers]
    nl = len(bufs)
    ptrs = (C.c_void_p * max(nl, 1))(*[b.ctypes.data if b.size else None for b in bufs])
    counts = np.asarray([b.size for b in bufs] or [0], np.uint32)
    first, count = np.zeros(max(nl, 1), np.uint32), np.zeros(max(nl, 1), np.uint32)
    if capacity is None:
        capacity = int(total) + sum(min(b.size, int(n_verts)) for b in bufs)
    lst = np.zeros(max(int(capacity), 1), np.uint32)
    tot = C.c_uint32(int(total))
    rc = L.clapgpu_skin_lod_lists(ptrs, counts.ctypes.data, nl, int(n_verts), lst.ctypes.data, int(capacity), C.byref(tot),
                                  first.ctypes.data, count.ctypes.data)
    return rc, first[:nl], count[:nl], lst[:int(capacity)], int(tot.value)


class SkinnedModel:
    """Device copy of one model3d's skeleton, animations and (optionally) skinned mesh."""

    def __init__(self, sk, anims, mesh=None, bind=None, device="cuda:0"):
        self.device = dev = torch.device(device)
        self.nr_joints = J = int(sk["nr_joints"])
        self.depth_host = joint_depths(sk["parent"])
        self.n_levels = int(self.depth_host.max()) + 1
        self.parent = upload(sk["parent"], np.int32, dev)
        self.depth = upload(self.depth_host, np.int32, dev)
        self.root_pose = upload(sk["root_pose"], np.float32, dev)
        self.invmx = upload(sk["invmx"], np.float32, dev)
        if bind is None:
            bind = skeleton_bind(sk["invmx"])
        self.bind = upload(bind, np.float32, dev)
        self.anims_host = anims
        ct = channel_table(anims, J)
        self.time_end = [float(a["time_end"]) for a in anims]
        self._ct = {k: upload(v, v.dtype, dev) for k, v in ct.items()}
        self.skel_desc = _lib.Skeleton(J, self.n_levels, _ptr(self.parent), _ptr(self.depth),
                                       _ptr(self.root_pose), _ptr(self.invmx), _ptr(self.bind))
        self.anim_desc = _lib.Animations(len(anims), int(ct["times"].shape[0]), _ptr(self._ct["chan_table"]),
                                         _ptr(self._ct["times"]),
                                         _ptr(self._ct["data"]), None, 0, 0, int(ct["data"].shape[0]), 0)
        # the key-major copy of the pools with the rotation intervals' constants (clapgpu_animations_pack): once per
        # model, required by clapgpu_pose_update
        self.packed = None
        max_keys = int(ct["chan_table"][..., 2].max()) if len(anims) else 0
        max_keys = max(max_keys, 1)                       # animations without a single key: every path keeps its value
        if J <= 256 and len(anims):
            nbytes = int(_lib.lib().clapgpu_animations_packed_bytes(len(anims), max_keys, J))
            self.packed = device_array((nbytes + 15) // 16 * 4, torch.float32, dev)
            layout = C.c_uint32(0)
            _lib.check(_lib.lib().clapgpu_animations_pack(_stream(), C.byref(self.anim_desc), J, max_keys, _ptr(self.packed),
                                                          C.byref(layout)), "clapgpu_animations_pack")
            self.anim_desc.packed = _ptr(self.packed)
            self.anim_desc.packed_keys = max_keys
            self.anim_desc.packed_layout = layout.value
        self.mesh = None
        if mesh is not None:
            self.mesh = dict(n_verts=int(mesh["n_verts"]), position=upload(mesh["position"], np.float32, dev),
                             normal=upload(mesh["normal"], np.float32, dev), joints=upload(mesh["joints"], np.uint8, dev),
                             weights=upload(mesh["weights"], np.float32, dev))


class CharacterBatch:
    """The animated entities of one SkinnedModel."""

    def __init__(self, model, n_chars, trs0, entity_mx, entity_index=None, vert_first=None, vert_count=None):
        self.model = model
        self.device = dev = model.device
        self.n = n = int(n_chars)
        J = model.nr_joints
        trs0 = np.asarray(trs0, np.float32)
        if trs0.ndim == 2:
            trs0 = np.broadcast_to(trs0, (n, J, 10))
        self.trs = upload(trs0, np.float32, dev)
        self.entity_mx = entity_mx if torch.is_tensor(entity_mx) else upload(entity_mx, np.float32, dev)
        self.entity_index = None if entity_index is None else upload(entity_index, np.uint32, dev)
        self.anim = device_array(n, torch.int32, dev)
        self.frame_time = device_array(n, torch.float32, dev)
        self.joint_transforms = device_array((n, J, 16), torch.float32, dev)
        self.joint_pos = device_array((n, J, 4), torch.float32, dev)
        # host animation state of animated_update(): start time, speed, current animation
        self.ani_time = np.zeros(n, np.float64)
        self.speed = np.ones(n, np.float64)
        self.anim_host = np.zeros(n, np.int32)
        self._clock = None                                   # start_clock()
        self._pose_desc = _lib.PoseBatch(n, 0, _ptr(self.anim), _ptr(self.frame_time), _ptr(self.entity_index),
                                         _ptr(self.entity_mx), _ptr(self.trs), _ptr(self.joint_transforms),
                                         _ptr(self.joint_pos))
        self._skin_desc = None
        if model.mesh is not None:
            if vert_first is None:                       # every character instances the whole mesh
                vert_first = np.zeros(n, np.uint32)
                vert_count = np.full(n, model.mesh["n_verts"], np.uint32)
            self.vert_first = upload(vert_first, np.uint32, dev)
            self.vert_count_host = np.asarray(vert_count, np.uint32)
            self.vert_count = upload(self.vert_count_host, np.uint32, dev)
            of = np.concatenate([[0], np.cumsum(self.vert_count_host.astype(np.int64))])
            self.out_first_host = of
            self.out_first = upload(of[:-1], np.uint32, dev)
            total = int(of[-1])
            self.n_out_verts = total
            self.out_position = device_array((total, 3), torch.float32, dev)
            self.out_normal = device_array((total, 3), torch.float32, dev)
            m = model.mesh
            self._skin_desc = _lib.SkinBatch(n, J, _ptr(self.vert_first), _ptr(self.vert_count), _ptr(self.out_first),
                                             _ptr(m["position"]), _ptr(m["normal"]), _ptr(m["joints"]),
                                             _ptr(m["weights"]), _ptr(self.joint_transforms),
                                             _ptr(self.out_position), _ptr(self.out_normal), None)
            self.out_w = None

    # ---- animated_update (model.c:1563-1592) --------------------------------------------
    def set_frame_times(self, frame_time, anim=None):
        """Directly set each character's (float)frame_time (and animation id)."""
        self.frame_time.copy_(upload(frame_time, np.float32, "cpu"))
        if anim is not None:
            self.anim_host[:] = anim
            self.anim.copy_(torch.from_numpy(self.anim_host))

    def animated_update(self, now):
        """animated_update (model.c:1563-1592) for the batch, all on the device: the clock kernel turns
        (now, ani_time, speed) into the float frame times, flags `ended` and restarts repeating queue
        entries (animation_next -> animation_start: ani_time = now); then pose + palette.  The host
        only reads `ended` back when it has non-repeating entries or callbacks to serve."""
        if self._clock is None:
            self.start_clock()
        if now is None:                                      # graph replay: the caller has written self.now_dev
            rc = _lib.lib().clapgpu_animation_time_dev(_stream(), C.byref(self._clock), _ptr(self.now_dev))
        else:
            rc = _lib.lib().clapgpu_animation_time(_stream(), C.byref(self._clock), float(now))
        _lib.check(rc, "clapgpu_animation_time")
        self.pose_update()

    def start_clock(self, ani_time=None, speed=None, repeat=None):
        """Device copies of entity3d.ani_time and the current queue entry's speed / repeat
        (model.h:417, model.c:1538-1541), from the host fields of the same names."""
        dev, n = self.device, self.n
        if ani_time is not None:
            self.ani_time[:] = ani_time
        if speed is not None:
            self.speed[:] = speed
        self.repeat_host = np.ones(n, np.uint8) if repeat is None else np.ascontiguousarray(repeat, np.uint8)
        self.ani_time_dev, self.speed_dev = upload(self.ani_time, np.float64, dev), upload(self.speed, np.float32, dev)
        self.repeat_dev = upload(self.repeat_host, np.uint8, dev)
        self.ended = device_array(max(n, 1), torch.uint8, dev)
        self.now_dev = device_array(1, torch.float64, dev)
        self.time_end_dev = upload(self.model.time_end, np.float32, dev)
        self._clock = _lib.AnimClock(n, len(self.model.time_end), _ptr(self.anim), _ptr(self.time_end_dev),
                                     _ptr(self.ani_time_dev), _ptr(self.speed_dev), _ptr(self.repeat_dev),
                                     _ptr(self.frame_time), _ptr(self.ended))

    def download_clock(self):
        torch.cuda.synchronize(self.device)
        return dict(ani_time=self.ani_time_dev.cpu().numpy(), frame_time=self.frame_time.cpu().numpy(),
                    ended=self.ended.cpu().numpy()[:self.n])

    def set_outputs(self, trs=True, joint_pos=True):
        """Which host-visible by-products pose_update writes besides the palette (clapgpu_pose_batch.skip)."""
        self._pose_desc.skip = (0 if trs else _lib.POSE_SKIP_TRS) | (0 if joint_pos else _lib.POSE_SKIP_JOINT_POS)

    def set_joint_pos_model_space(self, on=True):
        """CLAPGPU_POSE_JOINT_POS_MODEL: pose_update leaves the model-space joint positions (model.c:1392-1397) in joint_pos
        and does not read the entity matrices; joint_pos_world() finishes model.c:1400."""
        if on:
            self._pose_desc.skip |= _lib.POSE_JOINT_POS_MODEL
        else:
            self._pose_desc.skip &= ~_lib.POSE_JOINT_POS_MODEL

    def joint_pos_world(self):
        skip = self._pose_desc.skip
        self._pose_desc.skip = skip & ~_lib.POSE_JOINT_POS_MODEL
        rc = _lib.lib().clapgpu_joint_pos_world(_stream(), C.byref(self.model.skel_desc), C.byref(self._pose_desc))
        self._pose_desc.skip = skip
        _lib.check(rc, "clapgpu_joint_pos_world")

    def pose_update(self):
        rc = _lib.lib().clapgpu_pose_update(_stream(), C.byref(self.model.skel_desc), C.byref(self.model.anim_desc),
                                            C.byref(self._pose_desc))
        _lib.check(rc, "clapgpu_pose_update")

    def set_skin_w(self, on=True):
        """Also write total_local_pos.w per vertex (clapgpu_skin_batch.out_w; model.vert:36-38,44)."""
        if on and self.out_w is None:
            self.out_w = device_array(self.n_out_verts, torch.float32, self.device)
        self._skin_desc.out_w = _ptr(self.out_w) if on else None

    def skin(self):
        if self._skin_desc is None:
            raise ValueError("model has no skinned mesh")
        rc = _lib.lib().clapgpu_skin(_stream(), C.byref(self._skin_desc))
        _lib.check(rc, "clapgpu_skin")

    # ---- skinning that follows the cull and the LOD (clapgpu_skin_drawn) ------------------------
    def set_skin_select(self, planes, cur_lod=None, entity=None, row=None, lod_lists=None, n_entities=None):
        """What skin_drawn() skins (clapgpu_skin_select, include/clapgpu.h).  planes: the mask planes (1 .. 5 device tensors
        or uint64 arrays shaped like clapgpu_entities.vis_mask) -- a character is drawn when its entity's bit is set in
        one of them; None: left to the frame (FrameLoop(skin_select=...) supplies its batch's planes and cur_lod).
        cur_lod: int32 per entity (None: LOD 0).  entity: the characters' entity slots (None: the batch's entity_index;
        without one character c is entity c).
        lod_lists: (lod_first [n_rows, n_lods], lod_count [n_rows, n_lods], list) -- see skin_lod_lists(); row: the
        characters' rows (None: row 0).  n_entities: entities a plane covers (default: every bit of its words)."""
        if self._skin_desc is None:
            raise ValueError("model has no skinned mesh")
        dev, n = self.device, self.n
        s = _lib.SkinSelect()
        self._sel_planes = [] if planes is None else [
            p if torch.is_tensor(p) else upload(np.ascontiguousarray(p, np.uint64).view(np.int64), np.int64, dev) for p in planes]
        if len(self._sel_planes) > 1 + _lib.EXTRA_VIEWS_MAX:
            raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "set_skin_select", "at most 5 planes")
        s.n_planes = len(self._sel_planes)
        for k, p in enumerate(self._sel_planes):
            s.planes[k] = _ptr(p)
        if self._sel_planes:
            s.n_entities = int(n_entities) if n_entities is not None else 64 * min(p.numel() for p in self._sel_planes)
        self._sel_cur_lod = None if cur_lod is None else upload(cur_lod, np.int32, dev)
        self._sel_entity = self.entity_index if entity is None else upload(entity, np.uint32, dev)
        self._sel_row = None if row is None else upload(row, np.uint32, dev)
        s.cur_lod, s.entity, s.row = _ptr(self._sel_cur_lod), _ptr(self._sel_entity), _ptr(self._sel_row)
        self._sel_lists = self._sel_lists_host = None
        self._sel_row_host = None if row is None else np.asarray(row, np.int64)
        if lod_lists is not None:
            first, count, lst = lod_lists
            first = np.ascontiguousarray(first, np.uint32)
            first = first.reshape(-1, first.shape[-1])
            count = np.ascontiguousarray(count, np.uint32).reshape(first.shape)
            lst = np.ascontiguousarray(lst, np.uint32).reshape(-1)
            self._sel_lists = (upload(first, np.uint32, dev), upload(count, np.uint32, dev),
                               upload(lst if lst.size else np.zeros(1, np.uint32), np.uint32, dev))
            self._sel_lists_host = (first, count)
            s.n_rows, s.n_lods = first.shape
            s.lod_first, s.lod_count, s.list = (_ptr(t) for t in self._sel_lists)
            s.n_list = int(lst.size)
        self.skinned = device_array(max(n, 1), torch.uint8, dev, fill=_lib.SKIN_NOT_DRAWN)
        self.sel_chars = device_array(max(n, 1), torch.int32, dev)
        self.sel_count = device_array(1, torch.int32, dev)
        self.sel_status = device_array(1, torch.int32, dev)
        self._sel_scratch = device_array(int(_lib.lib().clapgpu_skin_select_scratch_bytes(n)), torch.uint8, dev)
        s.skinned, s.chars, s.count, s.status = _ptr(self.skinned), _ptr(self.sel_chars), _ptr(self.sel_count), _ptr(self.sel_status)
        s.scratch = _ptr(self._sel_scratch)
        self._sel_desc = s

    def skin_drawn(self):
        """clapgpu_skin_drawn: skin the characters set_skin_select's planes draw, at their LODs' vertices."""
        if getattr(self, "_sel_desc", None) is None:
            raise ValueError("set_skin_select() first")
        rc = _lib.lib().clapgpu_skin_drawn(_stream(), C.byref(self._skin_desc), C.byref(self._sel_desc))
        _lib.check(rc, "clapgpu_skin_drawn")

    def download(self):
        torch.cuda.synchronize(self.device)
        out = dict(trs=self.trs.cpu().numpy(), joint_transforms=self.joint_transforms.cpu().numpy(),
                   joint_pos=self.joint_pos.cpu().numpy())
        if self._skin_desc is not None:
            out["out_position"] = self.out_position.cpu().numpy()
            out["out_normal"] = self.out_normal.cpu().numpy()
            if self.out_w is not None:
                out["out_w"] = self.out_w.cpu().numpy()
            if getattr(self, "_sel_desc", None) is not None:
                out["count"] = int(self.sel_count.cpu().numpy().view(np.uint32)[0])
                out["status"] = int(self.sel_status.cpu().numpy().view(np.uint32)[0])
                out["skinned"] = self.skinned.cpu().numpy()[:self.n]
                out["chars"] = self.sel_chars.cpu().numpy().view(np.uint32)[:min(out["count"], self.n)]
        return out

    def pose_algorithmic_bytes(self):
        return 200 * self.n * self.model.nr_joints

    def skin_algorithmic_bytes(self):
        return 68 * self.n_out_verts + 64 * self.model.nr_joints * self.n

    def skin_drawn_algorithmic_bytes(self, skinned):
        """Bytes clapgpu_skin_drawn has to move for the downloaded `skinned` [n]: 68 B (72 with w) per written vertex, the
        64 * J palette bytes per drawn character, 4 B per list entry read.  (A listed index past the mesh counts as read
        and as written: the formula is for well-formed lists.)"""
        skinned = np.asarray(skinned)[:self.n]
        drawn = np.flatnonzero(skinned != _lib.SKIN_NOT_DRAWN)
        verts = self.vert_count_host[drawn].astype(np.int64)
        entries = np.zeros(drawn.size, np.int64)
        lists = getattr(self, "_sel_lists_host", None)
        if lists is not None:
            first, count = lists
            row = self._sel_row_host[drawn] if self._sel_row_host is not None else np.zeros(drawn.size, np.int64)
            ok = row < first.shape[0]
            f = first[np.where(ok, row, 0), skinned[drawn]]
            listed = ok & (f != _lib.SKIN_LOD_ALL)
            entries = np.where(listed, count[np.where(ok, row, 0), skinned[drawn]], 0).astype(np.int64)
            verts = np.where(listed, entries, verts)
        per_vertex = 72 if self._skin_desc.out_w else 68
        return int(per_vertex * verts.sum() + 64 * self.model.nr_joints * drawn.size + 4 * entries.sum())


QUEUE_ENTRY = np.dtype([("animation", "<u2"), ("repeat", "u1"), ("end", "u1"), ("speed", "<f4")])      # clapgpu_aniq_entry


def name_table(names):
    """name_anim of a model whose animations are called `names`: animation_by_name (model.c:1426-1434, the first match)
    of each of the twelve names character.c pushes, -1 where the model has none."""
    names = list(names)
    return np.asarray([names.index(k) if k in names else -1 for k in _lib.ANI_NAME_LIST], np.int32)


class AnimationQueues:
    """The character states and animation queues of one animated model (clapgpu_aniq), on the device.

    n characters in the order of `batch` (a CharacterBatch: the queue clock then writes its anim / frame_time, which the
    pose reads) or, without one, of arrays of its own.  name_anim [12]: name_table() of the model; time_end [n_anims].
    moves (a CharacterMoves) without `mover`: character c is mover c, and state, airborne, velocity and jump_params ARE the
    move's arrays, so the next frame's move reads the state these calls left.  mover [n]: index into the movers of the
    CharacterMoves given to characters_state(), -1 for none; the four arrays are then this object's own.
    set() uploads what the host decides: queue [n, 4] of QUEUE_ENTRY, len, cur, cleared, ani_time, state, airborne,
    velocity [n, 3], ch_motion [n, 2], jump_params [n, 2]."""

    _IN = dict(len=(np.uint8, ()), cur=(np.int8, ()), cleared=(np.uint8, ()), ani_time=(np.float64, ()), state=(np.uint8, ()),
               airborne=(np.uint8, ()), velocity=(np.float32, (3,)), ch_motion=(np.float32, (2,)), jump_params=(np.float32, (2,)))
    _TORCH = {np.uint8: torch.uint8, np.int8: torch.int8, np.float64: torch.float64, np.float32: torch.float32}

    def __init__(self, n, name_anim, time_end, device="cuda:0", batch=None, moves=None, mover=None, **state):
        self.device = dev = torch.device(device) if batch is None else batch.device
        self.n = n = int(n)
        self.batch, self.moves = batch, moves
        rows = max(n, 1)                                     # no null address when n is 0
        if batch is not None and batch.n != n:
            raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "AnimationQueues", "batch: a CharacterBatch of n characters")
        shared = moves is not None and mover is None
        if shared and moves.n != n:
            raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "AnimationQueues", "moves without mover: n movers")
        self.name_anim = upload(name_anim, np.int32, dev, (_lib.ANI_NAMES,))
        te = np.ascontiguousarray(time_end, np.float32).reshape(-1)
        self.n_anims = len(te)
        self.time_end = upload(te if len(te) else np.zeros(1, np.float32), np.float32, dev)
        self.queue = device_array((rows, 2 * _lib.ANIQ_MAX), torch.int32, dev)
        for k, (dt, tail) in self._IN.items():
            if shared and k in ("state", "airborne", "velocity", "jump_params"):
                setattr(self, k, getattr(moves, k))
            else:
                setattr(self, k, device_array((rows,) + tail, self._TORCH[dt], dev))
        self.mover = None if mover is None else upload(mover, np.int32, dev, (-1,))
        self.pose_anim = batch.anim if batch is not None else device_array(rows, torch.int32, dev)
        self.frame_time = batch.frame_time if batch is not None else device_array(rows, torch.float32, dev)
        self.events = device_array(rows, torch.int32, dev)
        self.now_dev = device_array(1, torch.float64, dev)
        self._desc = _lib.Aniq(n, self.n_anims, *[_ptr(getattr(self, k)) for k in
                                                   ("name_anim", "time_end", "queue", "len", "cur", "cleared", "ani_time",
                                                    "state", "airborne", "velocity", "ch_motion", "jump_params", "mover",
                                                    "pose_anim", "frame_time", "events")])
        self.set(**state)

    def set(self, queue=None, **arrays):
        if queue is not None and self.n:
            q = np.ascontiguousarray(queue, QUEUE_ENTRY).reshape(self.n, _lib.ANIQ_MAX)
            self.queue[:self.n].copy_(upload(q.view(np.uint32).reshape(self.n, 2 * _lib.ANIQ_MAX), np.uint32, self.device))
        for k, a in arrays.items():
            dt, tail = self._IN[k]
            if self.n:
                getattr(self, k)[:self.n].copy_(upload(a, dt, self.device, (-1,) + tail))

    def characters_state(self, moves, now):
        """clapgpu_characters_state behind moves' clapgpu_characters_move; now None: read from self.now_dev"""
        rc = _lib.lib().clapgpu_characters_state(_stream(), C.byref(self._desc), C.byref(moves._desc),
                                                 0.0 if now is None else float(now), _ptr(self.now_dev) if now is None else None)
        _lib.check(rc, "clapgpu_characters_state")

    def queue_time(self, now):
        """clapgpu_animation_queue_time: animated_update's clock, advance and callbacks; now None: self.now_dev"""
        rc = _lib.lib().clapgpu_animation_queue_time(_stream(), C.byref(self._desc), 0.0 if now is None else float(now),
                                                     _ptr(self.now_dev) if now is None else None)
        _lib.check(rc, "clapgpu_animation_queue_time")

    def download(self):
        torch.cuda.synchronize(self.device)
        n = self.n
        out = {k: getattr(self, k)[:n].cpu().numpy() for k in ("len", "cur", "cleared", "ani_time", "state", "airborne",
                                                                "velocity", "ch_motion", "jump_params", "frame_time")}
        out["queue"] = self.queue[:n].cpu().numpy().view(np.uint32).reshape(n, 2 * _lib.ANIQ_MAX).view(QUEUE_ENTRY)
        out["pose_anim"] = self.pose_anim[:n].cpu().numpy().view(np.uint32)
        out["events"] = self.events[:n].cpu().numpy().view(np.uint32)
        return out
