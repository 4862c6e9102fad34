"""Draw records on the device (include/clapgpu.h, "Draw records on the device"; ABI 53).

For one render pass ``records`` leaves what ``_models_render`` (core/model.c:742-1086) sets per drawn entity, in the order
it draws: txmodel by txmodel (model.c:784), inside a txmodel in the order of its entity list (model.c:959); one
192-byte record per draw and the range of every txmodel.  ``DrawOrder`` is that walk flattened, ``DrawInputs`` the
per-entity values (``entity3d_color()`` and friends stay one store), ``DrawOutputs`` one pass's buffers.
``records_host`` is the same over host arrays: the kernels' own decision functions (clapgpu_draw_records_host).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._dev import device_array, ptr as _ptr, stream as _stream, upload

# clapgpu_draw_record
RECORD = np.dtype([("mx", np.float32, 16), ("inv_mx", np.float32, 16), ("color", np.float32, 4),
                   ("bloom_intensity", np.float32), ("bloom_threshold", np.float32), ("edge_mode", np.uint32),
                   ("color_pt", np.int32), ("entity", np.uint32), ("lod", np.int32), ("group", np.uint32),
                   ("character", np.int32), ("flags", np.uint32), ("zero", np.uint32, 3)])
assert RECORD.itemsize == _lib.DRAW_RECORD_BYTES

INPUT_KEYS = (("color", np.float32), ("color_pt", np.int32), ("bloom_intensity", np.float32),
              ("bloom_threshold", np.float32), ("draw_flags", np.uint32), ("character", np.int32))


def draw_pass(shadow=False, ropts=None, mq_nr_characters=0, index_base=0):
    """clapgpu_draw_pass.  shadow: the pass has a shader override (model.c:786); ropts: None, or the render options'
    (bloom_intensity, bloom_threshold) (model.c:1002-1008)."""
    flags = (_lib.DRAW_PASS_SHADOW if shadow else 0) | (_lib.DRAW_PASS_HAS_ROPTS if ropts is not None else 0)
    bi, bt = (0.0, 0.0) if ropts is None else ropts
    return _lib.DrawPass(flags, float(np.float32(bi)), float(np.float32(bt)), int(mq_nr_characters), int(index_base))


class DrawOrder:
    """clapgpu_draw_order: order[r] is the entity at render position r, group g is one txmodel.  The host arrays are kept
    (order, group_start, group_flags); to(device) uploads them."""

    def __init__(self, order, group_start, group_flags, device=None):
        self.order = np.ascontiguousarray(order, np.uint32)
        self.group_start = np.ascontiguousarray(group_start, np.uint32)
        self.group_flags = np.ascontiguousarray(group_flags, np.uint32)
        self.n_order, self.n_groups = int(self.order.size), int(self.group_flags.size)
        self.device = None
        if device is not None:
            self.to(device)

    @classmethod
    def from_groups(cls, groups, skip_shadow=None, device=None):
        """groups: per txmodel, in the list order of mq->txmodels, the entity indices of its entity list in list order.
        skip_shadow: per txmodel model3d.skip_shadow (None: none has it)."""
        groups = [np.asarray(g, np.uint32).reshape(-1) for g in groups]
        start = np.zeros(len(groups) + 1, np.uint32)
        start[1:] = np.cumsum([g.size for g in groups], dtype=np.int64)
        order = np.concatenate(groups) if groups else np.zeros(0, np.uint32)
        skip = np.zeros(len(groups), bool) if skip_shadow is None else np.asarray(skip_shadow, bool)
        return cls(order, start, np.where(skip, _lib.DRAW_GROUP_SKIP_SHADOW, 0).astype(np.uint32), device)

    def to(self, device):
        self.device = torch.device(device)
        self._d = [upload(a if a.size else np.zeros(1, np.uint32), np.uint32, self.device)
                   for a in (self.order, self.group_start, self.group_flags)]
        self.desc = _lib.DrawOrder(self.n_order, self.n_groups, *[t.data_ptr() for t in self._d])
        return self

    def scratch_bytes(self):
        return int(_lib.lib().clapgpu_draw_records_scratch_bytes(self.n_order, self.n_groups))

    def host_desc(self):
        return _lib.DrawOrder(self.n_order, self.n_groups, self.order.ctypes.data, self.group_start.ctypes.data,
                              self.group_flags.ctypes.data)


class DrawInputs:
    """clapgpu_draw_inputs on `device`: per-entity color [n, 4], color_pt, bloom_intensity, bloom_threshold, draw_flags,
    character; any of them None (zeros; -1 for character)."""

    def __init__(self, device, **arrays):
        self.device = torch.device(device)
        self._d = {}
        for k, dt in INPUT_KEYS:
            a = arrays.pop(k, None)
            self._d[k] = None if a is None else upload(np.ascontiguousarray(a, dt), dt, self.device)
        if arrays:
            raise TypeError(f"DrawInputs: unknown arrays {sorted(arrays)}")
        self.desc = _lib.DrawInputs(*[_ptr(self._d[k]) or None for k, _dt in INPUT_KEYS])

    def __getitem__(self, k):
        return self._d[k]


class DrawOutputs:
    """One pass's buffers: records [capacity], count, group_first [n_groups + 1], status.  capacity 0: counts and ranges
    only."""

    def __init__(self, capacity, n_groups, device):
        self.capacity, self.n_groups = int(capacity), int(n_groups)
        self.device = torch.device(device)
        words = _lib.DRAW_RECORD_BYTES // 4
        self.records = device_array((self.capacity, words), torch.int32, self.device) if self.capacity else None
        self.count = device_array(1, torch.int32, self.device)
        self.group_first = device_array(self.n_groups + 1, torch.int32, self.device)
        self.status = device_array(1, torch.int32, self.device)

    def frame_block(self, dpass):
        """The clapgpu_frame_draw_pass of these buffers."""
        return _lib.FrameDrawPass(dpass, self.capacity, _ptr(self.records) or None, self.count.data_ptr(),
                                  self.group_first.data_ptr(), self.status.data_ptr())

    def download(self):
        """(records as RECORD[min(count, capacity)], count, group_first, status); synchronises."""
        torch.cuda.synchronize(self.device)
        count = int(self.count.cpu().numpy().view(np.uint32)[0])
        status = int(self.status.cpu().numpy().view(np.uint32)[0])
        first = self.group_first.cpu().numpy().view(np.uint32).copy()
        k = min(count, self.capacity)
        rec = (self.records[:k].cpu().numpy().view(np.uint8).reshape(-1).view(RECORD).copy() if k
               else np.zeros(0, RECORD))
        return rec, count, first, status


class FrameDraw:
    """clapgpu_frame_draw for FrameLoop(draw=...): main and every entry of views is None or (DrawOutputs, draw_pass(...));
    views[v] is the pass of the batch's further view v.  The scratch is shared by the passes."""

    def __init__(self, order, inputs=None, main=None, views=(), scratch=None):
        self.order, self.inputs, self.main, self.views = order, inputs, main, list(views)
        self.scratch = scratch if scratch is not None else scratch_for(order)

    def desc(self):
        d = _lib.FrameDraw()
        d.order = C.pointer(self.order.desc)
        if self.inputs is not None:
            d.inputs = C.pointer(self.inputs.desc)
        if self.main is not None:
            d.main = self.main[0].frame_block(self.main[1])
        for v, blk in enumerate(self.views):
            if blk is not None:
                d.view[v] = blk[0].frame_block(blk[1])
        d.scratch = self.scratch.data_ptr()
        return d


def scratch_for(order):
    """Device scratch for calls with this order (256-byte aligned: a device array's start)."""
    return device_array(order.scratch_bytes(), torch.uint8, order.device)


def records(batch, order, out, dpass, inputs=None, plane="main", lod=None, scratch=None):
    """clapgpu_draw_records on the current stream.  batch: entities.EntityBatch; plane: "main" (batch.vis_mask), a device
    tensor of mask words, or None: the pass without a view; lod: a device int32 tensor (cur_lod) or None."""
    if scratch is None:
        scratch = scratch_for(order)
    mask = batch.vis_mask if isinstance(plane, str) and plane == "main" else plane
    rc = _lib.lib().clapgpu_draw_records(_stream(), C.byref(batch._desc), _ptr(mask) or None, _ptr(lod) or None,
                                         C.byref(order.desc), C.byref(inputs.desc) if inputs is not None else None,
                                         C.byref(dpass), _ptr(out.records) or None, out.capacity, out.count.data_ptr(),
                                         out.group_first.data_ptr(), out.status.data_ptr(), scratch.data_ptr())
    _lib.check(rc, "clapgpu_draw_records")
    return scratch


def records_host(mx, inv_mx, order, dpass, capacity, flags=None, plane=None, lod=None, inputs=None, fill=0):
    """clapgpu_draw_records_host over host arrays.  mx / inv_mx: float32 [n, 16] (any bits); flags: uint32 [n] (read when
    plane is None); plane: uint64 mask words or None; lod: int32 [n] or None; inputs: a dict with any of INPUT_KEYS'
    names; fill: the byte the record buffer holds beforehand.  Returns (records RECORD[capacity], count, group_first,
    status): the whole buffer, so that what the call left untouched can be seen."""
    mx = np.ascontiguousarray(mx).view(np.float32).reshape(-1, 16)
    inv_mx = np.ascontiguousarray(inv_mx).view(np.float32).reshape(-1, 16)
    n = mx.shape[0]
    keep = [mx, inv_mx]
    e = _lib.Entities()
    e.n, e.mx, e.inv_mx = n, mx.ctypes.data, inv_mx.ctypes.data
    if flags is not None:
        fl = np.ascontiguousarray(flags, np.uint32)
        keep.append(fl)
        e.flags = fl.ctypes.data
    pl = None if plane is None else np.ascontiguousarray(plane).view(np.uint64)
    ld = None if lod is None else np.ascontiguousarray(lod, np.int32)
    ind = _lib.DrawInputs()
    for k, dt in INPUT_KEYS:
        a = (inputs or {}).get(k)
        if a is not None:
            a = np.ascontiguousarray(a, dt)
            keep.append(a)
            setattr(ind, k, a.ctypes.data)
    raw = np.full(max(int(capacity), 1) * RECORD.itemsize + 64, fill, np.uint8)
    at = -raw.ctypes.data % 64                          # the record buffer starts on a 64-byte line
    rec = raw[at:at + max(int(capacity), 1) * RECORD.itemsize]
    count, status = np.array([0xdead], np.uint32), np.array([0xdead], np.uint32)
    first = np.full(order.n_groups + 1, 0xdead, np.uint32)
    od = order.host_desc()
    _lib.lib().clapgpu_draw_records_host(C.byref(e), None if pl is None else pl.ctypes.data,
                                         None if ld is None else ld.ctypes.data, C.byref(od),
                                         C.byref(ind) if inputs is not None else None, C.byref(dpass),
                                         rec.ctypes.data if capacity else None, int(capacity), count.ctypes.data,
                                         first.ctypes.data, status.ctypes.data)
    return rec.view(RECORD)[:int(capacity)], int(count[0]), first, int(status[0])
