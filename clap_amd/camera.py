"""The camera controller on the device (include/clapgpu.h, "The camera controller on the device", ABI 50).

``CameraBlock`` holds a ``clapgpu_camera`` as a numpy record on the host and as 160 bytes on the device: the host writes
the inputs (``set``; ``camera_move``'s yaw and pitch stay the host's and arrive as the quaternion), ``upload`` is the one
small copy, ``calc`` is ``clapgpu_camera_calc`` -- camera_target, the pull-in rays against a ``PhysWorld``'s colliders and
the orbit in one launch, which also writes the pose into slot 0 of a ``views.ViewBlock``'s source -- and ``download``
reads the outputs back.  ``target`` / ``rays`` / ``decide`` / ``update_host`` are the host twins: the kernel's own
functions on host values.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._dev import device_array, ptr as _ptr, stream as _stream

# clapgpu_camera, field for field (tests/test_camera.py holds the offsets to the header's)
CAMERA = np.dtype([("quat", np.float32, 4), ("pos", np.float32, 3), ("dist", np.float32),
                   ("near_plane", np.float32), ("far_plane", np.float32), ("aspect", np.float32), ("moved", np.uint32),
                   ("ctl_entity", np.uint32), ("ctl_skip", np.int32), ("flags", np.uint32), ("head_joint", np.uint32),
                   ("target", np.float32, 3), ("updated", np.uint32), ("corner", np.float32, (4, 4)),
                   ("iterations", np.uint32), ("status", np.uint32), ("pad", np.uint32, 2)])
assert CAMERA.itemsize == _lib.CAMERA_BYTES

_F = C.POINTER(C.c_float)
_D = C.POINTER(C.c_double)


def _f(a):
    return a.ctypes.data_as(_F)


# ---- the host twins ---------------------------------------------------------------------------
def target(flags, pos_scale, lo, hi, center, head, far_plane):
    """camera_target (clapgpu_camera_target): (target [3] float32, dist float32)."""
    a = [np.ascontiguousarray(v, np.float32) for v in (pos_scale, lo, hi, center)]
    h = None if head is None else np.ascontiguousarray(head, np.float32)
    out, dist = np.zeros(3, np.float32), C.c_float(0.0)
    _lib.lib().clapgpu_camera_target(int(flags), *[_f(v) for v in a], None if h is None else _f(h), float(far_plane),
                                     _f(out), C.byref(dist))
    return out, np.float32(dist.value)


def rays(quat, tgt, dist, near_plane, aspect):
    """One iteration's corners [4, 4] float32 and rays [4, 8] float64 (clapgpu_camera_rays)."""
    q, t = np.ascontiguousarray(quat, np.float32), np.ascontiguousarray(tgt, np.float32)
    corner, ray = np.zeros((4, 4), np.float32), np.zeros((4, 8), np.float64)
    _lib.lib().clapgpu_camera_rays(_f(q), _f(t), float(np.float32(dist)), float(np.float32(near_plane)),
                                   float(np.float32(aspect)), _f(corner), ray.ctypes.data_as(_D))
    return corner, ray


def decide(dist, hit, depth, ray):
    """(good, min_scale, next_dist) of one iteration's four answers (clapgpu_camera_decide); next_dist is None when good."""
    h, d = np.ascontiguousarray(hit, np.int32), np.ascontiguousarray(depth, np.float64)
    r = np.ascontiguousarray(ray, np.float64)
    ms, nx = C.c_double(0.0), C.c_double(0.0)
    good = _lib.lib().clapgpu_camera_decide(float(np.float32(dist)), h.ctypes.data_as(C.POINTER(C.c_int32)), d.ctypes.data_as(_D),
                                            r.ctypes.data_as(_D), C.byref(ms), C.byref(nx))
    return bool(good), ms.value, (None if good else nx.value)


def update_host(rec, cast):
    """camera_update behind camera_target on a host record (clapgpu_camera_update_host): rec is a CAMERA record whose
    target and dist camera_target left; cast(ray [4, 8]) -> (hit [4], depth [4], flags [4]) answers one iteration's rays.
    Returns the updated record (a copy)."""
    out = np.array(rec, CAMERA).reshape(1).copy()

    def cb(_user, ray, hit, depth):
        r = np.ctypeslib.as_array(ray, shape=(4, 8)).copy()
        h, d, f = cast(r)
        anyf = 0
        for k in range(4):
            hit[k] = 1 if h[k] else 0
            depth[k] = float(d[k])
            anyf |= int(f[k])
        return anyf
    fn = _lib.CAMERA_CAST_FN(cb)
    _lib.lib().clapgpu_camera_update_host(out.ctypes.data_as(C.POINTER(_lib.Camera)), C.cast(fn, C.c_void_p), None)
    return out[0]


# ---- the block ----------------------------------------------------------------------------------
class CameraBlock:
    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        self._pinned = torch.zeros(CAMERA.itemsize // 4, dtype=torch.int32).pin_memory()
        self.host = self._pinned.numpy().view(CAMERA)                # one record, in pinned memory
        self.dev = device_array(CAMERA.itemsize // 4, torch.int32, self.device)

    def set(self, quat, near_plane, far_plane, aspect, ctl_entity, ctl_skip=-1, character=False, head_joint=None, moved=True,
            pos=(0.0, 0.0, 0.0), dist=0.0):
        """The inputs: c->xform.rotation after camera_move, the main view's planes, the control entity (its index in the
        batch, its rays' skip as clapgpu_ray_cast codes it or -1 without physics, whether it is a character and its head
        joint's index in the pose batch's joint positions) and camera_has_moved()."""
        h = self.host[0]
        h["quat"], h["pos"], h["dist"] = np.asarray(quat, np.float32), np.asarray(pos, np.float32), dist
        h["near_plane"], h["far_plane"], h["aspect"] = near_plane, far_plane, aspect
        h["moved"], h["ctl_entity"], h["ctl_skip"] = int(bool(moved)), int(ctl_entity), int(ctl_skip)
        h["flags"] = (_lib.CAMERA_IS_CHARACTER if character else 0) | (_lib.CAMERA_HAS_HEAD_JOINT if head_joint is not None else 0)
        h["head_joint"] = 0 if head_joint is None else int(head_joint)

    def upload(self):
        """The one small copy, on the current stream (pinned memory: asynchronous)."""
        self.dev.copy_(self._pinned, non_blocking=True)

    def calc(self, batch, world, views, joint_pos=None, grid=True, meshes=True):
        """clapgpu_camera_calc: batch an EntityBatch, world a PhysWorld (its body and static geoms, its mesh set when
        meshes, its index -- bp_index() first -- when grid), views a ViewBlock whose slot 0 is a pose, joint_pos the pose
        batch's world joint positions (a device tensor) or None."""
        g, sg = world.body_geoms(), world.static_geoms()
        rc = _lib.lib().clapgpu_camera_calc(_stream(), _ptr(self.dev), C.byref(batch._desc), _ptr(joint_pos),
                                            world._bp if grid else None, C.byref(g), C.byref(sg),
                                            world._meshes if meshes else None, _ptr(views.source))
        _lib.check(rc, "clapgpu_camera_calc")

    def download(self):
        """The block as a CAMERA record (host sync)."""
        torch.cuda.synchronize(self.device)
        return np.ascontiguousarray(self.dev.cpu().numpy()).view(CAMERA)[0].copy()
