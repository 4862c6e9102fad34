"""The shadow cascades on the device (include/clapgpu.h, "The shadow cascades on the device", ABI 51).

``CascadesBlock`` holds a ``clapgpu_cascades`` as a numpy record on the host and as 2416 bytes on the device: the host
writes the inputs (``set``: the light direction, the camera sub-frusta's projections, the flags -- none of them changes
with the camera), ``upload`` is the one small copy, ``calc`` is ``clapgpu_cascades_calc`` -- the camera's cascade
sub-frusta, near_backup, the shadow light's views and the cascades' projections in one launch, which also writes the
light's main view into its slot of a ``views.ViewBlock``'s source -- and ``download`` reads the outputs back.
``calc_host`` / ``near_backup`` / ``persp`` are the host twins: the kernel's own functions on host values.

What a renderer reads: ``cascade[v].mvp`` is UNIFORM_SHADOW_MVP[v], ``cascade[v].far_plane`` UNIFORM_LIGHT_FAR[v],
``cascade[v].view_mx`` / ``proj_mx`` the shadow pass's view and projection; ``view_mx`` is the light's main view, whose
frustum the shadow passes cull against (slot ``light_slot`` of the view block).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._dev import device_array, ptr as _ptr, stream as _stream

# clapgpu_cascade_view and clapgpu_cascades, field for field (tests/test_cascades.py holds the offsets to the header's)
CASCADE_VIEW = np.dtype([("view_mx", np.float32, 16), ("inv_view_mx", np.float32, 16), ("proj_mx", np.float32, 16),
                         ("inv_proj_mx", np.float32, 16), ("mvp", np.float32, 16), ("near_plane", np.float32),
                         ("far_plane", np.float32), ("pad", np.uint32, 2)])
CASCADES = np.dtype([("light_dir", np.float32, 3), ("nr_cascades", np.uint32), ("persp", np.float32, (4, 16)),
                     ("near_backup", np.float32), ("light_slot", np.uint32), ("flags", np.uint32), ("pad0", np.uint32),
                     ("cascade", CASCADE_VIEW, 4), ("view_mx", np.float32, 16), ("inv_view_mx", np.float32, 16),
                     ("near_backup_used", np.float32), ("bv_entity", np.uint32), ("status", np.uint32), ("pad1", np.uint32),
                     ("cam_corners", np.float32, (5, 8, 4))])
assert CASCADE_VIEW.itemsize == _lib.CASCADE_VIEW_BYTES and CASCADES.itemsize == _lib.CASCADES_BYTES

# clapgpu_view_source / clapgpu_views_source as records, for the twins' host copies
VIEW_SOURCE = np.dtype([("view_mx", np.float32, 16), ("proj_mx", np.float32, 16), ("pos", np.float32, 3), ("flags", np.uint32),
                        ("quat", np.float32, 4)])
VIEWS_SOURCE = np.dtype([("slot", VIEW_SOURCE, _lib.VIEW_SLOTS)])
assert VIEWS_SOURCE.itemsize == _lib.VIEWS_SOURCE_BYTES

_F = C.POINTER(C.c_float)


def _f(a):
    return a.ctypes.data_as(_F)


# ---- the host twins ---------------------------------------------------------------------------
def persp(fov, aspect, near_plane, far_plane, nr_cascades=0, ndc_z_zero_one=False):
    """persp[4, 16] of the block: the camera sub-frusta's projections by the splits of view.c:13-26
    (clapgpu_cascades_persp); rows at or past nr_cascades stay zero."""
    out = np.zeros((4, 16), np.float32)
    _lib.lib().clapgpu_cascades_persp(float(np.float32(fov)), float(np.float32(aspect)), float(np.float32(near_plane)),
                                      float(np.float32(far_plane)), int(nr_cascades), int(bool(ndc_z_zero_one)), _f(out))
    return out


def near_backup(light_dir, env_lo, env_hi, env_scale):
    """scene.c:1030-1037 for a bounding volume's model box and scale (clapgpu_cascades_near_backup): float32."""
    d, lo, hi = (np.ascontiguousarray(v, np.float32) for v in (light_dir, env_lo, env_hi))
    return np.float32(_lib.lib().clapgpu_cascades_near_backup(_f(d), _f(lo), _f(hi), float(np.float32(env_scale))))


def calc_host(rec, source, env=None):
    """clapgpu_cascades_calc on host copies (clapgpu_cascades_calc_host): rec a CASCADES record, source a VIEWS_SOURCE
    record, env None (the key 0) or (lo [3], hi [3], scale) of the picked entity's model box.  Returns the two updated
    records (copies)."""
    c = np.array(rec, CASCADES).reshape(1).copy()
    s = np.array(source, VIEWS_SOURCE).reshape(1).copy()
    lo, hi, scale = (np.zeros(3, np.float32), np.zeros(3, np.float32), 0.0) if env is None else \
        (np.ascontiguousarray(env[0], np.float32), np.ascontiguousarray(env[1], np.float32), float(np.float32(env[2])))
    _lib.lib().clapgpu_cascades_calc_host(c.ctypes.data_as(C.POINTER(_lib.Cascades)), s.ctypes.data_as(C.POINTER(_lib.ViewsSource)),
                                          _f(lo), _f(hi), scale, 0 if env is None else 1)
    return c[0], s[0]


# ---- the block ----------------------------------------------------------------------------------
class CascadesBlock:
    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        self._pinned = torch.zeros(CASCADES.itemsize // 4, dtype=torch.int32).pin_memory()
        self.host = self._pinned.numpy().view(CASCADES)              # one record, in pinned memory
        self.dev = device_array(CASCADES.itemsize // 4, torch.int32, self.device)

    def set(self, light_dir, persp_mx, light_slot=1, nr_cascades=0, near_backup=0.0, z_reverse=True, ndc_z_zero_one=False,
            near_backup_from_bv=False):
        """The inputs: s->light.dir, the sub-frusta's projections (persp()), the source slot of the light's main view,
        the number of cascades (0: 4), near_backup unless it comes from the bounding volume, and the two conventions."""
        h = self.host[0]
        h["light_dir"], h["nr_cascades"], h["persp"] = np.asarray(light_dir, np.float32), int(nr_cascades), np.asarray(persp_mx, np.float32)
        h["near_backup"], h["light_slot"] = near_backup, int(light_slot)
        h["flags"] = ((_lib.CASCADES_Z_REVERSE if z_reverse else 0) | (_lib.CASCADES_NDC_Z_ZERO_ONE if ndc_z_zero_one else 0) |
                      (_lib.CASCADES_NEAR_BACKUP_FROM_BV if near_backup_from_bv else 0))

    def upload(self):
        """The one small copy, on the current stream (pinned memory: asynchronous)."""
        self.dev.copy_(self._pinned, non_blocking=True)

    def calc(self, batch, views, bv_result=None):
        """clapgpu_cascades_calc: batch an EntityBatch, views a ViewBlock (slot 0 the camera, slot light_slot the light's
        matrices), bv_result a device uint64 tensor of one key (EntityBatch.bv_views) or None."""
        rc = _lib.lib().clapgpu_cascades_calc(_stream(), _ptr(self.dev), _ptr(views.source), C.byref(batch._desc), _ptr(bv_result))
        _lib.check(rc, "clapgpu_cascades_calc")

    def download(self):
        """The block as a CASCADES record (host sync)."""
        torch.cuda.synchronize(self.device)
        return np.ascontiguousarray(self.dev.cpu().numpy()).view(CASCADES)[0].copy()
