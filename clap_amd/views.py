"""The view block (include/clapgpu.h, "Views in device memory"): what a frame knows about its views, in device memory.

``ViewBlock`` holds a ``clapgpu_views_source`` in pinned host memory and on the device, and the
``clapgpu_views_state`` that ``clapgpu_views_calc`` derives from it.  The camera controller stays the host's: it
writes the source (``set_camera`` / ``set_matrices`` / ``set_pose``), ``upload`` is the one small copy, and every
``*_views`` entry point reads the state.  A captured frame therefore follows whatever was uploaded before the replay.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._dev import device_array, stream as _stream

_WORDS_SRC, _WORDS_STATE = _lib.VIEWS_SOURCE_BYTES // 4, _lib.VIEWS_STATE_BYTES // 4


class ViewBlock:
    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        self.host = torch.zeros(_WORDS_SRC, dtype=torch.int32).pin_memory()          # clapgpu_views_source, as words
        self.source = device_array(_WORDS_SRC, torch.int32, self.device)
        self.state = device_array(_WORDS_STATE, torch.int32, self.device)
        self._src = _lib.ViewsSource.from_buffer(self.host.numpy())                  # the pinned words, as the struct

    # ---- the source, on the host ----------------------------------------------------------
    def set_matrices(self, slot, view_mx, proj_mx, pos=(0.0, 0.0, 0.0), ndc_z_zero_one=False):
        s = self._src.slot[slot]
        s.view_mx[:] = np.asarray(view_mx, np.float32).ravel().tolist()
        s.proj_mx[:] = np.asarray(proj_mx, np.float32).ravel().tolist()
        s.pos[:] = np.asarray(pos, np.float32).tolist()
        s.quat[:] = [0.0, 0.0, 0.0, 0.0]
        s.flags = _lib.VIEW_NDC_Z_ZERO_ONE if ndc_z_zero_one else 0

    def set_pose(self, slot, pos, quat, proj_mx, ndc_z_zero_one=False):
        s = self._src.slot[slot]
        s.view_mx[:] = [0.0] * 16
        s.proj_mx[:] = np.asarray(proj_mx, np.float32).ravel().tolist()
        s.pos[:] = np.asarray(pos, np.float32).tolist()
        s.quat[:] = np.asarray(quat, np.float32).tolist()
        s.flags = _lib.VIEW_FROM_POSE | (_lib.VIEW_NDC_Z_ZERO_ONE if ndc_z_zero_one else 0)

    def set_camera(self, slot, cam):
        """A synth.camera() dict as a pose: the view matrix is then the device's clapgpu_view_matrix(pos, quat)."""
        proj = np.zeros(16, np.float32)
        fov, aspect, near, far = (float(v) for v in cam["persp"])
        z01 = int(cam["ndc_z_zero_one"][0])
        _lib.lib().clapgpu_perspective(fov, aspect, near, far, z01, proj.ctypes.data_as(C.POINTER(C.c_float)))
        self.set_pose(slot, cam["cam_pos"], cam["cam_quat"], proj, bool(z01))

    # ---- the device ---------------------------------------------------------------------
    def upload(self):
        """The one small copy, on the current stream (pinned memory: asynchronous, legal between graph replays)."""
        self.source.copy_(self.host, non_blocking=True)

    def calc(self, n_views=_lib.VIEW_SLOTS):
        rc = _lib.lib().clapgpu_views_calc(_stream(), self.source.data_ptr(), self.state.data_ptr(), int(n_views))
        _lib.check(rc, "clapgpu_views_calc")

    def download(self):
        """The state as a _lib.ViewsState (host sync)."""
        torch.cuda.synchronize(self.device)
        words = np.ascontiguousarray(self.state.cpu().numpy())
        return _lib.ViewsState.from_buffer_copy(words.tobytes())
