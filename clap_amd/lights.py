"""Host-side mirror of the reference's light slots and clustered-lighting grid.

``LightSet`` keeps what ``struct light`` keeps for the tile-mask pass (light.h:19-58): slot
allocation (``light_get`` / ``light_put``, light.c:311-352), the per-slot setters
(light.c:473-520) and the grid geometry (``light_handle_input`` resize, light.c:156-166, cell =
TILE_WIDTH, light.c:210).  ``grid_compute`` is ``light_grid_compute`` (light.c:88-154) on the GPU;
``from_entities`` the light hand-off of ``default_update`` (model.c:1689-1694); ``update_from_entities`` is
``light_update`` (light.c:462-471) for the lights that track an entity (``set_spots``): position, a spotlight's direction
and the pose of its shadow view, written on the device (include/clapgpu.h, "Spotlights on the device").
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._dev import device_array, ptr as _ptr, stream as _stream, upload  # noqa: F401

TILE_WIDTH = 64          # shader_constants.h:16


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def grid_dims(width, height, cell=TILE_WIDTH):
    tw, th = C.c_uint32(0), C.c_uint32(0)
    _lib.lib().clapgpu_light_grid_dims(width, height, cell, C.byref(tw), C.byref(th))
    return tw.value, th.value


class LightSet:
    def __init__(self, device="cuda:0", width=0, height=0, cell=TILE_WIDTH):
        self.device = dev = torch.device(device)
        M = _lib.LIGHTS_MAX
        # host slots (authoritative, like struct light); uploaded when touched
        self.pos = np.zeros((M, 3), np.float32)
        self.color = np.zeros((M, 3), np.float32)
        self.attenuation = np.zeros((M, 3), np.float32)
        self.is_dir = np.zeros(M, np.int32)
        self.active = np.zeros(M, np.uint32)
        self.dir = np.zeros((M, 3), np.float32)
        self.cutoff = np.zeros(M, np.float32)
        self.nr_lights = 0
        self.width, self.height, self.cell = int(width), int(height), int(cell)
        self._d = {k: device_array((M, 3), torch.float32, dev) for k in ("pos", "color", "attenuation")}
        self._d.update({k: device_array(M, torch.int32, dev) for k in ("is_dir", "active")})
        self._d["dir"] = device_array((M, 3), torch.float32, dev)
        self._d["cutoff"] = device_array(M, torch.float32, dev)
        self.spot_status = device_array(1, torch.int32, dev)
        self._spots, self._spot_slots = None, []
        self._dirty = set(self._d)
        self.tiles = None
        self._carriers = None

    # ---- slots (light.c:311-352, 473-520) ------------------------------------------------
    def light_get(self):
        free = np.flatnonzero(self.active == 0)
        if free.size == 0:
            raise _lib.ClapGpuError(_lib.ERR_TOO_LARGE, "light_get")
        idx = int(free[0])                                  # bitmap_set_lowest
        self.active[idx] = 1
        self.nr_lights = max(self.nr_lights, idx + 1)
        self.pos[idx] = 0
        self.color[idx] = 0
        self.attenuation[idx] = (1, 0, 0)
        self.is_dir[idx] = 1
        self.dir[idx] = 0
        self.cutoff[idx] = 0
        self._dirty.update(self._d)
        return idx

    def light_put(self, idx):
        if self.light_is_valid(idx):
            self.active[idx] = 0
            self._dirty.add("active")

    def light_is_valid(self, idx):
        return 0 <= idx < self.nr_lights and bool(self.active[idx])

    def _set(self, name, idx, value):
        if self.light_is_valid(idx):                        # every setter is a no-op on a released slot
            getattr(self, name)[idx] = value
            self._dirty.add(name)

    def light_set_pos(self, idx, pos):
        self._set("pos", idx, pos)

    def light_set_color(self, idx, color):
        self._set("color", idx, color)

    def light_set_attenuation(self, idx, att):
        self._set("attenuation", idx, att)

    def light_set_directional(self, idx, is_directional):
        self._set("is_dir", idx, int(bool(is_directional)))

    def light_set_cutoff(self, idx, cutoff):
        self._set("cutoff", idx, cutoff)                    # light.c:524-530

    def light_set_direction(self, idx, direction):
        """light.c:508-514: the slot holds (0,0,0) - direction, in float32."""
        self._set("dir", idx, np.float32(0.0) - np.asarray(direction, np.float32))

    def light_is_spotlight(self, idx):
        """light.c:516-522: a directional slot with a cutoff above zero (a NaN cutoff is none)."""
        return self.light_is_valid(idx) and bool(self.is_dir[idx]) and bool(float(self.cutoff[idx]) > 0.0)

    def load(self, lights):
        """Take all slots from a dict as made by clap_amd.synth.lights()."""
        n = int(lights["nr_lights"])
        self.nr_lights = n
        for k in ("pos", "color", "attenuation", "is_dir", "active"):
            getattr(self, k)[:] = 0
            getattr(self, k)[:n] = lights[k]
        for k in ("dir", "cutoff"):                         # optional: a dict without spotlights has neither
            getattr(self, k)[:] = 0
            if k in lights:
                getattr(self, k)[:n] = lights[k]
        self._dirty.update(self._d)

    def resize(self, width, height):
        self.width, self.height = int(width), int(height)

    # ---- device --------------------------------------------------------------------------
    def _upload(self):
        for k in self._dirty:
            self._d[k].copy_(torch.from_numpy(getattr(self, k).view(np.int32) if k == "active" else getattr(self, k)))
        self._dirty.clear()

    def _desc(self):
        d = self._d
        return _lib.Lights(self.nr_lights, 0, d["pos"].data_ptr(), d["color"].data_ptr(),
                           d["attenuation"].data_ptr(), d["is_dir"].data_ptr(), d["active"].data_ptr())

    def set_carriers(self, entity, light, off):
        """Entities that carry a light slot (e->light_idx, e->light_off; scene.c:1586-1608), in entity order."""
        dev = self.device
        self._carriers = (len(entity), upload(entity, np.uint32, dev), upload(light, np.int32, dev),
                          upload(off, np.float32, dev))

    def from_entities(self, batch, all_dirty=False):
        """model.c:1689-1694 for the carriers; run before batch.mq_update (which clears the dirty flags)."""
        if not self._carriers or not self._carriers[0]:
            return
        self._upload()
        n, ce, cl, co = self._carriers
        desc = self._desc()
        rc = _lib.lib().clapgpu_lights_from_entities(_stream(), C.byref(batch._desc),
                                                     _lib.UPDATE_ALL_DIRTY if all_dirty else 0, n, ce.data_ptr(),
                                                     cl.data_ptr(), co.data_ptr(), C.byref(desc))
        _lib.check(rc, "clapgpu_lights_from_entities")

    def set_spots(self, entity, light, off, view_slot=None):
        """The lights that track an entity's transform (light_set_update with light_update_from_entity, scene.c:1626-1631),
        in entity order.  view_slot: per carrier 0, or the slot of the view block's source that holds the spotlight's own
        shadow view (a pose slot the caller has given its projection, spot_persp); None: no carrier has one."""
        dev = self.device
        self._spots = (len(entity), upload(entity, np.uint32, dev), upload(light, np.int32, dev),
                       upload(np.asarray(off, np.float32).reshape(-1), np.float32, dev),
                       None if view_slot is None else upload(view_slot, np.uint32, dev))
        self._spot_slots = [] if view_slot is None else sorted(set(int(v) for v in np.asarray(view_slot, np.uint32) if v))

    def _spots_desc(self):
        n, ce, cl, co, cv = self._spots
        d = self._d
        return _lib.Spots(n, 0, ce.data_ptr(), cl.data_ptr(), co.data_ptr(), _ptr(cv), d["dir"].data_ptr(),
                          d["cutoff"].data_ptr(), self.spot_status.data_ptr())

    def spot_view_slots(self):
        """The source slots the device writes: those of the carriers' views."""
        return self._spot_slots if self._spots else []

    def update_from_entities(self, batch, views=None, all_dirty=False):
        """light_update (light.c:462-471) for the tracked lights; run before batch.mq_update (which clears the dirty
        flags).  views: the views.ViewBlock whose source gets the spotlights' poses (needed with view slots)."""
        if not self._spots:
            return
        self._upload()
        desc, sp = self._desc(), self._spots_desc()
        rc = _lib.lib().clapgpu_lights_update(_stream(), C.byref(batch._desc), _lib.UPDATE_ALL_DIRTY if all_dirty else 0,
                                              C.byref(sp), C.byref(desc), views.source.data_ptr() if views is not None else None)
        _lib.check(rc, "clapgpu_lights_update")

    def download_dir(self):
        """Light directions and the status word as the device holds them (after update_from_entities)."""
        torch.cuda.synchronize(self.device)
        if "dir" not in self._dirty:
            self.dir[:] = self._d["dir"].cpu().numpy()
        return self.dir.copy(), int(self.spot_status.item())

    def download_pos(self):
        """Light positions as the device holds them (after from_entities); also refreshes the host slots."""
        torch.cuda.synchronize(self.device)
        if "pos" not in self._dirty:
            self.pos[:] = self._d["pos"].cpu().numpy()
        return self.pos.copy()

    def alloc_tiles(self):
        """light_grid_update's (re)allocation of the tile array: device int32[theight][twidth][4], or None for an empty grid."""
        tw, th = grid_dims(self.width, self.height, self.cell)
        if not tw or not th:
            return None
        if self.tiles is None or self.tiles.shape[:2] != (th, tw):
            self.tiles = device_array((th, tw, 4), torch.int32, self.device)
        return self.tiles

    def grid_compute(self, view_mx, proj_mx):
        """light_grid_compute: returns the device tile masks int32[theight][twidth][4] (RGBA32UI texels)."""
        self._upload()
        if self.alloc_tiles() is None:
            return None
        desc = self._desc()
        vm = np.ascontiguousarray(view_mx, np.float32)
        pm = np.ascontiguousarray(proj_mx, np.float32)
        rc = _lib.lib().clapgpu_light_grid_compute(_stream(), C.byref(desc), _fp(vm), _fp(pm), self.width,
                                                   self.height, self.cell, self.tiles.data_ptr())
        _lib.check(rc, "clapgpu_light_grid_compute")
        return self.tiles

    def grid_compute_views(self, views):
        """grid_compute with view, mvp and proj_mx[0] read from slot 0 of a views.ViewBlock's state."""
        self._upload()
        if self.alloc_tiles() is None:
            return None
        desc = self._desc()
        rc = _lib.lib().clapgpu_light_grid_compute_views(_stream(), C.byref(desc), views.state.data_ptr(), self.width,
                                                         self.height, self.cell, self.tiles.data_ptr())
        _lib.check(rc, "clapgpu_light_grid_compute_views")
        return self.tiles

    def download_tiles(self):
        torch.cuda.synchronize(self.device)
        return self.tiles.cpu().numpy().view(np.uint32)

    def algorithmic_bytes(self):
        tw, th = grid_dims(self.width, self.height, self.cell)
        return 16 * tw * th                                 # the masks; the light slots are ~5 KB


def spot_persp(cutoff, ndc_z_zero_one=False):
    """The projection of a spotlight's shadow view (light.c:404-408): clapgpu_spot_persp, 16 floats."""
    p = np.zeros(16, np.float32)
    _lib.lib().clapgpu_spot_persp(float(np.float32(cutoff)), int(bool(ndc_z_zero_one)), _fp(p))
    return p


def update_host(pos_scale, rot, flags, carriers, lights, dir, cutoff, source=None, mode=0, status=0xdead):
    """clapgpu_lights_update on host arrays (clapgpu_lights_update_host, the kernel's own functions).  pos_scale / rot:
    float32 [n, 4]; flags: uint32 [n]; carriers: (entity, light, off[k, 3], view_slot or None); lights: a dict with
    nr_lights and the LIGHTS_MAX-row arrays pos, is_dir, active (color and attenuation are not read); dir [LIGHTS_MAX, 3],
    cutoff [LIGHTS_MAX]; source: a cascades.VIEWS_SOURCE record or None.  Returns copies: (pos, dir, status, source)."""
    from .cascades import VIEWS_SOURCE
    M = _lib.LIGHTS_MAX
    ps, rt = np.ascontiguousarray(pos_scale, np.float32).copy(), np.ascontiguousarray(rot, np.float32).copy()
    fl = np.ascontiguousarray(flags, np.uint32).copy()
    ce, cl = np.ascontiguousarray(carriers[0], np.uint32).copy(), np.ascontiguousarray(carriers[1], np.int32).copy()
    co = np.ascontiguousarray(carriers[2], np.float32).reshape(-1).copy()
    cv = None if carriers[3] is None else np.ascontiguousarray(carriers[3], np.uint32).copy()
    pos = np.ascontiguousarray(lights["pos"], np.float32).reshape(M, 3).copy()
    other = np.zeros((M, 3), np.float32)
    is_dir, active = np.ascontiguousarray(lights["is_dir"], np.int32).copy(), np.ascontiguousarray(lights["active"], np.uint32).copy()
    d, cut = np.ascontiguousarray(dir, np.float32).reshape(M, 3).copy(), np.ascontiguousarray(cutoff, np.float32).copy()
    st = np.array([status], np.uint32)
    src = None if source is None else np.array(source, VIEWS_SOURCE).reshape(1).copy()
    e = _lib.Entities()
    e.n, e.pos_scale, e.rot, e.flags = len(fl), ps.ctypes.data, rt.ctypes.data, fl.ctypes.data
    sp = _lib.Spots(len(ce), 0, ce.ctypes.data, cl.ctypes.data, co.ctypes.data, None if cv is None else cv.ctypes.data,
                    d.ctypes.data, cut.ctypes.data, st.ctypes.data)
    ld = _lib.Lights(int(lights["nr_lights"]), 0, pos.ctypes.data, other.ctypes.data, other.ctypes.data, is_dir.ctypes.data,
                     active.ctypes.data)
    _lib.lib().clapgpu_lights_update_host(C.byref(e), int(mode), C.byref(sp), C.byref(ld), None if src is None else src.ctypes.data)
    return pos, d, int(st[0]), (None if src is None else src[0])
