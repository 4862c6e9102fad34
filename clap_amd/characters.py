"""Host-side mirror of the reference's per-character update hook.

``CharacterFeed.character_update`` is ``character_update`` (character.c:583-611) for every character
of the scene, minus its tail call: the limbo teleport out of the position history, the body
read-back and ``history_push``.  The tail call (``orig_update`` = ``default_update``) is
``EntityBatch.mq_update``; ``character_motion_reset`` acts on the controlled character and stays with
the host.  ``CharacterMoves`` holds the state of ``struct character`` that ``character_move`` reads and writes,
for ``PhysWorld.characters_move`` (clapgpu_characters_move); ``physics.CharacterMoves`` is the same class.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._dev import device_array, ptr as _ptr, stream as _stream, upload


class CharacterFeed:
    def __init__(self, feed, device="cuda:0"):
        """feed: dict as made by clap_amd.synth.character_feed() (entity, body, hist_*, airborne, limbo_height)."""
        self.device = dev = torch.device(device)
        self.n = n = int(feed["n"])
        t = lambda a, dt: upload(a, dt, dev)
        self.entity = t(feed["entity"], np.uint32)
        self.body = t(feed["body"], np.int32)
        self.hist_pos = t(feed["hist_pos"], np.float32)
        self.hist_head = t(feed["hist_head"], np.uint32)
        self.hist_wrapped = t(feed["hist_wrapped"], np.uint8)
        self.airborne = t(feed["airborne"], np.uint8)
        self.moved = device_array(max(n, 1), torch.uint8, dev)
        self.limbo_height = float(feed["limbo_height"])
        self._desc = _lib.Characters(n, self.limbo_height, self.entity.data_ptr(), self.body.data_ptr(),
                                     self.hist_pos.data_ptr(), self.hist_head.data_ptr(),
                                     self.hist_wrapped.data_ptr(), self.airborne.data_ptr(), self.moved.data_ptr())

    def set_airborne(self, airborne):
        """character.airborne as the host's character_move left it."""
        self.airborne.copy_(upload(airborne, np.uint8, "cpu"))

    def character_update(self, batch, world=None):
        """batch: EntityBatch; world: PhysWorld holding the characters' bodies, or None."""
        rc = _lib.lib().clapgpu_characters_update(_stream(), C.byref(self._desc), C.byref(batch._desc),
                                                  C.byref(world._desc) if world is not None else None)
        _lib.check(rc, "clapgpu_characters_update")

    def download(self):
        torch.cuda.synchronize(self.device)
        return dict(hist_pos=self.hist_pos.cpu().numpy(), hist_head=self.hist_head.cpu().numpy().view(np.uint32),
                    hist_wrapped=self.hist_wrapped.cpu().numpy(), moved=self.moved.cpu().numpy()[:self.n])


class CharacterMoves:
    """The movers of clapgpu_characters_move (clapgpu_move): device arrays of the per-character state character_move reads
    and writes, the outputs, the scratch and the descriptor.  bodies [n]: the characters' bodies, each once; ray_off [n];
    jump_params [n, 2] (jump_forward, jump_upward).  entity [n] with entity_batch: the rotation hand-off (set yaw_quat
    every frame).  velocity / normal / airborne persist on the device from call to call, as the reference keeps them in
    struct character; set() uploads what the host changed."""

    _IN = dict(motion=(np.float32, 2), state=(np.uint8, 0), jump=(np.uint8, 0), jump_params=(np.float32, 2),
               velocity=(np.float32, 3), normal=(np.float32, 3), airborne=(np.uint8, 0), yaw_quat=(np.float32, 4))

    def __init__(self, world, bodies, ray_off, jump_params=None, entity=None, entity_batch=None, **state):
        if (entity is None) != (entity_batch is None):
            raise _lib.ClapGpuError(_lib.ERR_INVALID_ARGUMENTS, "CharacterMoves", "entity and entity_batch: both or neither")
        self.world, self.entity_batch = world, entity_batch
        self.device = dev = world.device
        self.n = n = len(bodies)
        out = lambda tail, dt, fill=0: world._out(n, tail, dt, fill)         # max(n, 1) rows: no null address when n is 0
        self.body = upload(bodies, np.uint32, dev) if n else out((), torch.int32)
        self.ray_off = upload(ray_off, np.float64, dev, (-1,)) if n else out((), torch.float64)
        self.motion, self.jump_params = out((2,), torch.float32), out((2,), torch.float32)
        self.state, self.jump, self.airborne = out((), torch.uint8), out((), torch.uint8), out((), torch.uint8)
        self.velocity, self.normal = out((3,), torch.float32), out((3,), torch.float32)
        self.request, self.applied = out((), torch.uint8), out((), torch.uint8)
        self.collision = out((), torch.int32, -1)
        self.first_frac = out((2,), torch.float32, 1)
        self.push_hit = out((6,), torch.int32, -1)
        self.flags = out((), torch.int32)
        self.entity = self.yaw_quat = None
        if entity is not None:
            self.entity = upload(entity, np.uint32, dev) if n else out((), torch.int32)
            self.yaw_quat = out((4,), torch.float32)
            self.yaw_quat[:, 3] = 1.0
        need = _lib.characters_move_scratch_bytes(world.n, n) if n else 0
        self.scratch = device_array(max(need, 256), torch.uint8, dev)
        self._desc = _lib.CharactersMove(n, *[_ptr(getattr(self, k)) for k in
                                              ("body", "ray_off", "motion", "state", "jump", "jump_params", "velocity",
                                               "normal", "airborne", "request", "applied", "collision", "first_frac",
                                               "push_hit", "flags", "entity", "yaw_quat")])
        if jump_params is not None:
            state["jump_params"] = jump_params
        self.set(**state)

    def set(self, **arrays):
        """Upload motion [n, 2], state [n], jump [n], jump_params [n, 2], velocity [n, 3], normal [n, 3], airborne [n],
        yaw_quat [n, 4] (x, y, z, w): those given, into the arrays the descriptor points at."""
        for k, a in arrays.items():
            dt, width = self._IN[k]
            a = np.asarray(a)
            if dt == np.uint8 and a.dtype != np.uint8:
                a = a != 0 if k != "state" else a
            if self.n:
                getattr(self, k)[:self.n].copy_(upload(a, dt, self.device, (-1, width) if width else (-1,)))

    def outputs(self):
        """dict of device tensors: velocity, normal, airborne (in / out), request, applied, collision, first_frac,
        push_hit, flags (ray flags | slide flags << 8)."""
        n = self.n
        return {k: getattr(self, k)[:n] for k in ("velocity", "normal", "airborne", "request", "applied", "collision",
                                                   "first_frac", "push_hit", "flags")}
