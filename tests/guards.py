"""Guard bands around device arrays: the suite's instrument for WHERE a kernel writes.

An out-of-bounds store on the device does not fault: the caching allocator packs tensors side by side, so the store lands
in a neighbour or in slack.  A Guards registry hands out arrays that sit between two bands of 0xA5 inside one private
allocation; check() asserts that every band of every array it handed out is still 0xA5.

  g = Guards(device)                       # band=4096 bytes on each side
  t = g.array((n, 16), torch.float32)      # exactly n * 64 bytes, 256-byte aligned, zero filled
  s = g.scratch(nbytes)                    # the same for byte scratch
  ... run kernels ...
  g.check("after the update")

install(monkeypatch, g) makes the host mirrors allocate through g: every device array of clap_amd.{physics, entities,
animation, particles, lights, characters, shard} is made by clap_amd._dev.device_array or upload, and both end in
_dev._new, which install replaces: a GPU target is served by g.array (outputs, scratch and uploaded inputs alike), every
other target by the real function.  test_guards.py holds the mirrors to that one path by their source.  A label names the
mirror's module:line that asked for the array.

What this proves and what it does not.  A band is a condition, not a measurement: 4096 bytes is many times the largest
record any kernel writes (160 bytes), so a one-record overrun in either direction stays inside memory the test owns and
is seen, to the byte (the trailing band starts at the first byte after the array, not at a rounded address).  A store
that jumps over a whole band is not seen.  READ overruns cannot be proven absent this way: a kernel that reads past a
guarded input reads 0xA5A5... (as a float -2.9e-16, as an index above 2^31), which the value comparison next to the
guard check has a chance to notice and no more; nothing is claimed about reads.

What the hook does not reach: tensors a test builds itself (guard_like(g, t) re-homes one by hand), .clone() snapshots,
upload of what is already a tensor (it is taken as it is), and what the library allocates for itself: broadphase
objects, mesh sets, the stream-ordered array between the two ray passes.
"""
import collections
import os
import sys

import numpy as np
import torch as _torch

POISON = 0xA5
ALIGN = 256
_HERE = os.path.abspath(__file__).rstrip("c")
# one guarded array: its label, the whole allocation, where the leading band starts in it, the array's bytes, the array and
# what it was filled with (None once it was given contents: an uploaded input)
Entry = collections.namedtuple("Entry", "label buf off nbytes view fill")


def _site():
    """module:line of the nearest caller outside this file and clap_amd._dev"""
    f = sys._getframe(1)
    while f is not None and (os.path.abspath(f.f_code.co_filename).rstrip("c") == _HERE
                             or f.f_globals.get("__name__") == "clap_amd._dev"):
        f = f.f_back
    if f is None:
        return "?"
    return f"{f.f_globals.get('__name__', os.path.basename(f.f_code.co_filename))}:{f.f_lineno}"


def _shape(shape):
    if isinstance(shape, (int, np.integer)):
        return (int(shape),)
    return tuple(int(s) for s in shape)


class Guards:
    """A registry of guarded arrays on one device."""

    def __init__(self, device, band=4096):
        assert band > 0 and band % ALIGN == 0, "the leading band keeps the array 256-byte aligned"
        self.device = _torch.device(device)
        self.band = int(band)
        self.entries = []                                    # Entry, in the order of allocation

    def array(self, shape, dtype, fill=0, label=None, contents=None):
        """A tensor of exactly `shape` x `dtype`, filled with `fill` (or holding a copy of the tensor `contents`), between
        two bands of 0xA5."""
        shape = _shape(shape)
        item = _torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * item
        band = self.band
        buf = _torch.empty(band + nbytes + band + ALIGN, dtype=_torch.uint8, device=self.device)
        off = -buf.data_ptr() % ALIGN                        # the device allocator aligns to 512 already; the host's does not
        lo = off + band
        buf[off:lo] = POISON
        buf[lo + nbytes:lo + nbytes + band] = POISON
        view = buf[lo:lo + nbytes].view(dtype).reshape(shape)
        if nbytes:
            view.fill_(fill) if contents is None else view.copy_(contents)
            assert view.data_ptr() == buf.data_ptr() + lo and view.data_ptr() % ALIGN == 0, "guarded array not 256-byte aligned"
        assert view.numel() * view.element_size() == nbytes and view.is_contiguous()
        self.entries.append(Entry(f"{label or _site()} {dtype} {list(shape)}".replace("torch.", ""), buf, off, nbytes, view,
                                  fill if contents is None else None))
        return view

    def scratch(self, nbytes, label=None):
        """`nbytes` of zeroed byte scratch under guard."""
        return self.array((int(nbytes),), _torch.uint8, 0, label)

    def bands(self, k=-1):
        """(leading, trailing) band of the k-th registered array, as views"""
        e = self.entries[k]
        lo = e.off + self.band
        return e.buf[e.off:lo], e.buf[lo + e.nbytes:lo + e.nbytes + self.band]

    def dirty(self):
        """[(label, side, [byte offsets])] of every band that is no longer 0xA5; trailing offsets count from the first byte
        after the array, leading ones backwards from the byte before it (0 is the byte next to the array on both sides)"""
        if not self.entries:
            return []
        both = [b for k in range(len(self.entries)) for b in self.bands(k)]
        host = _torch.cat(both).cpu().numpy().reshape(-1, self.band)       # one copy, one synchronisation
        out = []
        for row in np.flatnonzero((host != POISON).any(axis=1)):
            at = np.flatnonzero(host[row] != POISON)
            side = "after" if row & 1 else "before"
            if side == "before":
                at = (self.band - 1 - at)[::-1]
            out.append((self.entries[row >> 1].label, side, at.tolist()))
        return out

    def check(self, what=""):
        """Every band of every registered array is still 0xA5."""
        bad = self.dirty()
        assert not bad, (f"{what}: " if what else "") + "written outside the array: " + "; ".join(
            f"{label}: {len(at)} bytes {side}, first at offsets {at[:8]}" for label, side, at in bad[:8]) + (
            f" (and {len(bad) - 8} more arrays)" if len(bad) > 8 else "")

    def rewritten(self, start=0):
        """Labels of the arrays registered from entry `start` on that no longer hold, in every byte, the value they were
        filled with (arrays given contents are skipped): for calls that must return without writing anything."""
        out = []
        for e in self.entries[start:]:
            if e.fill is not None and e.nbytes:
                flat = e.view.reshape(-1)
                same = _torch.full_like(flat, e.fill).view(_torch.uint8) == flat.view(_torch.uint8)
                if not bool(same.all().item()):
                    out.append(e.label)
        return out

    def owns(self, t):
        """Tensor `t` starts where a registered array starts and is no longer than it."""
        at, nbytes = t.data_ptr(), t.numel() * t.element_size()
        return any(e.view.data_ptr() == at and e.nbytes >= nbytes for e in self.entries)

    def __len__(self):
        return len(self.entries)


def guard_like(g, t, label=None):
    """A guarded copy of tensor `t` (for tensors the hook does not reach); the caller re-points whatever held `t`."""
    return g.array(t.shape, t.dtype, 0, label, contents=t)


# ------------------------------------------------------------------------------------------------------ the hook
def _on_gpu(device):
    return device is not None and _torch.device(device).type == "cuda"


def install(monkeypatch, g):
    """Guard what the mirrors allocate from here on, until monkeypatch undoes it: clap_amd._dev._new, the one function
    that makes a mirror's device array, serves GPU targets from g and passes everything else on."""
    from clap_amd import _dev
    real = getattr(_dev._new, "real", _dev._new)                         # installing twice does not wrap twice

    def _new(shape, dtype, device, fill, contents):
        if not _on_gpu(device):
            return real(shape, dtype, device, fill, contents)
        if contents is None:
            return g.array(shape, dtype, 0 if fill is None else fill)   # uninitialised: any fill will do
        host = _torch.from_numpy(contents)
        return g.array(host.shape, host.dtype, contents=host)
    _new.real = real
    monkeypatch.setattr(_dev, "_new", _new)
