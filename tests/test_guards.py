"""tests/guards.py, the guard-band instrument of test_extents_gpu.py, on the CPU: what it hands out, what it reports, and
that the hook changes nothing but where GPU arrays are allocated; and the source rule that keeps the mirrors on that path."""
import numpy as np
import pytest
import torch

import guards
from guards import Guards


def bigger_view(g, k=-1):
    """(bytes of the whole guarded span of array k as one writable view, offset of the array's first byte in it, bytes)"""
    e = g.entries[k]
    return e.buf[e.off:e.off + 2 * g.band + e.nbytes], g.band, e.nbytes


@pytest.mark.parametrize("shape,dtype,fill", [((3, 5), torch.float32, 0), ((7,), torch.uint8, 9), (65, torch.int64, -1),
                                               ((2, 3, 16), torch.float64, 1.5), ((0, 3), torch.float32, 0), ((), torch.int32, 4),
                                               ((13,), torch.bool, True)])
def test_array_is_what_was_asked_for(shape, dtype, fill):
    g = Guards("cpu")
    t = g.array(shape, dtype, fill)
    want = torch.full((shape,) if isinstance(shape, int) else shape, fill, dtype=dtype)
    assert t.shape == want.shape and t.dtype == dtype and t.is_contiguous() and t.device.type == "cpu"
    assert torch.equal(t, want)
    lead, trail = g.bands()
    assert lead.numel() == trail.numel() == 4096
    assert (lead == 0xA5).all() and (trail == 0xA5).all()
    if t.numel():
        assert t.data_ptr() % 256 == 0
        nbytes = t.numel() * t.element_size()
        assert lead.data_ptr() + 4096 == t.data_ptr() and trail.data_ptr() == t.data_ptr() + nbytes      # no rounding: the
    g.check("fresh")                                                                                    # next byte is band


def test_scratch_is_bytes_and_a_band_can_be_smaller():
    g = Guards("cpu", band=256)
    s = g.scratch(1001)
    assert s.dtype == torch.uint8 and s.shape == (1001,) and not s.any() and s.data_ptr() % 256 == 0
    assert g.bands()[1].numel() == 256 and g.bands()[1].data_ptr() == s.data_ptr() + 1001
    with pytest.raises(AssertionError):
        Guards("cpu", band=100)                              # would break the alignment


def test_untouched_registry_passes_and_writes_inside_do_not_count():
    g = Guards("cpu")
    g.check("empty")
    a = g.array((65, 3), torch.float32)
    b = g.array((1,), torch.int32, label="the count")
    a[:] = 7.0
    a.view(torch.uint8)[-1] = 0xFF                           # the array's own last byte
    b[0] = -1
    g.check("written inside only")
    assert g.dirty() == [] and len(g) == 2


@pytest.mark.parametrize("side,at", [("after", 0), ("before", 0), ("after", 4095), ("before", 4095), ("after", 8)])
def test_overrun_is_reported_with_label_side_and_offset(side, at):
    g = Guards("cpu")
    g.array((4,), torch.float32, label="bystander")
    g.array((63, 2), torch.int32, label="pairs")
    g.array((4,), torch.float32)
    whole, first, nbytes = bigger_view(g, 1)
    whole[first + nbytes + at if side == "after" else first - 1 - at] = 0x00
    assert g.dirty() == [("pairs int32 [63, 2]", side, [at])]
    with pytest.raises(AssertionError) as e:
        g.check("the emit")
    msg = str(e.value)
    assert "the emit" in msg and "pairs int32 [63, 2]" in msg and f"1 bytes {side}" in msg and f"[{at}]" in msg
    assert "bystander" not in msg


def test_a_record_past_the_end_is_reported_byte_by_byte():
    g = Guards("cpu")
    t = g.array((5, 2), torch.int32)                         # labelled by this line
    whole, first, nbytes = bigger_view(g)
    whole[first:first + nbytes + 8].view(torch.int32).view(6, 2)[5] = torch.tensor([3, 4], dtype=torch.int32)
    (label, side, at), = g.dirty()
    assert label.startswith("test_guards:") and label.endswith("int32 [5, 2]") and side == "after"
    assert at == [0, 1, 2, 3, 4, 5, 6, 7]
    assert not t.any()
    with pytest.raises(AssertionError, match="8 bytes after, first at offsets"):
        g.check()


def test_rewritten_names_the_arrays_that_lost_their_fill():
    g = Guards("cpu")
    a = g.array((1, 6), torch.float64, float("nan"), label="dist")
    b = g.array((1,), torch.int32, -1, label="hit")
    c = guards.guard_like(g, torch.arange(5), label="an input")
    g.array((0,), torch.int32, label="nothing")
    assert g.rewritten() == []
    c[2] = 77                                                # contents, not a fill: not looked at
    b[0] = 3
    assert g.rewritten() == ["hit int32 [1]"] and g.rewritten(start=2) == []
    b[0] = -1
    a[0, 5] = float("nan")                                   # the same bits: still pristine
    assert g.rewritten() == []
    a[0, 5] = 0.0
    assert g.rewritten() == ["dist float64 [1, 6]"]
    g.check("inside only")


def test_writing_the_poison_value_is_the_one_blind_spot():
    g = Guards("cpu")
    g.array((3,), torch.uint8)
    whole, first, nbytes = bigger_view(g)
    whole[first + nbytes] = 0xA5
    g.check("0xA5 over 0xA5 is invisible: the reason the value is not 0")


def test_hook_leaves_cpu_targets_and_everything_else_alone(monkeypatch):
    from clap_amd import _dev, physics, shard
    g = Guards("cpu")
    real_new = _dev._new
    guards.install(monkeypatch, g)
    assert _dev._new is not real_new and _dev._new.real is real_new
    guards.install(monkeypatch, g)
    assert _dev._new.real is real_new, "installing twice wraps once"
    assert physics.device_array is _dev.device_array and shard.upload is _dev.upload      # the mirrors' names are not patched
    z = physics.device_array((3, 2), torch.int32, "cpu")
    assert torch.equal(z, torch.zeros((3, 2), dtype=torch.int32))
    assert torch.equal(shard.device_array((2,), torch.int64, torch.device("cpu"), 7), torch.full((2,), 7))
    assert shard.device_array(4, torch.uint8, "cpu", fill=None).shape == (4,)
    up = physics.upload(np.arange(6, dtype=np.uint32), np.uint32, "cpu", (3, 2))
    assert up.dtype == torch.int32 and up.shape == (3, 2) and physics.upload(z, np.int32, "cpu") is z
    assert len(g) == 0, "nothing on the CPU goes through the registry"
    monkeypatch.undo()
    assert _dev._new is real_new


def test_hook_routes_a_gpu_target_through_the_registry(monkeypatch):
    """Without a GPU: the registry stands on the CPU and the hook is told that every target is its own."""
    from clap_amd import _dev, physics, shard
    g = Guards("cpu")
    guards.install(monkeypatch, g)
    monkeypatch.setattr(guards, "_on_gpu", lambda device: device is not None)
    made = []

    def once(t):                                             # each call lands in the registry exactly once
        made.append(t)
        assert len(g) == len(made) and g.owns(t) and g.entries[-1].view.data_ptr() == t.data_ptr()
        return t
    a = once(physics.device_array((65, 2), torch.int32, "cuda:0"))
    b = once(physics.device_array((3,), torch.float64, "cuda:0", -1.0))
    c = once(shard.device_array(a.shape, torch.uint8, "cuda:0", fill=None))
    d = once(physics.upload(np.arange(6, dtype=np.uint16) + 0xFFFD, np.uint16, "cuda:0", (3, 2)))
    e = once(physics.device_array(0, torch.float32, "cuda:0"))
    assert a.shape == (65, 2) and a.dtype == torch.int32 and not a.any()
    assert b.shape == (3,) and b.dtype == torch.float64 and (b == -1).all()
    assert c.shape == (65, 2) and c.dtype == torch.uint8
    assert d.shape == (3, 2) and d.dtype == torch.int16 and d.tolist() == [[-3, -2], [-1, 0], [1, 2]]      # the same bits
    assert e.shape == (0,) and e.dtype == torch.float32
    assert g.entries[0].label.startswith("test_guards:") and g.entries[3].label.startswith("test_guards:")
    assert all(t.data_ptr() % 256 == 0 for t in (a, b, c, d))
    assert not g.owns(a[1:]) and not g.owns(torch.zeros(3))
    g.check("fresh")
    whole, first, nbytes = bigger_view(g, 3)
    whole[first + nbytes] = 0
    assert [(s, at) for _l, s, at in g.dirty()] == [("after", [0])]
    monkeypatch.undo()
    assert getattr(_dev._new, "real", None) is None


# ------------------------------------------------------------------------------------------------------ the source rule
MIRRORS = ("physics", "entities", "animation", "particles", "lights", "characters", "frame", "shard")
FACTORIES = {f + like for f in ("zeros", "empty", "ones", "full") for like in ("", "_like")} | {
    "tensor", "as_tensor", "from_numpy", "frombuffer", "arange"}


def off_the_path(source, module):
    """["line: what"] for every place in a mirror's source that could make a device array without clap_amd._dev: a
    reference to a torch factory, or a call of a method .to() / .cuda().  Two things are let through, because they make
    nothing on a device:
      frame      torch.zeros(...).pin_memory(): the pinned host word the frame's clock is read from
      any module torch.from_numpy(...) directly as the argument of x.copy_(...): a host view copied into an existing array"""
    import ast
    tree = ast.parse(source)
    parent = {child: node for node in ast.walk(tree) for child in ast.iter_child_nodes(node)}
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.module == "torch":
            out += [f"{node.lineno}: from torch import {a.name}" for a in node.names if a.name in FACTORIES]
        if not isinstance(node, ast.Attribute):
            continue
        call = parent.get(node)
        called = isinstance(call, ast.Call) and call.func is node
        if isinstance(node.value, ast.Name) and node.value.id == "torch" and node.attr in FACTORIES:
            user = parent.get(call) if called else None
            pinned = (module == "frame" and node.attr == "zeros" and isinstance(user, ast.Attribute)
                      and user.attr == "pin_memory" and user.value is call)
            copied = (node.attr == "from_numpy" and isinstance(user, ast.Call) and call in user.args
                      and isinstance(user.func, ast.Attribute) and user.func.attr == "copy_")
            if not (pinned or copied):
                out.append(f"{node.lineno}: torch.{node.attr}")
        elif called and node.attr in ("to", "cuda"):
            out.append(f"{node.lineno}: .{node.attr}()")
    return out


def test_the_rule_sees_what_it_is_for():
    dev = "def f(dev, a, t):\n    return "
    for bad in ("torch.zeros(3, dtype=torch.int32, device=dev)", "torch.full_like(t, 1)", "torch.from_numpy(a).to(dev)",
                "t.cuda()", "torch.tensor([1], device=dev)", "torch.as_tensor(a, device=dev)", "make(torch.empty)",
                "torch.zeros(1).pin_memory()", "t.add_(torch.from_numpy(a))", "t.copy_(torch.from_numpy(a).to(dev))"):
        assert off_the_path(dev + bad, "physics"), bad
    assert off_the_path("from torch import zeros, float32", "physics") == ["1: from torch import zeros"]
    assert len(off_the_path(dev + "torch.from_numpy(a).to(dev)", "physics")) == 2
    for fine, module in (("torch.zeros(1, dtype=torch.float64).pin_memory()", "frame"), ("t.copy_(torch.from_numpy(a))", "lights"),
                         ("device_array(3, torch.int32, dev)", "physics"), ("upload(a, np.int32, dev)", "shard"),
                         ("t.cpu().numpy().tolist()", "physics"), ("torch.cat([t, t])", "shard")):
        assert off_the_path(dev + fine, module) == [], fine


@pytest.mark.parametrize("module", MIRRORS)
def test_mirrors_make_device_arrays_through_dev_only(module):
    """What keeps a future allocation site from leaving the guard silently: the mirrors have no other way to a device."""
    import os
    import clap_amd
    with open(os.path.join(os.path.dirname(clap_amd.__file__), module + ".py")) as f:
        assert off_the_path(f.read(), module) == [], f"clap_amd/{module}.py makes a tensor past _dev.device_array / upload"


def test_guarded_scratch_of_the_older_tests_is_the_same_instrument():
    from meshscene import guarded_scratch
    s, tail = guarded_scratch(1000, "cpu")
    assert s.shape == (1000,) and s.dtype == torch.uint8 and not s.any() and s.data_ptr() % 256 == 0
    assert tail.shape == (4096,) and (tail == 0xA5).all() and tail.data_ptr() == s.data_ptr() + 1000
    s, tail = guarded_scratch(8, "cpu", guard=256)
    assert tail.shape == (256,)
