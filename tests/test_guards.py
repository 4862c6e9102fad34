"""tests/guards.py, the guard-band instrument of test_extents_gpu.py, on the CPU: what it hands out, what it reports, and
that the proxy changes nothing but where GPU factories allocate."""
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


def test_proxy_leaves_cpu_factories_and_everything_else_alone(monkeypatch):
    from clap_amd import _dev, entities, physics, shard, frame
    g = Guards("cpu")
    real_upload = physics.upload
    proxy = guards.install(monkeypatch, g)
    for mod in (entities, physics, shard, frame):
        assert mod.torch is proxy and mod.torch is not torch
    import clap_amd.animation as animation
    assert animation.torch is proxy and _dev.torch is torch              # _dev is not a mirror; torch itself is untouched
    z = physics.torch.zeros((3, 2), dtype=torch.int32, device="cpu")
    assert torch.equal(z, torch.zeros((3, 2), dtype=torch.int32)) and len(g) == 0
    assert torch.equal(physics.torch.zeros(2, 3), torch.zeros(2, 3))
    assert torch.equal(physics.torch.full((2,), 7, dtype=torch.int64, device=torch.device("cpu")), torch.full((2,), 7))
    assert physics.torch.empty(4, dtype=torch.uint8).shape == (4,)
    assert torch.equal(physics.torch.ones(2, dtype=torch.float64), torch.ones(2, dtype=torch.float64))
    assert torch.equal(shard.torch.zeros_like(z), z) and torch.equal(shard.torch.full_like(z, 3), torch.full_like(z, 3))
    assert torch.equal(shard.torch.ones_like(z), torch.ones_like(z)) and shard.torch.empty_like(z).shape == z.shape
    assert frame.torch.zeros(1, dtype=torch.float64, pin_memory=False).dtype == torch.float64
    assert len(g) == 0, "nothing on the CPU goes through the registry"
    for name in ("Tensor", "float32", "from_numpy", "cuda", "device", "is_tensor", "as_tensor", "uint8", "distributed", "cat"):
        assert getattr(entities.torch, name) is getattr(torch, name), name
    up = physics.upload(np.arange(6, dtype=np.uint32), np.uint32, "cpu", (3, 2))
    assert up.dtype == torch.int32 and up.shape == (3, 2) and len(g) == 0
    assert physics.upload is not real_upload and physics.upload(z, np.int32, "cpu") is z
    monkeypatch.undo()
    assert physics.torch is torch and physics.upload is real_upload


def test_proxy_routes_a_gpu_target_through_the_registry(monkeypatch):
    """Without a GPU: the registry stands on the CPU and the proxy is told that "cuda" targets are its own."""
    from clap_amd import physics, shard
    g = Guards("cpu")
    guards.install(monkeypatch, g)
    monkeypatch.setattr(guards, "_on_gpu", lambda device: device is not None)
    a = physics.torch.zeros((65, 2), dtype=torch.int32, device="cuda:0")
    b = physics.torch.full((3,), -1.0, dtype=torch.float64, device="cuda:0")
    c = shard.torch.zeros_like(a)
    d = physics.upload(np.arange(5, dtype=np.uint16), np.uint16, "cuda:0")
    e = physics.torch.zeros(0, dtype=torch.float32, device="cuda:0")
    assert len(g) == 5 and a.shape == (65, 2) and not a.any() and (b == -1).all() and c.shape == a.shape and c.dtype == a.dtype
    assert d.dtype == torch.int16 and d.tolist() == [0, 1, 2, 3, 4] and e.shape == (0,)
    assert g.entries[0].label.startswith("test_guards:") and all(t.data_ptr() % 256 == 0 for t in (a, b, c, d))
    g.check("fresh")
    with pytest.raises(AssertionError, match="pin_memory"):  # a GPU site the proxy could not guard is refused, not passed on
        physics.torch.zeros(4, dtype=torch.int32, device="cuda:0", pin_memory=False)
    with pytest.raises(AssertionError, match="requires_grad"):
        shard.torch.zeros_like(a, requires_grad=False)
    whole, first, nbytes = bigger_view(g, 3)
    whole[first + nbytes] = 0
    assert [(s, at) for _l, s, at in g.dirty()] == [("after", [0])]


def test_guarded_scratch_of_the_older_tests_is_the_same_instrument():
    from meshscene import guarded_scratch
    s, tail = guarded_scratch(1000, "cpu")
    assert s.shape == (1000,) and s.dtype == torch.uint8 and not s.any() and s.data_ptr() % 256 == 0
    assert tail.shape == (4096,) and (tail == 0xA5).all() and tail.data_ptr() == s.data_ptr() + 1000
    s, tail = guarded_scratch(8, "cpu", guard=256)
    assert tail.shape == (256,)
