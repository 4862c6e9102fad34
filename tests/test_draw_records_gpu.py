"""GPU: clapgpu_draw_records (include/clapgpu.h, "Draw records on the device", ABI 53) AS BYTES against its host twin --
records, count, group_first and status -- over the cases of tests/drawcases.py (tests/test_draw_records.py holds the twin
to the independent restatement tests/drawref.py on the CPU): every size around the kernels' 64-position words and
the 1 024 positions of sixteen words, three orders, four planes, group cuts at every edge, the character ordinals, the bloom values,
NaN words; capacity and invalid input leave what they must untouched; and the frame -- with `draw` it is the frame
without it followed by the calls in pieces, the further views' records carry the LODs the previous frame left, without
the field it is the frame before, and a graph captured once follows its camera.  Every array of the mirrors lies
between the guard bands of tests/guards.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from clap_amd import _dev, _lib, draw, entities, frame, synth
import drawcases as dc
import guards
import spotscases as sc

pytestmark = pytest.mark.gpu
FILL = 0x5A5A5A5A                                               # what the record buffer holds before a call


def as_bytes(a):
    return np.ascontiguousarray(np.atleast_1d(a)).view(np.uint8).reshape(-1)


@pytest.fixture
def g(cuda_device, monkeypatch):
    reg = guards.Guards(cuda_device)
    guards.install(monkeypatch, reg)
    yield reg
    reg.check("at the end of the test")


def outputs(capacity, n_groups, dev):
    out = draw.DrawOutputs(capacity, n_groups, dev)
    if out.records is not None:
        out.records.fill_(FILL)
    out.count.fill_(0xdead), out.status.fill_(0xdead), out.group_first.fill_(0xdead)
    return out


def whole_buffer(out):
    """(the WHOLE record buffer, count, group_first, status)"""
    torch.cuda.synchronize()
    rec = np.zeros(0, draw.RECORD) if out.records is None else out.records.cpu().numpy().view(np.uint8).reshape(-1).view(draw.RECORD)
    return (rec, int(out.count.cpu().numpy().view(np.uint32)[0]), out.group_first.cpu().numpy().view(np.uint32),
            int(out.status.cpu().numpy().view(np.uint32)[0]))


def run_device(dev, c, capacity=None, order=None):
    """clapgpu_draw_records over a case uploaded into guarded arrays"""
    up = _dev.upload
    cap = c.n_order if capacity is None else capacity
    keep = dict(mx=up(c.mx, np.float32, dev), inv=up(c.inv_mx, np.float32, dev), flags=up(c.flags, np.uint32, dev))
    plane = dc.plane_of(c)
    keep["plane"] = None if plane is None else up(plane.view(np.int64), np.int64, dev)
    keep["lod"] = None if c.lod is None else up(c.lod, np.int32, dev)
    e = _lib.Entities()
    e.n, e.mx, e.inv_mx, e.flags = c.n, keep["mx"].data_ptr(), keep["inv"].data_ptr(), keep["flags"].data_ptr()
    o = (order or dc.order_of(c)).to(dev)
    inputs = None if c.input_arrays() is None else draw.DrawInputs(dev, **c.input_arrays())
    out = outputs(cap, o.n_groups, dev)
    scratch = draw.scratch_for(o)
    p = dc.pass_of(c)
    rc = _lib.lib().clapgpu_draw_records(_dev.stream(), C.byref(e), _dev.ptr(keep["plane"]) or None, _dev.ptr(keep["lod"]) or None,
                                         C.byref(o.desc), C.byref(inputs.desc) if inputs is not None else None, C.byref(p),
                                         _dev.ptr(out.records) or None, cap, out.count.data_ptr(), out.group_first.data_ptr(),
                                         out.status.data_ptr(), scratch.data_ptr())
    _lib.check(rc, "clapgpu_draw_records")
    return whole_buffer(out)


def assert_same(got, want, what, fill_behind=True):
    rec, count, first, status = got
    w_rec, w_count, w_first, w_status = want
    assert (count, status) == (w_count, w_status), f"{what}: count {count} status {status}, the twin's {w_count} {w_status}"
    assert np.array_equal(first, w_first), f"{what}: group_first"
    k = min(count, len(rec))
    assert rec[:k].tobytes() == w_rec[:k].tobytes(), f"{what}: the records"
    if fill_behind:
        assert np.all(rec[k:].view(np.uint32) == FILL), f"{what}: written at or past the count"


# ------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("name", dc.NAMES)
def test_kernels_equal_the_host_twin_as_bytes(cuda_device, g, name):
    c = dc.get(name)
    assert_same(run_device(cuda_device, c), dc.twin(name), name)
    g.check(name)


@pytest.mark.parametrize("name", ("n1025-perm", "bounds-1-63-64-65-1024", "n64-identity"))
def test_capacity(cuda_device, g, name):
    c = dc.get(name)
    total = dc.twin(name)[1]
    for cap in (total, total - 1, 0, total + 3):
        got = run_device(cuda_device, c, cap)
        assert_same(got, dc.twin(name, cap), f"{name}, capacity {cap}")
        assert got[3] == (_lib.DRAW_CAPPED if cap < total else 0) and got[1] == total
        g.check(f"{name}, capacity {cap}")                          # no write past capacity


def test_invalid_input_writes_the_verdict_alone(cuda_device, g):
    from test_draw_records import invalid_orders
    c = dc.get("bounds-1-63-64-65-1024")
    for what, o in invalid_orders(c):
        rec, count, first, status = run_device(cuda_device, c, order=o)
        assert (count, status) == (0, _lib.DRAW_INVALID) and not first.any(), what
        assert np.all(rec.view(np.uint32) == FILL), what
    assert_same(run_device(cuda_device, c), dc.twin("bounds-1-63-64-65-1024"), "the valid order behind them")


def test_nothing_to_draw_still_writes_the_outputs(cuda_device, g):
    c = dc.get("n65-perm")
    empty = draw.DrawOrder.from_groups([[], []])
    rec, count, first, status = run_device(cuda_device, c, capacity=4, order=empty)
    assert (count, status) == (0, 0) and list(first) == [0, 0, 0] and np.all(rec.view(np.uint32) == FILL)
    none = draw.DrawOrder.from_groups([])                           # no txmodel at all
    rec, count, first, status = run_device(cuda_device, c, capacity=4, order=none)
    assert (count, status) == (0, 0) and list(first) == [0]


# ------------------------------------------------------------------------------------------------- the frame
def frame_draw(dev, batch, seed=3, capacity=None):
    """the draw field over a frame's batch: a seeded render order of its living entities in seven txmodels (one empty, one
    with skip_shadow), every per-entity input, a model pass and the shadow pass of further view 0"""
    n = batch.n
    flags = batch.flags.cpu().numpy().view(np.uint32)
    alive = np.flatnonzero(flags & _lib.E_ALIVE).astype(np.uint32)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(alive)
    cuts = sorted(rng.choice(len(perm), 5, replace=False))
    at = [0] + cuts[:2] + [cuts[2], cuts[2]] + cuts[3:] + [len(perm)]
    groups = [perm[a:b] for a, b in zip(at[:-1], at[1:])]
    order = draw.DrawOrder.from_groups(groups, skip_shadow=[False, True, False, False, False, False, False], device=dev)
    vals = dc.case(n_order=64, n=n, seed=seed)                      # per-entity values of n entities
    inputs = draw.DrawInputs(dev, **vals.input_arrays())
    cap = len(perm) if capacity is None else capacity
    main, shadow = outputs(cap, order.n_groups, dev), outputs(cap, order.n_groups, dev)
    fd = draw.FrameDraw(order, inputs, main=(main, draw.draw_pass(False, (0.5, 0.25), 3)),
                        views=[(shadow, draw.draw_pass(True, None, 3))])
    return fd


def twin_of(batch, fd, which, lod):
    """the host twin over what the device holds: the frame's own mx / inv_mx / flags / plane, and `lod`"""
    torch.cuda.synchronize()
    out, p = fd.main if which == "main" else fd.views[0]
    mask = batch.vis_mask if which == "main" else batch.view_masks[0]
    inp = {k: fd.inputs[k].cpu().numpy() for k, _dt in draw.INPUT_KEYS}
    return draw.records_host(batch.mx.cpu().numpy(), batch.inv_mx.cpu().numpy(), fd.order, p, out.capacity,
                             flags=batch.flags.cpu().numpy().view(np.uint32), plane=mask.cpu().numpy().view(np.uint64),
                             lod=np.ascontiguousarray(lod), inputs=inp)


def setup_frame(dev, with_draw):
    import test_cascades_gpu as tc
    loop, p = tc.frame_setup(dev, cascades=False, camera=False)
    fd = frame_draw(dev, p["batch"])
    if with_draw:
        loop.draw, loop._desc = fd, None
    return loop, dict(p, fd=fd)


def records_state(fd):
    a, b = whole_buffer(fd.main[0]), whole_buffer(fd.views[0][0])
    return dict(main_rec=as_bytes(a[0]), main_count=np.asarray([a[1], a[3]]), main_first=a[2], shadow_rec=as_bytes(b[0]),
                shadow_count=np.asarray([b[1], b[3]]), shadow_first=b[2])


@pytest.mark.parametrize("overlap", [False, True], ids=["one_stream", "overlap"])
def test_frame_with_draw_is_the_frame_in_pieces(cuda_device, g, overlap):
    """the pieces: the shadow pass's call with the cur_lod the frame found (its records are issued ahead of the LOD pick)
    and the plane the frame left, the model pass's with the cur_lod the frame left"""
    import test_cascades_gpu as tc
    dt = 1.0 / 120.0
    whole, pw = setup_frame(cuda_device, True)
    parts, pp = setup_frame(cuda_device, False)
    whole.overlap = parts.overlap = overlap
    for f in range(1, 4):
        whole.set_camera(synth.camera(pos=(0, 10, 60 + 40 * f))), parts.set_camera(synth.camera(pos=(0, 10, 60 + 40 * f)))
        batch, fd = pp["batch"], pp["fd"]
        batch.alloc_lod()
        before = batch.cur_lod.clone()
        whole.clap_frame(f * dt, dt)
        parts.clap_frame(f * dt, dt)
        draw.records(batch, fd.order, fd.views[0][0], fd.views[0][1], fd.inputs, plane=batch.view_masks[0], lod=before, scratch=fd.scratch)
        draw.records(batch, fd.order, fd.main[0], fd.main[1], fd.inputs, plane="main", lod=batch.cur_lod, scratch=fd.scratch)
        tc.assert_same_state(tc.frame_state(pw), tc.frame_state(pp), f"frame {f}")
        a, b = records_state(pw["fd"]), records_state(pp["fd"])
        tc.assert_same_state(a, b, f"frame {f}: the records")
        assert a["main_count"][1] == 0 and a["shadow_count"][1] == 0
        assert_same(whole_buffer(pw["fd"].main[0]), twin_of(pw["batch"], pw["fd"], "main", pw["batch"].cur_lod.cpu().numpy()),
                    f"frame {f}: the model pass against the twin", fill_behind=False)
    assert 0 < a["main_count"][0] < pw["fd"].order.n_order and 0 < a["shadow_count"][0]
    first = a["shadow_first"]
    assert first[1] == first[2]                                     # the skip_shadow txmodel draws nothing in the shadow pass
    assert a["main_first"][2] > a["main_first"][1]                  # ... and draws in the model pass


def test_shadow_records_carry_the_previous_frames_lods(cuda_device, g):
    """pipeline_render runs the shadow passes ahead of the model pass: their draws see the cur_lod the last model pass left
    (model.c:975), the model pass's see this frame's.  Two frames with the camera moved far enough that LODs change."""
    dt = 1.0 / 120.0
    loop, p = setup_frame(cuda_device, True)
    batch, fd = p["batch"], p["fd"]
    loop.clap_frame(dt, dt)
    torch.cuda.synchronize()
    lod1 = batch.cur_lod.cpu().numpy().copy()
    loop.set_camera(synth.camera(pos=(0, 10, 400)))
    loop.clap_frame(2 * dt, dt)
    torch.cuda.synchronize()
    lod2 = batch.cur_lod.cpu().numpy().copy()
    main, shadow = fd.main[0].download()[0], fd.views[0][0].download()[0]
    assert len(main) and len(shadow)
    assert np.array_equal(main["lod"], lod2[main["entity"]]), "the model pass draws with this frame's LODs"
    assert np.array_equal(shadow["lod"], lod1[shadow["entity"]]), "a shadow pass draws with the LODs the last model pass left"
    both = np.intersect1d(main["entity"], shadow["entity"])
    assert (lod1[both] != lod2[both]).any(), "the camera moved far enough that a LOD drawn by both passes changed"
    assert_same(whole_buffer(fd.views[0][0]), twin_of(batch, fd, "shadow", lod1), "the shadow pass against the twin", fill_behind=False)
    assert_same(whole_buffer(fd.main[0]), twin_of(batch, fd, "main", lod2), "the model pass against the twin", fill_behind=False)


def test_frame_without_draw_is_the_frame_before(cuda_device, g):
    """draw NULL: the same arrays as a FrameLoop that never heard of it (the launches are compared by what they leave)"""
    import test_cascades_gpu as tc
    dt = 1.0 / 120.0
    a, pa = setup_frame(cuda_device, True)
    f = a._build()
    assert f.draw
    f.draw = None                                                   # built with it, then only the new field taken out
    b, pb = setup_frame(cuda_device, False)
    assert not b._build().draw
    for fr in range(1, 4):
        a.clap_frame(fr * dt, dt)
        b.clap_frame(fr * dt, dt)
        tc.assert_same_state(tc.frame_state(pa), tc.frame_state(pb), f"frame {fr}")
    for out in (pa["fd"].main[0], pa["fd"].views[0][0]):            # never written
        rec, count, first, status = whole_buffer(out)
        assert np.all(rec.view(np.uint32) == FILL) and count == status == 0xdead and np.all(first == 0xdead)


def ring_camera(k):
    """the camera at the ring's centre, turned k * 0.7 rad about Y"""
    return synth.camera(pos=(0, 0, 0), quat=tuple(float(v) for v in sc.ring_quat(k)))


def test_captured_graph_follows_its_camera(cuda_device, g):
    """six replays of a frame captured once while the camera turns 0.7 rad a replay at the centre of the ring; after every
    replay the records equal the twin's over the plane that camera leaves, and the drawn sets differ pairwise"""
    dt = 1.0 / 120.0
    batch = entities.EntityBatch(sc.ring_scene(), cuda_device)
    n = batch.n
    rng = np.random.default_rng(9)
    perm = rng.permutation(n).astype(np.uint32)
    order = draw.DrawOrder.from_groups([perm[:100], perm[100:101], perm[101:]], device=cuda_device)
    vals = dc.case(n_order=64, n=n, seed=9)
    inputs = draw.DrawInputs(cuda_device, **vals.input_arrays())
    fd = draw.FrameDraw(order, inputs, main=(outputs(n, 3, cuda_device), draw.draw_pass(False, (0.5, 0.25), 3)))
    loop = frame.FrameLoop(batch, ring_camera(0), views_dev=True, draw=fd)
    loop.capture(dt, warmup_now=0.0)
    seen = []
    for k in range(1, sc.RING_REPLAYS + 1):
        loop.set_camera(ring_camera(k))
        loop.clap_frame_replay(k * dt)
        got = whole_buffer(fd.main[0])
        assert_same(got, twin_of(batch, fd, "main", batch.cur_lod.cpu().numpy()), f"replay {k}", fill_behind=False)
        drawn = np.sort(got[0][:got[1]]["entity"])
        ring = drawn[drawn < sc.RING_N]
        print("replay", k, "ring entities drawn:", len(ring))
        assert got[3] == 0 and 0 < len(ring) < sc.RING_N
        seen.append(ring)
    assert all(not np.array_equal(x, y) for i, x in enumerate(seen) for y in seen[i + 1:])
    g.check("the ring")
