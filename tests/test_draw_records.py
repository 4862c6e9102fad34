"""CPU: the draw records (include/clapgpu.h, "Draw records on the device", ABI 53) without a device -- the version, the
symbols, the record's layout as gcc makes it, the refusals the entry points owe before any HIP call, and the host twin
(clapgpu_draw_records_host: the kernels' own decision functions) against tests/drawref.py, the independent restatement of
_models_render's loop (core/model.c:784-1050), as bytes over the cases of tests/drawcases.py.

The records are UNPINNED: no trace of the reference's own _models_render is committed, so drawref stands alone as the
statement of the rule (README, DESIGN)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import drawcases as dc
import drawref
from clap_amd import _lib, draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("clapgpu_draw_records_scratch_bytes", "clapgpu_draw_records", "clapgpu_draw_records_host")
OFFSETS = dict(mx=0, inv_mx=64, color=128, bloom_intensity=144, bloom_threshold=148, edge_mode=152, color_pt=156, entity=160,
               lod=164, group=168, character=172, flags=176, zero=180)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


# ---- ABI ---------------------------------------------------------------------------------------------
def test_abi_version_symbols_and_exports(L):
    assert _lib.ABI_VERSION >= 53 and L.clapgpu_abi_version() == _lib.ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {l.split()[-1] for l in out.stdout.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "clapgpu.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name) and name in exported and name + "(" in header, name


def test_record_size_and_offsets_equal_gcc(tmp_path):
    prints = "".join(f'printf("%zu\\n", offsetof(clapgpu_draw_record, {n}));' for n in OFFSETS)
    prints += 'printf("%zu\\n", offsetof(clapgpu_frame, draw));'
    src, exe = tmp_path / "draw.c", tmp_path / "draw"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "clapgpu.h"\nint main(void) { '
                   'printf("%zu %d\\n", sizeof(clapgpu_draw_record), CLAPGPU_DRAW_RECORD_BYTES);' + prints + ' return 0; }\n')
    p = subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [[int(v) for v in l.split()] for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert rows[0] == [192, 192] and C.sizeof(_lib.DrawRecord) == 192 and draw.RECORD.itemsize == 192 and drawref.REC.itemsize == 192
    for (name, at), row in zip(OFFSETS.items(), rows[1:]):
        assert row == [at] and getattr(_lib.DrawRecord, name).offset == at and draw.RECORD.fields[name][1] == at, name
        assert drawref.REC.fields[name][1] == at, name
    assert rows[1 + len(OFFSETS)] == [_lib.FrameDesc.draw.offset]
    names = [f for f, _t in _lib.FrameDesc._fields_]                # in front of camera, behind view_visible_count
    assert names[-3:] == ["draw", "camera", "camera_bp"] and names[-4] == "view_visible_count"
    assert not _lib.FrameDesc().draw                                # zeroed: the frame as before


# ---- the twin against the restatement ----------------------------------------------------------------
@pytest.mark.parametrize("name", dc.NAMES)
def test_twin_equals_drawref_as_bytes(L, name):
    ref_bytes, count, first, status = dc.ref(name)
    rec, t_count, t_first, t_status = dc.twin(name)
    assert (t_count, t_status) == (count, status) and np.array_equal(t_first, first)
    assert rec[:count].tobytes() == ref_bytes
    assert not rec[count:].tobytes().strip(b"\0")                   # nothing behind the last record


def test_cases_cover_what_they_are_named_for(L):
    """The population the edge cases promise is really there, seen through drawref."""
    R = lambda name: (np.frombuffer(dc.ref(name)[0], drawref.REC),) + dc.ref(name)[1:]
    # the 16th drawn character of a txmodel gets 0 and the 17th gets 1; the ordinal restarts at every group
    c = dc.get("ordinals")
    rec, count, first, _s = R("ordinals")
    is_chr = (c.draw_flags[rec["entity"]] & dc.IS_CHARACTER) != 0
    for g, cnt in enumerate(c.counts):
        mine = rec[first[g]:first[g + 1]]
        chars = mine[is_chr[first[g]:first[g + 1]]]
        assert len(chars) == cnt and len(mine) > cnt               # drawn non-characters stand between them
        assert [int(e) & 15 for e in chars["edge_mode"]] == [(k + 1) & 15 for k in range(cnt)]
        assert all(int(e) & 15 == 0 for e in mine[~is_chr[first[g]:first[g + 1]]]["edge_mode"])
    assert np.all((R("ordinals-mq0")[0]["edge_mode"] & 15) == 0)
    assert set(np.unique(rec["edge_mode"] & 0x80)) == {0, 0x80}
    # bloom: every value of the list is drawn, both with and without render options; float(1e-3) is taken, the float below is not
    for name, has in (("plane-full", True), ("no-ropts-full", False)):
        c = dc.get(name)
        rec, _c, _f, _s = R(name)
        for field, bit in (("bloom_intensity", 1), ("bloom_threshold", 2)):
            src = getattr(c, field)[rec["entity"]]
            assert set(src.view(np.uint32)) == set(dc.BLOOMS.view(np.uint32))
            own = np.abs(src.astype(np.float64)) > 1e-3
            assert own[src == dc.F1].all() and not own[src == np.nextafter(dc.F1, np.float32(0))].any() and not own[np.isnan(src)].any()
            assert np.array_equal(rec[field][own], src.view(np.uint32)[own])
            assert np.all((rec["flags"][own] & bit) != 0)
            if has:
                assert np.all((rec["flags"] & bit) != 0) and np.all(rec[field][~own] == np.float32(c.ropts[bit - 1]).view(np.uint32))
            else:
                assert np.all((rec["flags"][~own] & bit) == 0) and np.all(rec[field][~own] == 0)
    # NaN payloads and denormals among the drawn words
    rec = R("plane-full-one-word")[0]
    assert set(dc.ODD_WORDS) <= set(rec["mx"][:, 0]) and set(dc.ODD_WORDS) <= set(rec["color"][:, 3])
    # groups: empty ones at the front, in the middle and at the end; one with nothing drawn; three in one word
    first = dc.ref("empty-groups")[2]
    assert first[0] == first[1] == first[2] == 0 and first[3] == first[4] == first[5] and first[-1] == first[-2] == first[-3]
    c, first = dc.get("group-with-nothing-drawn"), dc.ref("group-with-nothing-drawn")[2]
    assert len(c.groups[1]) == 100 and first[1] == first[2] and first[1] > 0 and first[3] > first[2]
    first = dc.ref("group-with-nothing-drawn-null-plane")[2]
    assert first[1] == 0 and first[2] > 0
    first = dc.ref("word-straddled-by-three-groups")[2]
    assert list(first[:4]) == [0, 70, 90, 100]                      # positions 64 .. 127 hold groups 0, 1, 2 and 3
    a, b = dc.ref("skip-shadow-in-shadow-pass"), dc.ref("skip-shadow-in-model-pass")
    assert a[2][1] == 0 and a[2][3] == a[2][2] and b[2][1] > 0 and b[2][3] > b[2][2] and a[1] < b[1]
    for p in ("empty", "full", "mixed", "null"):
        c, count = dc.get(f"plane-{p}"), dc.ref(f"plane-{p}")[1]
        assert (count == 0) if p == "empty" else (count == c.n_order) if p == "full" else (0 < count < c.n_order)


# ---- capacity and what the host cannot see -----------------------------------------------------------
@pytest.mark.parametrize("name", ("n1025-perm", "bounds-1-63-64-65-1024"))
def test_twin_capacity(L, name):
    ref_bytes, total, first, _s = dc.ref(name)
    for cap in (total, total - 1, 0):
        rec, count, t_first, status = dc.twin(name, cap, 0xA5)
        want = dc.ref(name, cap)
        assert (count, status) == (total, _lib.DRAW_CAPPED if cap < total else 0) == (want[1], want[3])
        assert np.array_equal(t_first, first) and rec.tobytes() == ref_bytes[:192 * cap] == want[0]
    rec, count, _f, status = dc.twin(name, total + 3, 0xA5)          # room to spare: nothing behind the last record
    assert (count, status) == (total, 0) and rec[total:].tobytes() == b"\xa5" * (3 * 192)


def invalid_orders(c):
    """(what, DrawOrder) for everything the host cannot see before a launch"""
    o = dc.order_of(c)
    bad = o.order.copy(); bad[c.n_order // 2] = c.n
    yield "order[r] = n", draw.DrawOrder(bad, o.group_start, o.group_flags)
    bad = o.order.copy(); bad[-1] = 0xffffffff
    yield "order[last] = 2^32 - 1", draw.DrawOrder(bad, o.group_start, o.group_flags)
    gs = o.group_start.copy(); gs[1], gs[2] = gs[2], gs[1]
    yield "a descending group_start", draw.DrawOrder(o.order, gs, o.group_flags)
    gs = o.group_start.copy(); gs[-1] -= 1
    yield "last group_start != n_order", draw.DrawOrder(o.order, gs, o.group_flags)
    gs = o.group_start.copy(); gs[-1] += 1
    yield "last group_start beyond n_order", draw.DrawOrder(o.order, gs, o.group_flags)
    gs = o.group_start.copy(); gs[0] = 1
    yield "group_start[0] != 0", draw.DrawOrder(o.order, gs, o.group_flags)


def test_twin_invalid_input_writes_the_verdict_alone(L):
    c = dc.get("bounds-1-63-64-65-1024")
    for what, o in invalid_orders(c):
        rec, count, first, status = draw.records_host(c.mx, c.inv_mx, o, dc.pass_of(c), c.n_order, flags=c.flags, plane=dc.plane_of(c),
                                                      lod=c.lod, inputs=c.input_arrays(), fill=0xA5)
        assert (count, status) == (0, _lib.DRAW_INVALID) and not first.any(), what
        assert rec.tobytes() == b"\xa5" * (192 * c.n_order), what


# ---- the refusals ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mem():
    raw = C.create_string_buffer(16384 + 256)
    at = (C.addressof(raw) + 255) & ~255

    def filled(cls):
        d = cls()
        for name, t in cls._fields_:
            if t is C.c_void_p:
                setattr(d, name, at)
        return d
    ent = filled(_lib.Entities)
    ent.n = 64
    order = filled(_lib.DrawOrder)
    order.n_order, order.n_groups = 64, 2
    views = _lib.Views()
    views.n = 2
    for v in range(2):
        views.vis_mask[v] = views.vis_row_pop[v] = at
    return dict(raw=raw, ok=at, ent=ent, order=order, inputs=filled(_lib.DrawInputs), views=views, dpass=draw.draw_pass())


def test_draw_records_refuses_before_any_hip_call(L, mem, monkeypatch):
    """No device exists here, and the launch check is set to fail: a call that got as far as a launch would return
    another code."""
    monkeypatch.setenv("CLAPGPU_TEST_HOOKS", "1")                # read by the library's first clapgpu_test_fail_after
    ok, bad = mem["ok"], _lib.ERR_INVALID_ARGUMENTS
    e, o, i, p = C.byref(mem["ent"]), C.byref(mem["order"]), C.byref(mem["inputs"]), C.byref(mem["dpass"])

    def call(ent=e, mask=ok, lod=ok, order=o, inputs=i, dpass=p, records=ok, capacity=8, count=ok, first=ok, status=ok, scratch=ok):
        return L.clapgpu_draw_records(None, ent, mask, lod, order, inputs, dpass, records, capacity, count, first, status, scratch)
    L.clapgpu_test_fail_after(0)
    try:
        assert call() != bad                                         # the launch check's own failure, not a refusal
        for kw in (dict(ent=None), dict(order=None), dict(dpass=None), dict(count=None), dict(first=None), dict(status=None),
                   dict(records=None), dict(records=ok + 16), dict(records=ok + 32), dict(scratch=None), dict(scratch=ok + 64),
                   dict(scratch=ok + 128)):
            assert call(**kw) == bad, kw
        assert call(records=None, capacity=0) != bad                 # counts and ranges only: legal
        for name in ("mx", "inv_mx"):
            ent = _lib.Entities.from_buffer_copy(mem["ent"])
            setattr(ent, name, None)
            assert call(ent=C.byref(ent)) == bad, name
            setattr(ent, name, ok + 4)
            assert call(ent=C.byref(ent)) == bad, name
        ent = _lib.Entities.from_buffer_copy(mem["ent"])
        ent.flags = None
        assert call(ent=C.byref(ent)) != bad                         # flags are read without a plane only
        assert call(ent=C.byref(ent), mask=None) == bad
        for name in ("order", "group_start", "group_flags"):
            od = _lib.DrawOrder.from_buffer_copy(mem["order"])
            setattr(od, name, None)
            assert call(order=C.byref(od)) == bad, name
        od = _lib.DrawOrder.from_buffer_copy(mem["order"])
        od.n_groups = 0                                              # positions and no txmodel
        assert call(order=C.byref(od)) == bad
        ind = _lib.DrawInputs.from_buffer_copy(mem["inputs"])
        ind.color = ok + 4
        assert call(inputs=C.byref(ind)) == bad
        assert call(inputs=None, lod=None, mask=None) != bad         # every optional input absent
    finally:
        L.clapgpu_test_fail_after(-1)
    # the twin returns without writing where the device call refuses
    count = np.array([0xdead], np.uint32)
    L.clapgpu_draw_records_host(e, ok, ok, None, i, p, ok, 8, count.ctypes.data, ok, ok)
    assert count[0] == 0xdead


def test_frame_refuses_draw_before_any_launch(L, mem, monkeypatch):
    monkeypatch.setenv("CLAPGPU_TEST_HOOKS", "1")
    ok, bad = mem["ok"], _lib.ERR_INVALID_ARGUMENTS

    def issue(main_view=True, order=True, scratch=ok, main=True, view=None, views=True, records=ok, capacity=4, **block):
        ent = _lib.Entities.from_buffer_copy(mem["ent"])
        v = _lib.Views.from_buffer_copy(mem["views"])
        ent.views = C.pointer(v) if views else None
        f = _lib.FrameDesc()
        f.entities = C.pointer(ent)
        if main_view:                                                # the view block: its clapgpu_views_calc is the first launch
            f.views_source = f.views_state = ok
        f.visible_scratch = ok
        d = _lib.FrameDraw()
        if order:
            d.order = C.pointer(mem["order"])
        d.scratch = scratch
        blk = _lib.FrameDrawPass(mem["dpass"], capacity, records, block.get("count", ok), block.get("group_first", ok),
                                 block.get("status", ok))
        if main:
            d.main = blk
        if view is not None:
            d.view[view] = blk
        f.draw = C.pointer(d)
        return L.clapgpu_frame_issue(None, C.byref(f), 0.0, 0)
    L.clapgpu_test_fail_after(0)
    try:
        assert issue() != bad                                        # the launch check's own failure, not a refusal
        assert issue(records=None, capacity=0) != bad                # counts and ranges only
        assert issue(main_view=False) == bad                         # no main view
        assert issue(order=False) == bad
        assert issue(scratch=None) == bad and issue(scratch=ok + 16) == bad
        assert issue(records=None) == bad and issue(records=ok + 16) == bad
        assert issue(group_first=None) == bad and issue(status=None) == bad
        assert issue(main=False, view=2) == bad                      # v >= entities->views->n
        assert issue(main=False, view=0, views=False) == bad
        assert issue(main=False, view=1, status=None) == bad
        assert issue(main=False, view=1) != bad
    finally:
        L.clapgpu_test_fail_after(-1)
