"""GPU: clapgpu_skin_drawn -- skinning that follows the cull and the LOD -- against oracle.skin with the same palette in and
the rule as tests/skinselref.py restates it from the header.

Every case asserts: the selected (character, vertex) elements are bit-equal to the oracle's (out_w included when on);
every other element of the outputs still holds the sentinel the test filled in; skinned, chars, count and status equal
the reference; nothing was written outside any device array (tests/guards.py).  The fixtures are tests/skinselcases.py,
held to their own properties on the CPU by tests/test_skin_drawn.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import guards
import skinselcases as cases
import skinselref as ref
from clap_amd import _lib, animation, synth
from helpers import assert_bits_equal
from oracle import binding as ob

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
_MODELS = {}


def parts(J, n_verts, seed=3):
    """skeleton, animation and mesh of a case (host side, made once per shape)"""
    key = (J, n_verts, seed)
    if key not in _MODELS:
        sk = synth.skeleton(J, min(8, J), seed=seed)
        sk["bind"] = ob.skeleton_bind(sk)
        _MODELS[key] = (sk, synth.animation(J, 12, 2.0, seed=seed), synth.skinned_mesh(n_verts, J, seed=seed))
    return _MODELS[key]


def make_batch(c, device, w=False):
    sk, an, mesh = parts(c["J"], c["n_verts"])
    ch = synth.characters(c["n"], c["J"], seed=3)
    model = animation.SkinnedModel(sk, [an], mesh=mesh, bind=sk["bind"], device=device)
    batch = animation.CharacterBatch(model, c["n"], ch["trs0"], ch["char_mx"], vert_first=c["vert_first"], vert_count=c["vert_count"])
    batch.set_frame_times(ch["phase"])
    batch.pose_update()
    if w:
        batch.set_skin_w(True)
    return batch, mesh


def select_args(c, planes=None):
    lists = None if c["lod_first"] is None else (c["lod_first"], c["lod_count"], c["list"])
    return dict(planes=c["planes"] if planes is None else planes, cur_lod=c["cur_lod"], entity=c["entity"], row=c["row"],
                lod_lists=lists, n_entities=c["n_entities"])


def fill(batch):
    for t in (batch.out_position, batch.out_normal, batch.out_w):
        if t is not None:
            t.fill_(SENTINEL)


def expected(batch, mesh, c, w):
    jt = batch.joint_transforms.cpu().numpy()
    return ob.skin(mesh, c["vert_first"], c["vert_count"], jt, with_w=True) if w else ob.skin(mesh, c["vert_first"], c["vert_count"], jt)


def assert_follows_the_rule(out, exp, sel, batch, what):
    """out: batch.download(); exp: the oracle's whole outputs; sel: skinselref.select's answer"""
    m = ref.written_mask(sel, batch.out_first_host[:-1], batch.n_out_verts)
    names = ("out_position", "out_normal") + (("out_w",) if len(exp) == 3 else ())
    for k, e in zip(names, exp):
        got = out[k]
        assert_bits_equal(got[m], e[m], f"{what}: {k} of the selected vertices")
        assert (got[~m] == SENTINEL).all(), f"{what}: {k} written outside the selection"
    assert out["count"] == sel["count"], what
    assert np.array_equal(out["chars"], sel["chars"]), what
    assert np.array_equal(out["skinned"], sel["skinned"]), what
    assert out["status"] == sel["status"], what


def run_case(c, device, monkeypatch, what, w=False):
    g = guards.Guards(device)
    guards.install(monkeypatch, g)
    batch, mesh = make_batch(c, device, w)
    batch.set_skin_select(**select_args(c))
    fill(batch)
    batch.skin_drawn()
    out = batch.download()
    sel = ref.select(**cases.ref_args(c))
    assert_follows_the_rule(out, expected(batch, mesh, c, w), sel, batch, what)
    g.check(what)
    return batch, out, sel


# ------------------------------------------------------------------------------------------------- (a) character counts
@pytest.mark.parametrize("n", cases.COUNTS)
def test_character_counts(n, cuda_device, monkeypatch):
    _b, out, sel = run_case(cases.counts(n), cuda_device, monkeypatch, f"{n} characters")
    assert sel["count"] >= 1


# ------------------------------------------------------------------------------------------------- (b) planes
@pytest.mark.parametrize("with_entity", [True, False], ids=["entity_list", "entity_null"])
def test_five_planes(with_entity, cuda_device, monkeypatch):
    _b, out, _sel = run_case(cases.planes(with_entity), cuda_device, monkeypatch, "five planes", w=with_entity)
    assert out["skinned"][5] != _lib.SKIN_NOT_DRAWN and out["skinned"][6] == _lib.SKIN_NOT_DRAWN


# ------------------------------------------------------------------------------------------------- (c) LOD lists
@pytest.mark.parametrize("with_tables", [True, False], ids=["three_rows", "no_rows"])
def test_lod_lists(with_tables, cuda_device, monkeypatch):
    run_case(cases.lod_lists(with_tables), cuda_device, monkeypatch, "ragged meshes", w=with_tables)


# ------------------------------------------------------------------------------------------------- (d) joint counts
@pytest.mark.parametrize("J", [1, 200])
def test_joint_counts(J, cuda_device, monkeypatch):
    run_case(cases.joints(J), cuda_device, monkeypatch, f"{J} joints")


# ------------------------------------------------------------------------------------------------- (e) the range bits
@pytest.mark.parametrize("which,bit", [("entity", _lib.SKINSEL_ENTITY_RANGE), ("lod", _lib.SKINSEL_LOD_RANGE),
                                       ("list", _lib.SKINSEL_LIST_RANGE)])
def test_range_bits(which, bit, cuda_device, monkeypatch):
    batch, out, _sel = run_case(cases.range_bit(which), cuda_device, monkeypatch, f"{which} out of range")
    assert out["status"] == bit
    batch.skin_drawn()                                          # sticky: a second call leaves the bit
    assert batch.download()["status"] == bit


# ------------------------------------------------------------------------------------------------- (f) the plain call
def test_everything_drawn_without_tables_is_the_plain_call(cuda_device, monkeypatch):
    c = cases.plain()
    batch, out, _sel = run_case(c, cuda_device, monkeypatch, "plain")
    fill(batch)
    batch.skin()
    plain = batch.download()
    assert_bits_equal(out["out_position"], plain["out_position"], "positions: skin_drawn vs skin")
    assert_bits_equal(out["out_normal"], plain["out_normal"], "normals: skin_drawn vs skin")
    assert np.array_equal(out["chars"], np.arange(c["n"])) and (out["skinned"] == 0).all()


# ------------------------------------------------------------------------------------------------- (g) a captured graph
def test_captured_graph_follows_the_planes(cuda_device, monkeypatch):
    c, second = cases.graph_planes()
    g = guards.Guards(cuda_device)
    guards.install(monkeypatch, g)
    batch, mesh = make_batch(c, cuda_device)
    batch.set_skin_select(**select_args(c))
    plane = batch._sel_planes[0]
    first_words = plane.clone()
    second_words = torch.from_numpy(second.view(np.int64)).to(plane.device)
    exp = expected(batch, mesh, c, False)
    batch.skin_drawn()                                          # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        batch.skin_drawn()                                      # three launches on one stream: a linear graph
    for words, planes in ((first_words, c["planes"]), (second_words, [second]), (first_words, c["planes"])):
        plane.copy_(words)
        fill(batch)
        graph.replay()
        sel = ref.select(**{**cases.ref_args(c), "planes": planes})
        assert_follows_the_rule(batch.download(), exp, sel, batch, "replay")
    g.check("graph")


# ------------------------------------------------------------------------------------------------- (h) the frame
def build_frame(device, skin_select, overlap=False):
    from clap_amd import entities, frame
    scene, cam, light, ent, lists = cases.frame_scene()
    batch = entities.EntityBatch(scene, device)
    batch.set_views([entities.view_calc_frustum(light)[0]])
    nc, J, vpc = cases.FRAME_CHARS, cases.FRAME_J, cases.FRAME_VPC
    sk, an, mesh = parts(J, vpc, seed=12)
    ch = synth.characters(nc, J, seed=12)
    model = animation.SkinnedModel(sk, [an], mesh=mesh, bind=sk["bind"], device=device)
    cb = animation.CharacterBatch(model, nc, ch["trs0"], batch.mx, entity_index=ent)
    cb.start_clock(ani_time=np.zeros(nc), speed=np.ones(nc, np.float32))
    loop = frame.FrameLoop(batch, cam, characters=cb, pose_readers=(),
                           skin_select=dict(lod_lists=lists) if skin_select else None)
    loop.overlap = overlap
    return loop, ent, lists, mesh


@pytest.mark.parametrize("overlap", [False, True], ids=["one_stream", "three_chains"])
def test_frame_skins_what_it_draws(overlap, cuda_device):
    plain, ent, lists, mesh = build_frame(cuda_device, False, overlap)
    drawn, _e, _l, _m = build_frame(cuda_device, True, overlap)
    for loop in (plain, drawn):
        loop.characters.out_position.fill_(SENTINEL)
        loop.characters.out_normal.fill_(SENTINEL)
    dt = 1.0 / 60.0
    for f in range(1, 3):
        plain.clap_frame(f * dt, dt)
        drawn.clap_frame(f * dt, dt)
    torch.cuda.synchronize()
    a, b = plain.characters.download(), drawn.characters.download()
    ea, eb = plain.batch.download(), drawn.batch.download()
    for k in ea:                                                # every other output of the frame is identical
        assert np.array_equal(ea[k], eb[k]), k
    for k in ("trs", "joint_transforms", "joint_pos"):
        assert np.array_equal(a[k], b[k]), k
    n_vis = len(ea["visible"])
    assert np.array_equal(plain.batch.draw_lod[:n_vis].cpu().numpy(), drawn.batch.draw_lod[:n_vis].cpu().numpy())
    assert np.array_equal(plain.batch.cur_lod.cpu().numpy(), drawn.batch.cur_lod.cpu().numpy())
    # the rule over what the frame left on the device: its own planes and the LODs it just picked
    cb = drawn.characters
    planes = [ea["vis_mask"], drawn.batch.view_masks[0].cpu().numpy().view(np.uint64)]
    cur_lod = drawn.batch.cur_lod.cpu().numpy()
    sel = ref.select(cb.n, cb.vert_count_host, planes, drawn.batch.n, entity=ent, cur_lod=cur_lod, n_lods=4, lod_first=lists[0],
                     lod_count=lists[1], lst=lists[2])
    assert 0.2 * cb.n <= sel["count"] <= 0.8 * cb.n, f"{sel['count']} of {cb.n} characters drawn"
    assert set(sel["skinned"][sel["chars"]]) == {0, 1, 2, 3}
    main_only = ref.select(cb.n, cb.vert_count_host, planes[:1], drawn.batch.n, entity=ent)
    assert sel["count"] > main_only["count"], "a character drawn in the light's view only"
    m = ref.written_mask(sel, cb.out_first_host[:-1], cb.n_out_verts)
    for k in ("out_position", "out_normal"):
        assert_bits_equal(b[k][m], a[k][m], f"{k}: the two frames on the selected vertices")
        assert (b[k][~m] == SENTINEL).all(), f"{k} written outside the selection"
        assert (a[k] != SENTINEL).all()
    assert b["count"] == sel["count"] and np.array_equal(b["chars"], sel["chars"]) and np.array_equal(b["skinned"], sel["skinned"])
    assert b["status"] == 0


def test_frame_with_skin_select_replays_from_a_graph(cuda_device):
    eager, ent, lists, _m = build_frame(cuda_device, True)
    graph, _e, _l, _m2 = build_frame(cuda_device, True)
    dt = 1.0 / 60.0
    eager.clap_frame(dt, dt)
    graph.capture(dt, warmup_now=dt)
    for f in range(2, 4):
        for loop in (eager, graph):
            loop.characters.out_position.fill_(SENTINEL)
        eager.clap_frame(f * dt, dt)
        graph.clap_frame_replay(f * dt)
        a, b = eager.characters.download(), graph.characters.download()
        for k in ("out_position", "out_normal", "skinned", "chars"):
            assert np.array_equal(a[k], b[k]), f"frame {f}: {k}"
        assert a["count"] == b["count"] and 0 < a["count"] < eager.characters.n


# ------------------------------------------------------------------------------------------------- (i) launch failures
def test_reported_launch_failures(cuda_device, monkeypatch):
    monkeypatch.setenv("CLAPGPU_TEST_HOOKS", "1")              # read by the library's first clapgpu_test_fail_after
    c = cases.counts(65)
    batch, mesh = make_batch(c, cuda_device)
    batch.set_skin_select(**select_args(c))
    exp = expected(batch, mesh, c, False)
    sel = ref.select(**cases.ref_args(c))
    L = _lib.lib()
    failed = 0
    try:
        for k in range(8):
            L.clapgpu_test_fail_after(k)
            rc = L.clapgpu_skin_drawn(animation._stream(), C.byref(batch._skin_desc), C.byref(batch._sel_desc))
            L.clapgpu_test_fail_after(-1)
            torch.cuda.synchronize()
            if rc == _lib.OK:
                break
            failed += 1
            assert rc == _lib.ERR_UNKNOWN, rc
            assert L.clapgpu_last_error()
            fill(batch)
            batch.skin_drawn()                                  # a call that succeeds gives the whole answer
            assert_follows_the_rule(batch.download(), exp, sel, batch, f"after failure {k}")
    finally:
        L.clapgpu_test_fail_after(-1)
    assert failed == 3, f"{failed} launches failed: is the hook armed (CLAPGPU_TEST_HOOKS)?"   # select, compaction, skin
