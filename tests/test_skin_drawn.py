"""CPU: clapgpu_skin_lod_lists against tests/skinselref.py, the refusals of clapgpu_skin_drawn that need no device, and the
properties of the GPU tests' own fixtures (tests/skinselcases.py) -- so that tests/test_skin_drawn_gpu.py cannot pass by
selecting nothing or everything."""
import ctypes as C

import numpy as np
import pytest

import skinselcases as cases
import skinselref as ref
from clap_amd import _lib, animation


# ------------------------------------------------------------------------------------------------- the host helper
def helper_and_ref(index, n_verts, capacity, total=0):
    rc, first, count, lst, tot = animation.skin_lod_lists(index, n_verts, capacity=capacity, total=total)
    erc, efirst, ecount, elist, etot = ref.lod_lists(index, n_verts, capacity, total)
    assert rc == erc and tot == etot
    if erc != ref.ERR_OUT_OF_BOUNDS:
        assert np.array_equal(first, efirst) and np.array_equal(count, ecount)
        assert np.array_equal(lst[total:total + len(elist)], elist)
    return rc, first, count, lst, tot


def test_lod_lists_match_the_reference():
    R = cases.rng(1)
    nv = 300
    everything = R.permutation(np.repeat(np.arange(nv), 3)).astype(np.uint16)        # a LOD that references every vertex
    single = np.full(9, 17, np.uint16)                                                 # one that references a single vertex
    repeated = R.integers(0, nv, 500).astype(np.uint16)                                # repeated indices
    empty = np.zeros(0, np.uint16)                                                     # an empty LOD
    index = [everything, single, repeated, empty]
    rc, first, count, lst, tot = helper_and_ref(index, nv, 1000)
    assert rc == _lib.OK
    assert first[0] == _lib.SKIN_LOD_ALL and count[0] == nv
    assert (first[1], count[1]) == (0, 1) and lst[0] == 17
    assert first[2] == 1 and 1 < count[2] < nv and tot == 1 + count[2]
    body = lst[1:tot]
    assert (np.diff(body.astype(np.int64)) > 0).all() and set(body) == set(repeated.tolist())
    assert (first[3], count[3]) == (tot, 0)
    # capacity one short: TOO_LARGE, the total still right, nothing written at or past the capacity
    lst2 = animation.skin_lod_lists(index, nv, capacity=tot - 1)
    assert lst2[0] == _lib.ERR_TOO_LARGE and lst2[4] == tot and np.array_equal(lst2[3], lst[:tot - 1])
    helper_and_ref(index, nv, tot - 1)
    helper_and_ref(index, nv, 0)
    # appended behind entries that are there already
    rc, first, count, lst3, tot3 = helper_and_ref([repeated, single], nv, 2000, total=700)
    assert rc == _lib.OK and first[0] == 700 and tot3 == 700 + count[0] + 1
    # an index past the mesh
    assert helper_and_ref([np.asarray([0, nv], np.uint16)], nv, 10)[0] == _lib.ERR_OUT_OF_BOUNDS
    assert animation.skin_lod_lists([single] * 5, nv)[0] == _lib.ERR_INVALID_ARGUMENTS
    assert animation.skin_lod_lists([single], 0)[0] == _lib.ERR_INVALID_ARGUMENTS


def test_lod_lists_feed_the_rule():
    """The helper's row, given to the rule: each LOD names exactly the vertices its index buffer references."""
    R = cases.rng(2)
    nv = 120
    index = [np.arange(nv, dtype=np.uint16)] + [R.integers(0, nv, k).astype(np.uint16) for k in (90, 30, 6)]
    rc, first, count, lst, tot = animation.skin_lod_lists(index, nv)
    assert rc == _lib.OK
    for lod in range(4):
        sel = ref.select(1, [nv], [ref.pack_plane([True])], 1, cur_lod=[lod], n_lods=4, lod_first=first, lod_count=count,
                         lst=lst[:tot])
        assert np.array_equal(sel["verts"][0], np.unique(index[lod])) and sel["status"] == 0 and sel["skinned"][0] == lod


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals_that_need_no_device():
    L = _lib.lib()
    one = (C.c_uint32 * 4)()
    p = C.addressof(one)                                       # any non-NULL address: nothing is dereferenced before the checks
    b = _lib.SkinBatch(3, 64, p, p, p, p, p, p, p, p, p, p, None)
    aligned = (C.addressof((C.c_char * 1024)()) + 255) & ~255

    def sel(**kw):
        s = _lib.SkinSelect()
        s.n_planes, s.n_entities = 1, 3
        s.planes[0] = p
        s.skinned, s.chars, s.count, s.status, s.scratch = p, p, p, p, aligned
        for k, v in kw.items():
            if k.startswith("plane"):
                s.planes[int(k[5:])] = v
            else:
                setattr(s, k, v)
        return s

    call = lambda bb, ss: L.clapgpu_skin_drawn(None, None if bb is None else C.byref(bb), None if ss is None else C.byref(ss))
    bad = _lib.ERR_INVALID_ARGUMENTS
    assert call(None, sel()) == bad and call(b, None) == bad
    empty = _lib.SkinBatch(0, 64, *([None] * 11))
    assert call(empty, sel(n_planes=0)) == _lib.OK             # n_chars == 0: nothing is asked, nothing is launched
    assert call(_lib.SkinBatch(3, 64, p, p, p, p, None, p, p, p, p, p, None), sel()) == bad
    assert call(_lib.SkinBatch(3, 0, p, p, p, p, p, p, p, p, p, p, None), sel()) == _lib.ERR_TOO_LARGE
    assert call(_lib.SkinBatch(3, 257, p, p, p, p, p, p, p, p, p, p, None), sel()) == _lib.ERR_TOO_LARGE
    assert call(b, sel(n_planes=0)) == bad and call(b, sel(n_planes=6)) == bad
    assert call(b, sel(n_planes=2)) == bad                     # a NULL plane
    assert call(b, sel(n_planes=5, plane1=p, plane2=p, plane3=p)) == bad
    for n_lods in (0, 5):
        assert call(b, sel(n_rows=1, n_lods=n_lods, lod_first=p, lod_count=p)) == bad
    assert call(b, sel(n_lods=5)) == bad
    assert call(b, sel(n_rows=1, n_lods=4, lod_count=p)) == bad and call(b, sel(n_rows=1, n_lods=4, lod_first=p)) == bad
    assert call(b, sel(n_list=3)) == bad
    for k in ("skinned", "chars", "count", "status", "scratch"):
        assert call(b, sel(**{k: None})) == bad, k
    assert call(b, sel(scratch=aligned + 128)) == bad
    assert L.clapgpu_skin_select_scratch_bytes(0) % 256 == 0
    for n in (1, 64, 65, 50_000):
        words = (n + 63) // 64
        assert L.clapgpu_skin_select_scratch_bytes(n) % 256 == 0 and L.clapgpu_skin_select_scratch_bytes(n) >= 9 * words


def test_frame_with_skin_select_needs_skin_pose_and_frustum():
    L = _lib.lib()
    ent, fr, s = _lib.Entities(), _lib.Frustum(), _lib.SkinSelect()
    f = _lib.FrameDesc()
    f.entities, f.frustum, f.skin_select = C.pointer(ent), C.pointer(fr), C.pointer(s)
    assert L.clapgpu_frame_issue(None, C.byref(f), 0.0, 0) == _lib.ERR_INVALID_ARGUMENTS    # no skin, no pose


# ------------------------------------------------------------------------------------------------- the fixtures' own properties
@pytest.mark.parametrize("name", sorted(cases.SELECTIVE))
def test_fixture_selects_some_characters_and_not_all(name):
    c = cases.SELECTIVE[name]()
    sel = ref.select(**cases.ref_args(c))
    assert 0.2 * c["n"] <= sel["count"] <= 0.8 * c["n"], f"{name}: {sel['count']} of {c['n']} drawn"
    assert np.array_equal(sel["chars"], np.flatnonzero(sel["skinned"] != ref.NOT_DRAWN))
    if c["cur_lod"] is not None and c["n"] >= 9:
        assert set(sel["skinned"][sel["chars"]]) == {0, 1, 2, 3}, f"{name}: every LOD is used"


def test_single_character_fixture_is_drawn():
    c = cases.counts(1)
    sel = ref.select(**cases.ref_args(c))
    assert sel["count"] == 1 and c["entity"][0] == 63


def test_counts_fixtures_use_the_word_edges():
    for n in cases.COUNTS[1:]:
        c = cases.counts(n)
        assert list(c["entity"][:3]) == [63, 64, 127] and len(set(c["entity"].tolist())) == n
        sel = ref.select(**cases.ref_args(c))
        assert sel["skinned"][0] != ref.NOT_DRAWN and sel["skinned"][1] == ref.NOT_DRAWN and sel["skinned"][2] != ref.NOT_DRAWN


@pytest.mark.parametrize("with_entity", [True, False])
def test_planes_fixture_has_a_character_in_the_last_plane_only(with_entity):
    c = cases.planes(with_entity)
    assert len(c["planes"]) == 5
    sel = ref.select(**cases.ref_args(c))
    main_only = ref.select(**{**cases.ref_args(c), "planes": c["planes"][:1]})
    first_four = ref.select(**{**cases.ref_args(c), "planes": c["planes"][:4]})
    assert sel["skinned"][5] != ref.NOT_DRAWN and first_four["skinned"][5] == ref.NOT_DRAWN
    assert sel["skinned"][7] != ref.NOT_DRAWN and main_only["skinned"][7] == ref.NOT_DRAWN      # drawn in an extra plane only
    assert sel["skinned"][6] == ref.NOT_DRAWN
    assert sel["count"] > main_only["count"]


def test_lists_fixture_covers_every_length_and_row():
    c = cases.lod_lists(True)
    assert sorted(c["lod_count"][c["lod_first"] != ref.LOD_ALL].tolist()) == [0, 1, 63, 64, 65, 255, 256, 257]
    assert (c["lod_first"][2] == ref.LOD_ALL).all() and c["lod_first"].shape == (3, 4)
    assert c["vert_count"].min() == 1 and c["vert_count"].max() == 700
    sel = ref.select(**cases.ref_args(c))
    assert sel["status"] == 0
    used = {(int(c["row"][ch]), int(sel["skinned"][ch])) for ch in sel["chars"]}
    assert used == {(r, l) for r in range(3) for l in range(4)}
    assert max(int(v.max()) for v in sel["verts"] if v.size) > 256
    assert cases.lod_lists(False)["lod_first"] is None


@pytest.mark.parametrize("which,bit", [("entity", ref.ENTITY_RANGE), ("lod", ref.LOD_RANGE), ("list", ref.LIST_RANGE)])
def test_range_fixtures_set_their_bit_alone(which, bit):
    c = cases.range_bit(which)
    sel = ref.select(**cases.ref_args(c))
    assert sel["status"] == bit
    if which == "entity":
        assert sel["skinned"][4] == ref.NOT_DRAWN and sel["skinned"][11] == ref.NOT_DRAWN
    elif which == "lod":
        assert sel["skinned"][2] == 0 and sel["skinned"][7] == 0
    else:
        lod1 = [ch for ch in sel["chars"] if sel["skinned"][ch] == 1]
        assert lod1 and all(len(sel["verts"][ch]) == 11 for ch in lod1)


def test_plain_and_graph_fixtures():
    c = cases.plain()
    assert ref.select(**cases.ref_args(c))["count"] == c["n"]
    c, second = cases.graph_planes()
    a = ref.select(**cases.ref_args(c))
    b = ref.select(**{**cases.ref_args(c), "planes": [second]})
    assert not np.array_equal(a["skinned"], b["skinned"]) and 0.2 * c["n"] <= b["count"] <= 0.8 * c["n"]
    assert a["skinned"][0] != ref.NOT_DRAWN and b["skinned"][0] == ref.NOT_DRAWN and b["skinned"][1] != ref.NOT_DRAWN


def test_frame_fixture_draws_some_characters_at_every_lod_and_one_in_the_lights_view_only():
    """The frame fixture through the oracle's entity update, cull and LOD pick (what the GPU frame leaves on the device)."""
    from oracle import binding as ob
    scene, cam, light, ent, lists = cases.frame_scene()
    st = ob.entity_state(scene)
    ob.entities_update(scene, st)
    n = scene["n"]
    vis, main = ob.entities_cull(n, st["flags"], st["aabb"], ob.frustum_from_camera(cam)[0])
    _v, other = ob.entities_cull(n, st["flags"], st["aabb"], ob.frustum_from_camera(light)[0])
    cur = np.zeros(n, np.int32)
    ob.entities_lod(scene, st, vis, cam["cam_pos"], scene["model_lod"], np.full(n, -1, np.int32), cur)
    vc = np.full(len(ent), cases.FRAME_VPC)
    sel = ref.select(len(ent), vc, [main, other], n, entity=ent, cur_lod=cur, n_lods=4, lod_first=lists[0], lod_count=lists[1],
                     lst=lists[2])
    assert 0.2 * len(ent) <= sel["count"] <= 0.8 * len(ent)
    assert set(sel["skinned"][sel["chars"]]) == {0, 1, 2, 3} and sel["status"] == 0
    assert sel["count"] > ref.select(len(ent), vc, [main], n, entity=ent)["count"] > 0


def test_algorithmic_bytes_formula():
    """68 B (72 with w) per written vertex + 64 J per drawn character + 4 B per list entry read."""
    class B:                                                    # the fields the formula reads
        pass
    c = cases.lod_lists(True)
    sel = ref.select(**cases.ref_args(c))
    b = B()
    b.n, b.vert_count_host, b._sel_lists_host, b._sel_row_host = c["n"], c["vert_count"], (c["lod_first"], c["lod_count"]), c["row"].astype(np.int64)
    b.model, b._skin_desc = B(), B()
    b.model.nr_joints, b._skin_desc.out_w = 64, None
    written = sum(len(v) for v in sel["verts"])
    entries = sum(len(sel["verts"][ch]) for ch in sel["chars"] if c["lod_first"][c["row"][ch], sel["skinned"][ch]] != ref.LOD_ALL)
    want = 68 * written + 64 * 64 * sel["count"] + 4 * entries
    assert animation.CharacterBatch.skin_drawn_algorithmic_bytes(b, sel["skinned"]) == want
    b._skin_desc.out_w = 1
    assert animation.CharacterBatch.skin_drawn_algorithmic_bytes(b, sel["skinned"]) == want + 4 * written
