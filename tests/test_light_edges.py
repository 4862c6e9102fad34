"""CPU: the chosen light cases of tests/lightcases.py are what they claim, and the oracle gives on them what the
reference gives (tests/golden/lightgrid_edges.npz; live against oracle/_ref in test_light.py).

The claims are conditions on the inputs, not measurements: every slot of a disc-edge pair is bracketed by two adjacent
floats with different bit columns, the gate pairs are adjacent floats on either side of the gate, the degenerate radii
are NaN or infinite, a lone slot gives 1 << s in every tile."""
import os

import numpy as np
import pytest

import lightcases as lc
from oracle import binding as ob

F32 = np.float32


def ulps_apart(a, b):
    """Steps between two float32 arrays of one sign"""
    return np.abs(np.asarray(a, F32).view(np.int32).astype(np.int64) - np.asarray(b, F32).view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------------- 1. disc edges
def test_cameras_and_grids():
    assert len(lc.CAMERAS) >= 3 and len(lc.GRIDS) >= 2
    assert any(w % cell for w, _h, cell in lc.GRIDS), "one grid's width is no multiple of its cell"
    assert int(lc.CAMERAS["tilted_z01"]["ndc_z_zero_one"][0]) == 1
    assert len(lc.disc_edge_pairs()) == len(lc.CAMERAS) * len(lc.GRIDS)


@pytest.mark.parametrize("k", range(len(lc.CAMERAS) * len(lc.GRIDS)))
def test_every_slot_is_bracketed_by_adjacent_floats(k):
    near, far, found = lc.disc_edge_pairs()[k]
    assert found.all(), f"{near['name']}: slots without a bracket: {np.flatnonzero(~found)}"
    for c in (near, far):
        L = c["lights"]
        assert L["nr_lights"] == 128 and L["active"].all() and not L["is_dir"].any()
    steps = ulps_apart(near["lights"]["pos"], far["lights"]["pos"])
    assert np.array_equal((steps != 0).sum(axis=1), np.ones(128)), "one coordinate of every light differs"
    assert steps.max() == 1, "and by one float32 step"
    a, b = lc.columns(lc.oracle_tiles(near)), lc.columns(lc.oracle_tiles(far))
    differ = (a != b).any(axis=(0, 1))
    assert differ.all(), f"{near['name']}: the bit column of slots {np.flatnonzero(~differ)} is the same in both sets"
    lit = a.any(axis=(0, 1))
    assert lit.all() and not a.all(axis=(0, 1)).any(), "every light lights at least one tile and not all of them"


# ------------------------------------------------------------------------------------------------- 2. gate edges
@pytest.mark.parametrize("k", range(len(lc.GATE_CAMERAS)))
def test_gate_pairs_are_adjacent_and_the_gate_decides(k):
    c, info = lc.gate_cases()[k]
    cols = lc.columns(lc.oracle_tiles(c)).any(axis=(0, 1))
    S = lc.GATE_SLOTS
    lit = {S["far_lit"], S["eye_lit"]}
    assert set(np.flatnonzero(cols)) == lit, "the lit side of each gate lights tiles, the gated side and the lights behind none"
    assert min(lit | {S["far_gated"], S["eye_gated"]} | set(S["behind"])) < 64 <= max(lit), "both ballots"
    for name in ("far", "eye"):
        p, q, ax = info[name]
        steps = ulps_apart(p, q)
        assert steps[ax] == 1 and steps.sum() == 1, f"{name}: {p} and {q} are not adjacent floats"
    # it is the gate that decides and not the disc: a light 10^4 times as strong gets the same answers
    strong = lc.copy_set(c["lights"])
    strong["color"] = strong["color"] * F32(1e4)
    cols2 = lc.columns(lc.oracle_tiles(dict(c, lights=strong))).any(axis=(0, 1))
    assert np.array_equal(cols, cols2)
    # where the gates lie: the far plane is at 500, the eye gate at |w| = 1e-3 (view depth of the two sides)
    cam = c["cam"]
    depth = lambda p: float(np.linalg.norm(p.astype(np.float64) - cam["cam_pos"].astype(np.float64)))    # noqa: E731
    assert 499.0 < depth(info["far"][0]) < 501.0 and 0.9e-3 < depth(info["eye"][1]) < 1.1e-3
    if k == 0:                                             # the identity camera: the eye bracket is -0.001 / -0.0009999999
        assert info["eye"][0][2] == F32(-0.001) and info["eye"][1][2] == np.nextafter(F32(-0.001), F32(0))


# ------------------------------------------------------------------------------------------------- 3. radius edges
def test_degenerate_radii():
    c = lc.radius_cases()[0]
    L = c["lights"]
    rad = {name: ob.light_radius(L["color"][s], L["attenuation"][s], False) for name, s, *_ in lc.RADIUS_LIGHTS}
    for name in ("linear_only", "constant_only", "neg_discriminant", "colour_zero_nan"):
        assert np.isnan(rad[name]), f"{name}: radius {rad[name]}"
    assert rad["linear_only_neg"] == np.inf and rad["colour_inf"] == np.inf
    assert rad["colour_zero_negative_radius"] < 0
    with np.errstate(over="ignore"):
        assert np.isfinite(rad["radius_sq_overflows"]) and np.isinf(F32(rad["radius_sq_overflows"]) * F32(rad["radius_sq_overflows"]))


@pytest.mark.parametrize("k", range(2))
def test_degenerate_lights_by_the_oracle(k):
    c = lc.radius_cases()[k]
    cols = lc.columns(lc.oracle_tiles(c))
    n_tiles = cols.shape[0] * cols.shape[1]
    count = {name: int(cols[..., s].sum()) for name, s, *_ in lc.RADIUS_LIGHTS}
    for name in ("linear_only", "constant_only", "neg_discriminant", "colour_zero_nan", "on_the_camera_plane", "pos_x_inf",
                 "pos_z_minus_inf", "pos_z_plus_inf"):
        assert count[name] == 0, f"{name} lights {count[name]} tiles"
    for name in ("linear_only_neg", "radius_sq_overflows", "colour_inf", "colour_zero_negative_radius"):
        assert count[name] == n_tiles, f"{name} lights {count[name]} of {n_tiles} tiles"
    assert 0 < count["ordinary"] < n_tiles
    used = {s for _n, s, *_ in lc.RADIUS_LIGHTS}
    assert not cols[..., sorted(set(range(128)) - used)].any()


# ------------------------------------------------------------------------------------------------- 4. slots and words
def test_slot_cases():
    cases = {c["name"]: c for c in lc.slot_cases()}
    for s in lc.LONE_SLOTS:
        for kind in ("dir", "point"):
            c = cases[f"lone_{kind}_{s}"]
            assert c["lights"]["nr_lights"] == s + 1 and c["lights"]["active"].sum() == 1
            t = lc.oracle_tiles(c)
            assert np.array_equal(t, np.broadcast_to(lc.lone_bit(s), t.shape)), f"{c['name']}: every tile is 1 << {s}"
    full = lc.columns(lc.oracle_tiles(cases["nr_lights_128"]))
    for n in lc.NR_LIGHTS:
        got = lc.columns(lc.oracle_tiles(cases[f"nr_lights_{n}"]))
        assert np.array_equal(got[..., :n], full[..., :n]) and not got[..., n:].any()
        assert got[..., n - 1].any(), "the last slot in use lights a tile"
    d = lc.columns(lc.oracle_tiles(cases["dir_in_every_word"]))
    assert {s // 32 for s in lc.DIR_SLOTS} == {0, 1, 2, 3}
    assert d[..., list(lc.DIR_SLOTS)].all() and not full[..., list(lc.DIR_SLOTS)].all(axis=(0, 1)).any()
    r = lc.oracle_tiles(cases["released_between_two_lit"])
    assert np.all(r[..., 0] == (1 << 9 | 1 << 11)) and not r[..., 1:].any()


# ------------------------------------------------------------------------------------------------- 5. grid shapes
def test_grid_shapes():
    assert set(lc.SHAPES) == {1, 15, 16, 17, 63, 64, 65, 129}
    shapes = {}
    for c in lc.shape_cases():
        t = lc.oracle_tiles(c)
        n = int(c["name"].split("_")[1])
        assert t.shape[0] * t.shape[1] == n and t.shape[:2] == ob.light_grid_dims(c["width"], c["height"], c["cell"])[::-1]
        cols = lc.columns(t)
        assert cols.any() and not cols.all(), "both answers of the disc test"
        shapes[n] = t.shape[:2]
    assert shapes[15][0] == 1 and shapes[16][1] == 1, "theight = 1 and twidth = 1"
    assert lc.SHAPES[1][2] > lc.SHAPES[1][0], "cell > width"
    assert sum(1 for w, _h, cell in lc.SHAPES.values() if w % cell) >= 4, "width % cell != 0"


# ------------------------------------------------------------------------------------------------- 7. carriers
@pytest.mark.parametrize("nc", lc.CARRIER_COUNTS)
def test_carrier_cases(nc):
    c = lc.carrier_case(nc)
    car, scene, L = c["carriers"], c["scene"], c["lights"]
    named = np.flatnonzero(car["light"] == c["twice"])
    assert list(named) == list(range(c["k"], nc, 128)), "carrier k, k + 128, k + 256 name one slot"
    assert len(named) == {1: 1, 127: 1, 128: 1, 129: 2, 257: 3}[nc]
    for all_dirty in (False, True):
        exp = lc.carrier_expected(c, all_dirty)
        last = named[-1]
        want = scene["pos_scale"][car["entity"][last], :3] + car["off"][last]
        assert np.array_equal(exp[c["twice"]], want), "the later carrier of the slot wins"
        if nc > 60:
            want = scene["pos_scale"][car["entity"][60], :3] + car["off"][60]
            assert np.array_equal(exp[4], want), "carriers 1 and 60 name slot 4"
        sp = c["special"]
        if sp:
            assert car["entity"][sp["entity_past_n"]] >= scene["n"] and car["light"][sp["slot_negative"]] < 0
            assert car["light"][sp["slot_past_nr"]] >= L["nr_lights"] and not L["active"][car["light"][sp["released"]]]
            assert scene["parent"][car["entity"][sp["child"]]] >= 0 and not c["dirty"][car["entity"][sp["clean"]]]
            assert np.array_equal(exp[5], L["pos"][5]), "the released slot keeps its position"
            for key in ("entity_past_n", "child") + (() if all_dirty else ("clean",)):
                slot = car["light"][sp[key]]
                others = np.flatnonzero(car["light"] == slot)
                assert list(others) == [sp[key]] and np.array_equal(exp[slot], L["pos"][slot]), f"{key}: skipped"
            if all_dirty:
                slot = car["light"][sp["clean"]]
                assert not np.array_equal(exp[slot], L["pos"][slot]), "all_dirty: the clean entity's carrier applies"


# ------------------------------------------------------------------------------------------------- the fixture
def load_fixture(golden_dir):
    """[(case, the reference's tiles)] of tests/golden/lightgrid_edges.npz: the cases are stacked along a leading axis and
    their tiles follow one another."""
    z = np.load(os.path.join(golden_dir, "lightgrid_edges.npz"))
    out, at = [], 0
    for k, name in enumerate(str(z["names"]).split(",")):
        L = {f: z["in_" + f][k] for f in ("pos", "color", "attenuation", "is_dir", "active")}
        L["nr_lights"] = len(L["active"])
        w, h, cell = (int(v) for v in z["in_grid"][k])
        tw, th = ob.light_grid_dims(w, h, cell)
        out.append((dict(name=name, lights=L, view=z["ref_view_mx"][k], proj=z["ref_proj_mx"][k], width=w, height=h, cell=cell),
                    z["ref_tiles"][at:at + tw * th].reshape(th, tw, 4)))
        at += tw * th
    assert at == len(z["ref_tiles"])
    return out


def test_fixture_holds_the_cases_and_the_oracle_matches_the_reference(golden_dir):
    fx = load_fixture(golden_dir)
    cases = lc.fixture_cases()
    assert [c["name"] for c, _ in fx] == [c["name"] for c in cases]
    assert sum(c["name"].startswith("gate_") for c in cases) == 4 and sum(c["name"].startswith("radius_") for c in cases) == 2
    assert sum(c["name"].startswith("disc_") for c in cases) == 2
    for (got, ref_tiles), c in zip(fx, cases):
        for f in ("pos", "color", "attenuation", "is_dir", "active"):
            assert np.array_equal(got["lights"][f].view(np.uint32), np.asarray(c["lights"][f]).view(np.uint32)), f"{c['name']}: {f}"
        assert np.array_equal(got["view"].view(np.uint32), c["view"].view(np.uint32)), "the reference's view matrix is the oracle's"
        assert np.array_equal(got["proj"].view(np.uint32), c["proj"].view(np.uint32))
        assert np.array_equal(lc.oracle_tiles(got), ref_tiles), f"{c['name']}: the oracle's tiles against the reference's"
    path = os.path.join(golden_dir, "lightgrid_edges.npz")
    others = max(os.path.getsize(os.path.join(golden_dir, n + ".npz")) for n in ("lightgrid_1080p", "lightgrid_odd_z01"))
    assert os.path.getsize(path) <= others, "no larger than the larger of the two other light fixtures"
