"""CPU: the chosen particle cases of tests/partcases.py are what they claim.  Conditions on the inputs, checked with the
oracle: the first frame's respawn count and set are the chosen ones, the threshold pairs are adjacent floats on either
side of dd > radius_squared, and the fixture pinned on the reference holds the case it is said to hold."""
import os

import numpy as np
import pytest

import partcases as pc
from clap_amd import synth
from helpers import assert_bits_equal
from oracle import binding as ob
from test_oracle_particles import load_particles


def respawned_by_oracle(ps, pos, vel):
    """(count, indices of the particles the oracle's first frame respawned, pos, vel, state after it)"""
    p, v = pos.copy(), vel.copy()
    k, st = ob.particles_update(ps, p, v, pc.STATE0)
    # a respawned particle gets a velocity; one that stayed has none, and stayed where it was
    return k, np.flatnonzero((v != 0).any(axis=1)), p, v, st


def test_layouts():
    for name, ps in pc.layouts().items():
        rows = ps["n"] // 64
        assert (rows == 3 * pc.GROUP_ROWS) == (name == "full") and 2 * pc.GROUP_ROWS < rows <= 3 * pc.GROUP_ROWS
        assert (rows % pc.WAVE_ROWS != 0) == (name == "partial"), "the last wave is partial in the second layout"
        ends = (ps["sys"]["first"][1:] // 64).astype(int)
        assert all(e % pc.WAVE_ROWS and e % pc.GROUP_ROWS for e in ends), "no system ends where a wave or a group ends"
        assert (ps["sys"]["count"] % 64 != 0).any(), "a system with padded lanes"
        assert set(ps["sys"]["dist"]) == {synth.PART_DIST_LIN, synth.PART_DIST_SQRT, synth.PART_DIST_CBRT}
        assert not pc.live_mask(ps).all() and pc.live_mask(ps).sum() == ps["n_real"]
    assert pc.layouts()["full"]["n"] == 196608


@pytest.mark.parametrize("which", ["full", "partial"])
def test_the_oracle_respawns_exactly_the_chosen_particles(which):
    ps = pc.layouts()[which]
    pats = pc.patterns(ps)
    assert tuple(pats) == pc.PATTERN_NAMES
    live = pc.live_mask(ps)
    for name, chosen in pats.items():
        pos, vel = pc.at_rest(ps, chosen)
        k, moved, p, _v, st = respawned_by_oracle(ps, pos, vel)
        assert k == len(chosen) and np.array_equal(moved, chosen), f"{which} {name}: {k} respawns, {len(chosen)} chosen"
        assert_bits_equal(p[~live], pos[~live], "the oracle leaves the padded lanes alone")
        stay = live.copy()
        stay[chosen] = False
        assert_bits_equal(p[stay], pos[stay], "the others stay on their centre")
        assert st == synth.drand48_stream(pc.STATE0, 7 * k)[1] if k else st == pc.STATE0, "7 draws per respawn"


def test_patterns_are_what_their_names_say():
    ps = pc.layouts()["full"]
    pats = pc.patterns(ps)
    rows = {k: v >> 6 for k, v in pats.items()}
    pop = {k: np.bincount(v >> 6, minlength=ps["n"] // 64) for k, v in pats.items()}
    assert len(pats["none"]) == 0 and len(pats["all"]) == ps["n_real"]
    assert pats["particle_0"].tolist() == [0] and pats["last_live"].tolist() == [ps["n"] - 1]
    assert pats["lane_63_of_the_last_full_row"][0] % 64 == 63
    assert pop["one_full_row"].max() == 64 and len(pats["one_full_row"]) == 64, "a popcount byte of 64"
    for wave in (pc.WAVE_IN_GROUP_0, pc.WAVE_IN_GROUP_1):
        tag = f"wave_{wave}"
        for count in (255, 256, 257):
            for shape in ("thin", "as_rows"):
                r = rows[f"{count}_{shape}_in_{tag}"]
                assert len(r) == count and (r // pc.WAVE_ROWS == wave).all(), "all inside one wave's 64 rows"
            assert pop[f"{count}_thin_in_{tag}"].max() <= 5 and len(np.unique(rows[f"{count}_thin_in_{tag}"])) == 64
            assert (pop[f"{count}_as_rows_in_{tag}"] == 64).sum() == (3 if count == 255 else 4)
    assert pc.LIST_MAX == 256, "255 and 256 fit the LDS list, 257 takes the row-by-row walk"
    assert pc.WAVE_IN_GROUP_0 * 64 < pc.GROUP_ROWS <= pc.WAVE_IN_GROUP_1 * 64 < 2 * pc.GROUP_ROWS
    assert set(rows["rows_1023_and_1024"]) == {1023, 1024}
    assert rows["group_2_only"].min() >= 2 * pc.GROUP_ROWS and rows["group_0_only"].max() == pc.GROUP_ROWS - 1
    w = pats["x5555_in_every_row_of_a_wave"]
    assert np.array_equal(pc.mask_words(ps["n"], w)[pc.WAVE_IN_GROUP_1 * 64:pc.WAVE_IN_GROUP_1 * 64 + 64],
                          np.full(64, 0x5555555555555555, np.uint64)) and len(w) == 64 * 32
    for which in ("full", "partial"):
        one = pc.patterns(pc.layouts()[which])["one_bit_per_wave"] >> 6
        assert np.array_equal(one // pc.WAVE_ROWS, np.arange((pc.layouts()[which]["n"] // 64 + 63) // 64))
    part = pc.layouts()["partial"]
    assert pc.patterns(part)["last_live"][0] % 64 != 63, "the last live particle of the partial layout is not lane 63"
    assert set(pc.PARTIAL_PATTERNS) <= set(pats) and set(pc.VIEWS_PATTERNS) <= set(pats)


def test_threshold_pairs_are_adjacent_floats_on_either_side():
    t = pc.threshold_case()
    ps, pos = t["ps"], t["pos"]
    assert len(t["inside"]) >= 512 and len(t["inside"]) == len(t["outside"])
    a, b = pos[t["inside"]].view(np.int32).astype(np.int64), pos[t["outside"]].view(np.int32).astype(np.int64)
    assert np.array_equal((a != b).sum(axis=1), np.ones(len(a))) and np.abs(a - b).max() == 1, "one coordinate, one step"
    k, moved, _p, _v, _st = respawned_by_oracle(ps, pos, t["vel"])
    assert k == len(t["expect"]) and np.array_equal(moved, t["expect"])
    assert set(t["outside"]) <= set(moved) and not set(t["inside"]) & set(moved)
    # exact equality: centre 0, radius 4, the particle on the sphere -- dd == radius^2 is not dd > radius^2
    s = ps["sys"][-1]
    assert not s["center"].any() and s["radius_squared"] == 16.0
    for i in t["equal"]:
        assert float(np.dot(pos[i].astype(np.float64), pos[i].astype(np.float64))) == 16.0 and i not in moved


def test_fixture_holds_the_case(golden_dir):
    path = os.path.join(golden_dir, "particles_edges_wave.npz")
    ps, _view, state, ref = load_particles(path)
    c = pc.fixture_case()
    assert np.array_equal(ps["sys"], c["ps"]["sys"]) and state == pc.STATE0
    live = pc.live_mask(ps)                                 # the reference has no padded lanes: they come back as zeros
    assert_bits_equal(ref["pos0"][live], c["pos"][live], "the reference started from the chosen positions")
    assert_bits_equal(ref["vel0"], c["vel"], "and velocities")
    assert not ref["pos0"][~live].any() and not ref["pos"][:, ~live].any()
    moved = np.flatnonzero((ref["vel"][0] != 0).any(axis=1))
    assert np.array_equal(moved, c["expect"]), "the reference respawned the chosen particles in the first frame"
    pop = np.bincount(c["expect"] >> 6, minlength=ps["n"] // 64)
    assert pop[:64].sum() == 256 and pop[64:128].sum() == 257 and pop[128:].sum() == 3
    assert os.path.getsize(path) < (1 << 20)
