"""CPU: the multi-level broadphase grid (clapgpu_bp_create_levels, clap_amd/csrc/bp_levels.h).  The rule restated in
numpy (tests/bplevelref.py) reaches exactly the brute-force pairs of the mixed scene, and two mutants of it lose pairs;
the per-level statics image holds its invariants under the sanitizers (tests/c/test_bp_levels.cpp, a stand-alone
program); the entry points exist and refuse bad level counts before any device work.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bplevelref as ref
from clap_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELL0, LEVELS = 0.25, 6


@pytest.fixture(scope="module")
def mixed():
    aabb = ref.sphere_aabb(synth.mixed_bodies(3000, box=24.0, cell0=CELL0, seed=4))
    return aabb, ref.brute_pairs(aabb)


def test_abi_and_symbols():
    assert _lib.ABI_VERSION >= 41
    for name in ("clapgpu_bp_create_levels", "clapgpu_bp_levels", "clapgpu_bp_cell_slot"):
        assert name in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "clapgpu.h")).read()
    assert "#define CLAPGPU_BP_LEVELS_MAX 16" in hdr


def test_level_counts_are_refused_before_any_device_work():
    L = _lib.lib()
    bp = C.c_void_p()
    for levels in (0, 17, 1 << 31):
        assert L.clapgpu_bp_create_levels(C.byref(bp), 16, 1.0, levels, 0, None) == _lib.ERR_INVALID_ARGUMENTS
        assert not bp.value
    assert L.clapgpu_bp_create_levels(C.byref(bp), (1 << 28) + 1, 1.0, 2, 0, None) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_bp_create_levels(C.byref(bp), 16, 0.0, 2, 0, None) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_bp_levels(None) == 0
    assert L.clapgpu_bp_cell_slot(None, 0, 0, 0, 0) == 0xffffffff


def test_mixed_bodies_recipe():
    b, s = synth.mixed_bodies(20_000, box=48.0, cell0=CELL0, seed=9), synth.sphere_bodies(16, seed=9)
    assert sorted(b) == sorted(s) and b["cell"] == CELL0 and b["n"] == 20_000
    for k in s:
        assert np.shape(b[k]) == (() if np.ndim(s[k]) == 0 else (20_000, *np.shape(s[k])[1:])), k
    r = b["radius"]
    k = np.log2(2.0 * r / CELL0)
    exact = (k == np.round(k)) & (k >= 0)                                   # a diameter of exactly cell0 * 2^k
    assert 0.07 < exact.mean() < 0.13
    cls = np.digitize(r[~exact], [0.0625, 0.25, 1.0])                       # the classes' upper ends (1.25 x the class radius)
    share = np.bincount(cls, minlength=4) / np.count_nonzero(~exact)
    assert np.all(np.abs(share - [0.70, 0.20, 0.09, 0.01]) < [0.03, 0.03, 0.02, 0.005]), share
    level, over = ref.box_level(ref.sphere_aabb(b), CELL0, LEVELS)
    assert not over.any() and np.all(np.bincount(level, minlength=LEVELS) > 0)


def test_level_of_a_box_at_the_cell_boundaries():
    for l in range(LEVELS):
        c = CELL0 * 2.0 ** l
        rows = np.array([[0, c, 0, 0.1, 0, 0.1], [0, 0.1, 0, np.nextafter(c, 0.0), 0, 0.1], [0, 0.1, 0, 0.1, 0, np.nextafter(c, np.inf)]])
        level, over = ref.box_level(rows, CELL0, LEVELS)
        assert list(level) == [l, l, min(l + 1, LEVELS - 1)] and list(over) == [False, False, l == LEVELS - 1]
    level, over = ref.box_level(np.array([[0, np.nan, 0, 0.1, 0, 0.1]]), CELL0, LEVELS)
    assert level[0] == 0 and not over[0]


def test_the_rule_reaches_every_pair_of_the_mixed_scene(mixed):
    aabb, pairs = mixed
    level, over = ref.box_level(aabb, CELL0, LEVELS)
    assert not over.any() and len(pairs) > 1000
    cross = level[pairs[:, 0]] != level[pairs[:, 1]]
    assert cross.sum() > (~cross).sum() > 0, "the scene must test both branches of the rule, mostly the cross-level one"
    own = ref.owner(pairs[:, 0], pairs[:, 1], level)
    assert np.all(level[own[cross]] < np.maximum(level[pairs[cross, 0]], level[pairs[cross, 1]])) and np.all(own[~cross] == -1)
    reached = ref.rule_reaches(aabb, pairs, CELL0, LEVELS)
    assert np.array_equal(pairs[reached], pairs), f"the rule misses {np.count_nonzero(~reached)} of {len(pairs)} pairs"
    # a finer body never looks up more than 3 cells an axis on a coarser level
    for a in range(3):
        for l in range(1, LEVELS):
            fine = level < l
            first, last = ref.coarse_lookup(aabb[fine, 2 * a], aabb[fine, 2 * a + 1], CELL0 * 2.0 ** l)
            assert np.all(last - first <= 2)


@pytest.mark.parametrize("mutant", [dict(grow=0.0), dict(inclusive=False)], ids=["grow-by-nothing", "exclusive-upper-cell"])
def test_a_mutant_of_the_rule_loses_pairs(mixed, mutant):
    aabb, pairs = mixed
    reached = ref.rule_reaches(aabb, pairs, CELL0, LEVELS, **mutant)
    assert 0 < np.count_nonzero(~reached), "this mutant is not caught by the mixed scene"


def test_per_level_statics_image_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_bp_levels")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall",
                    "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "clap_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "test_bp_levels.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "test_bp_levels OK" in p.stdout
