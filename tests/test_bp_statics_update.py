"""CPU: moving statics (clapgpu_bp_statics_update).  The entry points are bound, and the yardstick of the GPU test
(tests/bpstaticsref.py: the image rule in numpy) equals the image the host code makes at create time, printed by the
stand-alone program tests/c/dump_bp_statics.cpp under the address and undefined-behaviour sanitizers.  No GPU, no HIP call.

What the box set must exercise is asserted here, per tested level count (1, 4, 16): registered statics whose own blocks
collide in a bucket, buckets holding several statics, large and registered statics side by side; and the two edge sets of
the GPU test are what they are called: every level all-large, every level none-large."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bpstaticsref as ref
from clap_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (1, 4, 16)


def test_entry_points_are_bound():
    assert _lib.ABI_VERSION >= 45
    for name in ("clapgpu_bp_statics_update", "clapgpu_bp_statics_sizes", "clapgpu_bp_statics_read"):
        assert name in _lib.SYMBOLS


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dump") / "dump_bp_statics")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall",
                    "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "clap_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "dump_bp_statics.cpp"), "-o", exe], check=True)
    return exe


def host_image(exe, path, boxes, levels):
    boxes = np.ascontiguousarray(boxes, np.float64).reshape(-1, 6)
    with open(path, "wb") as f:
        f.write(struct.pack("<IIIId", ref.BUCKETS, levels, len(boxes), 0, ref.CELL))
        f.write(boxes.tobytes())
    p = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert p.returncode == 0 and "dump_bp_statics OK" in p.stdout, p.stdout[-500:] + p.stderr[-4000:]
    out = {}
    for line in p.stdout.splitlines()[:-1]:
        name, *words = line.split()
        if name in ("bounds", "entry_boxes", "large_boxes"):
            out[name] = np.array([int(w, 16) for w in words], np.uint64).view(np.float64)
        else:
            out[name] = np.array([int(w) for w in words], np.uint32)
    return out


def same_image(host, want):
    assert int(host["n_entries"][0]) == want["n_entries"] and int(host["n_large"][0]) == want["n_large"]
    for name in ("start", "entries", "large", "large_start"):
        assert host[name].tobytes() == want[name].tobytes(), name
    for name in ("entry_boxes", "large_boxes"):
        assert host[name].tobytes() == want[name].tobytes(), name
    assert np.all(host["bounds"] == want["bounds"]), (host["bounds"], want["bounds"])


@pytest.mark.parametrize("levels", LEVELS)
def test_host_image_equals_the_rule(dump_exe, tmp_path, levels):
    a = ref.boxes(11)
    assert 280 <= len(a) <= 320
    want = ref.image(a, levels)
    # what the set exercises, at this level count
    assert sum(want["self_collisions"]) > 0, "no registered static has two blocks in one bucket"
    assert sum(want["shared"]) > 0, "no bucket holds several statics"
    assert want["n_large"] > 0 and want["n_entries"] > 0
    assert all(0 < n < len(a) for n in want["level_large"]), "every level has large and registered statics"
    assert len(np.unique(a, axis=0)) < len(a), "coincident duplicates"
    assert np.isnan(a).any() and np.isinf(a).any() and (a[:, 1] - a[:, 0] >= 1.0e9).any() and (a < 0).any()
    same_image(host_image(dump_exe, tmp_path / "a.bin", a, levels), want)
    b = ref.boxes_moved(a, 12)
    assert 80 <= np.sum(np.any(a != b, axis=1) | np.any(np.isnan(b) != np.isnan(a), axis=1)) <= len(a) // 3 + 9
    same_image(host_image(dump_exe, tmp_path / "b.bin", b, levels), ref.image(b, levels))


@pytest.mark.parametrize("levels", LEVELS)
def test_edge_sets_are_all_large_and_none_large(dump_exe, tmp_path, levels):
    big = ref.boxes_all_large()
    want = ref.image(big, levels)
    assert want["level_large"] == [len(big)] * levels and want["n_entries"] == 0
    assert np.all(want["bounds"][:3] == np.inf) and np.all(want["bounds"][3:] == -np.inf)
    same_image(host_image(dump_exe, tmp_path / "big.bin", big, levels), want)
    small = ref.boxes_none_large(13)
    want = ref.image(small, levels)
    assert want["level_large"] == [0] * levels and want["n_large"] == 0
    same_image(host_image(dump_exe, tmp_path / "small.bin", small, levels), want)
    many = ref.boxes_many(14)
    assert ref.image(many, 1)["n_entries"] > 4 * ref.image(ref.boxes(11), 1)["n_entries"]
