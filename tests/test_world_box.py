"""CPU: lmd::world_aabb, the world box from its extreme corners (clap_amd/csrc/lm_dev.h), against the literal
eight-corner chain it replaces, bit for bit in box and centre.  lm_dev.h is __host__ __device__: the stand-alone program
tests/c/test_world_box.cpp is compiled for the host with contraction off, as the kernels are, and makes no HIP call.
Bar: 0 differences over 3 M seeded cases that reach both the extreme-corner path and the literal fallback.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = 3_000_000


def test_extreme_corner_box_is_the_literal_box(tmp_path):
    exe = str(tmp_path / "test_world_box")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-O2", "-std=c++17",
                    "-ffp-contract=off", "-Wall", "-Wno-unused-function",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "clap_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "test_world_box.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe, str(CASES)], capture_output=True, text=True)
    print(p.stdout)
    m = re.search(r"cases (\d+) differences (\d+) fast (\d+) literal (\d+)", p.stdout)
    assert m, p.stdout[-2000:] + p.stderr[-2000:]
    cases, diffs, fast, literal = map(int, m.groups())
    assert cases == CASES and cases >= 1_000_000
    assert diffs == 0 and p.returncode == 0, p.stdout[-4000:]
    assert fast > 0 and literal > 0 and fast + literal == cases          # both paths taken
    cov = dict((k, int(v)) for k, v in re.findall(r"(\w+) (\d+)", p.stdout.split("covered", 1)[1]))
    for what in ("neg0_translation", "inverted_box", "negative_scale", "zero_scale", "overflow", "nan", "ties"):
        assert cov[what] > 1000, (what, cov)
