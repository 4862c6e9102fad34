"""CPU: the host binning of a broadphase's static boxes (clap_amd/csrc/bp_statics.h), checked by the stand-alone program
tests/c/test_bp_statics.cpp under the address and undefined-behaviour sanitizers.  No GPU, no HIP call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_statics_image_invariants_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_bp_statics")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall",
                    "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "clap_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "test_bp_statics.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "test_bp_statics OK" in p.stdout
