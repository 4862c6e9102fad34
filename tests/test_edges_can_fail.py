"""CPU: the chosen light and particle cases can fail.  oracle/light.c and oracle/particles.c are built a second time with
-ffp-contract=fast -mfma -- the mistake a kernel build or a refactor is most likely to make -- and compared with the
normal build (-ffp-contract=off) on the random cases of test_light.py and on the chosen cases of lightcases.py and
partcases.py.  A plain second shared object opened with ctypes; no GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lightcases as lc
import partcases as pc
from oracle import binding as ob
from test_light import _random_case

ORACLE = os.path.dirname(os.path.abspath(ob.__file__))


def cpu_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma" in line for line in f)
    except OSError:
        return False


@pytest.fixture(scope="module")
def contracted(tmp_path_factory):
    cc = os.environ.get("CC") or "gcc"
    if shutil.which(cc) is None or not cpu_has_fma():
        pytest.skip("no compiler or no FMA on this CPU")
    out = str(tmp_path_factory.mktemp("contracted") / "libclap_oracle_contracted.so")
    cmd = [cc, "-O2", "-std=gnu11", "-ffp-contract=fast", "-mfma", "-fno-fast-math", "-fPIC", "-shared", "-o", out,
           os.path.join(ORACLE, "light.c"), os.path.join(ORACLE, "particles.c"), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "mfma" in r.stderr:
        pytest.skip("the compiler has no -mfma")
    assert r.returncode == 0, r.stderr
    return ob.second_build(out)


def test_a_contracted_build_passes_the_random_cases_and_fails_the_chosen_ones(contracted):
    """The agreement on the random cases is the gap the chosen cases close: a light grid with fused multiply-adds gives
    the normal build's tiles on all 12 random cases of test_light.py::test_hip_matches_oracle_random (seeds 200-211), so
    those cases cannot tell such a kernel from a right one.  The chosen cases can.  Measured with gcc 11 on x86-64
    (shares of the normal oracle build's answers, never of the kernel's):

      random light cases, seeds 200-211     0 of 12 grids differ
      disc-edge sets (6 pairs of 128)      12 of 12 sets differ; 391 of 1536 lights (25 %) get another bit column
      particle threshold case              71 of 1288 particles (5.5 %) decide differently

    The floors asserted are the issue's: one in ten of the disc-edge lights, one particle."""
    # the random cases: whole grids equal
    for seed in range(12):
        lights, cam, w, h, cell = _random_case(200 + seed)
        _fr, vm, pm = ob.frustum_from_camera(cam)
        assert np.array_equal(ob.light_grid_compute(lights, vm, pm, w, h, cell),
                              ob.light_grid_compute(lights, vm, pm, w, h, cell, L=contracted)), f"seed {200 + seed}"

    # the disc edges: a case is one light on one side of its edge
    cases = differ = sets = 0
    for near, far, _found in lc.disc_edge_pairs():
        for c in (near, far):
            a = lc.columns(lc.oracle_tiles(c))
            b = lc.columns(lc.oracle_tiles(c, lambda *args: ob.light_grid_compute(*args, L=contracted)))
            d = (a != b).any(axis=(0, 1))
            cases, differ, sets = cases + d.size, differ + int(d.sum()), sets + bool(d.any())
    print(f"disc edges: {differ} of {cases} lights differ, in {sets} sets")
    assert 10 * differ >= cases, f"the contracted build differs on {differ} of {cases} disc-edge lights only"

    # the particle thresholds: which particles the first frame respawns
    t = pc.threshold_case()
    moved = []
    for L in (None, contracted):
        pos, vel = t["pos"].copy(), t["vel"].copy()
        ob.particles_update(t["ps"], pos, vel, pc.STATE0, L=L)
        moved.append((pos.view(np.uint32) != t["pos"].view(np.uint32)).any(axis=1))
    assert np.array_equal(np.flatnonzero(moved[0]), t["expect"])
    wrong = int((moved[0] != moved[1]).sum())
    print(f"particle thresholds: {wrong} of {t['ps']['n_real']} particles decide differently")
    assert wrong >= 1, "the contracted build decides every threshold particle as the normal build does"
