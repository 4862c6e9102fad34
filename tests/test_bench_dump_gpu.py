"""GPU: `bench.py --dump-outputs DIR` writes what the timed step computed in its last step.  Two runs with the same
workload and different --steps give the same files bit for bit, and the files are the oracle's frame of that seeded
workload: world matrices, inverses, AABBs and centres of the sampled rows, and the whole ascending visible list."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from clap_amd import synth, tiler
from oracle import binding as ob
from helpers import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS, DEPTH = 30_000, 8                  # 240 000 rows: more than bench.DUMP_ROWS, so the entity rows are a sample


def _bench(out, steps):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "1",
                        "--chains", str(CHAINS), "--depth", str(DEPTH), "--no-extras", "--cpu-frames", "0",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0
    return {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}, line


def test_dumped_outputs_are_the_timed_steps_results(tmp_path):
    import bench
    a, line = _bench(tmp_path / "a", 2)
    b, _ = _bench(tmp_path / "b", 5)
    assert sorted(a) == sorted(b) == sorted(["entity_mx", "entity_inv_mx", "entity_aabb", "entity_center", "entity_rows",
                                             "visible", "visible_count"])
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    total = sum(x.nbytes for x in a.values())
    assert total <= 64 << 20 and line["dump_outputs"]["bytes"] == total

    scene = tiler.tiled_scene(synth.entities_chains(CHAINS, DEPTH, seed=2))[0]      # bench.RankStep's workload, rank 0
    st = ob.entity_state(scene)
    st["flags"] |= np.where(st["flags"] & synth.E_ALIVE, synth.E_DIRTY, 0).astype(np.uint32)
    ob.entities_update(scene, st)
    vis, _mask = ob.entities_cull(scene["n"], st["flags"], st["aabb"], ob.frustum_from_camera(synth.camera())[0])
    rows = a["entity_rows"].astype(np.int64)
    assert rows.size == bench.DUMP_ROWS and np.all(np.diff(rows) > 0) and rows[-1] < scene["n"]
    for k in ("mx", "inv_mx", "aabb", "center"):
        assert_bits_equal(a["entity_" + k], st[k][rows], k)
    assert a["visible_count"][0] == vis.size > 0
    assert np.array_equal(a["visible"], vis.astype(np.float64))


def test_a_plain_run_times_the_headline_alone(tmp_path):
    """A plain run prints the headline and no section that takes a pass of its own; --full adds them (here the roofline
    pass and the digest: --no-extras --cpu-frames 0 keep the secondary workloads and the CPU legs out)."""
    import bench

    def line(*extra):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1",
                            "--chains", str(CHAINS), "--depth", str(DEPTH), *extra], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    plain = line()
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["unit"] == "entity updates/s"
    assert plain["higher_is_better"] is True and plain["dtype"] == "f32"
    assert plain["config"]["entities_per_gpu"] == CHAINS * DEPTH
    assert not set(bench.FULL_ONLY) & set(plain)
    full = line("--full", "--no-extras", "--cpu-frames", "0")
    assert full["roofline"]["step_us"] == pytest.approx(full["ms_per_step"] * 1e3) and full["roofline"]["mean_launch_us"] > 0
    assert "summary" in full and not {"c5", "cpu_baseline", "extra"} & set(full)
    assert [k for k in full if k not in bench.FULL_ONLY] == list(plain)
