"""GPU: the pose kernel (clap_amd/csrc/pose.hip) against the oracle on the chosen cases of tests/posecases.py, bit for bit.

Every model runs two frames -- its frame times (every key of every channel length, the floats beside it, inside, before,
past, 0, time_end, -inf, +inf), then the list rotated by one character -- and T / R / S, the palette and the joint positions
must be the oracle's bit patterns.  tests/test_pose_edges.py holds the cases to what they claim, with the oracle alone.

Each model must run the kernel instantiation it was built for: the launch's CLAPGPU_POSE_DEBUG line names MISSING,
TIMES_LDS and kp, and they are asserted per case -- a later change of POSE_TIMES_LDS_MAX would otherwise move every
boundary case to one side without a test noticing.

Measured on the MI355X: see the CHANGELOG entry (every `pose edges` row of parity_bounds.json at 0.0)."""
import re

import numpy as np
import pytest

import posecases as pc
from oracle import binding as ob
from test_pose_skin_gpu import assert_pose_equal, oracle_pose

pytestmark = pytest.mark.gpu

DEBUG_LINE = re.compile(r"k_pose<(\d+), (\d+)>: .*static LDS (\d+) \+ dynamic (\d+), (\d+) program passes, "
                        r"MISSING (\d), TIMES_LDS (\d), kp (\d+)")


def times_in_lds(c):
    """What the launch must choose.  The key times fit by the head_floats rule (posecases.times_lds_rule); at 256 lanes per
    character the kernel's static LDS leaves room for two passes of the level program, and a skeleton of more than 64
    joints needs at least six (posecases.program_passes_wanted): pose_launch then takes the times through L2."""
    return c["times_lds"] and c["lanes"] < 256


def run_case(name, cuda_device, monkeypatch, capfd, trs_on=True, blocks=None):
    from clap_amd import animation
    c = pc.case(name)
    sk = dict(c["sk"])
    sk["bind"] = ob.skeleton_bind(sk)
    monkeypatch.setenv("CLAPGPU_POSE_DEBUG", "1")
    if blocks:
        monkeypatch.setenv("CLAPGPU_POSE_BLOCKS", str(blocks))
    model = animation.SkinnedModel(sk, c["anims"], bind=sk["bind"], device=cuda_device)
    batch = animation.CharacterBatch(model, c["n_chars"], c["trs0"], c["char_mx"])
    batch.set_outputs(trs=trs_on, joint_pos=True)
    trs = np.ascontiguousarray(np.tile(c["trs0"], (c["n_chars"], 1, 1)))
    reach = sk["order"]
    capfd.readouterr()
    for f, (t, which) in enumerate(pc.frames(c)):
        jt, _gl, jp = oracle_pose(sk, c["anims"], which, t, c["char_mx"], trs)
        batch.set_frame_times(t, which)
        batch.pose_update()
        out = batch.download()
        lines = DEBUG_LINE.findall(capfd.readouterr().err)
        assert len(lines) == 1, f"{name} frame {f}: {len(lines)} launches of k_pose reported"
        lpc, _block, _stat, _dyn, _passes, missing, lds, kp = (int(x) for x in lines[0])
        assert (lpc, missing, lds, kp) == (c["lanes"], int(c["missing"]), int(times_in_lds(c)), c["kp"]), \
            f"{name}: k_pose<{lpc}> ran with MISSING {missing}, TIMES_LDS {lds}, kp {kp}; the case was built for " \
            f"k_pose<{c['lanes']}> MISSING {int(c['missing'])}, TIMES_LDS {int(times_in_lds(c))}, kp {c['kp']}"
        try:
            assert_pose_equal(out, trs, jt, jp, reach, f"{name} frame {f}", trs_on=trs_on, key="pose edges")
        except AssertionError as e:
            raise AssertionError(f"{e}\n{pc.first_difference(c, f, t, out, trs, jt, jp, reach, trs_on)}") from None
    assert np.isfinite(trs).all()
    return c


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_pose_edges_match_oracle(name, cuda_device, monkeypatch, capfd):
    run_case(name, cuda_device, monkeypatch, capfd)


def test_pose_edges_palette_only(cuda_device, monkeypatch, capfd):
    """set_outputs(trs=False): the same edges through the stores of a launch that leaves T / R / S unwritten (a model
    without missing channels; the palette and the joint positions carry the comparison)"""
    c = run_case("search_31", cuda_device, monkeypatch, capfd, trs_on=False)
    assert not c["missing"]


def test_pose_edges_two_blocks(cuda_device, monkeypatch, capfd):
    """CLAPGPU_POSE_BLOCKS=2: two persistent blocks of 12 characters take 2 000 characters, more than 64 rounds each, so
    the edges also pass the reload of the per-character scalars (animation, frame time, entity) every 64 iterations"""
    c = run_case("search_127", cuda_device, monkeypatch, capfd, blocks=2)
    assert c["n_chars"] > 2 * 12 * 64
