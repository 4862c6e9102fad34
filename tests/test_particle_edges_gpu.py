"""GPU: the particle kernels (clap_amd/csrc/particles.hip) against the oracle on the chosen cases of tests/partcases.py,
bit for bit, every device array between guard bands.

The respawn ranking is driven through its edges by construction: the first frame's respawn set is chosen bit by bit
(tests/test_particle_edges.py checks with the oracle that it is the chosen one), the next frames run free.  Every
pattern goes down every route of particles_update -- with the group counts, without them, and the ordered compaction
with the list kernel, which a popcount array that is not 16-byte aligned selects at any size -- and the routes must give
the same bits.  The threshold case holds particles one float32 step on either side of dd > radius_squared."""
import numpy as np
import pytest
import torch

import guards
import partcases as pc
from clap_amd import particles
from clap_amd.views import ViewBlock
from helpers import assert_bits_equal
from oracle import binding as ob
from test_frame_views_gpu import cam_source, host_view, put
from clap_amd import synth

pytestmark = pytest.mark.gpu

FRAMES = 4                   # frame 0 and three that run free: both banks of the group counts are filled and cleared twice
ROUTES = ("group_counts", "no_group_counts", "list")
CAM = synth.camera(pos=(5, 8, 40), quat=(0.0, 0.2588190451, 0.0, 0.9659258263))


@pytest.fixture
def g(cuda_device, monkeypatch):
    """The registry of the test: every array the mirrors allocate from here on stands between guard bands."""
    reg = guards.Guards(cuda_device)
    guards.install(monkeypatch, reg)
    return reg


def oracle_frames(ps, pos, vel, frames=FRAMES):
    """[(respawn count, pos, vel, state)] of `frames` frames from STATE0"""
    p, v, st, out = pos.copy(), vel.copy(), pc.STATE0, []
    for _ in range(frames):
        k, st = ob.particles_update(ps, p, v, st)
        out.append((k, p.copy(), v.copy(), st))
    return out


def make_batch(ps, pos, vel, route, g, device):
    batch = particles.ParticleBatch(ps, pos.copy(), vel.copy(), pc.STATE0, device)
    for name in ("pos", "vel", "sys", "row_sys", "rng_state", "billboard_mx", "respawn_mask", "respawn_row_pop", "respawn_list",
                 "respawn_count", "scratch", "respawn_groups"):
        assert g.owns(getattr(batch, name)), f"ParticleBatch.{name} is not under guard"
    batch.billboard_mx.fill_(-3.0)
    if route == "no_group_counts":
        batch._desc.respawn_groups = None
    elif route == "list":
        # one byte into a larger guarded array: not 16-byte aligned, so particles_update takes the compaction and the list
        # kernel at this size too
        batch.unaligned_pop = g.array((batch.respawn_row_pop.numel() + 16,), torch.uint8)
        batch._desc.respawn_row_pop = batch.unaligned_pop.data_ptr() + 1
        assert batch._desc.respawn_row_pop % 16 == 1
    return batch


def run_and_compare(ps, pos, vel, exp, route, g, device, chosen=None, block=None, view=None):
    """FRAMES frames of one batch against the oracle's; frame 0's respawn mask against the chosen bits.  Returns the last
    frame's download and billboards."""
    batch = make_batch(ps, pos, vel, route, g, device)
    what = f"{route}{' through the view block' if block is not None else ''}"
    for f, (k, p, v, st) in enumerate(exp):
        batch.particles_update(view) if block is None else batch.particles_update_views(block)
        out = batch.download()
        assert out["respawned"] == k, f"{what}, frame {f}: {out['respawned']} respawns, the oracle has {k}"
        assert_bits_equal(out["pos"], p, f"{what}, frame {f}: pos_array")
        assert_bits_equal(out["vel"], v, f"{what}, frame {f}: velocity")
        assert out["rng_state"] == st, f"{what}, frame {f}: drand48 state"
        if f == 0 and chosen is not None:
            mask = batch.respawn_mask.cpu().numpy().view(np.uint64)[:ps["n"] // 64]
            assert np.array_equal(mask, pc.mask_words(ps["n"], chosen)), f"{what}: frame 0's respawn mask is not the chosen bits"
        g.check(f"{what}, frame {f}")
    return out


def billboards(ps, view):
    return np.stack([ob.particles_billboard(view, c) for c in ps["sys"]["center"]])


CASES = [("full", name) for name in pc.PATTERN_NAMES] + [("partial", name) for name in pc.PARTIAL_PATTERNS]


@pytest.mark.parametrize("which,name", CASES, ids=[f"{w}-{n}" for w, n in CASES])
def test_chosen_respawn_pattern_down_every_route(which, name, g, cuda_device):
    ps = pc.layouts()[which]
    chosen = pc.patterns(ps)[name]
    pos, vel = pc.at_rest(ps, chosen)
    exp = oracle_frames(ps, pos, vel)
    assert exp[0][0] == len(chosen)
    view = host_view(CAM["cam_pos"], CAM["cam_quat"])
    live = pc.live_mask(ps)
    for route in ROUTES:
        out = run_and_compare(ps, pos, vel, exp, route, g, cuda_device, chosen, view=view)
        assert_bits_equal(out["pos"][~live], pos[~live], f"{route}: the padded lanes are where they were parked")
        assert not out["vel"][~live].any(), f"{route}: the padded lanes have no velocity"
        assert_bits_equal(out["billboard_mx"], billboards(ps, view), f"{route}: billboards")
    if which == "full" and name in pc.VIEWS_PATTERNS:
        s = cam_source(CAM)
        block = ViewBlock(cuda_device)
        put(block, 0, s)
        block.upload()
        block.calc(1)
        for route in ("group_counts", "list"):
            out = run_and_compare(ps, pos, vel, exp, route, g, cuda_device, chosen, block=block)
            assert_bits_equal(out["billboard_mx"], billboards(ps, view), f"{route} through the view block: billboards")


@pytest.mark.parametrize("route", ROUTES)
def test_threshold_edges(route, g, cuda_device):
    t = pc.threshold_case()
    exp = oracle_frames(t["ps"], t["pos"], t["vel"], 3)
    assert exp[0][0] == len(t["expect"])
    run_and_compare(t["ps"], t["pos"], t["vel"], exp[:3], route, g, cuda_device, t["expect"], view=np.eye(4, dtype=np.float32).ravel())
