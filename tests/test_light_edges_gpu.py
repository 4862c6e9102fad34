"""GPU: the light-grid kernel and the carrier kernel (clap_amd/csrc/lights.hip) against the oracle on the chosen cases of
tests/lightcases.py, bit for bit, every device array between guard bands.

The random cases of test_light.py almost never put a light next to a decision of the kernel; these cases put one on
either side of every decision, one float32 step apart (tests/test_light_edges.py checks that they do).  A kernel that
fuses one multiply-add, or that makes one of the two double comparisons in float, gets them wrong."""
import numpy as np
import pytest
import torch

import guards
import lightcases as lc
from clap_amd import entities, lights as gl
from clap_amd.views import ViewBlock
from test_frame_views_gpu import matrix_source, put
from test_light_edges import load_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture
def g(cuda_device, monkeypatch):
    """The registry of the test: every array the mirrors allocate from here on stands between guard bands."""
    reg = guards.Guards(cuda_device)
    guards.install(monkeypatch, reg)
    return reg


def gpu_tiles(c, device, block=None):
    ls = gl.LightSet(device, c["width"], c["height"], c["cell"])
    ls.load(c["lights"])
    tiles = ls.grid_compute(c["view"], c["proj"]) if block is None else ls.grid_compute_views(block)
    assert tiles is not None
    tiles.fill_(-1)                                         # every tile is written by the launch that follows
    ls.grid_compute(c["view"], c["proj"]) if block is None else ls.grid_compute_views(block)
    return ls.download_tiles()


def view_block(c, device):
    """A view block whose slot 0 holds the case's camera"""
    block = ViewBlock(device)
    put(block, 0, matrix_source(c["view"], c["proj"], pos=c["cam"]["cam_pos"], z01=int(c["cam"]["ndc_z_zero_one"][0])))
    block.upload()
    block.calc(1)
    return block


def differing(got, exp):
    bad = np.argwhere(lc.columns(got) != lc.columns(exp))
    return f"{len(bad)} bits differ, first (gy, gx, slot): {bad[:6].tolist()}"


def check(c, g, device, views=False):
    exp = lc.oracle_tiles(c)
    got = gpu_tiles(c, device)
    assert got.shape == exp.shape and np.array_equal(got, exp), f"{c['name']}: {differing(got, exp)}"
    if views:
        twin = gpu_tiles(c, device, view_block(c, device))
        assert np.array_equal(twin, exp), f"{c['name']} through the view block: {differing(twin, exp)}"
    g.check(c["name"])
    return exp


# ------------------------------------------------------------------------------------------------- 1. disc edges
@pytest.mark.parametrize("k", range(len(lc.CAMERAS) * len(lc.GRIDS)))
def test_disc_edges(k, g, cuda_device):
    near, far, found = lc.disc_edge_pairs()[k]
    assert found.all()
    a = check(near, g, cuda_device, views=True)
    b = check(far, g, cuda_device, views=True)
    assert (lc.columns(a) != lc.columns(b)).any(axis=(0, 1)).all(), "every slot's column differs between the two sets"


# ------------------------------------------------------------------------------------------------- 2. gate edges
@pytest.mark.parametrize("k", range(len(lc.GATE_CAMERAS)))
def test_gate_edges(k, g, cuda_device):
    c, _info = lc.gate_cases()[k]
    exp = check(c, g, cuda_device, views=True)
    lit = np.flatnonzero(lc.columns(exp).any(axis=(0, 1)))
    assert set(lit) == {lc.GATE_SLOTS["far_lit"], lc.GATE_SLOTS["eye_lit"]}


# ------------------------------------------------------------------------------------------------- 3. radius edges
@pytest.mark.parametrize("k", range(2))
def test_degenerate_lights(k, g, cuda_device):
    check(lc.radius_cases()[k], g, cuda_device)


# ------------------------------------------------------------------------------------------------- 4. slots and words
def test_slots_and_words(g, cuda_device):
    for c in lc.slot_cases():
        exp = check(c, g, cuda_device, views=True)
        if c["name"].startswith("lone_"):
            s = int(c["name"].split("_")[2])
            assert np.array_equal(exp, np.broadcast_to(lc.lone_bit(s), exp.shape))


# ------------------------------------------------------------------------------------------------- 5. grid shapes
@pytest.mark.parametrize("n_tiles", sorted(lc.SHAPES))
def test_grid_shapes(n_tiles, g, cuda_device):
    c = {int(c["name"].split("_")[1]): c for c in lc.shape_cases()}[n_tiles]
    exp = check(c, g, cuda_device)
    assert exp.shape[0] * exp.shape[1] == n_tiles


# ------------------------------------------------------------------------------------------------- the fixture
def test_hip_matches_the_reference_on_the_edge_fixture(g, cuda_device, golden_dir):
    for c, ref_tiles in load_fixture(golden_dir):
        got = gpu_tiles(c, cuda_device)
        assert np.array_equal(got, ref_tiles), f"{c['name']}: {differing(got, ref_tiles)}"
    g.check("lightgrid_edges")


# ------------------------------------------------------------------------------------------------- 7. carriers
@pytest.mark.parametrize("nc", lc.CARRIER_COUNTS)
def test_carriers_across_the_stride(nc, g, cuda_device):
    c = lc.carrier_case(nc)
    batch = entities.EntityBatch(c["scene"], cuda_device)
    assert g.owns(batch.pos_scale) and g.owns(batch.flags), "the entity arrays stand under guard"
    ls = gl.LightSet(cuda_device, 640, 360, 64)
    car = c["carriers"]
    ls.set_carriers(car["entity"], car["light"], car["off"])
    n = c["lights"]["nr_lights"]
    for all_dirty in (False, True):
        ls.load(c["lights"])
        ls.from_entities(batch, all_dirty=all_dirty)
        exp = lc.carrier_expected(c, all_dirty)
        got = ls.download_pos()
        assert np.array_equal(got[:n].view(np.uint32), exp.view(np.uint32)), \
            f"{nc} carriers, all_dirty={all_dirty}: slots {np.flatnonzero((got[:n] != exp).any(axis=1))} differ"
        assert not got[n:].any(), "slots at and past nr_lights are not written"
        g.check(f"{nc} carriers, all_dirty={all_dirty}")
    torch.cuda.synchronize()
