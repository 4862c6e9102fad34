"""CPU: the view block's ABI (include/clapgpu.h, "Views in device memory", ABI 49) -- the version, the symbols, the struct
sizes as gcc makes them, and the refusals every new entry point owes before any HIP call: a NULL or misaligned block,
n_views out of 1 .. CLAPGPU_VIEW_SLOTS, and the three inconsistent clapgpu_frame descriptors.  No GPU is touched: every call
here must return CLAPGPU_ERR_INVALID_ARGUMENTS from its argument checks."""
import ctypes as C
import os
import subprocess

import pytest

from clap_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("clapgpu_views_calc", "clapgpu_entities_cull_views", "clapgpu_entities_lod_views",
               "clapgpu_visible_compact_lod_views", "clapgpu_light_grid_compute_views", "clapgpu_particles_update_views")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def mem():
    """Host memory standing in for device blocks (no call here gets as far as reading it): an aligned address, the same
    address + 4 (misaligned), and descriptors whose pointer fields all hold the aligned address."""
    raw = C.create_string_buffer(8192 + 256)
    at = (C.addressof(raw) + 255) & ~255

    def filled(cls):
        d = cls()
        for name, t in cls._fields_:
            if t is C.c_void_p:
                setattr(d, name, at)
        return d
    ent, lights, parts = filled(_lib.Entities), filled(_lib.Lights), filled(_lib.Particles)
    ent.n, lights.nr_lights, parts.n, parts.n_sys = 64, 4, 64, 1
    return dict(raw=raw, ok=at, odd=at + 4, ent=ent, lights=lights, parts=parts)


def test_abi_version_and_symbols(L):
    assert _lib.ABI_VERSION >= 49 and L.clapgpu_abi_version() == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert dict(_lib.FrameDesc._fields_)["views_source"] is C.c_void_p and dict(_lib.FrameDesc._fields_)["views_state"] is C.c_void_p


def test_struct_sizes_equal_the_headers(tmp_path):
    src, exe = tmp_path / "views.c", tmp_path / "views"
    src.write_text('#include <stdio.h>\n#include "clapgpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(clapgpu_views_source), sizeof(clapgpu_views_state), '
                   'sizeof(clapgpu_view_source), sizeof(clapgpu_view_state), CLAPGPU_VIEW_SLOTS, CLAPGPU_VIEWS_SOURCE_BYTES, '
                   'CLAPGPU_VIEWS_STATE_BYTES); return 0; }\n')
    p = subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.ViewsSource), C.sizeof(_lib.ViewsState), C.sizeof(_lib.ViewSource), C.sizeof(_lib.ViewState),
                   _lib.VIEW_SLOTS, _lib.VIEWS_SOURCE_BYTES, _lib.VIEWS_STATE_BYTES]
    assert got[0] == got[5] and got[1] == got[6] and got[4] == 1 + _lib.EXTRA_VIEWS_MAX
    assert C.sizeof(_lib.ViewState) % 16 == 0 and C.sizeof(_lib.ViewSource) % 16 == 0     # every slot is 16-byte aligned


def test_views_calc_refuses_bad_blocks_and_counts(L, mem):
    ok, odd, bad = mem["ok"], mem["odd"], _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_views_calc(None, None, ok, 1) == bad
    assert L.clapgpu_views_calc(None, ok, None, 1) == bad
    assert L.clapgpu_views_calc(None, odd, ok, 1) == bad
    assert L.clapgpu_views_calc(None, ok, odd, 1) == bad
    assert L.clapgpu_views_calc(None, ok, ok, 0) == bad
    assert L.clapgpu_views_calc(None, ok, ok, _lib.VIEW_SLOTS + 1) == bad and _lib.VIEW_SLOTS + 1 == 6


@pytest.mark.parametrize("which", ["null", "misaligned"])
def test_every_twin_refuses_a_bad_state(L, mem, which):
    st = None if which == "null" else mem["odd"]
    ok, bad = mem["ok"], _lib.ERR_INVALID_ARGUMENTS
    e, li, pa = C.byref(mem["ent"]), C.byref(mem["lights"]), C.byref(mem["parts"])
    assert L.clapgpu_entities_cull_views(None, e, st) == bad
    assert L.clapgpu_entities_lod_views(None, e, ok, ok, 0, st, None, ok, ok) == bad
    assert L.clapgpu_visible_compact_lod_views(None, e, 0, st, None, ok, ok, ok, ok, ok) == bad
    assert L.clapgpu_light_grid_compute_views(None, li, st, 1280, 720, 64, ok) == bad
    assert L.clapgpu_particles_update_views(None, pa, st) == bad


def test_twins_validate_the_rest_as_their_originals(L, mem):
    """A good block does not excuse what the original refuses: a NULL batch, a NULL output."""
    ok, bad = mem["ok"], _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_entities_cull_views(None, None, ok) == bad
    assert L.clapgpu_entities_lod_views(None, C.byref(mem["ent"]), ok, ok, 0, ok, None, None, ok) == bad
    assert L.clapgpu_visible_compact_lod_views(None, None, 0, ok, None, ok, ok, ok, ok, ok) == bad
    assert L.clapgpu_light_grid_compute_views(None, None, ok, 1280, 720, 64, ok) == bad
    assert L.clapgpu_particles_update_views(None, None, ok) == bad


def test_frame_refuses_inconsistent_views(L, mem):
    ok, bad = mem["ok"], _lib.ERR_INVALID_ARGUMENTS
    fr = _lib.Frustum()

    def issue(frustum, source, state):
        f = _lib.FrameDesc()
        f.entities = C.pointer(mem["ent"])
        if frustum:
            f.frustum = C.pointer(fr)
        f.views_source, f.views_state = source, state
        return L.clapgpu_frame_issue(None, C.byref(f), 0.0, 0)
    assert issue(True, ok, ok) == bad                        # frustum and views_state
    assert issue(False, ok, None) == bad                     # views_source without views_state
    assert issue(False, None, ok) == bad                     # and the reverse
    assert issue(False, mem["odd"], ok) == bad and issue(False, ok, mem["odd"]) == bad
