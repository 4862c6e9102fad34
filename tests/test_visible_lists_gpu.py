"""GPU: the ordered mask compaction driven bit by bit, against tests/visref.py.

Every ordered list the library hands out comes from the kernels of clap_amd/csrc/visible.hip: clapgpu_visible_compact's
single-launch path (k_visible_expand_rp over the per-row popcount bytes) and its two-launch path (k_mask_group_count +
k_visible_expand), clapgpu_visible_compact_ranges over a gathered mask, and the LOD pick that walks the list.  The scene
tests feed them whatever a frustum cull leaves; here the mask is chosen: visref.patterns() at an n on either side of every
boundary the kernels have, padding bits set, index bases up to the last 32-bit id -- through the C ABI with raw device
pointers, as tests/test_c5_gpu.py::_compact does.  Every case fills `visible`, `count` and a guard word behind them with
0xDEADBEEF and asserts the count, the list bit for bit, that nothing at or past `count` was written, and the guard.

Section 3.3 holds the producers (clapgpu_entities_cull, clapgpu_entities_update / _update_tiles) to their half of the
single-launch path's contract: vis_row_pop[w] == popcount(vis_mask[w]), no bit at or past n, no byte past the rows."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import visref
from clap_amd import synth, tiler

pytestmark = pytest.mark.gpu

# ---- the kernels' constants, read from the source: the case list below is built from them ---------------------------------------
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "clap_amd", "csrc")


def _constexpr(filename, name):
    with open(os.path.join(_CSRC, filename)) as f:
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, f.read())
    assert m, f"{name} not found in {filename}"
    return int(eval(re.sub(r"(\d)u\b", r"\1", m.group(1)), {"__builtins__": {}}))


RP_ROWS = _constexpr("visible.hip", "RP_ROWS")              # mask rows one wavefront of k_visible_expand_rp ranks
RP_MAX_ROWS = _constexpr("visible.hip", "RP_MAX_ROWS")      # the last row count of the single-launch path
GROUP_WORDS = _constexpr("visible.hip", "GROUP_WORDS")      # mask words of one workgroup of the two-launch path
MAX_SEGMENTS = _constexpr("visible.hip", "MAX_SEGMENTS")
ENT_BLOCK = _constexpr("entities_row.h", "ENT_BLOCK")
WAVE = 64
WG_ROWS = RP_ROWS * ENT_BLOCK // WAVE                       # R: rows of one workgroup of k_visible_expand_rp
WG_N = 64 * WG_ROWS
GROUP_N = 64 * GROUP_WORDS                                  # 4096 entities
STRIDE_N = GROUP_N * WAVE                                   # 64 groups: one trip of the two-launch path's prefix loop
BYTE_SUM_TRIP_N = 64 * 16 * WAVE * 8                        # wave_byte_sum: 8 loads of 16 bytes per lane and trip = 8192 rows
LAST_RP_N = 64 * RP_MAX_ROWS                                # 2^22

SINGLE_N = ([1, 63, 64, 65, 1023, 1024, 1025]
            + [WG_N * k + d for k in (1, 2) for d in (-1, 0, 1)]
            + [BYTE_SUM_TRIP_N - 1, BYTE_SUM_TRIP_N, BYTE_SUM_TRIP_N + 1, BYTE_SUM_TRIP_N + 64 * RP_ROWS + 1]
            + [LAST_RP_N - 63, LAST_RP_N])
TWO_N = ([1, 63, 64, 65, GROUP_N - 1, GROUP_N, GROUP_N + 1, STRIDE_N - 1, STRIDE_N, STRIDE_N + 1, STRIDE_N + GROUP_N + 1,
          LAST_RP_N + 1, LAST_RP_N + GROUP_N + 1])


def test_the_case_list_is_the_one_the_source_implies():
    """(needs no device, but belongs to the list above) the constants still give the sizes the cases were chosen for"""
    assert (RP_ROWS, RP_MAX_ROWS, GROUP_WORDS, MAX_SEGMENTS, ENT_BLOCK) == (16, 1 << 16, 64, 64, 256)
    assert SINGLE_N == [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 524287, 524288, 524289, 525313,
                        (1 << 22) - 63, 1 << 22]
    assert TWO_N == [1, 63, 64, 65, 4095, 4096, 4097, 262143, 262144, 262145, 266241, (1 << 22) + 1, (1 << 22) + 4097]


SENT = int(np.uint32(visref.SENTINEL).view(np.int32))
GARBAGE_U = 0xA5C3F00F
GARBAGE = int(np.uint32(GARBAGE_U).view(np.int32))


class Bufs:
    """visible[cap] | count | guard word in ONE device allocation (one download a case), and exactly
    clapgpu_visible_scratch_bytes(n) bytes of scratch with a sentinel word behind them."""

    def __init__(self, L, dev, n, cap=None):
        import torch
        self.cap = n if cap is None else cap
        self.out = torch.empty(self.cap + 2, dtype=torch.int32, device=dev)
        self.scratch_bytes = L.clapgpu_visible_scratch_bytes(n)
        assert self.scratch_bytes % 4 == 0
        self.scr = torch.empty(self.scratch_bytes // 4 + 1, dtype=torch.int32, device=dev)
        self.reset()

    def reset(self):
        self.out.fill_(SENT)
        self.scr.fill_(GARBAGE)
        self.scr[-1:].fill_(SENT)

    visible = property(lambda s: s.out.data_ptr())
    count = property(lambda s: s.out.data_ptr() + 4 * s.cap)
    scratch = property(lambda s: s.scr.data_ptr())

    def host(self):
        return self.out.cpu().numpy().view(np.uint32)

    def scratch_host(self):
        return self.scr.cpu().numpy().view(np.uint32)


def _dev_mask(words, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, np.uint64).view(np.int64)).to(dev)


def _dev_row_pop(words, n, dev, offset=0):
    """vis_row_pop as the update / cull kernels leave it, in a buffer rounded up to 16 bytes whose pad bytes are 0xFF (they
    must not be read as counts); offset: bytes the array is shifted by inside its allocation (1: not 16-byte aligned)."""
    import torch
    pop = visref.row_pop(words, n)
    host = np.full((pop.size + 15) // 16 * 16 + 16, 0xFF, np.uint8)
    host[offset:offset + pop.size] = pop
    t = torch.from_numpy(host).to(dev)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + offset


def _check(host, cap, want, what, tail=True):
    cnt = int(host[cap])
    assert cnt == want.size, f"{what}: count {cnt}, expected {want.size}"
    assert np.array_equal(host[:cnt], want), f"{what}: the list differs from the bit-level reference"
    if tail:
        assert np.all(host[cnt:cap] == visref.SENTINEL), f"{what}: written at or past count"
    assert int(host[cap + 1]) == visref.SENTINEL, f"{what}: the word behind count was written"


def _compact(L, b, mask_t, rp_ptr, n, base, scratch="own"):
    return L.clapgpu_visible_compact(None, mask_t.data_ptr(), rp_ptr, n, base, b.visible, b.count,
                                     b.scratch if scratch == "own" else scratch)


def _variants(words, n):
    """The mask with its padding bits clear and, where n leaves any, with all of them set."""
    yield "padding clear", visref.mask_padding(words, n)
    if n % 64:
        yield "padding set", visref.set_padding(words, n)


def _patterns_for(n, seed):
    return visref.patterns(visref.n_words(n), np.random.default_rng(seed), n, only=visref.pattern_names(n))


# ---- 3.1 clapgpu_visible_compact ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SINGLE_N)
def test_single_launch_path(n, cuda_device):
    """k_visible_expand_rp: vis_row_pop given, 16-byte aligned, n <= 2^22.  The scratch is garbage and stays garbage: the
    single launch ranks from the popcount bytes alone."""
    import torch
    from clap_amd import _lib
    L = _lib.lib()
    b = Bufs(L, cuda_device, n)
    for name, words in _patterns_for(n, n).items():
        want = visref.expand(words, n)
        for pad, w in _variants(words, n):
            b.reset()
            mask_t = _dev_mask(w, cuda_device)
            rp_t, rp = _dev_row_pop(words, n, cuda_device)           # from the masked word, whatever the padding holds
            assert _compact(L, b, mask_t, rp, n, 0) == _lib.OK
            torch.cuda.synchronize()
            _check(b.host(), n, want, f"n={n} {name}, {pad}")
            s = b.scratch_host()
            assert np.all(s[:-1] == GARBAGE_U) and int(s[-1]) == visref.SENTINEL, f"n={n} {name}: the single launch wrote scratch"


@pytest.mark.parametrize("n", TWO_N)
def test_two_launch_path(n, cuda_device):
    """k_mask_group_count + k_visible_expand: vis_row_pop NULL.  Exactly clapgpu_visible_scratch_bytes(n) bytes of scratch,
    garbage before the call; the word behind them survives."""
    import torch
    from clap_amd import _lib
    L = _lib.lib()
    b = Bufs(L, cuda_device, n)
    assert b.scratch_bytes == 4 * max(1, -(-n // GROUP_N))
    for name, words in _patterns_for(n, n + 1).items():
        want = visref.expand(words, n)
        for pad, w in _variants(words, n):
            b.reset()
            mask_t = _dev_mask(w, cuda_device)
            assert _compact(L, b, mask_t, None, n, 0) == _lib.OK
            torch.cuda.synchronize()
            _check(b.host(), n, want, f"n={n} {name}, {pad}")
            assert int(b.scratch_host()[-1]) == visref.SENTINEL, f"n={n} {name}: written behind the scratch"


def test_first_n_past_the_single_launch_path_with_row_pops_given(cuda_device):
    """n = 2^22 + 1 is 65 537 rows: the two-launch path even with vis_row_pop given -- and the bytes are not read: they are
    all 0xFF here."""
    import torch
    from clap_amd import _lib
    L = _lib.lib()
    n = LAST_RP_N + 1
    b = Bufs(L, cuda_device, n)
    rp_t = torch.full(((visref.n_words(n) + 15) // 16 * 16,), 0xFF, dtype=torch.uint8, device=cuda_device)
    for name, words in _patterns_for(n, 5).items():
        want = visref.expand(words, n)
        for pad, w in _variants(words, n):
            b.reset()
            mask_t = _dev_mask(w, cuda_device)
            assert _compact(L, b, mask_t, rp_t.data_ptr(), n, 0) == _lib.OK
            torch.cuda.synchronize()
            _check(b.host(), n, want, f"n={n} {name}, {pad}, vis_row_pop given")
            assert int(b.scratch_host()[-1]) == visref.SENTINEL
    # no scratch: the path that needs it refuses, and writes nothing
    b.reset()
    assert _compact(L, b, mask_t, rp_t.data_ptr(), n, 0, scratch=None) == _lib.ERR_INVALID_ARGUMENTS
    torch.cuda.synchronize()
    assert np.all(b.host() == visref.SENTINEL)


def test_which_path_runs(cuda_device):
    """What the cases above rely on.  The single-launch path leaves the scratch alone (it is how this suite tells the paths
    apart: garbage in, the same garbage out) up to and including 2^22; NULL or misaligned popcounts, or one more row, need
    the scratch: without it the call is refused."""
    import torch
    from clap_amd import _lib
    L = _lib.lib()
    for n in (64, WG_N + 1, LAST_RP_N):
        words = visref.patterns(visref.n_words(n), np.random.default_rng(1), n, only=("density_1_2",))["density_1_2"]
        mask_t = _dev_mask(words, cuda_device)
        rp_t, rp = _dev_row_pop(words, n, cuda_device)
        b = Bufs(L, cuda_device, n)
        assert _compact(L, b, mask_t, rp, n, 0) == _lib.OK
        torch.cuda.synchronize()
        _check(b.host(), n, visref.expand(words, n), f"n={n}")
        s = b.scratch_host()
        assert np.all(s[:-1] == GARBAGE_U) and int(s[-1]) == visref.SENTINEL, f"n={n}: the single launch wrote scratch"
        assert _compact(L, b, mask_t, None, n, 0, scratch=None) == _lib.ERR_INVALID_ARGUMENTS
        assert _compact(L, b, mask_t, None, n, 0) == _lib.OK
        torch.cuda.synchronize()
        assert np.any(b.scratch_host()[:-1] != GARBAGE_U), f"n={n}: the two-launch path counts into scratch"


@pytest.mark.parametrize("n", [65, WG_N * 2 + 1, BYTE_SUM_TRIP_N + 64 * RP_ROWS + 1])
def test_unaligned_row_pop_falls_back_to_two_launches(n, cuda_device):
    """A vis_row_pop pointer that is not 16-byte aligned cannot feed wave_byte_sum's 16-byte loads: the call takes the
    two-launch path, gives the same list, and without scratch is refused."""
    import torch
    from clap_amd import _lib
    L = _lib.lib()
    b = Bufs(L, cuda_device, n)
    for name, words in visref.patterns(visref.n_words(n), np.random.default_rng(n), n,
                                       only=("ones", "bits31_63", "density_1_2", "single_last")).items():
        want = visref.expand(words, n)
        w = visref.set_padding(words, n)
        mask_t = _dev_mask(w, cuda_device)
        rp_t, rp = _dev_row_pop(words, n, cuda_device, offset=1)
        assert rp % 16 == 1
        b.reset()
        assert _compact(L, b, mask_t, rp, n, 0) == _lib.OK
        torch.cuda.synchronize()
        _check(b.host(), n, want, f"n={n} {name}, vis_row_pop + 1")
        s = b.scratch_host()
        assert int(s[-1]) == visref.SENTINEL and np.any(s[:-1] != GARBAGE_U)
        b.reset()
        assert _compact(L, b, mask_t, rp, n, 0, scratch=None) == _lib.ERR_INVALID_ARGUMENTS
        torch.cuda.synchronize()
        assert np.all(b.host() == visref.SENTINEL), "a refused call wrote"


@pytest.mark.parametrize("path,n", [("single", 65), ("single", LAST_RP_N - 63), ("two", 65), ("two", LAST_RP_N + GROUP_N + 1)])
def test_index_base_up_to_the_last_id(path, n, cuda_device):
    """index_base 0, 7 and 2^32 - n: the last possible id is 0xFFFFFFFF, and the sum must not leave 32 bits on the way."""
    import torch
    from clap_amd import _lib
    L = _lib.lib()
    b = Bufs(L, cuda_device, n)
    for name, words in visref.patterns(visref.n_words(n), np.random.default_rng(3), n, only=("ones", "single_last")).items():
        mask_t = _dev_mask(visref.set_padding(words, n), cuda_device)
        rp_t, rp = _dev_row_pop(words, n, cuda_device) if path == "single" else (None, None)
        for base in (0, 7, (1 << 32) - n):
            want = visref.expand(words, n, base)
            assert int(want[-1]) == base + n - 1
            b.reset()
            assert _compact(L, b, mask_t, rp, n, base) == _lib.OK
            torch.cuda.synchronize()
            _check(b.host(), n, want, f"{path} n={n} {name} index_base={base}")


def test_arguments(cuda_device):
    import torch
    from clap_amd import _lib
    L = _lib.lib()
    n = 4097
    words = np.full(visref.n_words(n), visref.ONES, np.uint64)
    mask_t = _dev_mask(words, cuda_device)
    rp_t, rp = _dev_row_pop(words, n, cuda_device)
    b = Bufs(L, cuda_device, n)
    # n = 0: count becomes 0, nothing else is touched -- with and without the other pointers
    for args in ((mask_t.data_ptr(), rp, b.visible, b.scratch), (None, None, None, None)):
        b.reset()
        assert L.clapgpu_visible_compact(None, args[0], args[1], 0, 7, args[2], b.count, args[3]) == _lib.OK
        torch.cuda.synchronize()
        host = b.host()
        assert int(host[n]) == 0 and np.all(host[:n] == visref.SENTINEL) and int(host[n + 1]) == visref.SENTINEL
        s = b.scratch_host()
        assert np.all(s[:-1] == GARBAGE_U) and int(s[-1]) == visref.SENTINEL
    # refusals write nothing: count NULL, mask NULL, visible NULL
    b.reset()
    for rp_arg in (rp, None):
        assert L.clapgpu_visible_compact(None, mask_t.data_ptr(), rp_arg, n, 0, b.visible, None, b.scratch) == _lib.ERR_INVALID_ARGUMENTS
        assert L.clapgpu_visible_compact(None, None, rp_arg, n, 0, b.visible, b.count, b.scratch) == _lib.ERR_INVALID_ARGUMENTS
        assert L.clapgpu_visible_compact(None, mask_t.data_ptr(), rp_arg, n, 0, None, b.count, b.scratch) == _lib.ERR_INVALID_ARGUMENTS
    assert L.clapgpu_visible_compact(None, None, None, 0, 0, None, None, None) == _lib.ERR_INVALID_ARGUMENTS
    torch.cuda.synchronize()
    assert np.all(b.host() == visref.SENTINEL)
    # the scratch size at every n of this module
    for m in [0] + SINGLE_N + TWO_N:
        assert L.clapgpu_visible_scratch_bytes(m) == 4 * max(1, -(-m // GROUP_N)), m


@pytest.mark.parametrize("path,n", [("single", WG_N * 2 + 1), ("single", BYTE_SUM_TRIP_N + 1), ("two", WG_N * 2 + 1),
                                    ("two", STRIDE_N + 1)])
def test_no_state_between_calls(path, n, cuda_device):
    """ones, then zeros, then bit 63 of every word into the same visible / count / scratch, nothing cleared in between:
    each result is exact (the list up to its count; what lies behind is the previous call's)."""
    import torch
    from clap_amd import _lib
    L = _lib.lib()
    b = Bufs(L, cuda_device, n)
    pats = visref.patterns(visref.n_words(n), np.random.default_rng(0), n, only=("ones", "zeros", "bit63"))
    before = None
    for name in ("ones", "zeros", "bit63", "ones"):
        words = pats[name]
        mask_t = _dev_mask(visref.set_padding(words, n), cuda_device)
        rp_t, rp = _dev_row_pop(words, n, cuda_device) if path == "single" else (None, None)
        assert _compact(L, b, mask_t, rp, n, 0) == _lib.OK
        torch.cuda.synchronize()
        host = b.host()
        want = visref.expand(words, n)
        _check(host, n, want, f"{path} n={n} {name} after {before}", tail=False)
        if before is not None:
            assert np.array_equal(host[want.size:n], before[want.size:n]), f"{name}: written at or past count"
        before = host.copy()


# ---- 3.2 clapgpu_visible_compact_ranges -----------------------------------------------------------------------------------------
_DESCS = visref.range_descriptors()


@pytest.mark.parametrize("desc", _DESCS, ids=[d[0] for d in _DESCS])
def test_compact_ranges_matches_reference_and_host_twin(desc, cuda_device):
    import torch
    from clap_amd import _lib
    L = _lib.lib()
    name, cap_pad, base, n_pad = desc
    n_ranges = len(base)
    assert n_ranges <= MAX_SEGMENTS
    total = n_ranges * cap_pad
    b = Bufs(L, cuda_device, total)
    rng = np.random.default_rng(len(name))
    for pat in visref.RANGE_PATTERNS:
        g = visref.gathered_mask(cap_pad, n_pad, pat, rng)            # ones past every segment's n_pad
        want = visref.expand_ranges(g, cap_pad, base, n_pad)
        twin = np.zeros(max(want.size, 1), np.uint32)
        got = L.clapgpu_visible_expand_ranges_host(g.ctypes.data, n_ranges, cap_pad, base.ctypes.data, n_pad.ctypes.data,
                                                   twin.ctypes.data, want.size)
        assert got == want.size and np.array_equal(twin[:want.size], want), f"{name} {pat}: host twin"
        b.reset()
        g_t = _dev_mask(g, cuda_device)
        rc = L.clapgpu_visible_compact_ranges(None, g_t.data_ptr(), n_ranges, cap_pad, base.ctypes.data, n_pad.ctypes.data,
                                              b.visible, b.count, b.scratch)
        assert rc == _lib.OK, f"{name} {pat}: rc {rc}"
        torch.cuda.synchronize()
        _check(b.host(), total, want, f"{name} {pat}")
        assert int(b.scratch_host()[-1]) == visref.SENTINEL, f"{name} {pat}: written behind the scratch"


def test_compact_ranges_refuses_what_the_host_twin_refuses(cuda_device):
    import torch
    from clap_amd import _lib
    L = _lib.lib()
    codes = dict(invalid=_lib.ERR_INVALID_ARGUMENTS, too_large=_lib.ERR_TOO_LARGE)
    b = Bufs(L, cuda_device, 65 * 128)
    g_t = _dev_mask(np.full(65 * 2 + 4, visref.ONES, np.uint64), cuda_device)
    for name, n_ranges, cap_pad, base, n_pad, code in visref.refused_descriptors():
        rc = L.clapgpu_visible_compact_ranges(None, g_t.data_ptr(), n_ranges, cap_pad, base.ctypes.data, n_pad.ctypes.data,
                                              b.visible, b.count, b.scratch)
        assert rc == codes[code], f"{name}: rc {rc}"
    base, n_pad = np.zeros(1, np.uint32), np.full(1, 64, np.uint32)
    for args in ((None, base.ctypes.data, b.visible, b.count, b.scratch), (g_t.data_ptr(), None, b.visible, b.count, b.scratch),
                 (g_t.data_ptr(), base.ctypes.data, None, b.count, b.scratch), (g_t.data_ptr(), base.ctypes.data, b.visible, None, b.scratch),
                 (g_t.data_ptr(), base.ctypes.data, b.visible, b.count, None)):
        assert L.clapgpu_visible_compact_ranges(None, args[0], 1, 64, args[1], n_pad.ctypes.data, args[2], args[3],
                                                args[4]) == _lib.ERR_INVALID_ARGUMENTS
    torch.cuda.synchronize()
    assert np.all(b.host() == visref.SENTINEL) and int(b.scratch_host()[-1]) == visref.SENTINEL, "a refused call wrote"


# ---- 3.3 the producers keep their half of the contract ---------------------------------------------------------------------------
# With CLAPGPU_E_SKIP_CULLING on every entity no plane of any view is consulted (include/clapgpu.h, clapgpu_views): bit i of
# the main plane and of every further view's plane is ALIVE && VISIBLE of entity i, whatever the cameras see.
PRODUCER_N = (1, 63, 64, 65, 255, 256, 257, 1025)
VIEW_CAMS = [dict(pos=(40, 120, 30), quat=synth.quat_from_euler_xyz(-1.2, 0.3, 0.0), fov_deg=40.0, aspect=1.0, near=1.0, far=400.0),
             dict(pos=(-200, 10, -50), quat=synth.quat_from_euler_xyz(0.1, 1.9, 0.0)),
             dict(pos=(0, 0, 0), quat=synth.quat_from_euler_xyz(0.0, 3.1, 0.0), ndc_z_zero_one=1),
             dict(pos=(5, 400, 5), quat=synth.quat_from_euler_xyz(-1.57, 0.0, 0.0), far=90.0)]


def _flag_layouts(n):
    A, V = np.uint32(synth.E_ALIVE), np.uint32(synth.E_VISIBLE)
    i = np.arange(n)
    last = np.zeros(n, np.uint32)
    last[n - 1] = A | V
    return [("all set", np.full(n, A | V, np.uint32)),
            ("none alive", np.full(n, V, np.uint32)),
            ("alternating", np.where(i % 2 == 0, A | V, np.where(i % 4 == 1, A, V)).astype(np.uint32)),
            ("only entity n-1", last)]


def _popcounts(words):
    return np.unpackbits(np.ascontiguousarray(words, "<u8").view(np.uint8)).reshape(-1, 64).sum(axis=1).astype(np.uint8)


def _producer_scenes(layout):
    """[(n, scene)]: levels takes every n as it is (one level: nothing to pad); the tiler lays rows of 64, so it admits
    the row counts nearest to them."""
    out, seen = [], set()
    for n in PRODUCER_N:
        flat = synth.entities_flat(n, 100 + n)
        scene = synth.pad_levels(flat) if layout == "levels" else tiler.tiled_scene(flat)[0]
        if scene["n"] not in seen:
            seen.add(scene["n"])
            out.append((scene["n"], scene))
    return out


@pytest.mark.parametrize("n_extra", [0, 1, 4])
@pytest.mark.parametrize("layout", ["levels", "tiles"])
def test_producers_leave_popcounts_and_clean_padding(layout, n_extra, cuda_device):
    import torch
    from clap_amd import entities
    fr = entities.view_calc_frustum(synth.camera(pos=(3, 4, 60)))[0]
    frs = [entities.view_calc_frustum(synth.camera(**kw))[0] for kw in VIEW_CAMS[:n_extra]]
    scenes = _producer_scenes(layout)
    if layout == "levels":
        assert [n for n, _s in scenes] == list(PRODUCER_N)
    else:
        assert [n for n, _s in scenes] == sorted({-(-n // 64) * 64 for n in PRODUCER_N})
    for n, scene in scenes:
        batch = entities.EntityBatch(scene, cuda_device)
        assert batch.n == n
        if n_extra:
            batch.set_views(frs)
        n_rows = visref.n_words(n)
        planes = [("main", batch.vis_mask, batch.vis_row_pop, None)]
        planes += [(f"view {v}", batch.view_masks[v], batch.view_row_pops[v], v) for v in range(n_extra)]
        for m_t, p_t in [(p[1], p[2]) for p in planes]:
            assert m_t.numel() == n_rows and p_t.numel() == (n_rows + 15) // 16 * 16 and p_t.data_ptr() % 16 == 0
        for lname, flags in _flag_layouts(n):
            keep = flags & np.uint32(synth.E_ALIVE | synth.E_VISIBLE)
            bits = keep == np.uint32(synth.E_ALIVE | synth.E_VISIBLE)
            want_mask = np.packbits(np.concatenate([bits, np.zeros(n_rows * 64 - n, bool)]), bitorder="little").view("<u8").astype(np.uint64)
            want_list = visref.expand(want_mask, n)
            assert want_list.size == int(bits.sum())
            fl = (flags | np.uint32(synth.E_SKIP_CULLING | synth.E_DIRTY)).view(np.int32)
            for producer in ("update", "cull"):
                what = f"{layout} n={n} views={n_extra} {lname} {producer}"
                batch.flags.copy_(torch.from_numpy(fl))
                for _name, m_t, p_t, _v in planes:                   # garbage where the launch has to write
                    m_t.fill_(-1)
                    p_t.fill_(0xFF)
                if producer == "update":
                    batch.mq_update(fr)
                else:
                    batch.cull(fr)
                torch.cuda.synchronize()
                for pname, m_t, p_t, v in planes:
                    mask = m_t.cpu().numpy().view(np.uint64)
                    pop = p_t.cpu().numpy()
                    assert np.array_equal(mask, want_mask), f"{what}, {pname}: bit i != ALIVE && VISIBLE of entity i (or a bit at or past n)"
                    assert np.array_equal(pop[:n_rows], _popcounts(mask)), f"{what}, {pname}: vis_row_pop != popcount(vis_mask)"
                    assert np.all(pop[n_rows:] == 0xFF), f"{what}, {pname}: vis_row_pop written past ceil(n / 64)"
                    # ... and the consumer on exactly what the producer left
                    batch.visible.fill_(SENT)
                    if v is None:
                        batch.compact_visible()
                    else:
                        batch.compact_view(v)
                    out = batch.download()
                    assert out["visible_count"] == want_list.size, f"{what}, {pname}: count"
                    assert np.array_equal(out["visible"], visref.expand(mask, n)), f"{what}, {pname}: list"
                    tail = batch.visible.cpu().numpy().view(np.uint32)[want_list.size:]
                    assert np.all(tail == visref.SENTINEL), f"{what}, {pname}: written at or past count"
                batch.compact_visible(two_pass=True)
                assert np.array_equal(batch.download()["visible"], want_list), f"{what}: two-launch list of the main plane"


# ---- 3.4 the list's consumer -------------------------------------------------------------------------------------------------------
LOD_KEEP = -9                                                   # cur_lod / draw_lod entries nobody may write


def _lod_batch(n, dev, seed=9):
    """A flat batch of n entities whose every entity has a forced LOD: the expected draw_lod is the forced value, no
    distance and no cube root are involved."""
    from clap_amd import entities
    scene = synth.pad_levels(synth.entities_flat(n, seed))
    scene["model_lod"] = np.asarray([[0, 7]], np.uint8)
    batch = entities.EntityBatch(scene, dev)
    batch.mq_update(None, all_dirty=True)                               # boxes and centres (read only without a forced LOD)
    force = ((np.arange(n) * 7 + 3) % 5).astype(np.int32)
    return batch, force


def _lod_call(L, batch, vis_t, cnt_t, base, force_t, cur_t, draw_t):
    from clap_amd import _lib
    cp = (C.c_float * 3)(1.0, 2.0, 3.0)
    rc = L.clapgpu_entities_lod(None, C.byref(batch._desc), vis_t.data_ptr(), cnt_t.data_ptr(), base, cp, force_t.data_ptr(),
                                cur_t.data_ptr(), draw_t.data_ptr())
    _lib.check(rc, "clapgpu_entities_lod")


def test_lod_walks_the_list_it_is_given(cuda_device):
    import torch
    from clap_amd import _lib
    L = _lib.lib()
    n = 300
    batch, force = _lod_batch(n, cuda_device)
    force_t = torch.from_numpy(force).to(cuda_device)
    dev = cuda_device

    def buffers(ids, count):
        vis_t = torch.from_numpy(np.asarray(ids, np.uint32).view(np.int32).copy()).to(dev)
        cnt_t = torch.tensor([count], dtype=torch.int32, device=dev)
        cur_t = torch.full((2 * n,), LOD_KEEP, dtype=torch.int32, device=dev)     # [n, 2n): where a stray cur_lod entry would land
        draw_t = torch.full((n + 64,), LOD_KEEP, dtype=torch.int32, device=dev)
        return vis_t, cnt_t, cur_t, draw_t

    # a list with index_base = 7
    own = np.flatnonzero(np.arange(n) % 3 != 1)
    vis_t, cnt_t, cur_t, draw_t = buffers(own + 7, own.size)
    _lod_call(L, batch, vis_t, cnt_t, 7, force_t, cur_t, draw_t)
    torch.cuda.synchronize()
    draw, cur = draw_t.cpu().numpy(), cur_t.cpu().numpy()
    assert np.array_equal(draw[:own.size], force[own]) and np.all(draw[own.size:] == LOD_KEEP)
    want_cur = np.full(2 * n, LOD_KEEP, np.int32)
    want_cur[own] = force[own]
    assert np.array_equal(cur, want_cur), "cur_lod follows the entities on the list, and only them"

    # ids of another shard on the list (id - index_base >= n, below the base included): drawn with 0, no cur_lod entry
    base = 640
    ids = np.asarray([0, 6, base - 1, base, base + 5, base + n - 1, base + n, base + n + 17, base + 2 * n - 1, 0xFFFFFFFF], np.uint64)
    mine = (ids >= base) & (ids < base + n)
    vis_t, cnt_t, cur_t, draw_t = buffers(ids, ids.size)
    _lod_call(L, batch, vis_t, cnt_t, base, force_t, cur_t, draw_t)
    torch.cuda.synchronize()
    draw, cur = draw_t.cpu().numpy(), cur_t.cpu().numpy()
    local = (ids[mine] - base).astype(np.int64)
    want_draw = np.where(mine, force[np.where(mine, ids - base, 0).astype(np.int64)], 0)
    assert np.array_equal(draw[:ids.size], want_draw) and np.all(draw[ids.size:] == LOD_KEEP)
    want_cur = np.full(2 * n, LOD_KEEP, np.int32)
    want_cur[local] = force[local]
    assert np.array_equal(cur, want_cur), "an id of another shard wrote a cur_lod entry"

    # *count larger than n: n entries are walked, draw_lod[n:] keeps what it held
    vis_t, cnt_t, cur_t, draw_t = buffers(np.arange(n) + 7, n + 50)
    _lod_call(L, batch, vis_t, cnt_t, 7, force_t, cur_t, draw_t)
    torch.cuda.synchronize()
    draw, cur = draw_t.cpu().numpy(), cur_t.cpu().numpy()
    assert np.array_equal(draw[:n], force) and np.all(draw[n:] == LOD_KEEP)
    assert np.array_equal(cur[:n], force) and np.all(cur[n:] == LOD_KEEP)

    # count = 0: nothing is written
    vis_t, cnt_t, cur_t, draw_t = buffers(np.arange(n), 0)
    _lod_call(L, batch, vis_t, cnt_t, 0, force_t, cur_t, draw_t)
    torch.cuda.synchronize()
    assert np.all(draw_t.cpu().numpy() == LOD_KEEP) and np.all(cur_t.cpu().numpy() == LOD_KEEP)


@pytest.mark.parametrize("n", [1, 65, 4097])
def test_compact_lod_is_compact_then_lod(n, cuda_device):
    """clapgpu_visible_compact_lod: the list of clapgpu_visible_compact and the draw_lod / cur_lod of the two calls, over a
    mask put into the batch bit by bit (index_base 7)."""
    import torch
    from clap_amd import _lib
    L = _lib.lib()
    batch, force = _lod_batch(n, cuda_device, seed=n)
    force_t = torch.from_numpy(force).to(cuda_device)
    cp = (C.c_float * 3)(1.0, 2.0, 3.0)
    for name, words in visref.patterns(visref.n_words(n), np.random.default_rng(n), n,
                                       only=("ones", "zeros", "bits31_63", "density_1_2", "single_last")).items():
        want = visref.expand(words, n, 7)
        ids = (want - 7).astype(np.int64)
        batch.vis_mask.copy_(_dev_mask(visref.set_padding(words, n), cuda_device))
        batch.vis_row_pop.fill_(0xFF)
        batch.vis_row_pop[:visref.n_words(n)].copy_(torch.from_numpy(visref.row_pop(words, n)))
        results = []
        for fused in (False, True):
            b = Bufs(L, cuda_device, n)
            cur_t = torch.full((n,), LOD_KEEP, dtype=torch.int32, device=cuda_device)
            draw_t = torch.full((n + 1,), LOD_KEEP, dtype=torch.int32, device=cuda_device)
            if fused:
                rc = L.clapgpu_visible_compact_lod(None, C.byref(batch._desc), 7, cp, force_t.data_ptr(), cur_t.data_ptr(), b.visible,
                                                   b.count, draw_t.data_ptr(), b.scratch)
                _lib.check(rc, "clapgpu_visible_compact_lod")
            else:
                assert _compact(L, b, batch.vis_mask, batch.vis_row_pop.data_ptr(), n, 7) == _lib.OK
                rc = L.clapgpu_entities_lod(None, C.byref(batch._desc), b.visible, b.count, 7, cp, force_t.data_ptr(), cur_t.data_ptr(),
                                            draw_t.data_ptr())
                _lib.check(rc, "clapgpu_entities_lod")
            torch.cuda.synchronize()
            host = b.host()
            _check(host, n, want, f"n={n} {name} fused={fused}")
            results.append((host, draw_t.cpu().numpy(), cur_t.cpu().numpy()))
        (h0, d0, c0), (h1, d1, c1) = results
        assert np.array_equal(h0, h1) and np.array_equal(d0, d1) and np.array_equal(c0, c1), f"n={n} {name}: one call != two calls"
        assert np.array_equal(d1[:want.size], force[ids]) and np.all(d1[want.size:] == LOD_KEEP), f"n={n} {name}: draw_lod"
        want_cur = np.full(n, LOD_KEEP, np.int32)
        want_cur[ids] = force[ids]
        assert np.array_equal(c1, want_cur), f"n={n} {name}: cur_lod"
