"""CPU: the reference of the ordered mask compaction checks itself (tests/visref.py), and the host twin of the segment
expansion -- clapgpu_visible_expand_ranges_host, what a rank without the device list runs -- is held to it at the
descriptors and masks tests/test_visible_lists_gpu.py puts to the kernels.  Every comparison is equality of integers."""
import numpy as np
import pytest

import visref


def _lib():
    from clap_amd import _lib as L
    return L.lib()


def _host(g, n_ranges, cap_pad, base, n_pad, out=None, capacity=0):
    g = np.ascontiguousarray(g, np.uint64)
    return _lib().clapgpu_visible_expand_ranges_host(g.ctypes.data, n_ranges, cap_pad, base.ctypes.data,
                                                     None if n_pad is None else n_pad.ctypes.data,
                                                     None if out is None else out.ctypes.data, capacity)


# ---- the reference against itself ---------------------------------------------------------------------------------------------
def _expand_by_loop(words, n, index_base=0):
    out = []
    for w, word in enumerate(words):
        v = int(word)
        while v:
            low = v & -v
            i = w * 64 + low.bit_length() - 1
            if i < n:
                out.append(index_base + i)
            v ^= low
    assert all(x < (1 << 32) for x in out)
    return np.asarray(out, np.uint32)


SMALL_N = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4097)


@pytest.mark.parametrize("n", SMALL_N)
def test_reference_agrees_with_a_plain_loop_and_ignores_padding(n):
    rng = np.random.default_rng(n)
    nw = visref.n_words(n)
    pats = visref.patterns(nw, rng, n)
    assert set(visref.pattern_names(n)) == set(pats) and set(visref.LARGE_SUBSET) <= set(pats)
    for name, words in pats.items():
        for base in (0, 7, (1 << 32) - n):
            want = _expand_by_loop(words, n, base)
            assert np.array_equal(visref.expand(words, n, base), want), (name, base)
            assert np.array_equal(visref.expand(visref.set_padding(words, n), n, base), want), (name, base, "padding set")
            assert np.array_equal(visref.expand(visref.mask_padding(words, n), n, base), want), (name, base, "padding clear")
        pop = visref.row_pop(visref.set_padding(words, n), n)
        assert pop.dtype == np.uint8 and pop.size == nw
        assert [int(x) for x in pop] == [bin(int(w)).count("1") for w in visref.mask_padding(words, n)], name
        assert int(pop.astype(np.int64).sum()) == want.size
    assert np.array_equal(visref.expand(pats["single_last"], n), [n - 1])
    assert np.array_equal(visref.expand(pats["single_first"], n), [0])
    assert np.array_equal(visref.expand(pats["ones"], n), np.arange(n))
    assert visref.expand(pats["ones"], n, (1 << 32) - n)[-1] == 0xFFFFFFFF


def test_reference_patterns_put_the_prefix_where_they_say():
    rng = np.random.default_rng(1)
    p = visref.patterns(2048, rng)
    for m in (16, 64, 1024):
        rows = np.flatnonzero(p[f"rows_last_of_{m}"])
        assert np.array_equal(rows, np.arange(m - 1, 2048, m)) and np.all(p[f"rows_last_of_{m}"][rows] == visref.ONES)
        assert np.array_equal(np.flatnonzero(p[f"rows_first_of_{m}"]), np.arange(0, 2048, m))
    for name, dens in (("density_1_64", 1 / 64), ("density_1_2", 0.5), ("density_63_64", 63 / 64)):
        got = visref.expand(p[name], 2048 * 64).size / (2048 * 64)
        assert abs(got - dens) < 0.01, name                       # 131 072 draws: sigma <= 0.0014
    assert int(p["bits31_63"][5]) == (1 << 31) | (1 << 63) and int(p["x5555"][0]) ^ int(p["xAAAA"][0]) == (1 << 64) - 1


def test_reference_refuses_an_id_past_32_bits():
    with pytest.raises(AssertionError):
        visref.expand(np.full(1, visref.ONES, np.uint64), 64, (1 << 32) - 63)


def test_reference_expand_ranges_is_expand_per_segment():
    rng = np.random.default_rng(2)
    for name, cap_pad, base, n_pad in visref.range_descriptors():
        g = visref.gathered_mask(cap_pad, n_pad, "density_1_2", rng)
        cw = cap_pad // 64
        want = []
        for r in range(len(base)):
            want.extend(_expand_by_loop(g[r * cw:r * cw + int(n_pad[r]) // 64], int(n_pad[r]), int(base[r])))
        got = visref.expand_ranges(g, cap_pad, base, n_pad)
        assert np.array_equal(got, np.asarray(want, np.uint32)), name
        assert np.all(np.diff(got.astype(np.int64)) > 0), name
        zeroed = g.copy()                                           # the words past n_pad[r]: ones or zeros, the same list
        for r in range(len(base)):
            zeroed[r * cw + int(n_pad[r]) // 64:(r + 1) * cw] = 0
        assert np.array_equal(visref.expand_ranges(zeroed, cap_pad, base, n_pad), got), name
    names = [d[0] for d in visref.range_descriptors()]
    last = visref.range_descriptors()[-1]
    assert "ends_at_2_32" in names[-1] and int(last[2][-1]) + int(last[3][-1]) == 1 << 32


# ---- the host twin --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("desc", visref.range_descriptors(), ids=[d[0] for d in visref.range_descriptors()])
def test_host_twin_matches_reference(desc):
    name, cap_pad, base, n_pad = desc
    rng = np.random.default_rng(len(name))
    for pat in visref.RANGE_PATTERNS:
        g = visref.gathered_mask(cap_pad, n_pad, pat, rng)
        want = visref.expand_ranges(g, cap_pad, base, n_pad)
        # visible = NULL: the count alone
        assert _host(g, len(base), cap_pad, base, n_pad) == want.size, (pat, "count")
        out = np.full(want.size + 2, visref.SENTINEL, np.uint32)
        assert _host(g, len(base), cap_pad, base, n_pad, out, want.size) == want.size, pat
        assert np.array_equal(out[:want.size], want), (pat, "list")
        assert np.all(out[want.size:] == visref.SENTINEL), (pat, "written past the count")
        # a capacity below the count: the full count comes back, exactly `capacity` ids are written
        if want.size > 1:
            cap = want.size // 2
            out = np.full(want.size + 2, visref.SENTINEL, np.uint32)
            assert _host(g, len(base), cap_pad, base, n_pad, out, cap) == want.size, (pat, "short capacity: count")
            assert np.array_equal(out[:cap], want[:cap]) and np.all(out[cap:] == visref.SENTINEL), (pat, "short capacity")
        out = np.full(4, visref.SENTINEL, np.uint32)
        assert _host(g, len(base), cap_pad, base, n_pad, out, 0) == want.size and np.all(out == visref.SENTINEL)
    # n_pad = NULL: every segment holds cap_pad slots (descriptors whose bases leave room for that)
    full = np.full(len(base), cap_pad, np.uint32)
    ends = base.astype(np.int64) + cap_pad
    if np.all(ends[:-1] <= base[1:].astype(np.int64)) and ends[-1] <= 1 << 32:
        g = visref.gathered_mask(cap_pad, full, "density_1_2", rng)
        want = visref.expand_ranges(g, cap_pad, base, full)
        out = np.zeros(max(want.size, 1), np.uint32)
        assert _host(g, len(base), cap_pad, base, None, out, want.size) == want.size
        assert np.array_equal(out[:want.size], want)


@pytest.mark.parametrize("case", visref.refused_descriptors(), ids=[c[0] for c in visref.refused_descriptors()])
def test_host_twin_refuses(case):
    _name, n_ranges, cap_pad, base, n_pad, _code = case
    g = np.full(max(1, (cap_pad // 64) * max(n_ranges, 1)) + 4, visref.ONES, np.uint64)
    out = np.full(8, visref.SENTINEL, np.uint32)
    assert _host(g, n_ranges, cap_pad, base, n_pad, out, 8) == 0
    assert np.all(out == visref.SENTINEL), "a refused descriptor wrote ids"
    assert _host(g, n_ranges, cap_pad, base, n_pad) == 0


def test_host_twin_refuses_null_mask_and_null_bases():
    base, n_pad = np.zeros(1, np.uint32), np.full(1, 64, np.uint32)
    L = _lib()
    assert L.clapgpu_visible_expand_ranges_host(None, 1, 64, base.ctypes.data, n_pad.ctypes.data, None, 0) == 0
    g = np.full(1, visref.ONES, np.uint64)
    assert L.clapgpu_visible_expand_ranges_host(g.ctypes.data, 1, 64, None, n_pad.ctypes.data, None, 0) == 0
    assert L.clapgpu_visible_expand_ranges_host(g.ctypes.data, 1, 64, base.ctypes.data, n_pad.ctypes.data, None, 0) == 64
