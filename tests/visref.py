"""The bit-level truth of the ordered mask compaction, and the masks that drive it (no device code).

Every ordered list the library hands out -- clapgpu_visible_compact's two paths, clapgpu_visible_compact_ranges and its
host twin -- is, by definition, "the positions of the set bits of a mask, ascending, plus a base".  expand() says that
with numpy's unpackbits / flatnonzero and nothing else; patterns() makes the masks at which a rank, a prefix or a tail
goes wrong: all / none, the sign bits of the two halves of a word, whole rows on one side of every boundary the kernels
have (a wavefront's 16 rows, a 64-word group, the 1024 rows of one load of the byte prefix), and single bits at the ends.
"""
import numpy as np

SENTINEL = 0xDEADBEEF
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def n_words(n):
    return (int(n) + 63) // 64


def _bits(words, n):
    w = np.ascontiguousarray(words, dtype="<u8")
    assert w.ndim == 1 and w.size * 64 >= n, "the mask is shorter than n bits"
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n]


def expand(words, n, index_base=0):
    """uint32 ids index_base + i of every set bit i < n of the uint64 mask `words`, ascending.  Bits at or past n are
    padding and are ignored; the base is added in uint64 and every id must be below 2^32."""
    ids = np.flatnonzero(_bits(words, int(n))).astype(np.uint64) + np.uint64(index_base)
    assert ids.size == 0 or int(ids[-1]) < (1 << 32), "an id does not fit 32 bits"
    return ids.astype(np.uint32)


def expand_ranges(gathered, cap_pad, base, n_pad):
    """expand() per segment of a gathered mask: rank r owns words [r * cap_pad / 64, r * cap_pad / 64 + n_pad[r] / 64),
    its bit i has id base[r] + i; the words of a segment past n_pad[r] are ignored, whatever they hold."""
    assert cap_pad % 64 == 0
    cw = cap_pad // 64
    g = np.ascontiguousarray(gathered, dtype="<u8")
    out = []
    for r in range(len(base)):
        npad = int(n_pad[r])
        assert npad % 64 == 0 and npad <= cap_pad
        out.append(expand(g[r * cw:r * cw + npad // 64], npad, int(base[r])))
    return np.concatenate(out) if out else np.zeros(0, np.uint32)


def mask_padding(words, n):
    """A copy of `words` cut to ceil(n / 64) words with every bit at or past n cleared."""
    w = np.array(words[:n_words(n)], dtype=np.uint64)
    if n % 64:
        w[-1] &= np.uint64((1 << (n % 64)) - 1)
    return w


def set_padding(words, n):
    """A copy of `words` cut to ceil(n / 64) words with every bit at or past n SET."""
    w = np.array(words[:n_words(n)], dtype=np.uint64)
    if n % 64:
        w[-1] |= ~np.uint64((1 << (n % 64)) - 1)
    return w


def row_pop(words, n):
    """Popcount of each mask word after masking the padding, as uint8: what the update / cull kernels leave in
    vis_row_pop for the single-launch compaction."""
    w = mask_padding(words, n)
    return np.unpackbits(w.astype("<u8").view(np.uint8)).reshape(-1, 64).sum(axis=1).astype(np.uint8) if w.size else np.zeros(0, np.uint8)


def _random_bits(rng, nw, density):
    bits = rng.random(nw * 64) < density
    return np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)


def patterns(nw, rng, n=None, only=None):
    """{name: uint64[nw]} -- the masks of the module docstring for a mask of nw words holding n bits (default: all of
    them); `only`: the names wanted.  Bits at or past n are whatever the pattern gives there: padding is the caller's to
    mask or to set."""
    if only is not None:
        return {k: v for k, v in _patterns(nw, rng, n, only).items() if k in only}
    return _patterns(nw, rng, n, None)


def _patterns(nw, rng, n, only):
    n = nw * 64 if n is None else int(n)
    assert 0 < n <= nw * 64 and nw == n_words(n)
    u = np.uint64
    p = {"zeros": np.zeros(nw, u), "ones": np.full(nw, ONES, u)}
    for b in (0, 31, 32, 63):
        p[f"bit{b}"] = np.full(nw, u(1) << u(b), u)
    p["bits31_63"] = np.full(nw, (u(1) << u(31)) | (u(1) << u(63)), u)
    p["x5555"] = np.full(nw, u(0x5555555555555555), u)
    p["xAAAA"] = np.full(nw, u(0xAAAAAAAAAAAAAAAA), u)
    r = np.arange(nw)
    for m in (16, 64, 1024):
        p[f"rows_last_of_{m}"] = np.where(r % m == m - 1, ONES, u(0)).astype(u)
        p[f"rows_first_of_{m}"] = np.where(r % m == 0, ONES, u(0)).astype(u)
    for name, dens in (("density_1_64", 1.0 / 64), ("density_1_2", 0.5), ("density_63_64", 63.0 / 64)):
        if only is None or name in only:                            # (the only patterns that cost time at 4 M bits)
            p[name] = _random_bits(rng, nw, dens)
    first = np.zeros(nw, u)
    first[0] = u(1)
    p["single_first"] = first
    last = np.zeros(nw, u)
    last[(n - 1) // 64] = u(1) << u((n - 1) % 64)
    p["single_last"] = last
    return p


# the subset for masks of 2^19 bits and more (download volume): every boundary pattern whose prefix sits on the far side
LARGE_SUBSET = ("zeros", "ones", "bits31_63", "rows_last_of_16", "rows_last_of_64", "rows_last_of_1024", "density_1_2",
                "single_last")
LARGE_FROM = 1 << 19


def pattern_names(n):
    """Names of the patterns a mask of n bits is run with."""
    return LARGE_SUBSET if n >= LARGE_FROM else tuple(patterns(1, np.random.default_rng(0)).keys())


# ---- the gathered masks of clapgpu_visible_compact_ranges / clapgpu_visible_expand_ranges_host -----------------------------
RANGE_PATTERNS = ("ones", "bits31_63", "density_1_2", "zeros")


def _bases(n_pad, gaps, end=None):
    """Ascending disjoint bases for segments of n_pad[r] slots, gaps[r] (multiples of 64) before segment r; with `end` the
    last range is moved up so that it ends exactly there."""
    base, at = [], 0
    for npad, gap in zip(n_pad, gaps):
        at += gap
        base.append(at)
        at += npad
    if end is not None:
        base[-1] = end - n_pad[-1]
        assert len(base) == 1 or base[-1] >= base[-2] + n_pad[-2]
    return base


def range_descriptors():
    """[(name, cap_pad, base[], n_pad[])]: the segment layouts of the issue -- one segment, MAX_SEGMENTS (64) segments,
    segments that end inside a 64-word group, an empty shard in the middle, uneven sizes over more than one group, gaps
    between the ranges, and a last range that ends at exactly 2^32 (its last id is 0xFFFFFFFF)."""
    d = []
    d.append(("cap64_one", 64, [0], [64]))
    d.append(("cap64_x64", 64, _bases([64] * 64, [0] * 64), [64] * 64))
    d.append(("cap192_x5_mid_group", 192, _bases([192, 128, 192, 64, 192], [0] * 5), [192, 128, 192, 64, 192]))
    d.append(("cap4096_empty_middle", 4096, _bases([4096, 0, 64], [0, 0, 0]), [4096, 0, 64]))
    uneven = [64 * 65, 64 * 3, 64 * 64, 64 * 17]
    d.append(("cap4160_x4_uneven", 64 * 65, _bases(uneven, [0] * 4), uneven))
    d.append(("cap192_x5_gaps", 192, _bases([192, 128, 192, 64, 192], [64, 640, 0, 64 * 1000, 128]), [192, 128, 192, 64, 192]))
    d.append(("cap4160_x4_ends_at_2_32", 64 * 65, _bases(uneven, [0, 64, 0, 0], end=1 << 32), uneven))
    return [(name, cap, np.asarray(b, np.uint32), np.asarray(npad, np.uint32)) for name, cap, b, npad in d]


def gathered_mask(cap_pad, n_pad, pattern, rng):
    """The gathered mask of one descriptor: every segment's own words from `pattern`, the words past its n_pad[r] all
    ones (they must not appear in any list)."""
    cw = cap_pad // 64
    g = np.full(cw * len(n_pad), ONES, np.uint64)
    for r, npad in enumerate(n_pad):
        nw = int(npad) // 64
        if nw:
            g[r * cw:r * cw + nw] = patterns(nw, rng)[pattern]
    return g


def refused_descriptors():
    """[(name, n_ranges, cap_pad, base[], n_pad[], code)]: descriptors both entry points refuse; code is "invalid" or
    "too_large" (the host twin returns 0 for either).  Arrays hold at least n_ranges entries, so a check that came too
    late would still read memory the caller owns."""
    u = lambda a: np.asarray(a, np.uint32)
    many = u(np.arange(65) * 64)
    return [
        ("base_descending", 3, 64, u([128, 64, 0]), u([64, 64, 64]), "invalid"),
        ("ranges_overlap", 3, 128, u([0, 64, 256]), u([128, 128, 128]), "invalid"),
        ("n_pad_above_cap", 2, 64, u([0, 256]), u([128, 64]), "invalid"),
        ("cap_pad_not_64", 1, 96, u([0]), u([64]), "invalid"),
        ("cap_pad_zero", 1, 0, u([0]), u([0]), "invalid"),
        ("base_not_64", 2, 64, u([0, 96]), u([64, 64]), "invalid"),
        ("n_pad_not_64", 2, 64, u([0, 64]), u([32, 64]), "invalid"),
        ("no_ranges", 0, 64, u([0]), u([64]), "invalid"),
        ("65_ranges", 65, 64, many, u([64] * 65), "invalid"),
        ("ends_past_2_32", 2, 128, u([0, (1 << 32) - 64]), u([64, 128]), "too_large"),
    ]
