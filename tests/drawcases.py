"""The cases the draw-record tests share (tests/test_draw_records.py: twin == drawref; tests/test_draw_records_gpu.py:
kernel == twin): seeded populations, render orders, planes and group cuts at every edge of the fill kernel's geometry
(64 positions a word, 1 024 positions: the issue's sixteen words a wavefront).  A case is built once and cached, and so are the two references of a
case: ref() is tests/drawref.py over it, twin() is clapgpu_draw_records_host over it."""
import functools

import numpy as np

E_VISIBLE, E_SKIP_CULLING, E_ALIVE = 1 << 0, 1 << 14, 1 << 31
IS_CHARACTER, OUTLINE_EXCLUDE = 1, 2                       # clapgpu_draw_inputs.draw_flags

F1 = np.float32(1e-3)                                      # above the double 1e-3: passes model.c:1000
BLOOMS = np.array([F1, np.nextafter(F1, np.float32(0)), np.nextafter(F1, np.float32(1)), -F1, -np.nextafter(F1, np.float32(0)),
                   -np.nextafter(F1, np.float32(1)), 0.0, -0.0, np.inf, -np.inf, np.nan, 0.75], np.float32)
ODD_WORDS = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x00000001, 0x80000001, 0x007fffff, 0x7f800000, 0xff800000], np.uint32)


class Case:
    """n entities; groups: per txmodel its entity list in list order; skip: model3d.skip_shadow per txmodel; in_frustum:
    None (the pass without a view) or a bool per entity; the per-entity arrays; the pass."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_order(self):
        return sum(len(g) for g in self.groups)

    def txmodels(self):
        return [dict(skip_shadow=bool(s), entities=[int(i) for i in g]) for g, s in zip(self.groups, self.skip)]

    def ents(self):
        """drawref's view of the entities"""
        z = np.zeros(self.n, np.float32)
        return dict(flags=self.flags, mx=self.mx, inv_mx=self.inv_mx,
                    color=self.color if self.inputs else np.zeros((self.n, 4), np.float32),
                    color_pt=self.color_pt if self.inputs else np.zeros(self.n, np.int32),
                    bloom_intensity=self.bloom_intensity if self.inputs else z,
                    bloom_threshold=self.bloom_threshold if self.inputs else z,
                    is_character=(self.draw_flags & IS_CHARACTER) != 0 if self.inputs else np.zeros(self.n, bool),
                    outline_exclude=(self.draw_flags & OUTLINE_EXCLUDE) != 0 if self.inputs else np.zeros(self.n, bool),
                    cur_lod=self.lod if self.lod is not None else np.zeros(self.n, np.int32),
                    character=self.character if self.inputs else np.full(self.n, -1, np.int32))

    def input_arrays(self):
        """clapgpu_draw_inputs' arrays, or None: every pointer NULL"""
        if not self.inputs:
            return None
        return dict(color=self.color, color_pt=self.color_pt, bloom_intensity=self.bloom_intensity,
                    bloom_threshold=self.bloom_threshold, draw_flags=self.draw_flags, character=self.character)


def _cut(order, bounds):
    """order cut into groups at the render positions `bounds` (repeats and 0 / n_order give empty groups)"""
    at = [0] + sorted(int(b) for b in bounds) + [len(order)]
    return [order[a:b] for a, b in zip(at[:-1], at[1:])]


@functools.lru_cache(maxsize=None)
def case(n_order, n=None, order="perm", plane="mixed", bounds=(), skip=(), shadow=False, ropts=True, mq=3, inputs=True,
         lod=True, index_base=0, seed=0, cull_groups=()):
    rng = np.random.default_rng(1000 + seed + n_order)
    if n is None:
        n = (n_order + 63) // 64 * 64 + 64                  # one padding row: entities no txmodel owns
        ids = np.arange(n_order, dtype=np.uint32)
    else:                                                   # the drawn population is a subset of the entities
        ids = np.sort(rng.choice(n, n_order, replace=False)).astype(np.uint32)
    ordr = {"identity": ids, "reversed": ids[::-1].copy(), "perm": rng.permutation(ids)}[order]
    groups = _cut(ordr, bounds)
    flags = np.full(n, E_ALIVE | E_VISIBLE, np.uint32)
    in_frustum = None
    if plane == "empty":
        in_frustum = np.zeros(n, bool)
    elif plane == "full":
        in_frustum = np.ones(n, bool)
    else:                                                   # mixed, and the pass without a view: every flag combination
        dead, hidden, skipc = rng.random(n) < 0.1, rng.random(n) < 0.1, rng.random(n) < 0.15
        flags = np.where(dead, flags & ~np.uint32(E_ALIVE), flags)
        flags = np.where(hidden, flags & ~np.uint32(E_VISIBLE), flags)
        flags = np.where(skipc, flags | np.uint32(E_SKIP_CULLING), flags).astype(np.uint32)
        flags |= (rng.integers(0, 1 << 8, n).astype(np.uint32) << 16) & ~np.uint32(E_ALIVE)      # bits the rule does not read
        in_frustum = None if plane == "null" else rng.random(n) < 0.6
    for g in cull_groups:                                   # a txmodel with nothing drawn
        flags[groups[g]] &= ~np.uint32(E_SKIP_CULLING)
        if in_frustum is not None:
            in_frustum[groups[g]] = False
        else:
            flags[groups[g]] &= ~np.uint32(E_VISIBLE)
    words = lambda shape: rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)      # every bit pattern
    mx, inv_mx, color = words((n, 16)), words((n, 16)), words((n, 4))
    mx[:, 0].flat[:ODD_WORDS.size] = ODD_WORDS[:n]
    color[:, 3].flat[:ODD_WORDS.size] = ODD_WORDS[:n]
    c = Case(n=n, groups=groups, skip=tuple(skip) + (False,) * (len(groups) - len(skip)), flags=flags, in_frustum=in_frustum,
             mx=mx.view(np.float32), inv_mx=inv_mx.view(np.float32), color=color.view(np.float32),
             color_pt=rng.integers(-2, 3, n).astype(np.int32),
             bloom_intensity=BLOOMS[rng.integers(0, BLOOMS.size, n)], bloom_threshold=BLOOMS[rng.integers(0, BLOOMS.size, n)],
             draw_flags=(np.where(rng.random(n) < 0.6, IS_CHARACTER, 0) | np.where(rng.random(n) < 0.3, OUTLINE_EXCLUDE, 0)).astype(np.uint32),
             character=np.where(rng.random(n) < 0.6, rng.integers(0, 1000, n), -1).astype(np.int32),
             lod=rng.integers(0, 4, n).astype(np.int32) if lod else None, shadow=shadow,
             ropts=(np.float32(0.5), np.float32(0.0009765625)) if ropts else None, mq=mq, inputs=inputs, index_base=index_base)
    return c


@functools.lru_cache(maxsize=None)
def ordinals_case(mq=3):
    """Groups with exactly 0, 1, 15, 16, 17 and 40 DRAWN characters, a culled character and a drawn non-character between
    every two of them; the ordinal restarts at every group (model.c:956)."""
    counts = (0, 1, 15, 16, 17, 40)
    groups, chars, culled = [], [], []
    at = 0
    for cnt in counts:
        g = []
        for _k in range(max(cnt, 2)):
            g += [at, at + 1, at + 2]                       # a character (drawn iff _k < cnt), a culled character, a non-character
            chars += [at, at + 1]
            culled += [at + 1] + ([at] if _k >= cnt else [])
            at += 3
        groups.append(np.array(g, np.uint32))
    n = (at + 63) // 64 * 64 + 64
    base = case(at, n=n, order="identity", plane="full", seed=77)
    draw_flags = np.zeros(n, np.uint32)
    draw_flags[chars] = IS_CHARACTER
    draw_flags[::5] |= OUTLINE_EXCLUDE
    in_frustum = np.ones(n, bool)
    in_frustum[culled] = False
    c = Case(**{**base.__dict__, "groups": groups, "skip": (False,) * len(groups), "draw_flags": draw_flags, "in_frustum": in_frustum,
                "mq": mq})
    c.counts = counts
    return c


# (id, keyword arguments of case()): every edge the issue names
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2113)
CASES = {}
for _n in SIZES:
    for _o in ("identity", "reversed", "perm"):
        CASES[f"n{_n}-{_o}"] = dict(n_order=_n, order=_o, bounds=tuple(b for b in (_n // 3, 2 * _n // 3) if 0 < b < _n))
CASES["n300-of-1024"] = dict(n_order=300, n=1024, bounds=(100, 200))
for _p in ("empty", "full", "mixed", "null"):
    CASES[f"plane-{_p}"] = dict(n_order=1025, plane=_p, bounds=(400,))
    CASES[f"plane-{_p}-one-word"] = dict(n_order=65, plane=_p)
CASES["one-group"] = dict(n_order=2113)
CASES["bounds-1-63-64-65-1024"] = dict(n_order=2113, bounds=(1, 63, 64, 65, 1024))
CASES["empty-groups"] = dict(n_order=1025, bounds=(0, 0, 300, 300, 300, 1024, 1025, 1025))
CASES["group-with-nothing-drawn"] = dict(n_order=300, bounds=(100, 200), cull_groups=(1,))
CASES["group-with-nothing-drawn-null-plane"] = dict(n_order=300, plane="null", bounds=(100, 200), cull_groups=(0,))
CASES["skip-shadow-in-shadow-pass"] = dict(n_order=1025, bounds=(10, 700, 1000), skip=(True, False, True, False), shadow=True)
CASES["skip-shadow-in-model-pass"] = dict(n_order=1025, bounds=(10, 700, 1000), skip=(True, False, True, False), shadow=False)
CASES["word-straddled-by-three-groups"] = dict(n_order=1025, plane="full", bounds=(70, 90, 100, 1023, 1024))
CASES["mq-nr-characters-0"] = dict(n_order=300, mq=0, bounds=(64,))
CASES["no-ropts"] = dict(n_order=1025, ropts=False, bounds=(500,))
CASES["no-ropts-full"] = dict(n_order=300, ropts=False, plane="full")
CASES["inputs-null"] = dict(n_order=1025, inputs=False, bounds=(500,))
CASES["lod-null"] = dict(n_order=300, lod=False)
CASES["index-base"] = dict(n_order=300, index_base=0x7ffffff0)


def get(name):
    if name == "ordinals":
        return ordinals_case()
    if name == "ordinals-mq0":
        return ordinals_case(mq=0)
    return case(**CASES[name])


@functools.lru_cache(maxsize=None)
def ref(name, capacity=None):
    """tests/drawref.py over the case: (records as bytes, count, group_first, status)"""
    import drawref
    c = get(name)
    rec, count, first, status = drawref.models_render(c.txmodels(), c.ents(), c.shadow, c.ropts, c.mq, c.in_frustum, c.index_base,
                                                      capacity)
    return rec.tobytes(), count, first, status


def plane_of(c):
    import drawref
    return None if c.in_frustum is None else drawref.plane_of(c.flags, c.in_frustum)


def order_of(c, device=None):
    from clap_amd import draw
    return draw.DrawOrder.from_groups(c.groups, c.skip, device)


def pass_of(c):
    from clap_amd import draw
    return draw.draw_pass(c.shadow, c.ropts, c.mq, c.index_base)


@functools.lru_cache(maxsize=None)
def twin(name, capacity=None, fill=0):
    """clapgpu_draw_records_host over the case: (the WHOLE record buffer as RECORD[capacity], count, group_first, status);
    capacity None: n_order"""
    from clap_amd import draw
    c = get(name)
    cap = c.n_order if capacity is None else capacity
    return draw.records_host(c.mx, c.inv_mx, order_of(c), pass_of(c), cap, flags=c.flags, plane=plane_of(c), lod=c.lod,
                             inputs=c.input_arrays(), fill=fill)


NAMES = tuple(CASES) + ("ordinals", "ordinals-mq0")
