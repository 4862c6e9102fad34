"""_models_render's draw loop (core/model.c:784-1050 of the reference) restated in plain Python, for the draw records.

Independent of clap_amd/draw.py and of csrc/draw_dev.h: it loops over txmodels, then over a txmodel's entities, exactly as
the reference does, keeps the shader's uniforms as STICKY state (a uniform holds what the last shader_set_var_* left), and
derives a record's SET_* bits from whether the draw called shader_set_var_float, not from the kernel's rule.  The record
layout is the table of include/clapgpu.h, restated.
"""
import numpy as np

E_VISIBLE, E_SKIP_CULLING, E_ALIVE = 1 << 0, 1 << 14, 1 << 31        # ENTITY3D_VISIBLE / _SKIP_CULLING / _ALIVE
EDGE_EXCLUDE, EDGE_SOLID_MASK, EDGE_SOLID_OFFSET = 1 << 7, (1 << 4) - 1, 0       # shader_constants.h:57-62

REC = np.dtype({"names": ["mx", "inv_mx", "color", "bloom_intensity", "bloom_threshold", "edge_mode", "color_pt", "entity", "lod",
                          "group", "character", "flags", "zero"],
                "formats": [("<u4", 16), ("<u4", 16), ("<u4", 4), "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4",
                            ("<u4", 3)],
                "offsets": [0, 64, 128, 144, 148, 152, 156, 160, 164, 168, 172, 176, 180], "itemsize": 192})
SET_BLOOM_INTENSITY, SET_BLOOM_THRESHOLD = 1, 2
CAPPED, INVALID = 1, 2


def bits(a, dtype=np.float32):
    return np.ascontiguousarray(a, dtype).view(np.uint32)


class Shader:
    """The recording double of shader_set_var_*: sticky uniforms and a count of the calls."""

    def __init__(self):
        self.value, self.calls = {}, {}

    def set(self, name, v):
        self.value[name] = v
        self.calls[name] = self.calls.get(name, 0) + 1


def models_render(txmodels, ents, shader_override, ropts, mq_nr_characters, in_frustum=None, index_base=0, capacity=None):
    """txmodels: the list mq->txmodels, each a dict(skip_shadow=bool, entities=[entity index, ...] in list order).
    ents: per-entity arrays flags, mx, inv_mx, color, color_pt, bloom_intensity, bloom_threshold, is_character,
    outline_exclude, cur_lod, character.  ropts: None or (bloom_intensity, bloom_threshold).  in_frustum: None (no view:
    model.c:970 `view &&`) or a bool per entity (view_entity_in_frustum).  Returns (records REC[...], count, group_first,
    status) with at most `capacity` records."""
    prog = Shader()
    out, group_first = [], []
    nr_ents = 0
    for g, txm in enumerate(txmodels):                                   # model.c:784
        group_first.append(nr_ents)
        if txm["skip_shadow"] and shader_override:                       # model.c:786
            continue
        nr_characters = 0                                                # model.c:956
        for i in txm["entities"]:                                        # model.c:959
            fl = int(ents["flags"][i])
            if not fl & E_ALIVE:                                         # model.c:960
                continue
            if not fl & E_VISIBLE:                                       # model.c:966
                continue
            if not fl & E_SKIP_CULLING and in_frustum is not None and not in_frustum[i]:      # model.c:969-973
                continue
            before = dict(prog.calls)
            bi, bt = float(np.float32(ents["bloom_intensity"][i])), float(np.float32(ents["bloom_threshold"][i]))
            if abs(bi) > 1e-3:                                           # model.c:1000: a double comparison
                prog.set("bloom_intensity", ents["bloom_intensity"][i])
            elif ropts is not None:
                prog.set("bloom_intensity", ropts[0])
            if abs(bt) > 1e-3:                                           # model.c:1005
                prog.set("bloom_threshold", ents["bloom_threshold"][i])
            elif ropts is not None:
                prog.set("bloom_threshold", ropts[1])
            edge_mode = 0                                                # model.c:1010
            if ents["outline_exclude"][i]:
                edge_mode |= EDGE_EXCLUDE
            if ents["is_character"][i] and mq_nr_characters:             # model.c:1012
                nr_characters += 1
                edge_mode |= (nr_characters & EDGE_SOLID_MASK) << EDGE_SOLID_OFFSET
            rec = np.zeros((), REC)
            set_i = prog.calls.get("bloom_intensity", 0) != before.get("bloom_intensity", 0)
            set_t = prog.calls.get("bloom_threshold", 0) != before.get("bloom_threshold", 0)
            rec["bloom_intensity"] = bits(prog.value["bloom_intensity"])[0] if set_i else 0
            rec["bloom_threshold"] = bits(prog.value["bloom_threshold"])[0] if set_t else 0
            rec["flags"] = (SET_BLOOM_INTENSITY if set_i else 0) | (SET_BLOOM_THRESHOLD if set_t else 0)
            rec["edge_mode"] = edge_mode                                 # model.c:1016
            rec["color"] = bits(ents["color"][i])                        # model.c:1017
            rec["color_pt"] = bits(ents["color_pt"][i], np.int32)[0]    # model.c:1018
            rec["mx"] = bits(ents["mx"][i])                              # model.c:1027
            rec["inv_mx"] = bits(ents["inv_mx"][i])                      # model.c:1028
            rec["lod"] = bits(ents["cur_lod"][i], np.int32)[0]          # model.c:1042
            rec["entity"] = index_base + i
            rec["group"] = g
            rec["character"] = bits(ents["character"][i], np.int32)[0]
            if capacity is None or nr_ents < capacity:
                out.append(rec)
            nr_ents += 1                                                 # model.c:1049
    group_first.append(nr_ents)
    status = CAPPED if capacity is not None and nr_ents > capacity else 0
    recs = np.array(out, REC) if out else np.zeros(0, REC)
    return recs, nr_ents, np.array(group_first, np.uint32), status


def plane_of(flags, in_frustum):
    """A view's mask plane as the cull leaves it: bit i = ALIVE && VISIBLE && (SKIP_CULLING || in the frustum)."""
    fl = np.asarray(flags, np.uint32)
    bit = ((fl & E_ALIVE) != 0) & ((fl & E_VISIBLE) != 0) & (((fl & E_SKIP_CULLING) != 0) | np.asarray(in_frustum, bool))
    n = fl.size
    pad = np.zeros((n + 63) // 64 * 64, np.uint8)
    pad[:n] = bit
    return np.packbits(pad.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint64) if n else np.zeros(1, np.uint64)
