"""numpy restatement of clapgpu_skin_drawn's rule and of clapgpu_skin_lod_lists, from the text of include/clapgpu.h and
include/clapgpu_scene.h alone (no code of the library is read): what tests/test_skin_drawn*.py hold the library to."""
import numpy as np

SKIN_LODS = 4
LOD_ALL = 0xFFFFFFFF
NOT_DRAWN = 0xFF
ENTITY_RANGE, LOD_RANGE, LIST_RANGE = 1, 2, 4
OK, ERR_INVALID_ARGUMENTS, ERR_TOO_LARGE, ERR_OUT_OF_BOUNDS = 0, -2, -11, -26


def pack_plane(bits):
    """bool [n_entities] -> the uint64 words of a mask plane (bit i of word i / 64 = entity i)"""
    bits = np.asarray(bits, bool)
    words = np.zeros((bits.size + 63) // 64, np.uint64)
    for i in np.flatnonzero(bits):
        words[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    return words


def select(n_chars, vert_count, planes, n_entities, entity=None, cur_lod=None, n_lods=0, row=None, lod_first=None,
           lod_count=None, lst=None):
    """-> dict(skinned u8 [n], chars u32 [count], count, status, verts: per character the ascending local vertices that
    are written (an empty array for a character that is not drawn))."""
    n_rows = 0 if lod_first is None else np.asarray(lod_first).reshape(-1, max(n_lods, 1)).shape[0]
    if n_rows == 0 and n_lods == 0:
        n_lods = SKIN_LODS
    lod_first = None if n_rows == 0 else np.asarray(lod_first, np.uint32).reshape(n_rows, n_lods)
    lod_count = None if n_rows == 0 else np.asarray(lod_count, np.uint32).reshape(n_rows, n_lods)
    lst = np.zeros(0, np.uint32) if lst is None else np.asarray(lst, np.uint32)
    skinned = np.full(n_chars, NOT_DRAWN, np.uint8)
    status, chars, verts = 0, [], []
    for c in range(n_chars):
        s = c if entity is None else int(entity[c])
        verts.append(np.zeros(0, np.int64))
        if s >= n_entities:
            status |= ENTITY_RANGE
            continue
        if not any((int(p[s >> 6]) >> (s & 63)) & 1 for p in planes):
            continue
        lod = 0
        if cur_lod is not None:
            lod = int(cur_lod[s])
            if lod < 0 or lod >= n_lods:
                lod, status = 0, status | LOD_RANGE
        skinned[c] = lod
        chars.append(c)
        vc = int(vert_count[c])
        named = np.arange(vc, dtype=np.int64)
        if n_rows:
            r = 0 if row is None else int(row[c])
            if r >= n_rows:
                status |= LIST_RANGE                         # no such row: skinned whole
            elif int(lod_first[r, lod]) != LOD_ALL:
                first, cnt = int(lod_first[r, lod]), int(lod_count[r, lod])
                if first > lst.size:
                    first, cnt, status = lst.size, 0, status | LIST_RANGE
                elif cnt > lst.size - first:
                    cnt, status = lst.size - first, status | LIST_RANGE
                named = lst[first:first + cnt].astype(np.int64)
                if (named >= vc).any():
                    status |= LIST_RANGE
                    named = named[named < vc]
        verts[-1] = named
    return dict(skinned=skinned, chars=np.asarray(chars, np.uint32), count=len(chars), status=status, verts=verts)


def written_mask(sel, out_first, n_out):
    """bool [n_out]: the output vertices select() says are written"""
    m = np.zeros(n_out, bool)
    for c, v in enumerate(sel["verts"]):
        m[int(out_first[c]) + v] = True
    return m


def lod_lists(index, n_verts, capacity, total=0):
    """clapgpu_skin_lod_lists: index = the LODs' index buffers (uint16 arrays).  -> (rc, lod_first, lod_count, appended
    entries that fit, total)."""
    first, count, out = [], [], []
    rc = OK
    for idx in index:
        idx = np.asarray(idx, np.uint16)
        if (idx >= n_verts).any():
            return ERR_OUT_OF_BOUNDS, None, None, None, total
        u = np.unique(idx).astype(np.uint32)                  # ascending, distinct
        if u.size == n_verts and n_verts:
            first.append(LOD_ALL)
            count.append(n_verts)
            continue
        first.append(total)
        count.append(u.size)
        for v in u:
            if total < capacity:
                out.append(v)
            else:
                rc = ERR_TOO_LARGE
            total += 1
    return rc, np.asarray(first, np.uint32), np.asarray(count, np.uint32), np.asarray(out, np.uint32), total
