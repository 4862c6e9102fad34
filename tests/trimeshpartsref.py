"""numpy reference of the mesh set in parts (clapgpu_trimesh_create_parts): the balanced split rule of the top tree and
its height, the height bound, and a checker of a read-back image (clapgpu_trimesh_read).  make_image builds a valid
image by hand for the checker's own tests; it shares nothing with the device build but the layout rules."""
import numpy as np

LEAF = 0x80000000
NONE = 0xFFFFFFFF
HEIGHT_MAX = 62                                             # the walk's stack: trimesh_dev.h TM_STACK = 64
NODE = np.dtype([("box", np.float32, (2, 6)), ("child", np.uint32, 2), ("pad", np.uint32, 2)])


class Broken(AssertionError):
    pass


def need(ok, *what):
    if not ok:
        raise Broken(" ".join(str(w) for w in what))


# ------------------------------------------------------------------------------------------------- the top tree
def split(lo, hi):
    """a top node covering sorted parts [lo, hi), hi - lo >= 2, splits here: the left half gets the odd one"""
    return lo + (hi - lo + 1) // 2


def top_height(P):
    """ceil(log2 P): the height of the balanced tree over P parts (0 for P <= 1), whatever the poses are"""
    return 0 if P <= 1 else int(P - 1).bit_length()


def top_height_by_rule(P):
    """the same by applying the split rule"""
    def h(lo, hi):
        if hi - lo <= 1:
            return 0
        s = split(lo, hi)
        return 1 + max(h(lo, s), h(s, hi))
    return h(0, P)


def top_shape(P):
    """the P - 1 top nodes in preorder: [(lo, hi, child0, child1)], a child ("node", j) or ("part", sorted position)"""
    out = [None] * max(P - 1, 0)

    def go(j, lo, hi):
        s = split(lo, hi)
        c0 = ("part", lo) if s - lo == 1 else ("node", j + 1)
        c1 = ("part", s) if hi - s == 1 else ("node", j + (s - lo))
        out[j] = (lo, hi, c0, c1)
        if c0[0] == "node":
            go(c0[1], lo, s)
        if c1[0] == "node":
            go(c1[1], s, hi)
    if P >= 2:
        go(0, 0, P)
    return out


def height_allowed(P, deepest_part):
    """clapgpu_trimesh_create_parts refuses (CLAPGPU_ERR_TOO_LARGE) a tree whose top plus deepest part exceeds 62"""
    return top_height(P) + deepest_part <= HEIGHT_MAX


def part_roots(tri_first):
    """part_root[m] of the layout: top nodes [0, P - 1), then each part's k - 1 nodes in mesh order"""
    tf = np.asarray(tri_first, np.int64)
    k = np.diff(tf)
    P = int((k > 0).sum())
    before = np.cumsum(k > 0) - (k > 0)                     # parts before m
    root = np.where(k == 0, NONE, np.where(k == 1, LEAF | tf[:-1], (P - 1) + tf[:-1] - before))
    return root.astype(np.uint32), P


# ------------------------------------------------------------------------------------------------- boxes
def leaf_boxes(tri):
    """[T, 6] float32 (min xyz, max xyz) of fp64 triangles [T, 9], rounded outward"""
    v = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    lo, hi = np.fmin(np.fmin(v[:, 0], v[:, 1]), v[:, 2]), np.fmax(np.fmax(v[:, 0], v[:, 1]), v[:, 2])
    with np.errstate(invalid="ignore", over="ignore"):
        fl, fh = lo.astype(np.float32), hi.astype(np.float32)
        fl = np.where(fl.astype(np.float64) > lo, np.nextafter(fl, np.float32(-np.inf)), fl)
        fh = np.where(fh.astype(np.float64) < hi, np.nextafter(fh, np.float32(np.inf)), fh)
    return np.concatenate([fl, fh], 1).astype(np.float32)


def union(a, b):
    return np.concatenate([np.fmin(a[:3], b[:3]), np.fmax(a[3:], b[3:])])


def same_box(a, b):
    """by value: -0 == +0, NaN == NaN"""
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------------------------------------- the checker
def check_image(nodes, key, tri, part_root, tri_first, static_index):
    """Verifies a read-back image of a set in parts and returns (top height, deepest part's height, the whole tree's):
      * every leaf slot is reachable from node 0 exactly once, every node at most once, T - 1 nodes in all;
      * each part's slots are exactly [tri_first[m], tri_first[m + 1]) and hang below part_root[m]; above the part roots
        there are only top nodes (indices below P - 1), below them none;
      * every child box equals the union of the outward-rounded leaf boxes below it, recomputed from tri;
      * the top's measured height is ceil(log2 P), and the whole tree's is top plus deepest part, or one less where the
        deepest part hangs from one of the balanced top's shorter branches (its leaves are on two levels);
      * key is (static, triangle of its mesh) of the slot: the part's static, the triangles a permutation of 0 .. k - 1.
    Raises Broken (an AssertionError) naming what is wrong."""
    tf = np.asarray(tri_first, np.int64)
    T, M = int(tf[-1]), len(tf) - 1
    key, tri = np.asarray(key).reshape(-1, 2), np.asarray(tri, np.float64).reshape(-1, 9)
    need(len(key) == T and len(tri) == T, "key / tri rows", len(key), len(tri), T)
    want_root, P = part_roots(tf)
    need(len(part_root) == M and np.array_equal(np.asarray(part_root, np.uint32), want_root), "part_root", list(part_root[:8]),
         list(want_root[:8]))
    for m in range(M):
        k = key[tf[m]:tf[m + 1]]
        need((k[:, 0] == static_index[m]).all(), "key: static of mesh", m)
        need(np.array_equal(np.sort(k[:, 1]), np.arange(len(k))), "key: triangles of mesh", m)
    if T == 0:
        return 0, 0, 0
    need(len(nodes) == max(T - 1, 1), "node rows", len(nodes))
    lb = leaf_boxes(tri)
    if T == 1:                                              # the root that holds the one leaf twice
        n = nodes[0]
        need(n["child"][0] == LEAF and n["child"][1] == LEAF, "one leaf: links", n["child"])
        need(same_box(n["box"][0], lb[0]) and same_box(n["box"][1], lb[0]), "one leaf: boxes")
        return 0, 1, 1
    root_mesh = {int(r): m for m, r in enumerate(want_root) if r != NONE}
    seen_node, seen_leaf = np.zeros(T - 1, bool), np.zeros(T, bool)
    parts_seen = []

    def subtree(link, part, depth):
        """(box, height, deepest leaf depth) of what hangs from link; part: the mesh whose part we are in, or None (top)"""
        if part is None and link in root_mesh:
            part = root_mesh[link]
            parts_seen.append((part, depth))
        if link & LEAF:
            s = link & ~LEAF
            need(part is not None, "a leaf", s, "hangs from a top node without being a part's root")
            need(s < T and not seen_leaf[s], "leaf slot", s, "out of range or reached twice")
            need(tf[part] <= s < tf[part + 1], "leaf slot", s, "below the root of mesh", part)
            seen_leaf[s] = True
            return lb[s], 0, depth
        need(link < T - 1 and not seen_node[link], "node", link, "out of range or reached twice")
        seen_node[link] = True
        need((link < P - 1) == (part is None), "node", link, "on the wrong side of the part roots (P =", P, ")")
        n = nodes[link]
        b0, h0, d0 = subtree(int(n["child"][0]), part, depth + 1)
        b1, h1, d1 = subtree(int(n["child"][1]), part, depth + 1)
        need(same_box(n["box"][0], b0), "node", link, "child 0 box", n["box"][0], b0)
        need(same_box(n["box"][1], b1), "node", link, "child 1 box", n["box"][1], b1)
        return union(b0, b1), 1 + max(h0, h1), max(d0, d1)

    import sys
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4 * HEIGHT_MAX + 1000))
    try:
        _box, _h, total = subtree(0, None, 0)
    finally:
        sys.setrecursionlimit(old)
    need(seen_leaf.all(), "unreached leaf slots", np.nonzero(~seen_leaf)[0][:8])
    need(seen_node.all(), "unreached nodes", np.nonzero(~seen_node)[0][:8])
    need(sorted(p for p, _d in parts_seen) == sorted(root_mesh.values()), "parts reached", len(parts_seen), "of", P)
    top = max(d for _p, d in parts_seen)
    need(top == top_height(P), "top height", top, "for", P, "parts")
    # a part's height: from its root link to its deepest leaf
    deepest = 0
    for m, _d in parts_seen:
        deepest = max(deepest, _height(nodes, int(want_root[m])))
    need(top + deepest - 1 <= total <= top + deepest, "height", total, "top", top, "deepest part", deepest)
    return top, deepest, total


def _height(nodes, link):
    h, level = 0, [link]
    while True:
        level = [int(c) for l in level if not l & LEAF for c in nodes[l]["child"]]
        if not level:
            return h
        h += 1


# ------------------------------------------------------------------------------------------------- an image by hand
def make_image(mesh_tris, static_index, order=None):
    """A valid image of meshes [fp64 [k, 9]] with the parts hung in `order` (a permutation of the parts' mesh indices;
    default ascending): balanced part subtrees in preorder (the checker asks no particular shape of a part)."""
    tf = np.concatenate([[0], np.cumsum([len(t) for t in mesh_tris])]).astype(np.int64)
    T = int(tf[-1])
    tri = np.concatenate([np.asarray(t, np.float64).reshape(-1, 9) for t in mesh_tris] + [np.zeros((0, 9))])
    key = np.zeros((T, 2), np.uint32)
    for m in range(len(mesh_tris)):
        key[tf[m]:tf[m + 1], 0] = static_index[m]
        key[tf[m]:tf[m + 1], 1] = np.arange(tf[m + 1] - tf[m])
    root, P = part_roots(tf)
    nodes = np.zeros(max(T - 1, 1), NODE)
    lb = leaf_boxes(tri)
    if T == 1:
        nodes[0]["child"][:] = LEAF
        nodes[0]["box"][:] = lb[0]
    box_of = {}

    def part(j, lo, hi):                                    # node j covers slots [lo, hi), hi - lo >= 2; returns its box
        s = split(lo, hi)
        kids = [(LEAF | lo, lb[lo]) if s - lo == 1 else (j + 1, None), (LEAF | s, lb[s]) if hi - s == 1 else (j + (s - lo), None)]
        for side, (link, b) in enumerate(kids):
            if b is None:
                b = part(link, lo, s) if side == 0 else part(link, s, hi)
            nodes[j]["child"][side], nodes[j]["box"][side] = link, b
        return union(nodes[j]["box"][0], nodes[j]["box"][1])

    for m in range(len(mesh_tris)):
        k = tf[m + 1] - tf[m]
        if k == 1:
            box_of[m] = lb[tf[m]]
        elif k >= 2 and T > 1:
            box_of[m] = part(int(root[m]), int(tf[m]), int(tf[m + 1]))
    order = [m for m in range(len(mesh_tris)) if tf[m + 1] > tf[m]] if order is None else list(order)
    shape = top_shape(P)

    def top(j):
        _lo, _hi, c0, c1 = shape[j]
        for side, c in enumerate((c0, c1)):
            if c[0] == "part":
                link, b = root[order[c[1]]], box_of[order[c[1]]]
            else:
                link, b = c[1], top(c[1])
            nodes[j]["child"][side], nodes[j]["box"][side] = link, b
        return union(nodes[j]["box"][0], nodes[j]["box"][1])
    if P >= 2:
        top(0)
    return dict(nodes=nodes, key=key, tri=tri, part_root=root, tri_first=tf.astype(np.uint32))
