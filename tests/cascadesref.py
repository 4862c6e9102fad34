"""The shadow cascades' rule (include/clapgpu.h, "The shadow cascades on the device"), restated once in numpy scalars:
float32 and float64 where core/view.c, core/scene.c and linmath.h have them, their order of operations, nothing shared
with csrc/lm_dev.h.  Matrices are m[c][r] lists of np.float32, as tests/cameraref.py has them (its mat_mul, invert and
view_matrix are used here).

    corners       (view.c:248-289)         the eight corners of a frustum
    near_backup   (scene.c:1030-1037)      from the bounding volume's model box and scale
    fit           (view.c:195-228)         the light's view fitted to eight corners
    projection    (view.c:129-146)         a cascade's orthographic projection
    calc                                   the whole of clapgpu_cascades_calc on records
"""
import warnings

import numpy as np

import cameraref as cr

F = np.float32
D = np.float64
INF = F(np.inf)
Z_REVERSE, NDC_Z_ZERO_ONE, NEAR_BACKUP_FROM_BV = 1, 2, 4
INVALID = 1
NO_ENTITY = 0xFFFFFFFF


def _quiet(fn):
    def run(*a, **k):
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            return fn(*a, **k)
    return run


def mat(flat):
    a = np.asarray(flat, F).reshape(4, 4)
    return [[a[c][r] for r in range(4)] for c in range(4)]


def flat(m):
    return np.asarray([[m[c][r] for r in range(4)] for c in range(4)], F).reshape(16)


def mul_vec4_post(m, v):
    """linmath.h:297-305"""
    out = []
    for i in range(4):
        t = m[0][i] * v[0] + m[1][i] * v[1] + m[2][i] * v[2]
        t = t + m[3][i] * v[3]
        out.append(t)
    return out


def corners(view, proj, z01):
    """view.c:248-289: the corners alone"""
    inv = cr.invert(cr.mat_mul(proj, view))
    zn = F(0) if z01 else F(-1)
    ndc = [(-1, -1, zn), (1, -1, zn), (1, 1, zn), (-1, 1, zn), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)]
    out = []
    for x, y, z in ndc:
        q = mul_vec4_post(inv, [F(x), F(y), F(z), F(1)])
        s = F(1) / q[3]
        out.append([q[k] * s for k in range(4)])
    return out


def inner3(a, b):
    p = F(0)
    for i in range(3):
        p = p + b[i] * a[i]
    return p


def norm3(v):
    k = F(D(1.0) / D(np.sqrt(inner3(v, v))))
    return [v[i] * k for i in range(3)]


def norm3_safe(v):
    return norm3(v) if np.sqrt(inner3(v, v)) != 0 else list(v)


def cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def look_at(eye, center, up):
    """linmath.h:777-817"""
    f = norm3([center[i] - eye[i] for i in range(3)])
    s = norm3(cross3(f, up))
    t = cross3(s, f)
    z, one = F(0), F(1)
    m = [[s[0], t[0], -f[0], z], [s[1], t[1], -f[1], z], [s[2], t[2], -f[2], z], [z, z, z, one]]
    x, y, zz = -eye[0], -eye[1], -eye[2]
    for i in range(4):                               # mat4x4_translate_in_place, linmath.h:525-534
        p = F(0)
        p = p + x * m[0][i]
        p = p + y * m[1][i]
        p = p + zz * m[2][i]
        p = p + F(0) * m[3][i]
        m[3][i] = m[3][i] + p
    return m


def look_at_safe(eye, center):
    """linmath.h:819-833 with up = (0, 1, 0); returns (matrix, whether the up vector was swapped)"""
    up = [F(0), F(1), F(0)]
    fw = norm3([center[i] - eye[i] for i in range(3)])
    swap = bool(np.abs(inner3(fw, up)) > F(0.999))
    return look_at(eye, center, [F(0), F(0), F(-1)] if swap else up), swap


def ortho(l, r, b, t, n, f, z01):
    """linmath.h:692-707 / 736-751"""
    z, one, two = F(0), F(1), F(2)
    m = [[z] * 4 for _ in range(4)]
    m[0][0] = two / (r - l)
    m[1][1] = two / (t - b)
    m[2][2] = -one / (f - n) if z01 else -two / (f - n)
    m[3][0] = -(r + l) / (r - l)
    m[3][1] = -(t + b) / (t - b)
    m[3][2] = -(n) / (f - n) if z01 else -(f + n) / (f - n)
    m[3][3] = one
    return m


def corners_box(cs, xlate=None):
    """util.c:59-78 over eight vec4 corners: ([min], [max])"""
    lo, hi = [INF] * 3, [-INF] * 3
    for c in cs:
        v = [c[0], c[1], c[2], F(1)]
        if xlate is not None:
            q = mul_vec4_post(xlate, v)
            s = F(1) / q[3]
            v = [q[0] * s, q[1] * s, q[2] * s]
        for j in range(3):
            lo[j] = v[j] if v[j] < lo[j] else lo[j]
            hi[j] = v[j] if v[j] > hi[j] else hi[j]
    return lo, hi


@_quiet
def near_backup(light_dir, lo, hi, scale):
    """scene.c:1030-1037"""
    light_dir, lo, hi, scale = np.asarray(light_dir, F), np.asarray(lo, F), np.asarray(hi, F), F(scale)
    X, Y, Z = (np.abs(hi[k] - lo[k]) * scale for k in range(3))
    d = norm3_safe(list(light_dir))
    blend = np.abs(inner3(d, [F(1), F(0), F(0)]))
    xz_mix = F(D(Z) * (D(1.0) - D(blend)) + D(X * blend))          # interp.h:25-29: b * blend is a float product
    ycos = np.fmax(np.abs(inner3(d, [F(0), F(1), F(0)])), F(0.2))
    q, edge = xz_mix / ycos, cr.cbrtf(X * Y * Z)
    return q if q < edge else edge


@_quiet
def fit(cs, light_dir, nb):
    """view.c:195-228: (view, inverse, how many of the two look_at calls swapped the up vector)"""
    lo, hi = corners_box(cs)
    pos = [(hi[k] - lo[k]) * F(0.5) + lo[k] for k in range(3)]
    pos[1] = lo[1]
    d = norm3_safe([-F(light_dir[0]), -F(light_dir[1]), -F(light_dir[2])])
    nb = np.fmax(F(nb), F(1.0))
    d = [c * nb for c in d]
    m, swap0 = look_at_safe([d[k] + pos[k] for k in range(3)], pos)
    llo, lhi = corners_box(cs, m)
    length = np.abs(llo[2] - lhi[2])
    k = (nb + length) / nb
    d = [c * k for c in d]
    m, swap1 = look_at_safe([d[i] + pos[i] for i in range(3)], pos)
    return m, cr.invert(m), int(swap0) + int(swap1)


@_quiet
def projection(view, cs, flags):
    """view.c:129-146: (proj, inverse, mvp, far_plane)"""
    lo, hi = corners_box(cs, view)
    near, far = F(0.1), -lo[2]
    z01 = bool(flags & NDC_Z_ZERO_ONE)
    p = ortho(lo[0], hi[0], lo[1], hi[1], far, near, z01) if flags & Z_REVERSE else ortho(lo[0], hi[0], lo[1], hi[1], near, far, z01)
    return p, cr.invert(p), cr.mat_mul(p, view), far


def one_nan(a):
    a = np.array(a, F)
    b = a.view(np.uint32)
    b[np.isnan(a)] = 0x7fc00000
    return a


@_quiet
def calc(c, s, env=None):
    """clapgpu_cascades_calc on a CASCADES record and a VIEWS_SOURCE record (clap_amd.cascades); env None (the key 0)
    or (lo, hi, scale).  Returns (copies of the two records, the number of up-vector swaps over all fits)."""
    c, s = np.array(c).reshape(1).copy()[0], np.array(s).reshape(1).copy()[0]      # records that view their own arrays
    nr = int(c["nr_cascades"]) or 4
    slot = int(c["light_slot"])
    if nr > 4 or not 1 <= slot <= 4 or int(s["slot"][slot]["flags"]) & 1:
        c["status"] = INVALID
        return c, s, 0
    flags = int(c["flags"])
    nb, ent = c["near_backup"], NO_ENTITY
    if flags & NEAR_BACKUP_FROM_BV:
        nb = F(0)
        if env is not None:
            nb, ent = near_backup(c["light_dir"], *env), 0
    c["near_backup_used"], c["bv_entity"], c["status"] = one_nan(nb), ent, 0
    s0 = s["slot"][0]
    view = cr.view_matrix(s0["pos"], s0["quat"]) if int(s0["flags"]) & 1 else mat(s0["view_mx"])
    swaps = 0
    for lane in list(range(nr)) + [4]:
        cs = corners(view, mat(s0["proj_mx"] if lane == 4 else c["persp"][lane]), bool(flags & NDC_Z_ZERO_ONE))
        c["cam_corners"][lane] = one_nan(np.asarray(cs, F))
        v, iv, n = fit(cs, c["light_dir"], nb)
        swaps += n
        if lane == 4:
            c["view_mx"], c["inv_view_mx"] = one_nan(flat(v)), one_nan(flat(iv))
            s["slot"][slot]["view_mx"] = one_nan(flat(v))
            continue
        p, ip, mvp, far = projection(v, cs, flags)
        o = c["cascade"][lane]
        o["view_mx"], o["inv_view_mx"], o["proj_mx"], o["inv_proj_mx"] = (one_nan(flat(x)) for x in (v, iv, p, ip))
        o["mvp"], o["near_plane"], o["far_plane"] = one_nan(flat(mvp)), F(0.1), one_nan(far)
    return c, s, swaps
