"""The tracked lights' rule (include/clapgpu.h, "Spotlights on the device"), restated once in numpy scalars: float32 where
core/light.c has floats, the one double-typed comparison in double, the carriers in list order, nothing shared with
csrc/lm_dev.h.

    is_spotlight  (light.c:516-522)
    direction     (light.c:398-400, 508-514; linmath.h:939-958)
    update        (light.c:462-471, 385-410) over a case of tests/spotscases.py
"""
import numpy as np

F = np.float32
QNAN = np.uint32(0x7fc00000)
STATUS_BEFORE = 0xdead                                       # what the tests put into the status word before a call


def one_nan(a):
    """every NaN as the one quiet NaN the library stores"""
    a = np.array(a, F)
    w = a.view(np.uint32)
    w[np.isnan(a)] = QNAN
    return a


def is_spotlight(is_dir, cutoff):
    return bool(is_dir != 0 and float(np.float64(F(cutoff))) > 0.0)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def direction(quat):
    """(0,0,0) - quat_mul_vec3(quat, (0,0,1)), every product kept"""
    q = [F(v) for v in quat]
    v = [F(0), F(0), F(1)]
    with np.errstate(all="ignore"):
        t = [c * F(2) for c in _cross(q[:3], v)]
        u = _cross(q[:3], t)
        t = [c * q[3] for c in t]
        r = [(v[i] + t[i]) + u[i] for i in range(3)]
        return one_nan([F(0) - c for c in r])


def update(case):
    """What clapgpu_lights_update leaves of a case: (pos [128, 3], dir [128, 3], status, source) -- copies."""
    ent, light, off, vslot = case["carriers"]
    L = case["lights"]
    n, nr = len(case["flags"]), int(L["nr_lights"])
    pos, dr = np.array(L["pos"], F).reshape(-1, 3).copy(), np.array(case["dir"], F).reshape(-1, 3).copy()
    src = None if case["source"] is None else case["source"].copy()
    if len(ent) == 0 or nr == 0:                             # nothing to do: nothing is launched, the status word keeps its value
        return pos, dr, STATUS_BEFORE, src
    for k in range(len(ent)):                                # what the host cannot see: any carrier, applying or not
        v = 0 if vslot is None else int(vslot[k])
        if v and (v >= len(src["slot"]) or not int(src["slot"][v]["flags"]) & 1):
            return np.array(L["pos"], F).reshape(-1, 3).copy(), np.array(case["dir"], F).reshape(-1, 3).copy(), 1, case["source"].copy()
    for k in range(len(ent)):
        l, e = int(light[k]), int(ent[k])
        if l < 0 or l >= nr or e >= n or not L["active"][l]:
            continue
        if not (case["mode"] & 1) and not (int(case["flags"][e]) & (1 << 16)):
            continue
        with np.errstate(all="ignore"):
            pos[l] = [F(case["pos_scale"][e][i]) + F(off[k][i]) for i in range(3)]
        if not is_spotlight(L["is_dir"][l], case["cutoff"][l]):
            continue
        dr[l] = direction(case["rot"][e])
        v = 0 if vslot is None else int(vslot[k])
        if v:
            src["slot"][v]["pos"].view(np.uint32)[:] = np.asarray(case["pos_scale"][e][:3], F).view(np.uint32)
            src["slot"][v]["quat"].view(np.uint32)[:] = np.asarray(case["rot"][e], F).view(np.uint32)
    return pos, dr, 0, src
