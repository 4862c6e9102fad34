"""What tests/test_cascades.py and tests/test_cascades_gpu.py share: the trace's cameras and the named edge cases as
(clapgpu_cascades record, clapgpu_views_source record, bounding volume) triples, the entity sets of the pick's cases, and
the camera path of the captured-frame test."""
import numpy as np

from clap_amd import _lib, cascades as cm

F = np.float32
SENTINEL = 0x7a7a7a7a                                       # what the outputs hold before a call
OUTPUTS = ("cascade", "view_mx", "inv_view_mx", "near_backup_used", "bv_entity", "status", "cam_corners")


def blank_block():
    c = np.zeros(1, cm.CASCADES)
    c.view(np.uint32)[:] = SENTINEL
    return c[0]


def blank_source(light_slot):
    """a source whose every byte is known: matrices in every slot (the light's among them), slot 0 to be filled"""
    s = np.zeros(1, cm.VIEWS_SOURCE)[0]
    for k in range(1, _lib.VIEW_SLOTS):
        s["slot"][k]["view_mx"] = np.arange(16, dtype=F) + k
        s["slot"][k]["proj_mx"] = (np.arange(16, dtype=F) + 0.5) * k
        s["slot"][k]["pos"], s["slot"][k]["flags"] = (k, k, k), 0
    return s


def inputs(light_dir, nr, persp, near_backup, light_slot, z_reverse, z01, from_bv):
    c = blank_block()
    c["light_dir"], c["nr_cascades"], c["persp"], c["near_backup"], c["light_slot"] = light_dir, nr, persp, near_backup, light_slot
    c["flags"] = (_lib.CASCADES_Z_REVERSE if z_reverse else 0) | (_lib.CASCADES_NDC_Z_ZERO_ONE if z01 else 0) | \
        (_lib.CASCADES_NEAR_BACKUP_FROM_BV if from_bv else 0)
    c["pad0"] = 0
    return c


def from_trace(t, i, light_slot=1):
    """camera i of tests/golden/cascades_trace.npz: (block, source, env); persp[] is the trace's own (the reference's)"""
    nr = int(t["nr"][i]) or 4
    persp = np.zeros((4, 16), F)
    persp[:nr] = t["persp"][i][:nr]
    c = inputs(t["light_dir"][i], t["nr"][i], persp, t["near_backup_in"][i], light_slot, t["z_reverse"][i], t["z01"][i], t["has_env"][i])
    s = blank_source(light_slot)
    s0 = s["slot"][0]
    s0["proj_mx"] = t["proj_main"][i]
    z = _lib.VIEW_NDC_Z_ZERO_ONE if t["z01"][i] else 0
    if t["from_pose"][i]:
        s0["pos"], s0["quat"], s0["flags"] = t["pos"][i], t["quat"][i], _lib.VIEW_FROM_POSE | z
    else:
        s0["view_mx"], s0["flags"] = t["view_in"][i], z
    env = (t["env_lo"][i], t["env_hi"][i], t["env_scale"][i]) if t["has_env"][i] else None
    return c, s, env


def _plain(light_slot, pos=(3.0, 12.0, -7.0), quat=(0.1, 0.7, -0.1, 0.69), light_dir=(0.3, -1.0, 0.2), nr=3, proj=None):
    persp = cm.persp(1.0, 1.6, 0.1, 500.0, nr, False)
    c = inputs(light_dir, nr, persp, 2.5, light_slot, True, False, False)
    s = blank_source(light_slot)
    s0 = s["slot"][0]
    s0["pos"], s0["quat"], s0["flags"] = pos, quat, _lib.VIEW_FROM_POSE
    main = np.zeros(16, F)
    _lib.lib().clapgpu_perspective(1.0, 1.6, 0.1, 500.0, 0, main.ctypes.data_as(cm._F))
    s0["proj_mx"] = main if proj is None else proj
    return c, s, None


def edge_cases(light_slot):
    """the named edge cases: name -> (block, source, env)"""
    nan, inf = np.nan, np.inf
    return {
        "nan_position": _plain(light_slot, pos=(nan, 1.0, 2.0)),
        "inf_position": _plain(light_slot, pos=(1.0, inf, 2.0)),
        "zero_quaternion": _plain(light_slot, quat=(0.0, 0.0, 0.0, 0.0)),
        "zero_projection": _plain(light_slot, proj=np.zeros(16, F)),
        "nan_light_direction": _plain(light_slot, light_dir=(0.2, nan, 0.1)),
        "nr_cascades_0": _plain(light_slot, nr=0),
    }


# ---- the pick -----------------------------------------------------------------------------------
PICK_N = (1, 63, 64, 65, 129, 4097)
PICK_CASES = ("none", "one", "three_equal", "only_the_control", "dead", "no_control", "nan_and_inverted", "on_a_face", "mask_only")
CAM, CTL = F([10.0, 20.0, 30.0]), F([-40.0, 5.0, 8.0])


def pick_case(name, n):
    """(flags, aabb, model, model_table, pos_scale, ctl_entity or None, wants result) of one case: n entities whose boxes are
    far from both points unless the case says otherwise.  Entity n - 1 is the control where there is one."""
    rng = np.random.default_rng(n * 31 + PICK_CASES.index(name))
    flags = np.full(n, _lib.E_ALIVE | _lib.E_VISIBLE, np.uint32)
    lo = rng.uniform(100.0, 200.0, (n, 3)).astype(F)
    aabb = np.concatenate([lo, lo + rng.uniform(1.0, 5.0, (n, 3)).astype(F)], 1)
    n_models = 3
    table = np.zeros((n_models, 2, 4), F)
    table[:, 0, :3], table[:, 1, :3] = [-1, -2, -3], [[1, 2, 3], [2, 2, 2], [4, 1, 0.5]]
    model = rng.integers(0, n_models, n).astype(np.int32)
    pos_scale = np.concatenate([rng.uniform(100, 200, (n, 3)), rng.uniform(0.5, 2.0, (n, 1))], 1).astype(F)
    ctl = n - 1
    pos_scale[ctl, :3] = CTL

    def around(i, p, half=3.0):
        aabb[i, :3], aabb[i, 3:] = p - F(half), p + F(half)
    want_result = True
    if name == "one":
        around(n // 2, CAM)
    elif name == "three_equal":                             # equal volumes: one model, one scale; the lowest index wins
        picks = sorted({0, n // 2, max(n - 2, 0)})
        for k, i in enumerate(picks):
            around(i, CAM if k % 2 == 0 else CTL, 2.0 + k)
            model[i], pos_scale[i, 3] = 1, 1.5
    elif name == "only_the_control":
        around(ctl, CTL)
    elif name == "dead":
        around(n // 2, CAM)
        flags[n // 2] &= ~np.uint32(_lib.E_ALIVE)
    elif name == "no_control":                              # a box around the control's position, and nobody asks for it
        around(0, CTL)
        ctl = None
    elif name == "nan_and_inverted":
        around(0, CAM)
        aabb[0, 1] = np.nan
        if n > 1:
            around(n // 2, CAM)
            aabb[n // 2, [0, 3]] = aabb[n // 2, [3, 0]]
    elif name == "on_a_face":
        around(n // 2, CAM)
        aabb[n // 2, 3] = CAM[0]                             # the camera's x is the box's max x, exactly
    elif name == "mask_only":
        if n > 1:
            around(0, CTL)
        around(n // 2, CAM)
        want_result = False
    if n == 1 and name != "only_the_control":               # the only entity cannot be both the volume and the control
        ctl = None
    return flags, aabb, model, table, pos_scale, ctl, want_result


# ---- the captured-frame test's camera path -----------------------------------------------------
FRAMES = 10


def path_quat(k):
    """camera_move's quaternion of frame k (the host's input): a yaw that turns 4 degrees a frame at a pitch of 25"""
    yaw, pitch = np.radians(25.0 + 4.0 * k), np.radians(25.0)
    cy, sy, cp, sp = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2)
    return F([cy * sp, sy * cp, -sy * sp, cy * cp])         # yaw about y, then pitch about x
