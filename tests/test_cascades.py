"""CPU: the shadow cascades on the device (include/clapgpu.h, "The shadow cascades on the device", ABI 51) -- the version
and the symbols, the block's layout against gcc and the Python mirror's dtype, the two new descriptor fields, the host
twins and tests/cascadesref.py against a trace of the reference's own view.c at every recorded intermediate, the refusals
every entry point owes before any HIP call, and that the cases of tests/test_cascades_gpu.py do what they are named for.
No GPU is touched.

tests/golden/cascades_trace.npz (README beside it) was recorded by a harness that is not part of the repository: the
reference's core/view.c and core/model.c included into one translation unit (the build recipe of SURVEY.md, Appendix A),
renderer_mat4x4_ortho / _perspective / renderer_get_caps doubled by a switch over the reference's own linmath.h
functions, run over 96 seeded cameras.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from clap_amd import _lib, cascades as cm
import cameraref as cr
import cascadescases as cc
import cascadesref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("clapgpu_cascades_calc", "clapgpu_cascades_calc_host", "clapgpu_cascades_near_backup", "clapgpu_cascades_persp",
               "clapgpu_entities_bv_views")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def as_bytes(a):
    return np.ascontiguousarray(np.atleast_1d(a)).view(np.uint8).reshape(-1)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def trace(golden_dir):
    t = dict(np.load(os.path.join(golden_dir, "cascades_trace.npz")))
    assert len(t["nr"]) >= 64
    return t


# ---- ABI ---------------------------------------------------------------------------------------------
def test_abi_version_symbols_and_exports(L):
    assert _lib.ABI_VERSION >= 51 and L.clapgpu_abi_version() == _lib.ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {l.split()[-1] for l in out.stdout.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "clapgpu.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name) and name in exported and name + "(" in header, name


def test_descriptor_fields_stand_behind_views_state():
    names = [f for f, _t in _lib.FrameDesc._fields_]
    at = names.index("views_state")
    assert names[at + 1:at + 5] == ["cascades", "bv_result", "bv_has_ctl", "bv_ctl_entity"]
    assert names[-2:] == ["camera", "camera_bp"]
    fields = dict(_lib.FrameDesc._fields_)
    assert fields["cascades"] is C.c_void_p and fields["bv_result"] is C.c_void_p


def test_block_size_and_offsets_equal_gcc_and_the_dtype(tmp_path):
    prints = ""
    for cname, dt in (("clapgpu_cascades", cm.CASCADES), ("clapgpu_cascade_view", cm.CASCADE_VIEW)):
        prints += "".join(f'printf("%zu %zu\\n", offsetof({cname}, {n}), sizeof((({cname} *)0)->{n}));' for n in dt.names)
    src, exe = tmp_path / "casc.c", tmp_path / "casc"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "clapgpu.h"\nint main(void) { '
                   'printf("%zu %d %zu %d\\n", sizeof(clapgpu_cascades), CLAPGPU_CASCADES_BYTES, sizeof(clapgpu_cascade_view), '
                   'CLAPGPU_CASCADE_VIEW_BYTES);' + prints + ' return 0; }\n')
    p = subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [[int(v) for v in l.split()] for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert rows[0] == [cm.CASCADES.itemsize, _lib.CASCADES_BYTES, cm.CASCADE_VIEW.itemsize, _lib.CASCADE_VIEW_BYTES]
    assert rows[0][0] % 16 == 0 and rows[0][2] % 16 == 0
    at = 1
    for dt, cls in ((cm.CASCADES, _lib.Cascades), (cm.CASCADE_VIEW, _lib.CascadeView)):
        for n in dt.names:
            d, off = dt.fields[n][:2]
            assert [off, d.itemsize] == rows[at], n
            assert getattr(cls, n).offset == off and getattr(cls, n).size == d.itemsize, n
            at += 1
    assert cm.VIEWS_SOURCE.itemsize == C.sizeof(_lib.ViewsSource)
    for n in cm.VIEW_SOURCE.names:
        assert cm.VIEW_SOURCE.fields[n][1] == getattr(_lib.ViewSource, n).offset, n


# ---- the trace ---------------------------------------------------------------------------------------
def test_trace_covers_what_it_must(trace):
    t = trace
    pose, z01, zr = t["from_pose"] == 1, t["z01"] == 1, t["z_reverse"] == 1
    for a in (pose, z01, zr):
        for b in (z01, zr):
            assert (a & b).any() and (a & ~b).any() and (~a & b).any() and (~a & ~b).any() or a is b
    assert set(t["nr"].tolist()) == {0, 1, 2, 3, 4}
    d = t["light_dir"]
    assert ((d[:, 0] == 0) & (d[:, 1] == -1) & (d[:, 2] == 0)).any() and (d == 0).all(1).any()       # straight down; zero
    nb = t["near_backup_in"][t["has_env"] == 0]
    assert (nb == 0).any() and ((nb > 0) & (nb < 1)).any() and (nb > 1).any()
    assert (t["has_env"] == 1).sum() >= 16
    # the up-vector swap: fits on both sides of 0.999f within a few ulp, found by the restatement's own forward vector
    near, swapped, kept = 0, 0, 0
    for i in range(len(t["nr"])):
        y = np.float32(abs(ref.norm3([-v for v in d[i]])[1])) if np.any(d[i] != 0) else np.float32(0)
        ulps = abs(int(bits(y).item()) - int(bits(np.float32(0.999)).item()))
        if ulps <= 8:
            near += 1
            swapped += int(y > np.float32(0.999))
            kept += int(y <= np.float32(0.999))
    assert near >= 8 and swapped >= 2 and kept >= 2, (near, swapped, kept)


def _check_against_trace(t, i, oc, os_, slot, what):
    nr = int(t["nr"][i]) or 4
    nn = ref.one_nan
    assert same(oc["cam_corners"][:nr], nn(t["cam_corners"][i][:nr])) and same(oc["cam_corners"][4], nn(t["cam_corners"][i][4])), \
        f"{what} {i}: the camera's frustum corners"
    assert same(oc["near_backup_used"], nn(t["near_backup"][i])), f"{what} {i}: near_backup"
    assert same(oc["view_mx"], nn(t["light_view"][i])) and same(oc["inv_view_mx"], nn(t["light_inv_view"][i])), f"{what} {i}: the main view"
    assert same(os_["slot"][slot]["view_mx"], nn(t["light_view"][i])), f"{what} {i}: the light's slot"
    for v in range(nr):
        k = oc["cascade"][v]
        assert same(k["view_mx"], nn(t["sub_view"][i, v])) and same(k["inv_view_mx"], nn(t["sub_inv_view"][i, v])), f"{what} {i}: view {v}"
        assert same(k["proj_mx"], nn(t["sub_proj"][i, v])) and same(k["inv_proj_mx"], nn(t["sub_inv_proj"][i, v])), f"{what} {i}: proj {v}"
        assert same(k["far_plane"], nn(t["sub_far"][i, v])) and same(k["near_plane"], t["sub_near"][i, v]), f"{what} {i}: planes {v}"
        assert same(k["mvp"], nn(ref.flat(cr.mat_mul(ref.mat(t["sub_proj"][i, v]), ref.mat(t["sub_view"][i, v]))))), f"{what} {i}: mvp {v}"
    return nr


@pytest.mark.parametrize("slot", [1, 4])
def test_host_twin_against_the_trace(L, trace, slot):
    t = trace
    for i in range(len(t["nr"])):
        c, s, env = cc.from_trace(t, i, slot)
        oc, os_ = cm.calc_host(c, s, env)
        nr = _check_against_trace(t, i, oc, os_, slot, "twin")
        assert oc["status"] == 0 and oc["bv_entity"] == (0 if env is not None else _lib.CASCADES_NO_ENTITY)
        # what is not an output of this call keeps its bytes: the surplus cascades, the inputs, every other slot
        assert np.array_equal(as_bytes(oc["cascade"][nr:]), as_bytes(c["cascade"][nr:]))
        assert np.array_equal(as_bytes(oc["cam_corners"][nr:4]), as_bytes(c["cam_corners"][nr:4]))
        for k in ("light_dir", "nr_cascades", "persp", "near_backup", "light_slot", "flags", "pad0", "pad1"):
            assert np.array_equal(as_bytes(oc[k]), as_bytes(c[k])), k
        want = s.copy()
        want["slot"][slot]["view_mx"] = oc["view_mx"]
        assert np.array_equal(as_bytes(os_), as_bytes(want))


def test_restatement_against_the_trace_and_the_twin(L, trace):
    t, swaps = trace, 0
    for i in range(len(t["nr"])):
        c, s, env = cc.from_trace(t, i, 2)
        rc, rs, n = ref.calc(c, s, env)
        swaps += n
        _check_against_trace(t, i, rc, rs, 2, "cascadesref")
        oc, os_ = cm.calc_host(c, s, env)
        assert np.array_equal(as_bytes(rc), as_bytes(oc)) and np.array_equal(as_bytes(rs), as_bytes(os_)), i
    assert swaps >= 8


def test_persp_and_near_backup_twins_against_the_trace(L, trace):
    t = trace
    for i in range(len(t["nr"])):
        nr = int(t["nr"][i]) or 4
        p = cm.persp(t["fov"][i], t["aspect"][i], t["near_plane"][i], t["far_plane"][i], int(t["nr"][i]), bool(t["z01"][i]))
        assert same(p[:nr], t["persp"][i][:nr]) and not p[nr:].any(), i
        if t["has_env"][i]:
            args = (t["light_dir"][i], t["env_lo"][i], t["env_hi"][i], t["env_scale"][i])
            want = ref.one_nan(t["near_backup"][i])
            assert same(cm.near_backup(*args), want) and same(np.float32(ref.near_backup(*args)), want), i


def test_edge_cases_do_what_they_are_named_for(L):
    for slot in (1, 4):
        for name, (c, s, env) in cc.edge_cases(slot).items():
            oc, os_ = cm.calc_host(c, s, env)
            rc, rs, _n = ref.calc(c, s, env)
            assert np.array_equal(as_bytes(rc), as_bytes(oc)) and np.array_equal(as_bytes(rs), as_bytes(os_)), name
            assert oc["status"] == 0
            nr = int(c["nr_cascades"]) or 4
            if name == "nr_cascades_0":
                assert nr == 4 and np.isfinite(oc["cascade"]["mvp"]).all()
            else:
                outs = np.concatenate([oc["view_mx"], oc["cascade"][:nr]["mvp"].ravel()])
                assert np.isnan(outs).any(), name                       # the non-finite input reaches the outputs ...
                out = oc.copy()
                out["bv_entity"] = 0                                      # (no float: CLAPGPU_CASCADES_NO_ENTITY)
                every = np.concatenate([as_bytes(out).view(np.uint32), as_bytes(os_).view(np.uint32)])
                f = every.view(np.float32)
                assert (every[np.isnan(f)] == 0x7fc00000).all(), name    # ... as the one quiet NaN


def test_invalid_blocks_are_reported_and_nothing_else_is_written(L):
    for what in ("from_pose", "slot_0", "slot_5", "nr_5"):
        c, s, env = cc.edge_cases(2)["nr_cascades_0"]
        if what == "from_pose":
            s["slot"][2]["flags"] = _lib.VIEW_FROM_POSE
        elif what == "nr_5":
            c["nr_cascades"] = 5
        else:
            c["light_slot"] = 0 if what == "slot_0" else 5
        oc, os_ = cm.calc_host(c, s, env)
        want = c.copy()
        want["status"] = _lib.CASCADES_INVALID
        assert np.array_equal(as_bytes(oc), as_bytes(want)) and np.array_equal(as_bytes(os_), as_bytes(s)), what
        rc, rs, _n = ref.calc(c, s, env)
        assert np.array_equal(as_bytes(rc), as_bytes(want)), what


# ---- the pick's cases --------------------------------------------------------------------------------
def _pick_ref(flags, aabb, model, table, pos_scale, ctl, cam):
    """model.c:1703-1713 in float32: (key, inside bits)"""
    n, key, inside = len(flags), 0, np.zeros(len(flags), bool)
    def holds(p, b):
        return bool((p >= b[:3]).all() and (p <= b[3:]).all())
    for i in range(n):
        if not flags[i] & _lib.E_ALIVE:
            continue
        hit = holds(cam, aabb[i]) or (ctl is not None and holds(pos_scale[ctl, :3], aabb[i]))
        if not hit or (ctl is not None and i == ctl):
            continue
        inside[i] = True
        e = np.abs(table[model[i], 1, :3] - table[model[i], 0, :3]) * pos_scale[i, 3]
        vol = np.float32(np.float32(e[0] * e[1]) * e[2])
        key = max(key, (int(bits(vol).item()) << 32) | (0xFFFFFFFF - i))
    return key, inside


def test_pick_cases_do_what_they_are_named_for():
    for n in cc.PICK_N:
        for name in cc.PICK_CASES:
            flags, aabb, model, table, ps, ctl, want_result = cc.pick_case(name, n)
            key, inside = _pick_ref(flags, aabb, model, table, ps, ctl, cc.CAM)
            who = -1 if key == 0 else 0xFFFFFFFF - (key & 0xFFFFFFFF)
            if name in ("none", "only_the_control", "dead", "no_control"):
                assert key == 0 and not inside.any(), (name, n)
            if name == "only_the_control":
                assert ctl == n - 1 and _pick_ref(flags, aabb, model, table, ps, None, ps[ctl, :3])[0] != 0
            if name == "dead":
                alive = flags | np.uint32(_lib.E_ALIVE)
                assert _pick_ref(alive, aabb, model, table, ps, ctl, cc.CAM)[0] != 0
            if name == "no_control":
                assert _pick_ref(flags, aabb, model, table, ps, 0 if n == 1 else n - 1, cc.CAM)[0] != 0 or n == 1
            if name in ("one", "on_a_face"):
                assert inside.sum() == 1 and who == n // 2, (name, n)
            if name == "three_equal":
                picks = np.flatnonzero(inside)
                assert who == picks[0] and len(picks) == len({0, n // 2, max(n - 2, 0)} - ({ctl} if ctl is not None else set()))
                e = [np.abs(table[model[i], 1, :3] - table[model[i], 0, :3]) * ps[i, 3] for i in picks]
                assert all(same(np.float32(x), np.float32(e[0])) for x in e)
            if name == "nan_and_inverted":
                assert key == 0 and not inside.any()
            if name == "mask_only":
                assert not want_result and inside.sum() >= 1


# ---- the captured-frame test's path ------------------------------------------------------------------
def test_the_graph_tests_light_view_changes_along_its_path(L):
    """the condition that keeps the captured-frame test from passing on a frozen view: along its camera path the host
    twin's light view differs from frame 0's in at least 8 of the 10 replayed frames"""
    target, dist = np.float32([3.0, 2.0, -4.0]), np.float32(6.0)
    views = []
    for k in range(cc.FRAMES + 1):
        q = cc.path_quat(k)
        c, s, env = cc._plain(1, pos=cr.orbit(q, target, dist), quat=q)
        oc, _s = cm.calc_host(c, s, env)
        assert np.isfinite(oc["view_mx"]).all()
        views.append(oc["view_mx"].copy())
    differ = sum(not same(v, views[0]) for v in views[1:])
    assert differ >= 8, differ


# ---- the refusals --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mem():
    raw = C.create_string_buffer(16384 + 256)
    at = (C.addressof(raw) + 255) & ~255

    def filled(cls):
        d = cls()
        for name, t in cls._fields_:
            if t is C.c_void_p:
                setattr(d, name, at)
        return d
    ent = filled(_lib.Entities)
    ent.n = 64
    views = _lib.Views()
    views.n = 1
    views.vis_mask[0] = views.vis_row_pop[0] = at
    return dict(raw=raw, ok=at, odd=at + 4, ent=ent, views=views)


def test_cascades_calc_refuses_before_any_hip_call(L, mem):
    """No device exists here: a call that got as far as a launch would fail with another code."""
    ok, odd, bad = mem["ok"], mem["odd"], _lib.ERR_INVALID_ARGUMENTS
    e = C.byref(mem["ent"])
    call = L.clapgpu_cascades_calc
    assert call(None, None, ok, e, None) == bad                 # a NULL block
    assert call(None, odd, ok, e, None) == bad                  # a misaligned block
    assert call(None, ok, None, e, None) == bad                 # a NULL source
    assert call(None, ok, odd, e, None) == bad                  # a misaligned source
    assert call(None, ok, ok, None, None) == bad                # no entities
    for name in ("pos_scale", "model", "model_table"):          # a key to resolve, and not the arrays to resolve it with
        ent = _lib.Entities.from_buffer_copy(mem["ent"])
        setattr(ent, name, None)
        assert call(None, ok, ok, C.byref(ent), ok) == bad, name


def test_bv_views_refuses_before_any_hip_call(L, mem):
    ok, odd, bad = mem["ok"], mem["odd"], _lib.ERR_INVALID_ARGUMENTS
    call = L.clapgpu_entities_bv_views
    assert call(None, C.byref(mem["ent"]), None, 0, 0, ok, None) == bad          # a NULL state
    assert call(None, C.byref(mem["ent"]), odd, 0, 0, ok, None) == bad           # a misaligned state
    assert call(None, None, ok, 0, 0, ok, None) == bad                           # no entities
    for name in ("flags", "aabb", "model", "model_table", "pos_scale"):
        ent = _lib.Entities.from_buffer_copy(mem["ent"])
        setattr(ent, name, None)
        assert call(None, C.byref(ent), ok, 0, 0, ok, None) == bad, name
    assert call(None, C.byref(mem["ent"]), ok, 1, 3, None, None) == _lib.OK      # nothing asked for: nothing launched


def test_frame_refuses_cascades_without_their_views(L, mem):
    ok, bad = mem["ok"], _lib.ERR_INVALID_ARGUMENTS
    fr = _lib.Frustum()

    def issue(cascades, block=True, frustum=False, views=True, n_views=1):
        ent = _lib.Entities.from_buffer_copy(mem["ent"])
        v = _lib.Views.from_buffer_copy(mem["views"])
        v.n = n_views
        ent.views = C.pointer(v) if views else None
        f = _lib.FrameDesc()
        f.entities = C.pointer(ent)
        if frustum:
            f.frustum = C.pointer(fr)
        if block:
            f.views_source = f.views_state = ok
        f.cascades = cascades
        return L.clapgpu_frame_issue(None, C.byref(f), 0.0, 0)
    assert issue(ok, block=False) == bad                         # no view block to write
    assert issue(ok, block=False, frustum=True) == bad           # host views
    assert issue(mem["odd"]) == bad                              # a misaligned block
    assert issue(ok, views=False) == bad                         # no further view: no slot for the light
    assert issue(ok, n_views=0) == bad
