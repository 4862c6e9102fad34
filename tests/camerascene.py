"""The one scene and the named cases of the camera tests (tests/test_camera.py chooses and checks them on the CPU with
cameraref's brute-force caster; tests/test_camera_gpu.py runs them): the smallest scene at which each path of
clapgpu_camera_calc can go wrong.

Bodies: 0 the control's capsule (skipped as self; the targets of entity 0 lie inside it), 1 and 2 spheres.
Statics: 0 a wall behind entity 0, 1 a ceiling over it, 2 a small box around entity 2's target, 3 a sphere that
coincides with body 1 (the same collider on the same numbers: the body/static tie), 4 the terrain (OTHER, with a
4 x 4-quad mesh), 5 an OTHER static without a mesh.
Entities (the controls the cases pick): 0 at the origin, 1 beside the spheres (not a character: the target is its
centre), 2 inside the small box, 3 beside the OTHER static, 4 over the terrain (with a head joint), 5 far from everything.
"""
import math

import numpy as np

SPHERE, CAPSULE, BOX, OTHER = 0, 1, 2, 3
IS_CHARACTER, HAS_HEAD_JOINT = 1, 2

# ---- colliders -----------------------------------------------------------------------------------
BODY_POS = np.array([[0.0, 1.0, 0.0], [20.0, 1.5, 2.0], [0.9, 2.1, 1.9]])
BODY_RADIUS = np.array([0.4, 0.5, 0.45])
BODY_LENGTH = np.array([1.0, 0.0, 0.0])
CELL = 2.0                                            # >= every body box's edge: the index is usable

TERRAIN_POS = np.array([80.0, 0.0, 80.0])


def terrain():
    """(vertices [25, 3] float32 in model space, indices [32, 3] uint16): 4 x 4 quads of 2 m, front faces up"""
    vx = np.array([[2.0 * i - 4.0, 0.15 * math.sin(1.3 * i) * math.cos(0.7 * j), 2.0 * j - 4.0]
                   for i in range(5) for j in range(5)], np.float32)
    at = lambda i, j: 5 * i + j
    idx = []
    for i in range(4):
        for j in range(4):
            idx += [[at(i, j), at(i, j + 1), at(i + 1, j)], [at(i + 1, j), at(i, j + 1), at(i + 1, j + 1)]]
    return vx, np.array(idx, np.uint16)


def terrain_tris():
    vx, idx = terrain()
    return (vx.astype(np.float64) + TERRAIN_POS)[idx.astype(int)]


def static_boxes():
    """[6, 6] (minx, maxx, miny, maxy, minz, maxz)"""
    t = terrain_tris().reshape(-1, 3)
    return np.array([
        [-5.0, 5.0, 0.0, 5.0, 3.0, 3.5],                                  # 0 the wall behind entity 0
        [-5.0, 5.0, 4.0, 4.5, -5.0, 5.0],                                 # 1 the ceiling
        [40.0 - 0.03, 40.0 + 0.03, 1.5 - 0.03, 1.5 + 0.03, -0.03, 0.03],  # 2 around entity 2's target
        [19.5, 20.5, 1.0, 2.0, 1.5, 2.5],                                 # 3 the sphere that coincides with body 1
        [t[:, 0].min(), t[:, 0].max(), t[:, 1].min() - 0.01, t[:, 1].max() + 0.01, t[:, 2].min(), t[:, 2].max()],  # 4 terrain
        [59.0, 61.0, 0.0, 3.0, 2.0, 3.0],                                 # 5 OTHER, no mesh
    ])


STATIC_KIND = np.array([BOX, BOX, BOX, SPHERE, OTHER, OTHER], np.uint8)
MESH_STATIC = 4


def static_geo():
    bb = static_boxes()
    pos = (bb[:, 0::2] + bb[:, 1::2]) / 2
    pos[3] = BODY_POS[1]
    radius = np.zeros(6)
    radius[3] = BODY_RADIUS[1]
    return pos, np.tile([0.0, 0.0, 1.0], (6, 1)), radius, np.zeros(6)


def brute_scene(meshes):
    """the scene for cameraref.brute_cast; without the mesh set the terrain is an OTHER static like any other"""
    bb = static_boxes()
    pos, _axis, radius, _length = static_geo()
    bodies = [dict(kind="capsule", pos=BODY_POS[0], axis=[0.0, 1.0, 0.0], radius=BODY_RADIUS[0], length=BODY_LENGTH[0]),
              dict(kind="sphere", pos=BODY_POS[1], radius=BODY_RADIUS[1]), dict(kind="sphere", pos=BODY_POS[2], radius=BODY_RADIUS[2])]
    names = {SPHERE: "sphere", BOX: "box", OTHER: "other"}
    statics = [dict(kind=names[int(k)], aabb=bb[s], pos=pos[s], radius=radius[s]) for s, k in enumerate(STATIC_KIND)]
    return dict(bodies=bodies, statics=statics, tris={MESH_STATIC: terrain_tris()} if meshes else {})


# ---- the control entities ------------------------------------------------------------------------
MODEL_TABLE = np.array([[[-0.5, 0.0, -0.5, 0.0], [0.5, 2.0, 0.5, 0.0]],          # 0: a character's box, Y = 2
                        [[-1.0, -1.0, -1.0, 0.0], [1.0, 1.0, 1.0, 0.0]]], np.float32)
ENT_POS_SCALE = np.array([[0, 0, 0, 1], [20, 0, 0, 1], [40, 0, 0, 1], [60, 0, 0, 1], [80, 0, 80, 1], [200, 0, 200, 1]], np.float32)
ENT_MODEL = np.array([0, 1, 0, 0, 0, 0], np.int32)
ENT_CENTER = np.array([[0, 1, 0], [20, 1.5, 0], [40, 1, 0], [60, 1, 0], [80, 1, 80], [200, 1, 200]], np.float32)
ENT_CHARACTER = np.array([1, 0, 1, 1, 1, 1], bool)
HEAD_JOINT = 3                                         # entity 4's head: joint_pos[3]
JOINT_POS = np.zeros((5, 4), np.float32)
JOINT_POS[HEAD_JOINT] = [80.0, 1.7, 80.0, 1.0]


def quat_yaw_pitch(yaw, pitch):
    """float32 (x, y, z, w) of a yaw about y then a pitch about x, in degrees"""
    y, p = math.radians(yaw) / 2, math.radians(pitch) / 2
    qy, qp = (0.0, math.sin(y), 0.0, math.cos(y)), (math.sin(p), 0.0, 0.0, math.cos(p))
    (ax, ay, az, aw), (bx, by, bz, bw) = qy, qp
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], np.float32)


def case(name, entity, yaw=0.0, pitch=0.0, near=0.1, far=500.0, aspect=16.0 / 9.0, skip=0, moved=1, head=False, quat=None):
    return dict(name=name, entity=entity, quat=quat_yaw_pitch(yaw, pitch) if quat is None else np.asarray(quat, np.float32),
                near=near, far=far, aspect=aspect, skip=skip, moved=moved,
                flags=(IS_CHARACTER if ENT_CHARACTER[entity] else 0) | (HAS_HEAD_JOINT if head else 0),
                head_joint=HEAD_JOINT if head else 0)


NAN = float("nan")
CASES = [
    case("no_hit", 5),
    case("one_pull_in", 0),
    case("three_pull_ins", 0, yaw=10.0, pitch=-35.0, near=0.6, aspect=1.0),
    case("triangle_wins", 4, pitch=60.0, head=True),
    case("body_static_tie", 1),
    case("collapse_inside_a_box", 2),
    case("unresolved", 3),
    case("no_physics", 0, skip=-1),
    case("not_moved", 0, moved=0),
    case("nan_quaternion", 0, quat=[NAN, 0.0, 0.0, 1.0]),
]


def entity_inputs(c):
    """what camera_target reads of the case's control entity"""
    e = c["entity"]
    m = MODEL_TABLE[ENT_MODEL[e]]
    return dict(flags=c["flags"], pos_scale=ENT_POS_SCALE[e], lo=m[0, :3], hi=m[1, :3], center=ENT_CENTER[e],
                head=JOINT_POS[c["head_joint"], :3])
