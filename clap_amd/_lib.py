"""ctypes binding of clap_amd/lib/libclapgpu.so (the C ABI of include/clapgpu.h).

There is no CPU fallback: if the HIP library is missing or a call fails the
binding raises.  Nothing here imports ``oracle``.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CLAPGPU_LIB") or os.path.join(_HERE, "lib", "libclapgpu.so")   # override: A/B builds
CSRC = os.path.join(_HERE, "csrc")
ABI_VERSION = 53

OK = 0
ERR_NOMEM = -1
ERR_INVALID_ARGUMENTS = -2
ERR_NOT_SUPPORTED = -3
ERR_TOO_LARGE = -11
ERR_INIT_FAILED = -14
ERR_OUT_OF_BOUNDS = -26
ERR_UNKNOWN = -32

E_VISIBLE = 1 << 0
E_SKIP_CULLING = 1 << 14
E_DIRTY = 1 << 16
E_JOINT_ATTACHED = 1 << 17
E_ALIVE = 1 << 31
RAY_INVALID = 1 << 0
RAY_UNRESOLVED = 1 << 1
RAY_MOVED_TARGET = 1 << 2
SLIDE_INVALID = 1 << 0
SLIDE_UNRESOLVED = 1 << 1
SLIDE_MOVED_TARGET = 1 << 2
UPDATE_ALL_DIRTY = 1 << 0

_ERR_NAMES = {ERR_NOMEM: "NOMEM", ERR_INVALID_ARGUMENTS: "INVALID_ARGUMENTS", ERR_NOT_SUPPORTED: "NOT_SUPPORTED",
              ERR_TOO_LARGE: "TOO_LARGE", ERR_INIT_FAILED: "INITIALIZATION_FAILED",
              ERR_OUT_OF_BOUNDS: "OUT_OF_BOUNDS", ERR_UNKNOWN: "UNKNOWN_ERROR"}


class ClapGpuError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        super().__init__(f"{where}: CERR_{_ERR_NAMES.get(code, code)} ({code}) {detail}".rstrip())


class Frustum(C.Structure):
    """clapgpu_frustum: planes[6][4], corners[8][4] (view.h:16-17)."""
    _fields_ = [("planes", C.c_float * 24), ("corners", C.c_float * 32)]


class BvQuery(C.Structure):
    """clapgpu_bv_query (include/clapgpu.h)."""
    _fields_ = [("cam_pos", C.c_float * 3), ("has_ctl", C.c_uint32), ("ctl_pos", C.c_float * 3),
                ("ctl_entity", C.c_uint32), ("result", C.c_void_p), ("inside_mask", C.c_void_p)]


EXTRA_VIEWS_MAX = 4


class Views(C.Structure):
    """clapgpu_views (include/clapgpu.h): the frame's other frusta, culled by the same launch as the main one."""
    _fields_ = [("n", C.c_uint32), ("pad", C.c_uint32), ("frustum", Frustum * EXTRA_VIEWS_MAX),
                ("vis_mask", C.c_void_p * EXTRA_VIEWS_MAX), ("vis_row_pop", C.c_void_p * EXTRA_VIEWS_MAX),
                ("host_vis_mask", C.c_void_p * EXTRA_VIEWS_MAX)]


VIEW_SLOTS = 1 + EXTRA_VIEWS_MAX
VIEW_FROM_POSE, VIEW_NDC_Z_ZERO_ONE = 1, 2


class ViewSource(C.Structure):
    """clapgpu_view_source (include/clapgpu.h): what one view is -- matrices, or a pose."""
    _fields_ = [("view_mx", C.c_float * 16), ("proj_mx", C.c_float * 16), ("pos", C.c_float * 3), ("flags", C.c_uint32),
                ("quat", C.c_float * 4)]


class ViewsSource(C.Structure):
    """clapgpu_views_source: slot 0 the main view, slot 1 + k further view k.  Lives in device memory."""
    _fields_ = [("slot", ViewSource * VIEW_SLOTS)]


class ViewState(C.Structure):
    """clapgpu_view_state (include/clapgpu.h): what the kernels read of one view."""
    _fields_ = [("frustum", Frustum), ("cull", C.c_uint32 * 8), ("view_mx", C.c_float * 16), ("proj_mx", C.c_float * 16),
                ("mvp", C.c_float * 16), ("cam_pos", C.c_float * 3), ("pad", C.c_uint32)]


class ViewsState(C.Structure):
    """clapgpu_views_state: written by clapgpu_views_calc alone.  Lives in device memory."""
    _fields_ = [("slot", ViewState * VIEW_SLOTS)]


VIEWS_SOURCE_BYTES, VIEWS_STATE_BYTES = 800, 2320           # CLAPGPU_VIEWS_*_BYTES
assert C.sizeof(ViewsSource) == VIEWS_SOURCE_BYTES and C.sizeof(ViewsState) == VIEWS_STATE_BYTES


CAMERA_IS_CHARACTER, CAMERA_HAS_HEAD_JOINT = 1, 2
CAMERA_UNRESOLVED, CAMERA_CAPPED, CAMERA_INVALID = 1, 2, 4
CAMERA_ITER_MAX = 16384


class Camera(C.Structure):
    """clapgpu_camera (include/clapgpu.h): the camera controller's block.  Lives in device memory."""
    _fields_ = [("quat", C.c_float * 4), ("pos", C.c_float * 3), ("dist", C.c_float),
                ("near_plane", C.c_float), ("far_plane", C.c_float), ("aspect", C.c_float), ("moved", C.c_uint32),
                ("ctl_entity", C.c_uint32), ("ctl_skip", C.c_int32), ("flags", C.c_uint32), ("head_joint", C.c_uint32),
                ("target", C.c_float * 3), ("updated", C.c_uint32), ("corner", C.c_float * 16),
                ("iterations", C.c_uint32), ("status", C.c_uint32), ("pad", C.c_uint32 * 2)]


CAMERA_BYTES = 160                                           # CLAPGPU_CAMERA_BYTES
assert C.sizeof(Camera) == CAMERA_BYTES
CAMERA_CAST_FN = C.CFUNCTYPE(C.c_uint32, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double))


CASCADES_MAX = 4
CASCADES_Z_REVERSE, CASCADES_NDC_Z_ZERO_ONE, CASCADES_NEAR_BACKUP_FROM_BV = 1, 2, 4
CASCADES_INVALID = 1
CASCADES_NO_ENTITY = 0xFFFFFFFF


class CascadeView(C.Structure):
    """clapgpu_cascade_view (include/clapgpu.h): one light sub-view of the cascades block."""
    _fields_ = [("view_mx", C.c_float * 16), ("inv_view_mx", C.c_float * 16), ("proj_mx", C.c_float * 16),
                ("inv_proj_mx", C.c_float * 16), ("mvp", C.c_float * 16), ("near_plane", C.c_float), ("far_plane", C.c_float),
                ("pad", C.c_uint32 * 2)]


class Cascades(C.Structure):
    """clapgpu_cascades (include/clapgpu.h): the shadow cascades' block.  Lives in device memory."""
    _fields_ = [("light_dir", C.c_float * 3), ("nr_cascades", C.c_uint32), ("persp", C.c_float * 64),
                ("near_backup", C.c_float), ("light_slot", C.c_uint32), ("flags", C.c_uint32), ("pad0", C.c_uint32),
                ("cascade", CascadeView * CASCADES_MAX), ("view_mx", C.c_float * 16), ("inv_view_mx", C.c_float * 16),
                ("near_backup_used", C.c_float), ("bv_entity", C.c_uint32), ("status", C.c_uint32), ("pad1", C.c_uint32),
                ("cam_corners", C.c_float * 160)]


CASCADE_VIEW_BYTES, CASCADES_BYTES = 336, 2416               # CLAPGPU_CASCADE*_BYTES
assert C.sizeof(CascadeView) == CASCADE_VIEW_BYTES and C.sizeof(Cascades) == CASCADES_BYTES


class Entities(C.Structure):
    """clapgpu_entities (include/clapgpu.h)."""
    _fields_ = [("n", C.c_uint32), ("n_models", C.c_uint32),
                ("pos_scale", C.c_void_p), ("rot", C.c_void_p), ("parent", C.c_void_p),
                ("model", C.c_void_p), ("model_table", C.c_void_p), ("flags", C.c_void_p),
                ("seqs", C.c_void_p), ("mx", C.c_void_p), ("inv_mx", C.c_void_p),
                ("aabb", C.c_void_p), ("center", C.c_void_p), ("vis_mask", C.c_void_p),
                ("vis_row_pop", C.c_void_p), ("n_attach", C.c_uint32), ("pad", C.c_uint32),
                ("attach", C.c_void_p), ("jt_pool", C.c_void_p), ("bind_pool", C.c_void_p),
                ("attach_local", C.c_void_p), ("bv", C.POINTER(BvQuery)), ("rebuilt_mask", C.c_void_p),
                ("views", C.POINTER(Views))]


class Particles(C.Structure):
    """clapgpu_particles (include/clapgpu.h)."""
    _fields_ = [("n", C.c_uint32), ("n_sys", C.c_uint32), ("sys", C.c_void_p), ("row_sys", C.c_void_p),
                ("pos", C.c_void_p), ("vel", C.c_void_p), ("rng_state", C.c_void_p),
                ("billboard_mx", C.c_void_p), ("respawn_mask", C.c_void_p), ("respawn_row_pop", C.c_void_p),
                ("respawn_list", C.c_void_p), ("respawn_count", C.c_void_p), ("scratch", C.c_void_p),
                ("respawn_groups", C.c_void_p)]


class AnimClock(C.Structure):
    """clapgpu_anim_clock (include/clapgpu.h)."""
    _fields_ = [("n_chars", C.c_uint32), ("n_anims", C.c_uint32), ("anim", C.c_void_p), ("time_end", C.c_void_p),
                ("ani_time", C.c_void_p), ("speed", C.c_void_p), ("restart", C.c_void_p), ("frame_time", C.c_void_p),
                ("ended", C.c_void_p)]


class Skeleton(C.Structure):
    _fields_ = [("nr_joints", C.c_uint32), ("n_levels", C.c_uint32), ("parent", C.c_void_p), ("depth", C.c_void_p),
                ("root_pose", C.c_void_p), ("invmx", C.c_void_p), ("bind", C.c_void_p)]


class Animations(C.Structure):
    _fields_ = [("n_anims", C.c_uint32), ("n_times", C.c_uint32), ("chan_table", C.c_void_p),
                ("times", C.c_void_p), ("data", C.c_void_p), ("packed", C.c_void_p), ("packed_keys", C.c_uint32),
                ("packed_layout", C.c_uint32), ("n_data", C.c_uint32), ("pad", C.c_uint32)]


class PoseBatch(C.Structure):
    _fields_ = [("n_chars", C.c_uint32), ("skip", C.c_uint32), ("anim", C.c_void_p), ("frame_time", C.c_void_p), ("entity", C.c_void_p),
                ("entity_mx", C.c_void_p), ("trs", C.c_void_p), ("joint_transforms", C.c_void_p),
                ("joint_pos", C.c_void_p)]


class SkinBatch(C.Structure):
    _fields_ = [("n_chars", C.c_uint32), ("nr_joints", C.c_uint32), ("vert_first", C.c_void_p),
                ("vert_count", C.c_void_p), ("out_first", C.c_void_p), ("position", C.c_void_p),
                ("normal", C.c_void_p), ("joints", C.c_void_p), ("weights", C.c_void_p),
                ("joint_transforms", C.c_void_p), ("out_position", C.c_void_p), ("out_normal", C.c_void_p),
                ("out_w", C.c_void_p)]


SKIN_LODS = 4
SKIN_LOD_ALL = 0xFFFFFFFF
SKIN_NOT_DRAWN = 0xFF
SKINSEL_ENTITY_RANGE, SKINSEL_LOD_RANGE, SKINSEL_LIST_RANGE = 1, 2, 4


class SkinSelect(C.Structure):
    """clapgpu_skin_select (include/clapgpu.h): which characters clapgpu_skin_drawn skins, and which of their vertices."""
    _fields_ = [("n_planes", C.c_uint32), ("n_entities", C.c_uint32), ("planes", C.c_void_p * (1 + EXTRA_VIEWS_MAX)),
                ("entity", C.c_void_p), ("cur_lod", C.c_void_p), ("n_rows", C.c_uint32), ("n_lods", C.c_uint32),
                ("row", C.c_void_p), ("lod_first", C.c_void_p), ("lod_count", C.c_void_p), ("list", C.c_void_p),
                ("n_list", C.c_uint32), ("pad", C.c_uint32), ("skinned", C.c_void_p), ("chars", C.c_void_p),
                ("count", C.c_void_p), ("status", C.c_void_p), ("scratch", C.c_void_p)]


class World(C.Structure):
    _fields_ = [("gravity", C.c_double * 3), ("linear_damping", C.c_double),
                ("linear_damping_threshold_sq", C.c_double), ("adis_linear_threshold_sq", C.c_double),
                ("adis_angular_threshold_sq", C.c_double), ("adis_time", C.c_double),
                ("adis_steps", C.c_int32), ("pad", C.c_int32)]


class Bodies(C.Structure):
    """clapgpu_bodies (include/clapgpu.h)."""
    _fields_ = [("n", C.c_uint32), ("adis_average_samples", C.c_uint32), ("pos", C.c_void_p), ("quat", C.c_void_p),
                ("lvel", C.c_void_p), ("avel", C.c_void_p), ("mass", C.c_void_p), ("radius", C.c_void_p),
                ("yoffset", C.c_void_p), ("bflags", C.c_void_p), ("adis_steps_left", C.c_void_p),
                ("adis_time_left", C.c_void_p), ("body_entity", C.c_void_p),
                ("length", C.c_void_p), ("inertia", C.c_void_p), ("geom_offset_R", C.c_double * 12),
                ("aabb", C.c_void_p), ("axis", C.c_void_p), ("adis_samples", C.c_void_p), ("adis_counter", C.c_void_p),
                ("geom_records", C.c_void_p), ("facc", C.c_void_p)]


class Geoms(C.Structure):
    """clapgpu_geoms (include/clapgpu.h)."""
    _fields_ = [("n", C.c_uint32), ("pad", C.c_uint32), ("pos", C.c_void_p), ("axis", C.c_void_p),
                ("radius", C.c_void_p), ("length", C.c_void_p), ("kind", C.c_void_p), ("aabb", C.c_void_p),
                ("material", C.c_void_p), ("records", C.c_void_p)]


class TrimeshDesc(C.Structure):
    """clapgpu_trimesh_desc (include/clapgpu.h): device arrays of the static meshes."""
    _fields_ = [("n_meshes", C.c_uint32), ("n_statics", C.c_uint32), ("static_index", C.c_void_p), ("vx_first", C.c_void_p),
                ("tri_first", C.c_void_p), ("vx", C.c_void_p), ("idx", C.c_void_p), ("scale", C.c_void_p),
                ("pos", C.c_void_p), ("quat", C.c_void_p)]


POSE_SKIP_TRS, POSE_SKIP_JOINT_POS, POSE_JOINT_POS_MODEL = 1, 2, 4
BODY_DISABLED, BODY_AUTO_DISABLE, BODY_NO_GRAVITY, BODY_GYROSCOPIC, BODY_HAS_JOINT, BODY_KINEMATIC = 1, 2, 4, 8, 16, 32
GEOM_SPHERE, GEOM_CAPSULE, GEOM_BOX, GEOM_OTHER = 0, 1, 2, 3
CONTACT_DEEP = 0x80000000


def mesh_contact_scratch(static_capacity):
    """CLAPGPU_MESH_CONTACT_SCRATCH: uint32 words of scratch clapgpu_contacts_meshes takes."""
    return (int(static_capacity) + 63) // 64 + 1


def bodies_push_scratch_bytes(n):
    """clapgpu_bodies_push_scratch_bytes: bytes of device scratch clapgpu_bodies_push takes for n movers (needs a device)."""
    return int(lib().clapgpu_bodies_push_scratch_bytes(int(n)))


def bodies_islands_scratch_bytes(n):
    """clapgpu_bodies_islands_scratch_bytes: bytes of device scratch clapgpu_bodies_islands takes for n bodies."""
    return int(lib().clapgpu_bodies_islands_scratch_bytes(int(n)))


def bodies_solve_scratch_bytes(n, rows_capacity):
    """clapgpu_bodies_solve_scratch_bytes: bytes of device scratch clapgpu_bodies_solve takes (needs a device)."""
    return int(lib().clapgpu_bodies_solve_scratch_bytes(int(n), int(rows_capacity)))


class Slide(C.Structure):
    """clapgpu_slide (include/clapgpu.h): a batch of movers for clapgpu_characters_slide."""
    _fields_ = [("n", C.c_uint32), ("body", C.c_void_p), ("velocity", C.c_void_p), ("airborne", C.c_void_p),
                ("first_frac", C.c_void_p), ("push_hit", C.c_void_p), ("flags", C.c_void_p)]


class CharactersMove(C.Structure):
    """clapgpu_move (include/clapgpu.h): a batch of movers for clapgpu_characters_move."""
    _fields_ = [("n", C.c_uint32), ("body", C.c_void_p), ("ray_off", C.c_void_p), ("motion", C.c_void_p),
                ("state", C.c_void_p), ("jump", C.c_void_p), ("jump_params", C.c_void_p), ("velocity", C.c_void_p),
                ("normal", C.c_void_p), ("airborne", C.c_void_p), ("request", C.c_void_p), ("applied", C.c_void_p),
                ("collision", C.c_void_p), ("first_frac", C.c_void_p), ("push_hit", C.c_void_p), ("flags", C.c_void_p),
                ("entity", C.c_void_p), ("yaw_quat", C.c_void_p)]


CS_START, CS_WAKING, CS_IDLE, CS_MOVING, CS_JUMP_START, CS_JUMPING, CS_FALLING, CS_NONE = 0, 1, 2, 3, 4, 5, 6, 0xff


# character states and animation queues (include/clapgpu.h, "Character states and animation queues")
ANIQ_MAX = 4
ANI_END_NONE, ANI_END_IDLE, ANI_END_START_MOTION, ANI_END_ANY_TO_JUMP, ANI_END_HOST = 0, 1, 2, 3, 0xff
(ANI_IDLE, ANI_START_TO_IDLE, ANI_MOTION_STOP, ANI_JUMP_TO_IDLE, ANI_FALL_TO_IDLE, ANI_MOTION, ANI_MOTION_START,
 ANI_JUMP_TO_MOTION, ANI_IDLE_TO_JUMP, ANI_MOTION_TO_JUMP, ANI_JUMP, ANI_FALL, ANI_NAMES) = range(13)
# the names character.c pushes, in the order of the ANI_* slots (animation_by_name of each fills name_anim)
ANI_NAME_LIST = ("idle", "start_to_idle", "motion_stop", "jump_to_idle", "fall_to_idle", "motion", "motion_start",
                 "jump_to_motion", "idle_to_jump", "motion_to_jump", "jump", "fall")
ANIQ_ENDED, ANIQ_STARTED, ANIQ_ADVANCED, ANIQ_CB_IDLE, ANIQ_CB_START_MOTION, ANIQ_CB_ANY_TO_JUMP, ANIQ_HOST, ANIQ_OVERFLOW = (
    1, 2, 4, 8, 16, 32, 64, 128)
ANIQ_STATE_SHIFT = 8


class AniqEntry(C.Structure):
    """clapgpu_aniq_entry (include/clapgpu.h): one struct queued_animation."""
    _fields_ = [("animation", C.c_uint16), ("repeat", C.c_uint8), ("end", C.c_uint8), ("speed", C.c_float)]


class Aniq(C.Structure):
    """clapgpu_aniq (include/clapgpu.h): one animated model's character states and animation queues."""
    _fields_ = [("n", C.c_uint32), ("n_anims", C.c_uint32), ("name_anim", C.c_void_p), ("time_end", C.c_void_p),
                ("queue", C.c_void_p), ("len", C.c_void_p), ("cur", C.c_void_p), ("cleared", C.c_void_p),
                ("ani_time", C.c_void_p), ("state", C.c_void_p), ("airborne", C.c_void_p), ("velocity", C.c_void_p),
                ("ch_motion", C.c_void_p), ("jump_params", C.c_void_p), ("mover", C.c_void_p), ("pose_anim", C.c_void_p),
                ("frame_time", C.c_void_p), ("events", C.c_void_p)]


def characters_move_scratch_bytes(n_bodies, n):
    """clapgpu_characters_move_scratch_bytes: bytes of device scratch clapgpu_characters_move takes (needs a device)."""
    return int(lib().clapgpu_characters_move_scratch_bytes(int(n_bodies), int(n)))


def characters_order_scratch_bytes(n, pair_capacity):
    """clapgpu_characters_order_scratch_bytes: bytes of device scratch clapgpu_characters_order takes."""
    return int(lib().clapgpu_characters_order_scratch_bytes(int(n), int(pair_capacity)))


def characters_move_ordered_scratch_bytes(n_bodies, n, pair_capacity):
    """clapgpu_characters_move_ordered_scratch_bytes: bytes of device scratch the ordered move takes (needs a device)."""
    return int(lib().clapgpu_characters_move_ordered_scratch_bytes(int(n_bodies), int(n), int(pair_capacity)))


class Characters(C.Structure):
    """clapgpu_characters (include/clapgpu.h)."""
    _fields_ = [("n", C.c_uint32), ("limbo_height", C.c_float), ("entity", C.c_void_p), ("body", C.c_void_p),
                ("hist_pos", C.c_void_p), ("hist_head", C.c_void_p), ("hist_wrapped", C.c_void_p),
                ("airborne", C.c_void_p), ("moved", C.c_void_p)]


class Lights(C.Structure):
    """clapgpu_lights (include/clapgpu.h)."""
    _fields_ = [("nr_lights", C.c_uint32), ("pad", C.c_uint32), ("pos", C.c_void_p), ("color", C.c_void_p),
                ("attenuation", C.c_void_p), ("is_dir", C.c_void_p), ("active", C.c_void_p)]


SPOTS_INVALID = 1


class Spots(C.Structure):
    """clapgpu_spots (include/clapgpu.h): the lights that track an entity, their dir / cutoff slots and a status word."""
    _fields_ = [("n", C.c_uint32), ("pad", C.c_uint32), ("carrier_entity", C.c_void_p), ("carrier_light", C.c_void_p),
                ("carrier_off", C.c_void_p), ("carrier_view_slot", C.c_void_p), ("dir", C.c_void_p), ("cutoff", C.c_void_p),
                ("status", C.c_void_p)]


SPOTS_BYTES = 64                                             # CLAPGPU_SPOTS_BYTES
assert C.sizeof(Spots) == SPOTS_BYTES


DRAW_GROUP_SKIP_SHADOW = 1
DRAW_IS_CHARACTER = 1
DRAW_OUTLINE_EXCLUDE = 2
DRAW_PASS_SHADOW = 1
DRAW_PASS_HAS_ROPTS = 2
DRAW_SET_BLOOM_INTENSITY = 1
DRAW_SET_BLOOM_THRESHOLD = 2
DRAW_CAPPED = 1
DRAW_INVALID = 2
DRAW_RECORD_BYTES = 192


class DrawOrder(C.Structure):
    """clapgpu_draw_order (include/clapgpu.h): the walk of model.c:784 / :959 flattened; device pointers."""
    _fields_ = [("n_order", C.c_uint32), ("n_groups", C.c_uint32), ("order", C.c_void_p), ("group_start", C.c_void_p),
                ("group_flags", C.c_void_p)]


class DrawInputs(C.Structure):
    """clapgpu_draw_inputs: per-entity arrays, any of them NULL."""
    _fields_ = [("color", C.c_void_p), ("color_pt", C.c_void_p), ("bloom_intensity", C.c_void_p),
                ("bloom_threshold", C.c_void_p), ("draw_flags", C.c_void_p), ("character", C.c_void_p)]


class DrawPass(C.Structure):
    """clapgpu_draw_pass: host values of one render pass."""
    _fields_ = [("flags", C.c_uint32), ("bloom_intensity", C.c_float), ("bloom_threshold", C.c_float),
                ("mq_nr_characters", C.c_uint32), ("index_base", C.c_uint32)]


class DrawRecord(C.Structure):
    """clapgpu_draw_record: 192 bytes, three 64-byte lines."""
    _fields_ = [("mx", C.c_float * 16), ("inv_mx", C.c_float * 16), ("color", C.c_float * 4), ("bloom_intensity", C.c_float),
                ("bloom_threshold", C.c_float), ("edge_mode", C.c_uint32), ("color_pt", C.c_int32), ("entity", C.c_uint32),
                ("lod", C.c_int32), ("group", C.c_uint32), ("character", C.c_int32), ("flags", C.c_uint32),
                ("zero", C.c_uint32 * 3)]


assert C.sizeof(DrawRecord) == DRAW_RECORD_BYTES


class FrameDrawPass(C.Structure):
    """clapgpu_frame_draw_pass: one pass's outputs inside a frame."""
    _fields_ = [("pass", DrawPass), ("capacity", C.c_uint32), ("records", C.c_void_p), ("count", C.c_void_p),
                ("group_first", C.c_void_p), ("status", C.c_void_p)]


class FrameDraw(C.Structure):
    """clapgpu_frame_draw: the frame's draw records, the main pass and one block per further view."""
    _fields_ = [("order", C.POINTER(DrawOrder)), ("inputs", C.POINTER(DrawInputs)), ("main", FrameDrawPass),
                ("view", FrameDrawPass * EXTRA_VIEWS_MAX), ("scratch", C.c_void_p)]


class Solver(C.Structure):
    """clapgpu_solver (include/clapgpu.h): quickstep's iteration count, SOR factor and global CFM; wide_rows: the rows from
    which an island is solved by a workgroup, level by level (0: never)."""
    _fields_ = [("iterations", C.c_uint32), ("wide_rows", C.c_uint32), ("sor_w", C.c_double), ("cfm", C.c_double)]


class FrameDesc(C.Structure):
    """clapgpu_frame (include/clapgpu.h)."""
    _fields_ = [("entities", C.POINTER(Entities)), ("tile_row_start", C.c_void_p), ("n_tiles", C.c_uint32),
                ("level_start", C.c_void_p), ("n_levels", C.c_uint32), ("frustum", C.POINTER(Frustum)),
                ("bodies", C.POINTER(Bodies)), ("world", C.POINTER(World)), ("bp", C.c_void_p),
                ("pairs", C.c_void_p), ("pair_capacity", C.c_uint32), ("pair_total", C.c_void_p),
                ("static_pairs", C.c_void_p), ("static_pair_capacity", C.c_uint32), ("static_pair_total", C.c_void_p),
                ("body_geoms", C.POINTER(Geoms)), ("static_geoms", C.POINTER(Geoms)),
                ("contacts", C.c_void_p), ("static_contacts", C.c_void_p),
                ("contact_total", C.c_void_p), ("static_contact_total", C.c_void_p),
                ("n_body_links", C.c_uint32), ("link_body", C.c_void_p), ("link_entity", C.c_void_p),
                ("characters", C.POINTER(Characters)),
                ("lights", C.POINTER(Lights)),
                ("n_light_carriers", C.c_uint32), ("carrier_entity", C.c_void_p), ("carrier_light", C.c_void_p),
                ("carrier_offset", C.c_void_p),
                ("light_width", C.c_uint32), ("light_height", C.c_uint32), ("light_cell", C.c_uint32), ("light_tiles", C.c_void_p),
                ("view_mx", C.POINTER(C.c_float)), ("proj_mx", C.POINTER(C.c_float)),
                ("anim_clock", C.POINTER(AnimClock)), ("now_dev", C.c_void_p),
                ("skeleton", C.POINTER(Skeleton)), ("animations", C.POINTER(Animations)), ("pose", C.POINTER(PoseBatch)),
                ("skin", C.POINTER(SkinBatch)),
                ("particles", C.POINTER(Particles)),
                ("index_base", C.c_uint32), ("visible", C.c_void_p), ("visible_count", C.c_void_p), ("visible_scratch", C.c_void_p),
                ("cam_pos", C.c_float * 3), ("force_lod", C.c_void_p), ("cur_lod", C.c_void_p), ("draw_lod", C.c_void_p),
                ("flags", C.c_uint32),
                ("meshes", C.c_void_p), ("mesh_contacts", C.c_void_p), ("mesh_ref", C.c_void_p),
                ("mesh_contact_capacity", C.c_uint32), ("mesh_contact_total", C.c_void_p), ("mesh_capped", C.c_void_p),
                ("mesh_scratch", C.c_void_p),
                ("island_scratch", C.c_void_p), ("island", C.c_void_p), ("island_woken", C.c_void_p),
                ("solver", C.POINTER(Solver)), ("solve_scratch", C.c_void_p), ("solve_rows_capacity", C.c_uint32),
                ("solve_status", C.c_void_p),
                ("move", C.POINTER(CharactersMove)), ("move_dt_sec", C.c_double), ("move_scratch", C.c_void_p),
                ("aniq", C.POINTER(Aniq)), ("skin_select", C.POINTER(SkinSelect)),
                ("views_source", C.c_void_p), ("views_state", C.c_void_p),
                ("cascades", C.c_void_p), ("bv_result", C.c_void_p), ("bv_has_ctl", C.c_uint32), ("bv_ctl_entity", C.c_uint32),
                ("spots", C.POINTER(Spots)), ("view_visible", C.c_void_p * EXTRA_VIEWS_MAX),
                ("view_visible_count", C.c_void_p * EXTRA_VIEWS_MAX),
                ("draw", C.POINTER(FrameDraw)),
                ("camera", C.c_void_p), ("camera_bp", C.c_void_p)]


LIGHTS_MAX = 128

# every struct of include/clapgpu.h the binding mirrors: header name -> ctypes class (tests/test_cabi.py holds each to gcc's layout)
STRUCTS = {
    "clapgpu_frustum": Frustum, "clapgpu_bv_query": BvQuery, "clapgpu_views": Views, "clapgpu_entities": Entities,
    "clapgpu_particles": Particles, "clapgpu_anim_clock": AnimClock, "clapgpu_skeleton": Skeleton,
    "clapgpu_animations": Animations, "clapgpu_pose_batch": PoseBatch, "clapgpu_skin_batch": SkinBatch,
    "clapgpu_skin_select": SkinSelect,
    "clapgpu_world": World, "clapgpu_bodies": Bodies, "clapgpu_geoms": Geoms, "clapgpu_trimesh_desc": TrimeshDesc,
    "clapgpu_slide": Slide, "clapgpu_move": CharactersMove, "clapgpu_characters": Characters, "clapgpu_lights": Lights,
    "clapgpu_view_source": ViewSource, "clapgpu_views_source": ViewsSource, "clapgpu_view_state": ViewState,
    "clapgpu_views_state": ViewsState, "clapgpu_camera": Camera,
    "clapgpu_cascade_view": CascadeView, "clapgpu_cascades": Cascades,
    "clapgpu_spots": Spots, "clapgpu_draw_order": DrawOrder, "clapgpu_draw_inputs": DrawInputs, "clapgpu_draw_pass": DrawPass,
    "clapgpu_draw_record": DrawRecord, "clapgpu_frame_draw_pass": FrameDrawPass, "clapgpu_frame_draw": FrameDraw,
    "clapgpu_solver": Solver, "clapgpu_aniq_entry": AniqEntry, "clapgpu_aniq": Aniq, "clapgpu_frame": FrameDesc,
}


# every symbol include/clapgpu.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "clapgpu_device_count": (C.c_int, []),
    "clapgpu_init": (C.c_int, [C.c_int]),
    "clapgpu_last_error": (C.c_char_p, []),
    "clapgpu_test_fail_after": (None, [C.c_int]),
    "clapgpu_abi_version": (C.c_uint32, []),
    "clapgpu_malloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "clapgpu_free": (C.c_int, [C.c_void_p]),
    "clapgpu_host_malloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "clapgpu_host_free": (C.c_int, [C.c_void_p]),
    "clapgpu_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "clapgpu_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "clapgpu_memset": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]),
    "clapgpu_stream_sync": (C.c_int, [C.c_void_p]),
    "clapgpu_view_matrix": (None, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "clapgpu_perspective": (None, [C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_float)]),
    "clapgpu_frustum_calc": (None, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.POINTER(Frustum)]),
    "clapgpu_entities_update": (C.c_int, [C.c_void_p, C.POINTER(Entities), C.POINTER(C.c_uint32), C.c_uint32,
                                          C.c_uint32, C.POINTER(Frustum)]),
    "clapgpu_entities_update_level": (C.c_int, [C.c_void_p, C.POINTER(Entities), C.c_uint32, C.c_uint32,
                                                C.c_uint32, C.POINTER(Frustum)]),
    "clapgpu_entities_update_tiles": (C.c_int, [C.c_void_p, C.POINTER(Entities), C.c_void_p, C.c_uint32,
                                                C.c_uint32, C.POINTER(Frustum)]),
    "clapgpu_entities_lod": (C.c_int, [C.c_void_p, C.POINTER(Entities), C.c_void_p, C.c_void_p, C.c_uint32,
                                       C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_entities_cull": (C.c_int, [C.c_void_p, C.POINTER(Entities), C.POINTER(Frustum)]),
    "clapgpu_visible_scratch_bytes": (C.c_size_t, [C.c_uint32]),
    "clapgpu_visible_compact": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "clapgpu_animation_time": (C.c_int, [C.c_void_p, C.POINTER(AnimClock), C.c_double]),
    "clapgpu_animation_time_dev": (C.c_int, [C.c_void_p, C.POINTER(AnimClock), C.c_void_p]),
    "clapgpu_animations_packed_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "clapgpu_animations_pack": (C.c_int, [C.c_void_p, C.POINTER(Animations), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]),
    "clapgpu_joint_pos_world": (C.c_int, [C.c_void_p, C.POINTER(Skeleton), C.POINTER(PoseBatch)]),
    "clapgpu_pose_update": (C.c_int, [C.c_void_p, C.POINTER(Skeleton), C.POINTER(Animations), C.POINTER(PoseBatch)]),
    "clapgpu_skin": (C.c_int, [C.c_void_p, C.POINTER(SkinBatch)]),
    "clapgpu_skin_select_scratch_bytes": (C.c_size_t, [C.c_uint32]),
    "clapgpu_skin_drawn": (C.c_int, [C.c_void_p, C.POINTER(SkinBatch), C.POINTER(SkinSelect)]),
    "clapgpu_phys_step_schedule": (C.c_int, [C.POINTER(C.c_double), C.c_double]),
    "clapgpu_world_defaults": (None, [C.POINTER(World)]),
    "clapgpu_bodies_step": (C.c_int, [C.c_void_p, C.POINTER(Bodies), C.POINTER(World), C.c_double]),
    "clapgpu_phys_body_update": (C.c_int, [C.c_void_p, C.POINTER(Bodies), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "clapgpu_geom_offset_rotation": (None, [C.POINTER(C.c_double)]),
    "clapgpu_mass_sphere_total": (None, [C.c_double, C.c_double, C.POINTER(C.c_double)]),
    "clapgpu_mass_capsule_total": (None, [C.c_double, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    "clapgpu_capsule_geom": (None, [C.c_float, C.c_float, C.c_float, C.c_double, C.c_double, C.POINTER(C.c_float),
                                    C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "clapgpu_bodies_aabb": (C.c_int, [C.c_void_p, C.POINTER(Bodies)]),
    "clapgpu_bp_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_double, C.c_uint32, C.c_void_p]),
    "clapgpu_bp_create_levels": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_double, C.c_uint32, C.c_uint32, C.c_void_p]),
    "clapgpu_bp_levels": (C.c_uint32, [C.c_void_p]),
    "clapgpu_bp_cell_slot": (C.c_uint32, [C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_int32]),
    "clapgpu_bp_destroy": (None, [C.c_void_p]),
    "clapgpu_bp_collide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                     C.c_void_p, C.c_uint32, C.c_void_p]),
    "clapgpu_bp_status": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
    "clapgpu_bp_static_aabb": (C.c_void_p, [C.c_void_p]),
    "clapgpu_bp_statics_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "clapgpu_bp_statics_sizes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                           C.POINTER(C.c_uint32), C.POINTER(C.c_double)]),
    "clapgpu_bp_statics_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_contacts_geoms": (C.c_int, [C.c_void_p, C.POINTER(Geoms), C.POINTER(Geoms), C.c_void_p, C.c_void_p, C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_contacts_geoms_both": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Geoms), C.POINTER(Geoms), C.c_void_p, C.c_void_p,
                                              C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "clapgpu_sweep_capsules": (C.c_int, [C.c_void_p, C.POINTER(Geoms), C.POINTER(Geoms), C.c_void_p, C.c_uint32, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_bodies_rotate_from_entities": (C.c_int, [C.c_void_p, C.POINTER(Bodies), C.POINTER(Entities), C.c_uint32,
                                                      C.c_uint32, C.c_void_p, C.c_void_p]),
    "clapgpu_contacts_spheres": (C.c_int, [C.c_void_p, C.POINTER(Bodies), C.c_void_p, C.c_void_p, C.c_uint32,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_contacts_sphere_box": (C.c_int, [C.c_void_p, C.POINTER(Bodies), C.c_uint32, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_shard_tile_range": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                           C.POINTER(C.c_uint32)]),
    "clapgpu_bodies_step_prebin": (C.c_int, [C.c_void_p, C.POINTER(Bodies), C.POINTER(World), C.c_double, C.c_void_p]),
    "clapgpu_bp_invalidate": (C.c_int, [C.c_void_p, C.c_void_p]),
    "clapgpu_bp_index": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "clapgpu_bp_index_status": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
    "clapgpu_bp_leveled_index": (C.c_int, [C.c_void_p, C.c_int]),
    "clapgpu_ray_cast": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Geoms), C.POINTER(Geoms), C.c_void_p, C.c_uint32,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_bodies_ground_collide": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Bodies), C.POINTER(Geoms), C.c_void_p,
                                                C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_trimesh_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(TrimeshDesc)]),
    "clapgpu_trimesh_pose": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_trimesh_status": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "clapgpu_trimesh_destroy": (None, [C.c_void_p]),
    "clapgpu_trimesh_create_parts": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(TrimeshDesc)]),
    "clapgpu_trimesh_pose_meshes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_trimesh_parts_status": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
    "clapgpu_trimesh_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_contacts_meshes": (C.c_int, [C.c_void_p, C.POINTER(Geoms), C.POINTER(Geoms), C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "clapgpu_sweep_capsules_grid": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Bodies), C.POINTER(Geoms), C.c_void_p, C.c_uint32,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_characters_slide": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Bodies), C.POINTER(Geoms), C.c_void_p, C.c_double,
                                           C.POINTER(Slide), C.c_void_p]),
    "clapgpu_bodies_push_scratch_bytes": (C.c_size_t, [C.c_uint32]),
    "clapgpu_bodies_push": (C.c_int, [C.c_void_p, C.POINTER(Bodies), C.POINTER(World), C.c_uint32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_characters_move_scratch_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "clapgpu_characters_move": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Bodies), C.POINTER(World), C.POINTER(Geoms),
                                          C.c_void_p, C.POINTER(Entities), C.c_double, C.POINTER(CharactersMove), C.c_void_p]),
    "clapgpu_characters_state": (C.c_int, [C.c_void_p, C.POINTER(Aniq), C.POINTER(CharactersMove), C.c_double, C.c_void_p]),
    "clapgpu_animation_queue_time": (C.c_int, [C.c_void_p, C.POINTER(Aniq), C.c_double, C.c_void_p]),
    "clapgpu_characters_order_scratch_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "clapgpu_characters_order": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Bodies), C.POINTER(World), C.c_double,
                                           C.POINTER(CharactersMove), C.c_uint32, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_uint32), C.c_void_p]),
    "clapgpu_characters_move_ordered_scratch_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "clapgpu_characters_move_ordered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Bodies), C.POINTER(World),
                                                  C.POINTER(Geoms), C.c_void_p, C.POINTER(Entities), C.c_double,
                                                  C.POINTER(CharactersMove), C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32),
                                                  C.c_void_p]),
    "clapgpu_bodies_islands_scratch_bytes": (C.c_size_t, [C.c_uint32]),
    "clapgpu_bodies_islands": (C.c_int, [C.c_void_p, C.POINTER(Bodies), C.POINTER(World), C.c_double, C.c_void_p, C.c_void_p,
                                         C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_solver_defaults": (None, [C.POINTER(Solver)]),
    "clapgpu_bodies_solve_scratch_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "clapgpu_bodies_solve": (C.c_int, [C.c_void_p, C.POINTER(Bodies), C.POINTER(World), C.POINTER(Solver), C.c_double, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "clapgpu_visible_compact_lod": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_characters_update_clock": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]),
    "clapgpu_host_malloc_mapped": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_size_t]),
    "clapgpu_entities_apply_inputs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "clapgpu_entities_place": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "clapgpu_entities_export_rebuilt": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_entities_export_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_entities_update_tiles_hostio": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                                       C.c_void_p]),
    "clapgpu_wait_word": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "clapgpu_exchange_set_library": (None, [C.c_char_p]),
    "clapgpu_exchange_available": (C.c_int, []),
    "clapgpu_exchange_unique_id": (C.c_int, [C.c_void_p]),
    "clapgpu_exchange_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int]),
    "clapgpu_exchange_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p]),
    "clapgpu_exchange_destroy": (None, [C.c_void_p]),
    "clapgpu_exchange_visible": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "clapgpu_exchange_visible_ranges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_visible_compact_ranges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]),
    "clapgpu_visible_expand_ranges_host": (C.c_uint32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "clapgpu_shard_bases": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
    "clapgpu_mat4_invert": (None, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "clapgpu_mat4_from_quat": (None, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "clapgpu_frame_issue": (C.c_int, [C.c_void_p, C.POINTER(FrameDesc), C.c_double, C.c_uint32]),
    "clapgpu_particles_update": (C.c_int, [C.c_void_p, C.POINTER(Particles), C.POINTER(C.c_float)]),
    "clapgpu_characters_update": (C.c_int, [C.c_void_p, C.POINTER(Characters), C.POINTER(Entities),
                                            C.POINTER(Bodies)]),
    "clapgpu_light_grid_dims": (None, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_uint32)]),
    "clapgpu_light_grid_compute": (C.c_int, [C.c_void_p, C.POINTER(Lights), C.POINTER(C.c_float),
                                             C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "clapgpu_views_calc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "clapgpu_camera_calc": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Entities), C.c_void_p, C.c_void_p, C.POINTER(Geoms),
                                      C.POINTER(Geoms), C.c_void_p, C.c_void_p]),
    "clapgpu_camera_target": (None, [C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                     C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_float),
                                     C.POINTER(C.c_float)]),
    "clapgpu_camera_rays": (None, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float,
                                   C.POINTER(C.c_float), C.POINTER(C.c_double)]),
    "clapgpu_camera_decide": (C.c_int, [C.c_float, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "clapgpu_camera_update_host": (None, [C.POINTER(Camera), C.c_void_p, C.c_void_p]),
    "clapgpu_cascades_calc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Entities), C.c_void_p]),
    "clapgpu_cascades_calc_host": (None, [C.POINTER(Cascades), C.POINTER(ViewsSource), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                          C.c_float, C.c_int]),
    "clapgpu_cascades_near_backup": (C.c_float, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float]),
    "clapgpu_cascades_persp": (None, [C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_int, C.POINTER(C.c_float)]),
    "clapgpu_entities_bv_views": (C.c_int, [C.c_void_p, C.POINTER(Entities), C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                            C.c_void_p]),
    "clapgpu_entities_cull_views": (C.c_int, [C.c_void_p, C.POINTER(Entities), C.c_void_p]),
    "clapgpu_entities_lod_views": (C.c_int, [C.c_void_p, C.POINTER(Entities), C.c_void_p, C.c_void_p, C.c_uint32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_visible_compact_lod_views": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_light_grid_compute_views": (C.c_int, [C.c_void_p, C.POINTER(Lights), C.c_void_p, C.c_uint32, C.c_uint32,
                                                   C.c_uint32, C.c_void_p]),
    "clapgpu_particles_update_views": (C.c_int, [C.c_void_p, C.POINTER(Particles), C.c_void_p]),
    "clapgpu_lights_from_entities": (C.c_int, [C.c_void_p, C.POINTER(Entities), C.c_uint32, C.c_uint32, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.POINTER(Lights)]),
    "clapgpu_lights_update": (C.c_int, [C.c_void_p, C.POINTER(Entities), C.c_uint32, C.POINTER(Spots), C.POINTER(Lights),
                                        C.c_void_p]),
    "clapgpu_lights_update_host": (None, [C.POINTER(Entities), C.c_uint32, C.POINTER(Spots), C.POINTER(Lights), C.c_void_p]),
    "clapgpu_spot_persp": (None, [C.c_float, C.c_int, C.POINTER(C.c_float)]),
    "clapgpu_draw_records_scratch_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "clapgpu_draw_records": (C.c_int, [C.c_void_p, C.POINTER(Entities), C.c_void_p, C.c_void_p, C.POINTER(DrawOrder),
                                       C.POINTER(DrawInputs), C.POINTER(DrawPass), C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "clapgpu_draw_records_host": (None, [C.POINTER(Entities), C.c_void_p, C.c_void_p, C.POINTER(DrawOrder),
                                         C.POINTER(DrawInputs), C.POINTER(DrawPass), C.c_void_p, C.c_uint32, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
}

_lib = None


def build(verbose=False):
    """Compile every HIP source for gfx950 into clap_amd/lib/libclapgpu.so (needs hipcc, no GPU)."""
    subprocess.run(["make", "-C", CSRC] + ([] if verbose else ["-s"]), check=True)


def lib():
    """Load the library; raise loudly if it is missing or its ABI differs."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ClapGpuError(ERR_INIT_FAILED, "clap_amd",
                               f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)")
        # This harness shares device memory and streams with torch, and torch ships its own copy of the HIP / HSA runtime:
        # whichever copy is loaded first serves the whole process, and a second HSA runtime finds no device ("no HIP
        # device" from clapgpu_init).  Let torch load its copy before the library resolves libamdhip64.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)           # AttributeError if the .so does not export it
            fn.restype = res
            fn.argtypes = args
        got = L.clapgpu_abi_version()
        if got & 0x80000000 and os.environ.get("CLAPGPU_ALLOW_EXPERIMENT") == "1":
            got &= 0x7FFFFFFF                # an experiment build (csrc/common.h), asked for by name: A/B tools only
        if got != ABI_VERSION:
            raise ClapGpuError(ERR_INIT_FAILED, "clap_amd",
                               "libclapgpu ABI version mismatch; rebuild" if not got & 0x80000000 else
                               "libclapgpu is an EXPERIMENT build (-DCLAPGPU_EXPERIMENT: kernels compiled with parts "
                               "switched off); rebuild without EXTRA=, or set CLAPGPU_ALLOW_EXPERIMENT=1 for an A/B run")
        _lib = L
    return _lib


def check(rc, where):
    if rc != OK:
        detail = lib().clapgpu_last_error()
        raise ClapGpuError(rc, where, detail.decode() if detail else "")
