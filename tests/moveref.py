"""character_move (character.c:450-537) between its ground ray and its character_apply_velocity call, restated in numpy
float32 / float64 scalars from the reference's text: what clapgpu_characters_move's k_move_decide is compared with.
Nothing here imports the device code.  The rule (include/clapgpu.h has the same, INTEGRATION.md the host's half):

  ray flagged INVALID or UNRESOLVED   the mover ends: velocity and airborne kept, request NONE, applied 0
  airborne = !grounded_out            :454
  state == JUMPING and velocity[1] > 0   airborne = 1 (:464)
  airborne      raw dt_sec > 1e-6: velocity[1] += gravity[1] * dt_sec (float += float * double, :481) and
                character_apply_velocity runs; request FALLING either way (:486)
  jump          (ch->jump && ch->can_jump; airborne is 0): velocity = (dx * jump_forward, jump_upward, dz * jump_forward),
                request JUMP_START, airborne = 1 out of MOVING (character_set_state, :388); no character_apply_velocity
  motion != 0   vec3_len(normal) > 0: newz = (1, 0, 0) x normal, newx = normal x newz, both normalised,
                velocity = newx * (dx * coef) + newz * (dz * coef), coef 1 in MOVING else 0.3f (:504-527); request MOVING;
                character_apply_velocity runs unless state < IDLE (character_set_state returns early, :319-326)
  else          request IDLE
"""
import numpy as np

f32 = np.float32
CS_START, CS_WAKING, CS_IDLE, CS_MOVING, CS_JUMP_START, CS_JUMPING, CS_FALLING, CS_NONE = 0, 1, 2, 3, 4, 5, 6, 0xff
RAY_INVALID, RAY_UNRESOLVED, RAY_MOVED_TARGET = 1, 2, 4


def vec3_len(v):
    """linmath.h:40-51: p = 0; p += v[i] * v[i]; sqrtf(p)"""
    p = f32(0.0)
    for i in range(3):
        p = f32(p + f32(f32(v[i]) * f32(v[i])))
    return np.sqrt(p, dtype=f32)


def vec3_mul_cross(a, b):
    """linmath.h:250-255"""
    a, b = [f32(x) for x in a], [f32(x) for x in b]
    return [f32(f32(a[1] * b[2]) - f32(a[2] * b[1])),
            f32(f32(a[2] * b[0]) - f32(a[0] * b[2])),
            f32(f32(a[0] * b[1]) - f32(a[1] * b[0]))]


def vec3_norm(v):
    """linmath.h:58-62: float k = 1.0 / vec3_len(v); r[i] = v[i] * k"""
    k = f32(np.float64(1.0) / np.float64(vec3_len(v)))
    return [f32(f32(x) * k) for x in v]


def character_move_decide_one(ray_flags, grounded_out, state, jump, motion, jump_params, velocity, normal, airborne,
                              gravity_y, dt_sec):
    """One character.  motion (dx, dz); gravity_y: phys_body_get_gravity's float; dt_sec: the raw frame delta.
    Returns (velocity[3] float32, airborne, request, applied)."""
    v = [f32(x) for x in velocity]
    if ray_flags & (RAY_INVALID | RAY_UNRESOLVED):
        return np.array(v, f32), int(airborne), CS_NONE, 0
    air = not grounded_out                                                # :454
    if state == CS_JUMPING and v[1] > 0:                                  # :464
        air = True
    if air:                                                               # :467-488
        applied = 0
        if float(dt_sec) > 1e-6:
            v[1] = f32(np.float64(v[1]) + np.float64(f32(gravity_y)) * np.float64(dt_sec))
            applied = 1
        return np.array(v, f32), 1, CS_FALLING, applied
    dx, dz = f32(motion[0]), f32(motion[1])
    if jump:                                                              # :501, character_jump
        fwd, up = f32(jump_params[0]), f32(jump_params[1])
        v = [f32(dx * fwd), up, f32(dz * fwd)]
        return np.array(v, f32), int(state == CS_MOVING), CS_JUMP_START, 0
    with np.errstate(all="ignore"):
        if vec3_len([dx, f32(0.0), dz]) != 0:                             # :504 (a NaN length is not 0)
            if np.float64(vec3_len(normal)) > 0.0:                        # :509
                newz = vec3_mul_cross([1.0, 0.0, 0.0], normal)
                newx = vec3_mul_cross(normal, newz)
                newx, newz = vec3_norm(newx), vec3_norm(newz)
                coef = f32(1.0) if state == CS_MOVING else f32(0.3)
                sx, sz = f32(dx * coef), f32(dz * coef)
                v = [f32(f32(newx[i] * sx) + f32(newz[i] * sz)) for i in range(3)]      # vec3_add_scaled, :526
            return np.array(v, f32), 0, CS_MOVING, int(state >= CS_IDLE)
    return np.array(v, f32), 0, CS_IDLE, 0


def character_move_decide(ray_flags, grounded_out, state, jump, motion, jump_params, velocity, normal, airborne, gravity_y,
                          dt_sec):
    """The batch: arrays [n] / [n, 2] / [n, 3].  Returns dict(velocity [n, 3] float32, airborne, request, applied: uint8 [n])."""
    n = len(state)
    out = dict(velocity=np.zeros((n, 3), f32), airborne=np.zeros(n, np.uint8), request=np.zeros(n, np.uint8),
               applied=np.zeros(n, np.uint8))
    with np.errstate(all="ignore"):
        for k in range(n):
            v, a, r, ap = character_move_decide_one(int(ray_flags[k]), bool(grounded_out[k]), int(state[k]), bool(jump[k]),
                                                    motion[k], jump_params[k], velocity[k], normal[k], int(airborne[k]),
                                                    gravity_y, dt_sec)
            out["velocity"][k], out["airborne"][k], out["request"][k], out["applied"][k] = v, a, r, ap
    return out
