"""phys_body_push over a slide batch (character.c:219-221, physics.c:677-693) and the step rule of a body with a force
accumulator (ODE 0.16 quickstep without constraint rows), restated in numpy: float32 where the reference uses float,
float64 elsewhere, every operation in the order the reference writes it.  What clapgpu_bodies_push and the force path of
clapgpu_bodies_step are compared with, bit for bit.  Nothing here imports the device code.

ODE is absent from the reference: like the rest of the rigid-body block this is PARITY UNPINNED."""
import numpy as np

f32, f64 = np.float32, np.float64

DISABLED, AUTO_DISABLE, NO_GRAVITY, GYROSCOPIC, HAS_JOINT, KINEMATIC = 1, 2, 4, 8, 16, 32

WORLD = dict(gravity=(0.0, -9.8, 0.0), linear_damping=0.001, linear_damping_threshold_sq=0.01 * 0.01,
             adis_linear_threshold_sq=0.05 * 0.05, adis_angular_threshold_sq=0.05 * 0.05, adis_time=0.0, adis_steps=30)


# ------------------------------------------------------------------------------------------------- the push
def force_of(mass, pusher, velocity, k):
    """vec3_scale(force, push_velocity, push_mass): float32 product; push_mass = (float)dMass.mass"""
    m = f32(f64(mass[pusher[k]]))
    return np.array([f32(m * f32(velocity[k][j])) for j in range(3)], f32)


def push(st, mass, pusher, velocity, push_hit, flags=None, world=WORLD, reverse=False):
    """The phys_body_push calls of a batch in the reference's order: mover 0's slots 0..5, then mover 1's, ...
    st: dict with facc [nb, 3] float64, bflags, adis_steps_left, adis_time_left -- changed in place.
    reverse: the same pushes in the opposite order (what the sum must NOT be).  Returns pushed [nb] uint32."""
    nb = len(mass)
    facc = st["facc"]
    pushed = np.zeros(nb, np.uint32)
    push_hit = np.asarray(push_hit, np.int64).reshape(-1, 6)
    slots = [(k, q) for k in range(len(pusher)) for q in range(6)]
    for k, q in (reversed(slots) if reverse else slots):
        if int(pusher[k]) >= nb or (flags is not None and int(flags[k]) != 0):
            continue
        h = int(push_hit[k, q])
        if h < 0 or h >= nb:
            continue
        force = force_of(mass, pusher, velocity, k)
        for j in range(3):
            facc[h, j] = f64(facc[h, j]) + f64(force[j])                  # dBodyAddForce
        st["bflags"][h] &= ~np.uint32(DISABLED)                          # dBodyEnable
        st["adis_steps_left"][h] = world["adis_steps"]
        st["adis_time_left"][h] = world["adis_time"]
        pushed[h] += 1
    return pushed


def push_state(b, facc=None):
    """the part of a body set the push touches, copied"""
    n = int(b["n"])
    return dict(facc=np.zeros((n, 3)) if facc is None else np.array(facc, f64),
                bflags=np.array(b["bflags"], np.uint32), adis_steps_left=np.array(b["adis_steps_left"], np.int32),
                adis_time_left=np.array(b["adis_time_left"], f64))


# ------------------------------------------------------------------------------------------------- the step
def _q_to_R(q):
    """dQtoR on columns q[0..3]: R as a list of 12"""
    qq1, qq2, qq3 = 2 * q[1] * q[1], 2 * q[2] * q[2], 2 * q[3] * q[3]
    z = np.zeros_like(q[0])
    return [1 - qq2 - qq3, 2 * (q[1] * q[2] - q[0] * q[3]), 2 * (q[1] * q[3] + q[0] * q[2]), z,
            2 * (q[1] * q[2] + q[0] * q[3]), 1 - qq1 - qq3, 2 * (q[2] * q[3] - q[0] * q[1]), z,
            2 * (q[1] * q[3] - q[0] * q[2]), 2 * (q[2] * q[3] + q[0] * q[1]), 1 - qq1 - qq2, z]


def _world_tensor(R, d):
    """R diag(d) R^T as quickstep builds it: tmp = D R^T, W = R tmp"""
    tmp = [None] * 12
    for i in range(3):
        for j in range(3):
            tmp[4 * i + j] = d[i] * R[4 * j + i]
    W = [None] * 12
    for i in range(3):
        for j in range(3):
            W[4 * i + j] = R[4 * i] * tmp[j] + R[4 * i + 1] * tmp[4 + j] + R[4 * i + 2] * tmp[8 + j]
        W[4 * i + 3] = np.zeros_like(R[0])
    return W


def _mul331(M, v):
    return [M[4 * i] * v[0] + M[4 * i + 1] * v[1] + M[4 * i + 2] * v[2] for i in range(3)]


def step_forces(b, st, h, world=WORLD):
    """One dWorldQuickStep(h) of bodies without constraint rows, with a force accumulator, on every body at once.
    b: mass [n], inertia [n, 3] (optional); st: pos, quat (w, x, y, z), lvel, avel, bflags, adis_steps_left,
    adis_time_left and facc [n, 3] -- changed in place.  An enabled body:
        f = facc + (NO_GRAVITY ? 0 : m g);  lvel += (h * invMass) * f,  invMass = 1 / m, 0 for KINEMATIC
        KINEMATIC: the world inverse inertia is all zeros, the product with the torque is still formed
        pose, damping, auto-disable as without forces;  facc = 0
    A DISABLED body (on entry, or put to sleep by this step) keeps its accumulator.  Averaged auto-disable samples
    (adis_average_samples > 1) are not restated.  Returns the mask of the bodies that were stepped."""
    assert int(b.get("adis_average_samples", 1)) == 1
    with np.errstate(all="ignore"):
        return _step_forces(b, st, f64(h), world)


def _step_forces(b, st, h, w):
    fl = st["bflags"].astype(np.uint32)
    n = len(fl)
    enabled = (fl & DISABLED) == 0
    v = [st["lvel"][:, a].copy() for a in range(3)]
    om = [st["avel"][:, a].copy() for a in range(3)]
    # dInternalHandleAutoDisabling: enabled bodies with the flag that hold a joint; the instantaneous velocity
    ad = enabled & ((fl & AUTO_DISABLE) != 0) & ((fl & HAS_JOINT) != 0)
    lin2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    ang2 = om[0] * om[0] + om[1] * om[1] + om[2] * om[2]
    idle = ~(lin2 > w["adis_linear_threshold_sq"]) & ~(ang2 > w["adis_angular_threshold_sq"])
    sl, tl = st["adis_steps_left"].copy(), st["adis_time_left"].copy()
    sl = np.where(ad, np.where(idle, sl - 1, np.int32(w["adis_steps"])), sl).astype(np.int32)
    tl = np.where(ad, np.where(idle, tl - h, f64(w["adis_time"])), tl)
    st["adis_steps_left"][:], st["adis_time_left"][:] = sl, tl
    sleep = ad & (sl <= 0) & (tl <= 0)
    st["bflags"][sleep] = (fl[sleep] | DISABLED) & ~np.uint32(HAS_JOINT)
    st["lvel"][sleep] = 0
    st["avel"][sleep] = 0
    s = enabled & ~sleep                                                   # the bodies the step steps
    st["bflags"][s] = fl[s] & ~np.uint32(HAS_JOINT)                      # dJointGroupEmpty after the step
    if not s.any():
        return s
    fl = fl[s]
    v, om = [x[s] for x in v], [x[s] for x in om]
    q = [st["quat"][s, a].copy() for a in range(4)]
    kin = (fl & KINEMATIC) != 0
    zero = np.zeros(len(fl))
    tacc = [zero.copy() for _ in range(3)]
    have_inertia = "inertia" in b and b["inertia"] is not None
    if have_inertia:
        Ib = [np.asarray(b["inertia"], f64)[s, a] for a in range(3)]
        invIb = [1.0 / x for x in Ib]
        R = _q_to_R(q)
        invIw = _world_tensor(R, invIb)
        invIw = [np.where(kin, 0.0, x) for x in invIw]
        gy = (fl & GYROSCOPIC) != 0                                        # implicit gyroscopic torque, quickstep stage 0
        Iw = _world_tensor(R, Ib)
        L = _mul331(Iw, om)
        It = [zero.copy() for _ in range(12)]
        It[1], It[2], It[4], It[6], It[8], It[9] = L[2], -L[1], -L[2], L[0], L[1], -L[0]   # dSetCrossMatrixMinus
        It = [It[k] * h + Iw[k] for k in range(12)]
        rh = 1.0 / h
        L = [x * rh for x in L]
        det = It[0] * (It[5] * It[10] - It[9] * It[6]) - It[1] * (It[4] * It[10] - It[8] * It[6]) + \
            It[2] * (It[4] * It[9] - It[8] * It[5])
        ok = det != 0
        r = 1.0 / det
        inv = [None] * 12                                                 # dInvertMatrix3
        inv[0] = (It[5] * It[10] - It[6] * It[9]) * r
        inv[1] = (It[9] * It[2] - It[1] * It[10]) * r
        inv[2] = (It[1] * It[6] - It[5] * It[2]) * r
        inv[4] = (It[6] * It[8] - It[4] * It[10]) * r
        inv[5] = (It[0] * It[10] - It[8] * It[2]) * r
        inv[6] = (It[4] * It[2] - It[0] * It[6]) * r
        inv[8] = (It[4] * It[9] - It[8] * It[5]) * r
        inv[9] = (It[8] * It[1] - It[0] * It[9]) * r
        inv[10] = (It[0] * It[5] - It[1] * It[4]) * r
        T = [None] * 12
        for rr in range(3):
            for c in range(3):
                T[4 * rr + c] = Iw[4 * rr] * inv[c] + Iw[4 * rr + 1] * inv[4 + c] + Iw[4 * rr + 2] * inv[8 + c]
            T[4 * rr + 3] = zero
        T[0], T[5], T[10] = T[0] - 1, T[5] - 1, T[10] - 1
        tau0 = _mul331(T, L)
        tacc = [np.where(gy & ok, tacc[a] + tau0[a], tacc[a]) for a in range(3)]
    m = np.asarray(b["mass"], f64)[s]
    k = h * np.where(kin, 0.0, 1.0 / m)
    grav = (fl & NO_GRAVITY) == 0
    facc = st["facc"]
    for j in range(3):
        f = facc[s, j] + np.where(grav, m * f64(w["gravity"][j]), 0.0)     # facc += m g
        v[j] = v[j] + k * f
    facc[s] = 0
    if have_inertia:
        tacc = [x * h for x in tacc]
        d = _mul331(invIw, tacc)
        om = [om[a] + d[a] for a in range(3)]
        for a in range(3):
            st["avel"][s, a] = om[a]
    for a in range(3):                                                     # dxStepBody
        st["pos"][s, a] = st["pos"][s, a] + h * v[a]
    d0 = 0.5 * (-om[0] * q[1] - om[1] * q[2] - om[2] * q[3])               # dWtoDQ
    d1 = 0.5 * (om[0] * q[0] + om[1] * q[3] - om[2] * q[2])
    d2 = 0.5 * (-om[0] * q[3] + om[1] * q[0] + om[2] * q[1])
    d3 = 0.5 * (om[0] * q[2] - om[1] * q[1] + om[2] * q[0])
    q = [q[0] + h * d0, q[1] + h * d1, q[2] + h * d2, q[3] + h * d3]
    l = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]              # dNormalize4
    pos_l = l > 0
    li = 1.0 / np.sqrt(l)
    ident = [1.0, 0.0, 0.0, 0.0]
    for a in range(4):
        st["quat"][s, a] = np.where(pos_l, q[a] * li, ident[a])
    if w["linear_damping"] != 0.0:
        speed2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
        damp = speed2 > w["linear_damping_threshold_sq"]
        sc = f64(1) - f64(w["linear_damping"])
        v = [np.where(damp, x * sc, x) for x in v]
    for a in range(3):
        st["lvel"][s, a] = v[a]
    return s


def step_state(b, facc=None):
    """a mutable copy of the dynamic state of a synth body dict, with an accumulator"""
    st = {k: np.ascontiguousarray(b[k]).copy() for k in ("pos", "quat", "lvel", "avel", "bflags", "adis_steps_left",
                                                           "adis_time_left")}
    st["bflags"] = st["bflags"].astype(np.uint32)
    st["facc"] = np.zeros((int(b["n"]), 3)) if facc is None else np.array(facc, f64)
    return st


# ------------------------------------------------------------------------------------------------- a crowd
def crowd(n_movers=16384, n_targets=96, seed=41, n_bodies=None):
    """Many movers packed around few bodies: the targets stand on a grid 4 apart, every mover stands within 3 of one of
    them and pushes, over its six slots, the targets nearer than 3.2 (nearest first, at most three, some slots left
    empty) -- what a slide of that crowd would report, without the sweeps.  Bodies 0 .. n_targets - 1 are the targets,
    the movers follow; their speeds span twelve decades.  Returns (mass [nb], pusher [n], velocity [n, 3] float32, push_hit [n, 6] int32)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    side = int(np.ceil(np.sqrt(n_targets)))
    tpos = np.stack([(np.arange(n_targets) % side) * 4.0, (np.arange(n_targets) // side) * 4.0], 1)
    home = rng.integers(0, n_targets, n_movers)
    ang, rad = rng.uniform(0, 2 * np.pi, n_movers), rng.uniform(0.5, 3.0, n_movers)
    mpos = tpos[home] + np.stack([np.cos(ang), np.sin(ang)], 1) * rad[:, None]
    d = np.linalg.norm(mpos[:, None, :] - tpos[None, :, :], axis=2)
    order = np.argsort(d, axis=1, kind="stable")[:, :3]
    push_hit = np.full((n_movers, 6), -1, np.int32)
    slot = np.stack([rng.permutation(6)[:3] for _ in range(n_movers)])
    for c in range(3):
        near = d[np.arange(n_movers), order[:, c]] < 3.2
        push_hit[np.flatnonzero(near), np.sort(slot, 1)[near, c]] = order[near, c]
    nb = int(n_bodies or n_targets + n_movers)
    mass = rng.uniform(0.5, 90.0, nb)
    pusher = (n_targets + np.arange(n_movers)).astype(np.uint32)
    # a float force holds 24 bits: sums of forces of one magnitude are exact in fp64 and every order gives the same bits.
    # Speeds over twelve decades make the sums round, so that the order shows
    velocity = (rng.normal(0, 6.0, (n_movers, 3)) * 10.0 ** rng.uniform(-10, 2, (n_movers, 1))).astype(np.float32)
    return mass, pusher, velocity, push_hit
