"""The hand-made scenes that tests/test_solve_lcp.py (solveref against lcpref) and tests/test_solve_lcp_gpu.py (the
kernels against lcpref) share: bodies and contact lists as plain arrays, with fixed seeds.  The solve does not care
whether the geometry is plausible: contact points lie off the line of centres, normals point anywhere.  Imports neither
reference."""
import numpy as np

H = 1.0 / 120.0
INF = float("inf")
NO_GRAVITY, KINEMATIC = 4, 32
CONTACT_BOUNCE = 0x004
C2 = np.dtype([("pos", np.float64, 3), ("normal", np.float64, 3), ("depth", np.float64), ("mu", np.float64),
               ("bounce", np.float64), ("bounce_vel", np.float64), ("soft_erp", np.float64), ("soft_cfm", np.float64),
               ("mode", np.uint32), ("nc", np.uint32), ("pos2", np.float64, 3), ("normal2", np.float64, 3),
               ("depth2", np.float64)])                                     # clapgpu_contact2, as tests/meshscene.py has it

# the seeds: the first of 1, 2, ... whose cond(A) is admissible (<= 1e8) and whose scene holds what the tests ask of it.
# cond(A): scene F 284, scene S 53.2, scene C 681 (seeds 2 .. 6 of scene F: 1.9e3, 538, 87, 1.1e3, 798)
SEED_F, SEED_C = 1, 1


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def record(R, anchor, mu, bounce, second, steep):
    """one record at `anchor` + an offset; steep: which dPlaneSpace branch its first normal takes (|n_z| > 1/sqrt 2)"""
    r = np.zeros(1, C2)[0]

    def normal(want_steep):
        while True:
            n = unit(R.normal(size=3))
            if (abs(n[2]) > 0.75) == want_steep and abs(abs(n[2]) - np.sqrt(0.5)) > 0.04:
                return n
    r["pos"], r["normal"], r["depth"] = anchor + R.uniform(-0.4, 0.4, 3), normal(steep), R.uniform(0.0, 0.05)
    r["mu"], r["bounce"], r["bounce_vel"], r["soft_erp"], r["soft_cfm"] = mu, bounce, 0.0, 0.05, 0.01
    r["mode"] = 0x018 | (CONTACT_BOUNCE if bounce > 0 else 0)               # SoftERP | SoftCFM [| Bounce]
    r["nc"] = 1
    if second:
        r["pos2"], r["normal2"], r["depth2"] = anchor + R.uniform(-0.4, 0.4, 3), normal(not steep), R.uniform(0.0, 0.05)
        r["nc"] = 2
    return r


def bodies(R, n):
    return dict(pos=R.uniform(-1, 1, (n, 3)), quat=unit(R.normal(size=(n, 4))), lvel=R.normal(size=(n, 3)),
                avel=R.normal(size=(n, 3)), mass=R.uniform(0.5, 3.0, n), inertia=R.uniform(0.05, 1.0, (n, 3)),
                facc=R.normal(size=(n, 3)), bflags=np.zeros(n, np.uint32))


C_CFM = 1e-3
F_PAIRS = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (0, 7), (2, 5), (1, 4), (3, 6), (0, 3)]
F_MU = [0.5, INF, 0.0, 0.0, 0.0, INF, 0.0, 0.0, 0.0, 0.0, 0.5, 0.0]
F_BOUNCE = [0.5, 0.0, 0.5, 0.0, 0.5, 0.5, 0.0, 0.5, 0.0, 0.5, 0.5, 0.0]
F_STATIC = [(2, 0.0, 0.5), (4, 0.5, 0.0), (1, INF, 0.0), (5, 0.0, 0.5)]    # (body, mu, bounce)


def scene_free(seed=SEED_F, inertia=True, closed=False):
    """Scene F: 8 rotated anisotropic bodies (6: NO_GRAVITY, 7: KINEMATIC and moving), 12 body records -- every third with
    a second contact -- and 4 static records: 34 rows on 36 freedoms.  inertia False: scene S, whose 21 freedoms are fewer
    than its rows, so that it takes the solver cfm of scene C (see there).  closed: body-body only, no kinematic body, no
    NO_GRAVITY flag -- a system whose momentum the solve cannot change."""
    R = rng(seed)
    st = bodies(R, 8)
    if not closed:
        st["bflags"][6], st["bflags"][7] = NO_GRAVITY, KINEMATIC
    recs = [record(R, (st["pos"][i] + st["pos"][j]) / 2, F_MU[k], F_BOUNCE[k], k % 3 == 0, k % 2 == 0)
            for k, (i, j) in enumerate(F_PAIRS)]
    srecs = [record(R, st["pos"][i], mu, bounce, False, k % 2 == 1) for k, (i, mu, bounce) in enumerate(F_STATIC)]
    if not inertia:
        st["inertia"] = None
    out = dict(st=st, body=(np.array(F_PAIRS, np.uint32), np.array(recs, C2)), cfm=1e-10 if inertia else C_CFM)
    if not closed:
        out["static"] = (np.array([(i, 0) for i, _mu, _b in F_STATIC], np.uint32), np.array(srecs, C2))
    return out


C_PAIRS = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (2, 3)]


def scene_chain(seed=SEED_C):
    """Scene C: a chain of 6 bodies, each touching the next and the next but one, (0, 1) listed a second time at another
    point; every record carries two contacts with friction (0.5 and inf in turn) and a static record holds body 0:
    12 records, 72 rows, one island, at least the default wide_rows (64).  More rows than the bodies have freedoms (36),
    so J invM J^T is singular and cond(A) is set by the friction rows' cfm / h: the solver's cfm is C_CFM here (a field of
    clapgpu_solver), which keeps the scene admissible."""
    R = rng(seed)
    st = bodies(R, 6)
    st["pos"][:, 0] = 0.8 * np.arange(6)
    recs = [record(R, (st["pos"][i] + st["pos"][j]) / 2, (0.5, INF)[k % 2], 0.0, True, k % 2 == 0)
            for k, (i, j) in enumerate(C_PAIRS)]
    srec = record(R, st["pos"][0], 0.5, 0.0, True, False)
    return dict(st=st, body=(np.array(C_PAIRS, np.uint32), np.array(recs, C2)),
                static=(np.array([(0, 0)], np.uint32), np.array([srec], C2)), cfm=C_CFM)


# ------------------------------------------------------------------------------------------------- the stack
K_STACK, R_STACK = 8, 0.5
STACK_MASS = np.linspace(1.0, 2.0, K_STACK)
FLOOR = np.array([[-4.0, 4.0, -1.0, 0.0, -4.0, 4.0]])                      # tests/test_solve.py's floor: top face at y = 0
SOFT_ERP, SOFT_CFM, G = 0.05, 0.01, 9.8


def stack_positions():
    return np.stack([np.zeros(K_STACK), R_STACK + 2 * R_STACK * np.arange(K_STACK), np.zeros(K_STACK)], 1)


def stack_depths_at_rest():
    """contact i (0: the floor, i: between sphere i - 1 and sphere i) carries the spheres from i up"""
    load = G * np.cumsum(STACK_MASS[::-1])[::-1]
    return SOFT_CFM * load * H / SOFT_ERP


def stack_depths(pos):
    y = np.asarray(pos)[:, 1]
    return np.concatenate([[R_STACK - y[0]], 2 * R_STACK - np.diff(y)])
