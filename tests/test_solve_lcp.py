"""CPU: tests/solveref.py -- the restatement the device is held to bit for bit -- against tests/lcpref.py, the dense boxed
LCP of the same rule, and against conservation of momentum and a closed-form resting stack.  Bit equality with a
restatement cannot tell a right rule from a wrong one; these can, and test_mutants shows that they do.

The bounds.  A converged lambda is compared with lambda* at K eps cond(A) |lambda*|_inf (K = 64, the chain constant of
tests/test_physics_geometry.py), the velocities at that times |h invM J^T|_inf, the complementarity residual at
K eps cond(A) max|b|; cond(A) <= 1e8 is a condition on the scene, asserted.  Momentum needs no convergence: every row's
impulse pair is equal and opposite at every sweep."""
import inspect
import textwrap
import types

import numpy as np
import pytest

import geomref as gr
import lcpref as lp
import lcpscenes as sc
import pushref as pr
import solveref as sr

H = sc.H
EPS = lp.EPS
K = 64                                                                      # tests/test_physics_geometry.py's chain constant
SOR_W = 1.3
# N: the sweeps of a "converged" solve: the smallest power of two at which solveref meets all three bounds, doubled; one N
# for every scene, so the largest any of them needs.  Measured (x86-64, numpy float64):
#   scene F (seed 1): 34 rows, cond(A) 284;  at 16 sweeps |lambda - lambda*| 1.1e-5, at 32: 1.5e-12 <= 3.9e-10   -> 32
#   scene S (seed 1): 34 rows, cond(A) 53.2; at 16: 1.5e-5, at 32: 6.4e-12 <= 2.2e-10                             -> 32
#   scene C (seed 1): 72 rows, cond(A) 681;  at 128: 6.7e-5, at 256: 7.8e-11 <= 1.1e-9                            -> 256
# At N = 512 the achieved distances are (lambda, velocity, kkt; each with its bound):
#   F: 3.8e-14 (3.9e-10), 4.3e-16 (3.0e-11), 2.3e-13 (2.2e-9)      S: 5.1e-14 (2.2e-10), 6.4e-16 (1.1e-11), 1.2e-13 (4.2e-10)
#   C: 3.4e-13 (1.1e-9),  5.0e-15 (1.1e-9),  9.6e-13 (5.0e-9)
# Momentum of the closed scene F: drift 8.6e-16 after 1 sweep (bound 1.7e-13), 1.2e-15 after 20 (1.3e-13); without inertia
# (P alone) 2.4e-16 and 5.2e-16.  One sweep against first_sweep: 8.5e-17 relative (bound 64 eps = 1.4e-14).  The stack ends
# 2.3e-9 (relative) from its closed form, max |v| 1.3e-9.  The device gives these same figures on both of its paths.
N = 512
COND_MAX = 1e8


def solver(scene, iterations):
    return dict(iterations=iterations, sor_w=SOR_W, cfm=scene["cfm"])


def lists(scene):
    return {k: scene[k] for k in ("static", "body") if k in scene}


def system(scene):
    return lp.System(scene["st"], H, cfm=scene["cfm"], **lists(scene))


def restated(scene, iterations, module=sr):
    return module.solve(scene["st"], np.zeros(len(scene["st"]["mass"]), np.uint32), H, solver=solver(scene, iterations),
                        **lists(scene))


class Truth:
    """a scene's dense system and its lambda*, made once"""

    def __init__(self, scene):
        self.scene, self.S = scene, system(scene)
        S = self.S
        self.lam, self.residual = lp.solve_box(S.A, S.b, S.lo, S.hi)
        self.bmax = float(np.abs(S.b).max())
        assert self.residual <= K * EPS * self.bmax, (self.residual, K * EPS * self.bmax)
        assert S.cond <= COND_MAX, S.cond
        self.lvel, self.avel = S.velocities(self.lam)
        self.lam_bound = K * EPS * S.cond * float(np.abs(self.lam).max())
        self.vel_bound = self.lam_bound * S.velocity_gain()
        self.kkt_bound = K * EPS * S.cond * self.bmax

    def checks(self, lam, lvel, avel):
        """{check: (achieved, bound)} of a converged answer"""
        S = self.S
        out = dict(velocity=(float(max(np.abs(lvel - self.lvel).max(), np.abs(avel - self.avel).max())), self.vel_bound))
        if len(lam) != S.rows:                                              # other rows than the rule's: nothing to compare
            out["lambda"] = out["kkt"] = (float("inf"), self.lam_bound)
            return out
        out["lambda"] = (float(np.abs(lp.ld(lam) - self.lam).max()), self.lam_bound)
        viol, outside = lp.kkt(S.A, S.b, S.lo, S.hi, lam)
        out["kkt"] = (float("inf") if outside.any() else float(np.abs(viol).max()), self.kkt_bound)
        return out

    def sweep_check(self, lam):
        """{check: (achieved, bound)} of the answer of ONE sweep"""
        if len(lam) != self.S.rows:
            return dict(sweep=(float("inf"), K * EPS))
        diff, scale = lp.first_sweep(self.S, SOR_W, lam)
        return dict(sweep=(float((diff / scale).max()), K * EPS))


def momentum_check(st, lvel, avel):
    """(achieved, bound): the change of P and L over a solve of a closed system, against
    K eps sum_i (|m dv| + |x x m dv| + |I dw|).  Without inertia the rule drops every torque -- an impulse off the line of
    centres then turns nothing, and L is not conserved by design: P alone is checked."""
    P0, L0 = lp.momentum(st, st["lvel"], st["avel"])
    P1, L1 = lp.momentum(st, lvel, avel)
    dv, dw = lp.ld(lvel) - lp.ld(st["lvel"]), lp.ld(avel) - lp.ld(st["avel"])
    m, x = lp.ld(st["mass"]), lp.ld(st["pos"])
    scale = lp.LD(0)
    for i in range(len(m)):
        scale += np.linalg.norm((m[i] * dv[i]).astype(float)) + np.linalg.norm(np.cross(x[i], m[i] * dv[i]).astype(float))
        if st.get("inertia") is not None:
            scale += np.linalg.norm((lp.world_inertia(st, i, False) @ dw[i]).astype(float))
    drift = np.abs(P1 - P0).max() if st.get("inertia") is None else max(np.abs(P1 - P0).max(), np.abs(L1 - L0).max())
    return float(drift), float(K * EPS * scale)


@pytest.fixture(scope="module")
def free():
    return Truth(sc.scene_free())


# ------------------------------------------------------------------------------------------------- the inputs
def test_the_scene_holds_what_it_should(free):
    scene, S = free.scene, free.S
    st = scene["st"]
    pairs, recs = scene["body"]
    spairs, srecs = scene["static"]
    assert len(st["mass"]) == 8 and len(recs) == 12 and len(srecs) == 4
    assert (st["bflags"] == sc.NO_GRAVITY).sum() == 1 and (st["bflags"] == sc.KINEMATIC).sum() == 1
    kin = int(np.flatnonzero(st["bflags"] == sc.KINEMATIC)[0])
    assert np.abs(st["lvel"][kin]).min() > 0 and np.abs(st["avel"][kin]).min() > 0
    assert (pairs == kin).sum() >= 2                                        # against bodies only: against a static it has no row to speak of
    spread = np.ptp(st["inertia"], axis=1)                                  # anisotropic
    assert (spread > 0.02).all() and (spread > 0.15).sum() >= 6
    assert (np.abs(st["quat"][:, 1:]).min(axis=1) > 0.01).all()             # rotated about no coordinate axis
    for (i, j), r in zip(pairs, recs):                                      # off the line of centres
        d = sc.unit(st["pos"][j] - st["pos"][i])
        off = r["pos"] - st["pos"][i]
        assert np.linalg.norm(off - (off @ d) * d) > 0.05
    normals = np.concatenate([recs["normal"], recs["normal2"][recs["nc"] == 2], srecs["normal"]])
    assert np.allclose(np.linalg.norm(normals, axis=1), 1, atol=1e-15)
    steep = np.abs(normals[:, 2]) > np.sqrt(0.5)
    assert steep.sum() >= 2 and (~steep).sum() >= 2
    assert (recs["nc"] == 2).sum() == 4 and (recs["nc"][0::3] == 2).all()
    mus = np.concatenate([recs["mu"], srecs["mu"]])
    assert (mus == 0).any() and (mus == 0.5).any() and np.isinf(mus).any()
    assert S.kind.count("bounce") >= 1 and S.kind.count("nobounce") >= 1 and S.kind.count("friction") >= 6
    contacts = int(recs["nc"].sum() + srecs["nc"].sum())
    assert S.rows == contacts + 2 * int((recs["nc"] * (recs["mu"] > 0)).sum() + (srecs["mu"] > 0).sum())
    lam = free.lam                                                          # rows at either bound, rows inside
    fr = np.array([k == "friction" for k in S.kind])
    assert (lam[~fr] == 0).any() and (lam[~fr] > 0).any()
    assert (lam[fr] == S.lo[fr]).any() and (lam[fr] == S.hi[fr]).any() and ((lam[fr] > S.lo[fr]) & (lam[fr] < S.hi[fr])).any()
    print(f"scene F: {S.rows} rows, cond(A) {S.cond:.3g}, |lambda*| {float(np.abs(lam).max()):.3g}, solve_box residual "
          f"{free.residual:.3g} (bound {K * EPS * free.bmax:.3g})")


def test_plane_space_is_a_right_handed_orthonormal_basis():
    """{n, t1, t2} with n x t1 = t2, on random normals of both branches and at |n_z| = 1/sqrt 2 -1, 0, +1 ulp (the
    comparison is >: at the constant itself the second branch); solveref's scalars give the same basis"""
    R = sc.rng(3)
    s = np.float64(np.sqrt(0.5))
    normals = list(sc.unit(R.normal(size=(200, 3))))
    for nz in (np.nextafter(s, 0), s, np.nextafter(s, 1)):
        for sign in (1, -1):
            a = R.uniform(0, 2 * np.pi)
            normals.append(np.array([np.sqrt(1 - nz * nz) * np.cos(a), np.sqrt(1 - nz * nz) * np.sin(a), sign * nz]))
    steep = 0
    for n in normals:
        first = abs(n[2]) > s
        steep += first
        t1, t2 = lp.plane_space(n)
        assert (t1[0] == 0) == first or n[1] == 0                           # the branch the header names
        nn = lp.ld(n)
        tol = 8 * EPS
        assert abs(t1 @ t1 - 1) <= tol and abs(t2 @ t2 - 1) <= tol
        assert abs(nn @ t1) <= tol and abs(nn @ t2) <= tol and abs(t1 @ t2) <= tol
        assert np.abs(np.cross(nn, t1) - t2).max() <= tol
        p, q = sr.plane_space([np.float64(x) for x in n])
        assert np.abs(lp.ld(p) - t1).max() <= tol and np.abs(lp.ld(q) - t2).max() <= tol
    assert steep >= 50 + 2 and len(normals) - steep >= 50 + 4


def test_rotation_is_the_rotation():
    """R of lcpref rotates as the quaternion product q v q* does, is orthonormal and proper"""
    R = sc.rng(4)
    for q in sc.unit(R.normal(size=(20, 4))):
        M = lp.rotation(q)
        assert np.abs(M @ M.T - np.eye(3)).max() <= 8 * EPS and abs(np.linalg.det(M.astype(float)) - 1) <= 8 * EPS
        v = R.normal(size=3)
        qv = gr.quat_mul(gr.quat_mul(lp.ld([q]), lp.ld([[0, *v]])), lp.ld([[q[0], -q[1], -q[2], -q[3]]]))
        assert np.abs(M @ lp.ld(v) - qv[0, 1:]).max() <= 16 * EPS


# ------------------------------------------------------------------------------------------------- converged
def report(name, checks):
    for k, (got, bound) in checks.items():
        print(f"{name}: {k} {got:.3g} (bound {bound:.3g}, {got / bound:.2g} of it)")


@pytest.mark.parametrize("name", ["F", "S", "C"])
def test_converged_solve_is_the_lcp_solution(name, free):
    """solveref after N sweeps is lambda*, leaves velocities(lambda*) and satisfies complementarity: the figures are beside N"""
    truth = {"F": lambda: free, "S": lambda: Truth(sc.scene_free(inertia=False)), "C": lambda: Truth(sc.scene_chain())}[name]()
    S = truth.S
    if name == "C":
        assert S.rows >= 64 and len({tuple(p) for p in truth.scene["body"][0]}) < len(truth.scene["body"][0])
    out = restated(truth.scene, N)
    assert out["rows_total"] == S.rows and out["status"] == 0
    assert [int(k) & 0xffffffff for k in out["row_key"]] == list(range(S.rows))
    checks = truth.checks(out["row_lambda"], out["lvel"], out["avel"])
    print(f"scene {name}: {S.rows} rows, cond(A) {S.cond:.3g}")
    report(f"scene {name} at {N} sweeps", checks)
    for k, (got, bound) in checks.items():
        assert got <= bound, (k, got, bound)


def test_one_sweep_is_the_projected_gauss_seidel_row(free):
    checks = free.sweep_check(restated(free.scene, 1)["row_lambda"])
    report("scene F, one sweep", checks)
    assert checks["sweep"][0] <= checks["sweep"][1]


# ------------------------------------------------------------------------------------------------- momentum
@pytest.mark.parametrize("iterations", [1, 20])
@pytest.mark.parametrize("inertia", [True, False], ids=["F", "S"])
def test_the_solve_conserves_momentum(iterations, inertia):
    scene = sc.scene_free(inertia=inertia, closed=True)
    out = restated(scene, iterations)
    assert out["rows_total"] >= 24
    got, bound = momentum_check(scene["st"], out["lvel"], out["avel"])
    print(f"closed scene {'F' if inertia else 'S'}, {iterations} sweeps: momentum drift {got:.3g} (bound {bound:.3g})")
    assert np.abs(out["lvel"] - scene["st"]["lvel"]).max() > 0.1           # and something happened
    assert got <= bound


# ------------------------------------------------------------------------------------------------- the stack
def stack_state():
    n = sc.K_STACK
    return dict(pos=sc.stack_positions(), quat=np.tile([1.0, 0, 0, 0], (n, 1)), lvel=np.zeros((n, 3)), avel=np.zeros((n, 3)),
                bflags=np.zeros(n, np.uint32), adis_steps_left=np.full(n, 30, np.int32), adis_time_left=np.zeros(n),
                facc=np.zeros((n, 3)), mass=sc.STACK_MASS.copy(), radius=np.full(n, sc.R_STACK), inertia=None)


def stack_contacts(st):
    n = sc.K_STACK
    rec = lambda c: sr.record(np.asarray(c["pos"][0], float), np.asarray(c["normal"][0], float), float(c["depth"][0]))
    floor = gr.sphere_box(st["pos"][0:1], st["radius"][0:1], sc.FLOOR)
    static = (np.array([[0, 0]], np.uint32), sr.records([rec(floor)])) if floor["nc"][0] else None
    pairs, recs = [], []
    for i in range(n - 1):
        c = gr.sphere_sphere(st["pos"][i:i + 1], st["radius"][i:i + 1], st["pos"][i + 1:i + 2], st["radius"][i + 1:i + 2])
        if c["nc"][0]:
            pairs.append((i, i + 1))
            recs.append(rec(c))
    body = (np.array(pairs, np.uint32).reshape(-1, 2), sr.records(recs)) if pairs else None
    return static, body


def test_a_stack_comes_to_rest_at_its_closed_form():
    """Eight spheres (masses 1 .. 2) on the floor, mu = 0.  The stack is statically determinate: at rest contact i (the
    floor for i = 0, else between spheres i - 1 and i) carries exactly the weight above it, lambda_i = g sum_{j >= i} m_j,
    whatever the stiffness.  At rest every velocity is 0 and the normal row's equation is
    A lambda = b with J invM J^T lambda + J invM f = 0 (the forces balance), leaving (cfm / h) lambda_i = c_i / h =
    erp depth_i / h^2:  depth_i* = soft_cfm lambda_i h / soft_erp.  The multi-row analogue of
    test_a_sphere_comes_to_rest_on_the_floor; no damping acts at rest and nothing here sleeps (no AUTO_DISABLE flag)."""
    st = stack_state()
    for _ in range(2400):
        static, body = stack_contacts(st)
        out = sr.solve(st, np.zeros(sc.K_STACK, np.uint32), H, static=static, body=body)
        st["lvel"], st["avel"] = out["lvel"], out["avel"]
        pr.step_forces(dict(mass=st["mass"]), st, H)
    depth, want = sc.stack_depths(st["pos"]), sc.stack_depths_at_rest()
    print("depth", depth, "depth*", want, "relative", np.abs(depth - want) / want, "max |v|", np.abs(st["lvel"]).max())
    assert abs(want[0] - sc.SOFT_CFM * 9.8 * sc.STACK_MASS.sum() * H / sc.SOFT_ERP) < 1e-15 and want[-1] < want[0] / 5
    assert (np.abs(depth - want) <= 1e-3 * want).all()
    assert np.abs(st["lvel"]).max() <= 1e-6


# ------------------------------------------------------------------------------------------------- mutants
def patched(target, *edits):
    """(target, a copy of solveref's `target` with each (old, new) text replaced -- old must occur exactly once)"""
    owner, name = (sr, target) if "." not in target else (getattr(sr, target.split(".")[0]), target.split(".")[1])
    src = textwrap.dedent(inspect.getsource(getattr(owner, name)))
    for old, new in edits:
        assert src.count(old) == 1, (target, old, src.count(old))
        src = src.replace(old, new)
    ns = {}
    exec(compile(src, f"<mutant of {target}>", "exec"), dict(sr.__dict__), ns)
    f = ns[name]
    return owner, name, types.FunctionType(f.__code__, sr.__dict__, f.__name__, f.__defaults__, f.__closure__)


MUTANTS = {
    "world_tensor builds R^T D R": [("world_tensor", ("d[i] * R[4 * j + i]", "d[i] * R[4 * i + j]"),
                                     ("R[4 * i] * tmp[j] + R[4 * i + 1] * tmp[4 + j] + R[4 * i + 2] * tmp[8 + j]",
                                      "R[i] * tmp[j] + R[4 + i] * tmp[4 + j] + R[8 + i] * tmp[8 + j]"))],
    "the sign of J2a flipped": [("Row.__init__", ("[-x for x in cross(r2, u)]", "cross(r2, u)"))],
    "r2 measured from body 1": [("contact_rows", ("pos[k] - B2.pos[k]", "pos[k] - B1.pos[k]"))],
    "invM f_ext left out of rhs": [("Row.finish", ("B1.v[k] / h + B1.invM * B1.fext[k]", "B1.v[k] / h"),
                                    ("B2.v[k] / h + B2.invM * B2.fext[k]", "B2.v[k] / h"))],
    "cfm / h left out of d": [("Row.finish", ("d = d + self.cfmh", "d = d"))],
    "a kinematic body with invM = 1 / m": [("Body.__init__", ("f64(0) if kin else f64(1) / m", "f64(1) / m"))],
    "the bounce condition on out, not -out": [("contact_rows", ("-out_v > bounce_vel", "out_v > bounce_vel"))],
    "the second contact of a record dropped": [("contact_rows", ("for j in range(nc):", "for j in range(min(nc, 1)):"))],
    "friction bounds +-mu lambda_normal (Approx1)": [
        ("contact_rows", ("-mu, mu, h, sor_w).finish())", "-mu, mu, h, sor_w).finish())\n"
                          "                out[-1].back, out[-1].mu = 1 + (t is t2), mu")),
        ("_solve", ("nl = lam[k] + delta\n", "nl = lam[k] + delta\n"
                    "                if hasattr(r, 'back'):\n"
                    "                    r.lo, r.hi = -r.mu * lam[k - r.back], r.mu * lam[k - r.back]\n"))],
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutants(mutant, free, monkeypatch):
    """Each subtly wrong rule, made by patching a copy of solveref's piece (nothing is committed broken), misses at least
    one check of scene F by a factor of 1e3 or more over its bound: the checks would notice such a kernel."""
    for target, *edits in MUTANTS[mutant]:
        monkeypatch.setattr(*patched(target, *edits))
    with np.errstate(all="ignore"):
        out = restated(free.scene, N)
        checks = free.checks(out["row_lambda"], out["lvel"], out["avel"])
        checks.update(free.sweep_check(restated(free.scene, 1)["row_lambda"]))
        closed = sc.scene_free(closed=True)
        for it in (1, 20):
            o = restated(closed, it)
            checks[f"momentum at {it}"] = momentum_check(closed["st"], o["lvel"], o["avel"])
    ratio = {k: (got / bound if np.isfinite(got) else float("inf")) for k, (got, bound) in checks.items()}
    caught = [k for k, r in ratio.items() if not r < 1e3]
    print(f"MUTANT {mutant}: caught by {', '.join(caught) or 'NOTHING'}   "
          + "  ".join(f"{k} x{r:.2g}" for k, r in ratio.items()))
    assert caught


def test_a_copy_with_nothing_replaced_is_the_rule(free):
    """the mutant machinery itself"""
    with pytest.MonkeyPatch.context() as mp:
        for target in ("contact_rows", "_solve", "Row.__init__", "Row.finish", "Body.__init__", "world_tensor"):
            mp.setattr(*patched(target))
        a = restated(free.scene, 3)
    b = restated(free.scene, 3)
    assert a["row_lambda"].tobytes() == b["row_lambda"].tobytes() and a["lvel"].tobytes() == b["lvel"].tobytes()
