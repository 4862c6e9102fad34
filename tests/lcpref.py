"""The contact solve of clapgpu_bodies_solve as a dense boxed LCP: the independent truth for the rule in include/clapgpu.h.

tests/solveref.py restates the rule scalar by scalar, as the kernels compute it, and the device is held to it bit for
bit; that cannot tell a right rule from a wrong one.  This module states what the rule MEANS, with matrices and in
np.longdouble, and shares neither code nor the order of any sum with solveref.py (which it does not import):

  - R from the quaternion by rotating the basis vectors, v + 2 w (u x v) + 2 u x (u x v), not dQtoR's expansion;
  - invM block diagonal [6n, 6n]: I3 / m and R diag(1 / inertia) R^T per body, all zeros for a KINEMATIC body, the
    angular block zero without inertia;  f = facc + m g (not for NO_GRAVITY), no torque;
  - J [rows, 6n], one row per row of the rule in the header's canonical order (static list, mesh list, body list; slot
    1, slot 2; normal, t1, t2 when mu > 0), every row built with np.cross;  c, cfm, lo, hi as the header has them;
  - A = J invM J^T + diag(cfm / h),  b = c / h - J (v / h + invM f);  the solve's answer is the unique lambda* with
    lo <= lambda <= hi and w = A lambda - b complementary to the box (A is symmetric positive definite: every cfm > 0),
    found by an active-set method with np.linalg.solve on the free set -- no relaxation, no sweep;
  - what the solve leaves in lvel and avel is v + h invM J^T lambda.

The friction directions are part of the contract (a force box is not rotation invariant), so plane_space below is
dPlaneSpace from the header's text; tests/test_solve_lcp.py holds it to a right-handed orthonormal basis on both
branches.  Islands are not an input: the dense system is block diagonal by itself.

ODE is absent from the reference: the rule stays PARITY UNPINNED; this pins it to mechanics instead."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
DISABLED, NO_GRAVITY, KINEMATIC = 1, 4, 32
CONTACT_BOUNCE, CONTACT_DEEP = 0x004, 0x80000000
GRAVITY = (0.0, -9.8, 0.0)
CFM = 1e-10                                                                 # clapgpu_solver_defaults' cfm


def ld(a):
    return np.asarray(a, dtype=LD)


def rotation(q):
    """R [3, 3] of the quaternion (w, x, y, z): column j is the basis vector e_j rotated"""
    q = ld(q)
    w, u = q[0], q[1:]
    cols = []
    for v in ld(np.eye(3)):
        uv = np.cross(u, v)
        cols.append(v + 2 * w * uv + 2 * np.cross(u, uv))
    return np.stack(cols, axis=1)


def plane_space(n):
    """dPlaneSpace as the header writes it; the branch is taken on the float64 the kernel compares"""
    n0, n1, n2 = ld(n)
    if abs(np.float64(n[2])) > np.float64(np.sqrt(0.5)):
        a = n1 * n1 + n2 * n2
        k = 1 / np.sqrt(a)
        t1 = ld([0, -n2 * k, n1 * k])
        t2 = ld([a * k, -n0 * t1[2], n0 * t1[1]])
    else:
        a = n0 * n0 + n1 * n1
        k = 1 / np.sqrt(a)
        t1 = ld([-n1 * k, n0 * k, 0])
        t2 = ld([-n2 * t1[1], n2 * t1[0], a * k])
    return t1, t2


def world_inertia(st, i, inverse):
    """R diag(I) R^T, or R diag(1 / I) R^T, of body i"""
    R = rotation(st["quat"][i])
    d = ld(st["inertia"][i])
    return R @ np.diag(1 / d if inverse else d) @ R.T


class System:
    """The dense problem of one solve.  st, static, mesh, body: as tests/solveref.py's solve takes them (dict of arrays;
    (static_pairs, records); (records, mesh_ref); (pairs, records))."""

    def __init__(self, st, h, static=None, mesh=None, body=None, cfm=CFM, gravity=GRAVITY):
        n = self.n = len(st["mass"])
        self.h = h = LD(h)
        fl = np.asarray(st["bflags"]).astype(np.uint32)
        m = ld(st["mass"])
        self.invM = np.zeros((6 * n, 6 * n), LD)
        self.f = np.zeros(6 * n, LD)
        self.v = np.concatenate([ld(st["lvel"]), ld(st["avel"])], axis=1).reshape(-1)
        for i in range(n):
            if not fl[i] & KINEMATIC:
                self.invM[6 * i:6 * i + 3, 6 * i:6 * i + 3] = ld(np.eye(3)) / m[i]
                if st.get("inertia") is not None:
                    self.invM[6 * i + 3:6 * i + 6, 6 * i + 3:6 * i + 6] = world_inertia(st, i, True)
            if st.get("facc") is not None:
                self.f[6 * i:6 * i + 3] = ld(st["facc"][i])
            if not fl[i] & NO_GRAVITY:
                self.f[6 * i:6 * i + 3] += m[i] * ld(gravity)
        contacts = []                                                       # (record, body 1, body 2 or None)
        spairs = None if static is None else np.asarray(static[0]).reshape(-1, 2)
        if static is not None:
            contacts += [(rec, int(spairs[k][0]), None) for k, rec in enumerate(static[1])]
        if mesh is not None:
            contacts += [(rec, int(spairs[int(ref[0])][0]), None) for rec, ref in zip(*mesh) if int(ref[0]) < len(spairs)]
        if body is not None:
            contacts += [(rec, int(p[0]), int(p[1])) for p, rec in zip(*body) if int(p[1]) < n and int(p[1]) != int(p[0])]
        J, c, cf, lo, hi, kind = [], [], [], [], [], []
        pos = ld(st["pos"])
        for rec, b1, b2 in contacts:
            if b1 >= n or fl[b1] & DISABLED:
                continue
            for slot in range(min(int(rec["nc"]) & ~CONTACT_DEEP, 2)):
                p = ld(rec["pos2"] if slot else rec["pos"])
                nrm = ld(rec["normal2"] if slot else rec["normal"])
                depth = LD(rec["depth2"] if slot else rec["depth"])

                def row(u):
                    r = np.zeros(6 * n, LD)
                    r[6 * b1:6 * b1 + 3], r[6 * b1 + 3:6 * b1 + 6] = u, np.cross(p - pos[b1], u)
                    if b2 is not None:
                        r[6 * b2:6 * b2 + 3], r[6 * b2 + 3:6 * b2 + 6] = -u, -np.cross(p - pos[b2], u)
                    return r
                jn = row(nrm)
                cn = LD(rec["soft_erp"]) / h * depth
                bounced = False
                if int(rec["mode"]) & CONTACT_BOUNCE:
                    out = jn @ self.v
                    if LD(rec["bounce_vel"]) >= 0 and -out > LD(rec["bounce_vel"]):
                        bounced = -LD(rec["bounce"]) * out > cn
                        cn = max(cn, -LD(rec["bounce"]) * out)
                J.append(jn), c.append(cn), cf.append(LD(rec["soft_cfm"])), lo.append(LD(0)), hi.append(LD(np.inf))
                kind.append("bounce" if bounced else "nobounce" if int(rec["mode"]) & CONTACT_BOUNCE else "normal")
                mu = LD(rec["mu"])
                if mu > 0:
                    for t in plane_space(nrm):
                        J.append(row(t)), c.append(LD(0)), cf.append(LD(cfm)), lo.append(-mu), hi.append(mu)
                        kind.append("friction")
        self.rows = len(J)
        self.kind = kind
        self.J = np.array(J, LD).reshape(self.rows, 6 * n)
        self.c, self.cfm, self.lo, self.hi = ld(c), ld(cf), ld(lo), ld(hi)
        self.A = self.J @ self.invM @ self.J.T + np.diag(self.cfm / h)
        self.b = self.c / h - self.J @ (self.v / h + self.invM @ self.f)
        self.cond = float(np.linalg.cond(self.A.astype(np.float64)))
        # the same two with every term taken absolutely: the scale of the rounding error of any way of summing them
        self.absA = np.abs(self.J) @ np.abs(self.invM) @ np.abs(self.J).T + np.diag(self.cfm / h)
        self.absb = np.abs(self.c / h) + np.abs(self.J) @ (np.abs(self.v / h) + np.abs(self.invM) @ np.abs(self.f))

    def velocities(self, lam):
        """(lvel [n, 3], avel [n, 3]) after the solve: v + h invM J^T lambda"""
        v = (self.v + self.h * (self.invM @ (self.J.T @ ld(lam)))).reshape(self.n, 6)
        return v[:, :3], v[:, 3:]

    def velocity_gain(self):
        """|| h invM J^T ||_inf: what an error of lambda does to a velocity at most"""
        return float(np.abs(self.h * (self.invM @ self.J.T)).sum(axis=1).max())


def kkt(A, b, lo, hi, lam):
    """The violation of complementarity by row: with w = A lambda - b, min(w, 0) at the lower bound (w must push up
    there), max(w, 0) at the upper bound, w strictly inside.  A lambda outside its box counts as at that bound; its
    distance outside is returned beside the violation (both [rows])."""
    lam = ld(lam)
    w = A @ lam - b
    viol = np.where(lam <= lo, np.minimum(w, 0), np.where(lam >= hi, np.maximum(w, 0), w))
    outside = np.maximum(np.maximum(lo - lam, lam - hi), 0)
    return viol, outside


def _solve_free(A, rhs):
    """A x = rhs for a symmetric positive definite A in long double: np.linalg.solve in float64, refined on the long
    double residual"""
    A64 = A.astype(np.float64)
    x = ld(np.linalg.solve(A64, rhs.astype(np.float64)))
    for _ in range(4):
        x = x + ld(np.linalg.solve(A64, (rhs - A @ x).astype(np.float64)))
    return x


def solve_box(A, b, lo, hi):
    """The solution of the boxed LCP  lo <= lambda <= hi, w = A lambda - b, w >= 0 at lo, w <= 0 at hi, w = 0 inside,
    by an active set: the rows are free, at lo or at hi; the free rows solve their linear system with the others held;
    a free row that left its box is put on the bound it crossed and a held row whose w has the wrong sign is freed.  All
    such rows change at once while that makes progress, then one at a time, the lowest index first (Murty's rule, which
    ends for a positive definite A).  Returns (lambda*, max |kkt|)."""
    k = len(b)
    state = np.zeros(k, int)                                                # 0 free, -1 at lo, +1 at hi
    lam = np.zeros(k, LD)
    if k == 0:
        return lam, 0.0
    best = k + 1
    patience = 8
    for _ in range(200 * k + 200):
        free = state == 0
        lam = np.where(state < 0, lo, np.where(state > 0, hi, LD(0)))
        lam = np.where(free, LD(0), lam)
        if free.any():
            held = A[np.ix_(free, ~free)] @ lam[~free] if (~free).any() else 0
            lam[free] = _solve_free(A[np.ix_(free, free)], b[free] - held)
        w = A @ lam - b
        tol = 4 * EPS * (np.abs(A) @ np.abs(lam) + np.abs(b))
        bad_lo, bad_hi = free & (lam < lo), free & (lam > hi)
        bad_w = ((state < 0) & (w < -tol)) | ((state > 0) & (w > tol))
        bad = bad_lo | bad_hi | bad_w
        count = int(bad.sum())
        if count == 0:
            break
        if count < best:
            best, patience = count, 8
        else:
            patience -= 1
        if patience < 0:                                                    # one at a time
            first = int(np.flatnonzero(bad)[0])
            bad = np.zeros(k, bool)
            bad[first] = True
        state = np.where(bad & bad_lo, -1, np.where(bad & bad_hi, 1, np.where(bad & bad_w, 0, state)))
    lam = np.minimum(np.maximum(lam, lo), hi)
    viol, _ = kkt(A, b, lo, hi, lam)
    return lam, float(np.abs(viol).max())


def first_sweep(S, sor_w, lam):
    """What ONE relaxation sweep from lambda = 0 leaves, row by row, given that sweep's own earlier rows:
    lambda_i = clamp(sor_w / A_ii (b_i - sum_{j < i} A_ij lambda_j)) -- the textbook projected Gauss-Seidel row, which
    also pins the step length sor_w / A_ii that a converged answer does not depend on.  Returns (|lambda_i - that|,
    scale_i): scale_i is the row's value with every term of A and b taken absolutely, the size of what rounds."""
    lam = ld(lam)
    d = np.diag(S.A)
    L = np.tril(S.A, -1)
    want = np.minimum(np.maximum(LD(sor_w) / d * (S.b - L @ lam), S.lo), S.hi)
    scale = LD(sor_w) / d * (S.absb + np.tril(S.absA, -1) @ np.abs(lam)) + np.abs(lam)
    return np.abs(lam - want), scale


def momentum(st, lvel, avel):
    """(P, L): sum m v and sum (R diag(I) R^T w + m x x v) about the origin; without inertia the spin term is absent"""
    m, x, lvel, avel = ld(st["mass"]), ld(st["pos"]), ld(lvel), ld(avel)
    P = (m[:, None] * lvel).sum(axis=0)
    L = np.cross(x, m[:, None] * lvel).sum(axis=0)
    if st.get("inertia") is not None:
        for i in range(len(m)):
            L = L + world_inertia(st, i, False) @ avel[i]
    return P, L
