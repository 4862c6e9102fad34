"""The contact solve of clapgpu_bodies_solve restated in numpy from the rule in include/clapgpu.h: quickstep's contact
rows and its SOR iteration with the row order fixed to the canonical order of the contact lists, one solve per island.
Plain loops over float64 scalars, one rounding per operation, every sum left to right as the header writes it; nothing
here imports the device code.  What the device is compared with, bit for bit.  Whether the rule itself is right is not
decided here: tests/lcpref.py states it as a dense boxed LCP, and tests/test_solve_lcp.py holds this module to that.

ODE is absent from the reference: like the rest of the rigid-body block this is PARITY UNPINNED."""
import numpy as np

f64 = np.float64
DISABLED, NO_GRAVITY, KINEMATIC = 1, 4, 32
CONTACT_BOUNCE, CONTACT_DEEP = 0x004, 0x80000000
SQRT1_2 = f64(0.70710678118654752440)
GRAVITY = (0.0, -9.8, 0.0)
SOLVER = dict(iterations=20, sor_w=1.3, cfm=1e-10)                        # clapgpu_solver_defaults

C2 = np.dtype([("pos", np.float64, 3), ("normal", np.float64, 3), ("depth", np.float64), ("mu", np.float64),
               ("bounce", np.float64), ("bounce_vel", np.float64), ("soft_erp", np.float64), ("soft_cfm", np.float64),
               ("mode", np.uint32), ("nc", np.uint32), ("pos2", np.float64, 3), ("normal2", np.float64, 3),
               ("depth2", np.float64)])


def record(pos, normal, depth, mu=0.0, bounce=0.0, bounce_vel=0.0, soft_erp=0.05, soft_cfm=0.01, second=None):
    """one clapgpu_contact2 as phys_contact_surface fills it (defaults: physics.c:293-294)"""
    r = np.zeros(1, C2)[0]
    r["pos"], r["normal"], r["depth"] = pos, normal, depth
    r["mu"], r["bounce"], r["bounce_vel"], r["soft_erp"], r["soft_cfm"] = mu, bounce, bounce_vel, soft_erp, soft_cfm
    r["mode"] = 0x018 | (CONTACT_BOUNCE if bounce > 0 else 0)
    r["nc"] = 1
    if second is not None:
        r["pos2"], r["normal2"], r["depth2"] = second
        r["nc"] = 2
    return r


def records(items):
    out = np.zeros(len(items), C2)
    for k, r in enumerate(items):
        out[k] = r
    return out


# ------------------------------------------------------------------------------------------------- pieces of the rule
def q_to_R(q):
    """dQtoR, ODE's dMatrix3 (3 rows of 4)"""
    two = f64(2)
    qq1, qq2, qq3 = two * q[1] * q[1], two * q[2] * q[2], two * q[3] * q[3]
    one, z = f64(1), f64(0)
    return [one - qq2 - qq3, two * (q[1] * q[2] - q[0] * q[3]), two * (q[1] * q[3] + q[0] * q[2]), z,
            two * (q[1] * q[2] + q[0] * q[3]), one - qq1 - qq3, two * (q[2] * q[3] - q[0] * q[1]), z,
            two * (q[1] * q[3] - q[0] * q[2]), two * (q[2] * q[3] + q[0] * q[1]), one - qq1 - qq2, z]


def world_tensor(R, d):
    """R diag(d) R^T the way the step builds it: tmp = D R^T, W = R tmp"""
    tmp = [f64(0)] * 12
    for i in range(3):
        for j in range(3):
            tmp[4 * i + j] = d[i] * R[4 * j + i]
    W = [f64(0)] * 12
    for i in range(3):
        for j in range(3):
            W[4 * i + j] = R[4 * i] * tmp[j] + R[4 * i + 1] * tmp[4 + j] + R[4 * i + 2] * tmp[8 + j]
    return W


def mul331(M, v):
    return [M[4 * i] * v[0] + M[4 * i + 1] * v[1] + M[4 * i + 2] * v[2] for i in range(3)]


def cross(r, n):
    return [r[1] * n[2] - r[2] * n[1], r[2] * n[0] - r[0] * n[2], r[0] * n[1] - r[1] * n[0]]


def plane_space(n):
    """dPlaneSpace"""
    z = f64(0)
    if abs(n[2]) > SQRT1_2:
        a = n[1] * n[1] + n[2] * n[2]
        k = f64(1) / np.sqrt(a)
        p = [z, -n[2] * k, n[1] * k]
        q = [a * k, -n[0] * p[2], n[0] * p[1]]
    else:
        a = n[0] * n[0] + n[1] * n[1]
        k = f64(1) / np.sqrt(a)
        p = [-n[1] * k, n[0] * k, z]
        q = [-n[2] * p[1], n[2] * p[0], a * k]
    return p, q


class Body:
    def __init__(self, st, i, gravity):
        fl = int(st["bflags"][i])
        kin = bool(fl & KINEMATIC)
        m = f64(st["mass"][i])
        self.invM = f64(0) if kin else f64(1) / m
        self.pos = [f64(x) for x in st["pos"][i]]
        self.v = [f64(x) for x in st["lvel"][i]]
        self.w = [f64(x) for x in st["avel"][i]]
        facc = st.get("facc")
        self.fext = []
        for j in range(3):
            fa = f64(0) if facc is None else f64(facc[i][j])
            self.fext.append(fa + (f64(0) if fl & NO_GRAVITY else m * f64(gravity[j])))
        inertia = st.get("inertia")
        if inertia is not None and not kin:
            inv = [f64(1) / f64(x) for x in inertia[i]]
            self.invI = world_tensor(q_to_R([f64(x) for x in st["quat"][i]]), inv)
        else:
            self.invI = [f64(0)] * 12


class Row:
    """the constants of one row along `u`"""

    def __init__(self, u, r1, r2, B1, B2, b1, b2, c, cfm, lo, hi, h, sor_w):
        two = B2 is not None
        J = list(u) + cross(r1, u)
        if two:
            J += [-x for x in u] + [-x for x in cross(r2, u)]
        self.J, self.two, self.b1, self.b2, self.lo, self.hi = J, two, b1, b2, f64(lo), f64(hi)
        self.c, self.cfm = c, cfm
        self.B = (B1, B2)
        self.h, self.sor_w = h, sor_w

    def velocity(self):
        """J . (v1, w1, v2, w2)"""
        B1, B2 = self.B
        x = B1.v + B1.w + ((B2.v + B2.w) if self.two else [])
        s = self.J[0] * x[0]
        for k in range(1, len(x)):
            s = s + self.J[k] * x[k]
        return s

    def finish(self):
        J, h = self.J, self.h
        B1, B2 = self.B
        iMJ = [B1.invM * J[0], B1.invM * J[1], B1.invM * J[2]] + mul331(B1.invI, J[3:6])
        terms = [B1.v[k] / h + B1.invM * B1.fext[k] for k in range(3)] + [B1.w[k] / h for k in range(3)]
        if self.two:
            iMJ += [B2.invM * J[6], B2.invM * J[7], B2.invM * J[8]] + mul331(B2.invI, J[9:12])
            terms += [B2.v[k] / h + B2.invM * B2.fext[k] for k in range(3)] + [B2.w[k] / h for k in range(3)]
        s = J[0] * terms[0]
        for k in range(1, len(terms)):
            s = s + J[k] * terms[k]
        self.rhs = self.c / h - s
        self.cfmh = self.cfm / h
        d = iMJ[0] * J[0]
        for k in range(1, len(J)):
            d = d + iMJ[k] * J[k]
        d = d + self.cfmh
        self.iMJ = iMJ
        self.dropped = bool(d == 0)
        self.Ad = self.sor_w / d
        return self


def contact_rows(rec, b1, b2, B1, B2, h, solver):
    """the rows of one record, in order: per contact the normal row, then the two friction rows when mu > 0"""
    out = []
    nc = min(int(rec["nc"]) & ~CONTACT_DEEP, 2)
    mu = f64(rec["mu"])
    erp_h = f64(rec["soft_erp"]) / h
    sor_w, cfm = f64(solver["sor_w"]), f64(solver["cfm"])
    for j in range(nc):
        pos = [f64(x) for x in (rec["pos2"] if j else rec["pos"])]
        n = [f64(x) for x in (rec["normal2"] if j else rec["normal"])]
        depth = f64(rec["depth2"] if j else rec["depth"])
        r1 = [pos[k] - B1.pos[k] for k in range(3)]
        r2 = [pos[k] - B2.pos[k] for k in range(3)] if B2 is not None else None
        c = erp_h * depth
        row = Row(n, r1, r2, B1, B2, b1, b2, c, f64(rec["soft_cfm"]), 0.0, np.inf, h, sor_w)
        if int(rec["mode"]) & CONTACT_BOUNCE:
            out_v = row.velocity()
            bounce_vel = f64(rec["bounce_vel"])
            if bounce_vel >= 0 and -out_v > bounce_vel:
                newc = (-f64(rec["bounce"])) * out_v
                if newc > row.c:
                    row.c = newc
        out.append(row.finish())
        if mu > 0:
            t1, t2 = plane_space(n)
            for t in (t1, t2):
                out.append(Row(t, r1, r2, B1, B2, b1, b2, f64(0), cfm, -mu, mu, h, sor_w).finish())
    return out


# ------------------------------------------------------------------------------------------------- the solve
def solve(st, island, h, static=None, mesh=None, body=None, solver=SOLVER, gravity=GRAVITY, rows_capacity=None):
    """st: dict of pos, quat, lvel, avel, mass, bflags [n] and optionally inertia [n, 3], facc [n, 3] (None: absent).
    static = (static_pairs [k, 2], records [k]); mesh = (records [k], mesh_ref [k, 2]) (needs static's pairs);
    body = (pairs [k, 2], records [k]) -- the downloaded prefixes min(total, capacity) of each list.
    Returns dict(lvel, avel (new arrays), row_lambda, row_key (canonical row order), rows_total, status, impulse_abs)."""
    with np.errstate(all="ignore"):
        return _solve(st, np.asarray(island), f64(h), static, mesh, body, solver, gravity, rows_capacity)


def _solve(st, island, h, static, mesh, body, solver, gravity, rows_capacity):
    n = len(st["mass"])
    fl = np.asarray(st["bflags"]).astype(np.uint32)
    contacts = []                                                         # (record, b1, b2) in canonical order
    spairs = None if static is None else np.asarray(static[0]).reshape(-1, 2)
    if static is not None and static[1] is not None:
        for k, rec in enumerate(static[1]):
            contacts.append((rec, int(spairs[k][0]), None))
    if mesh is not None:
        for k, rec in enumerate(mesh[0]):
            ref = int(mesh[1][k][0])
            if ref < len(spairs):
                contacts.append((rec, int(spairs[ref][0]), None))
    if body is not None:
        for k, rec in enumerate(body[1]):
            b1, b2 = int(body[0][k][0]), int(body[0][k][1])
            if b2 < n and b2 != b1:
                contacts.append((rec, b1, b2))
    rows = []
    cache = {}

    def load(i):
        if i not in cache:
            cache[i] = Body(st, i, gravity)
        return cache[i]
    for rec, b1, b2 in contacts:
        if b1 >= n or fl[b1] & DISABLED or int(island[b1]) >= n:
            continue
        if min(int(rec["nc"]) & ~CONTACT_DEEP, 2) == 0:
            continue
        isl = int(island[b1])
        for row in contact_rows(rec, b1, b2, load(b1), None if b2 is None else load(b2), h, solver):
            row.island = isl
            rows.append(row)
    total = len(rows)
    lvel, avel = np.array(st["lvel"], f64), np.array(st["avel"], f64)
    if rows_capacity is not None and total > rows_capacity:
        return dict(lvel=lvel, avel=avel, row_lambda=np.zeros(0), row_key=np.zeros(0, np.uint64), rows_total=total, status=1)
    key = np.array([(r.island << 32) | k for k, r in enumerate(rows)], np.uint64)
    lam = [f64(0)] * total
    a = {}                                                                # body -> six doubles
    impulse_abs = np.zeros((n, 3))                                        # sum of |h iMJ_lin dlambda| per body: a bound's scale
    by_island = {}
    for k, r in enumerate(rows):
        by_island.setdefault(r.island, []).append(k)
        for b in (r.b1, r.b2):
            if b is not None:
                a.setdefault(b, [f64(0)] * 6)
    for isl in sorted(by_island):                                         # islands share nothing: any order of them
        for _ in range(int(solver["iterations"])):
            for k in by_island[isl]:
                r = rows[k]
                if r.dropped:
                    continue
                x = a[r.b1] + (a[r.b2] if r.two else [])
                Ja = r.J[0] * x[0]
                for q in range(1, len(x)):
                    Ja = Ja + r.J[q] * x[q]
                delta = r.Ad * ((r.rhs - r.cfmh * lam[k]) - Ja)
                nl = lam[k] + delta
                if nl < r.lo:
                    nl = r.lo
                if nl > r.hi:
                    nl = r.hi
                dl = nl - lam[k]
                a[r.b1] = [x[q] + r.iMJ[q] * dl for q in range(6)]
                impulse_abs[r.b1] += [abs(h * r.iMJ[q] * dl) for q in range(3)]
                if r.two:
                    a[r.b2] = [x[6 + q] + r.iMJ[6 + q] * dl for q in range(6)]
                    impulse_abs[r.b2] += [abs(h * r.iMJ[6 + q] * dl) for q in range(3)]
                lam[k] = nl
    for b, ab in a.items():
        if fl[b] & (DISABLED | KINEMATIC):
            continue
        for q in range(3):
            lvel[b][q] = lvel[b][q] + h * ab[q]
            avel[b][q] = avel[b][q] + h * ab[3 + q]
    return dict(lvel=lvel, avel=avel, row_lambda=np.array(lam, f64).reshape(-1), row_key=key, rows_total=total, status=0,
                impulse_abs=impulse_abs)
