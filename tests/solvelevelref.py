"""The level rule of clapgpu_bodies_solve restated in numpy from include/clapgpu.h: which rows of an island may run
side by side without changing a bit of the sequential sweep.  The contacts are enumerated here anew from the lists (not
taken from solveref's solve); solveref supplies the record layout, the row constants and the sequential answer this
module's level-by-level execution is compared with.  Nothing here imports the device code."""
import numpy as np

import solveref as sr

f64 = np.float64


def contacts(st, island, static=None, mesh=None, body=None):
    """[(record, body 1, body 2 or None)]: the ACTIVE contacts' records in canonical order -- static list, mesh list, body
    list, each by record index -- with the arguments of solveref.solve"""
    n = len(st["mass"])
    fl = np.asarray(st["bflags"]).astype(np.uint32)
    island = np.asarray(island)
    listed = []
    sp = None if static is None else np.asarray(static[0]).reshape(-1, 2)
    if static is not None and static[1] is not None:
        listed += [(static[1][k], int(sp[k][0]), None) for k in range(len(static[1]))]
    if mesh is not None:
        for k in range(len(mesh[0])):
            ref = int(mesh[1][k][0])
            if ref < len(sp):
                listed.append((mesh[0][k], int(sp[ref][0]), None))
    if body is not None:
        pairs = np.asarray(body[0]).reshape(-1, 2)
        for k in range(len(body[1])):
            i, j = int(pairs[k][0]), int(pairs[k][1])
            if j < n and j != i:
                listed.append((body[1][k], i, j))
    out = []
    for rec, i, j in listed:
        if i >= n or (int(fl[i]) & sr.DISABLED) or int(island[i]) >= n:
            continue
        out.append((rec, i, j))
    return out


def rows_of(rec):
    """rows of a record: a normal row per contact, two friction rows behind it when mu > 0"""
    nc = min(int(rec["nc"]) & ~sr.CONTACT_DEEP, 2)
    return nc * (3 if f64(rec["mu"]) > 0 else 1)


def row_bodies(st, island, static=None, mesh=None, body=None):
    """(bodies, row_key): per row ordinal its (body 1, body 2 or None) -- a dropped row's too -- and its key"""
    bodies, keys = [], []
    for rec, i, j in contacts(st, island, static, mesh, body):
        for _ in range(rows_of(rec)):
            keys.append((int(island[i]) << 32) | len(bodies))
            bodies.append((i, j))
    return bodies, np.array(keys, np.uint64)


def levels(row_key, bodies):
    """level per ordinal: walking each island's rows in canonical order, 1 + the level of the latest earlier row of the
    island that names body 1 or body 2 (the higher of the two; 0 where there is none).  An absent body 2 is no dependency"""
    out = np.zeros(len(bodies), np.uint32)
    last = {}                                                             # (island, body) -> level of the latest row naming it
    for k in sorted(range(len(bodies)), key=lambda k: int(row_key[k])):   # island by island, ordinals rising
        isl = int(row_key[k]) >> 32
        named = [(isl, b) for b in bodies[k] if b is not None]
        lv = 1 + max(last.get(b, 0) for b in named)
        for b in named:
            last[b] = lv
        out[int(row_key[k]) & 0xffffffff] = lv
    return out


def island_rows(row_key):
    """{island: rows} from the keys"""
    isl, cnt = np.unique(np.asarray(row_key, np.uint64) >> np.uint64(32), return_counts=True)
    return dict(zip(isl.tolist(), cnt.tolist()))


def expected_levels(row_key, bodies, wide_rows):
    """(row_level, wide_total) the device reports: the level in islands of at least wide_rows rows, 0 elsewhere"""
    lv = levels(row_key, bodies)
    per = island_rows(row_key)
    wide = {i for i, c in per.items() if wide_rows and c >= wide_rows}
    mask = np.array([(int(k) >> 32) in wide for k in row_key], bool)
    return np.where(mask, lv, 0).astype(np.uint32), len(wide)


# ------------------------------------------------------------------------------------------------- the schedule, run
def solver_rows(st, island, h, static=None, mesh=None, body=None, solver=sr.SOLVER, gravity=sr.GRAVITY):
    """solveref's Row objects (its constants, nothing of its sweep) in canonical order"""
    h = f64(h)
    cache = {}

    def load(i):
        if i not in cache:
            cache[i] = sr.Body(st, i, gravity)
        return cache[i]
    out = []
    with np.errstate(all="ignore"):
        for rec, i, j in contacts(st, island, static, mesh, body):
            if rows_of(rec):
                out += sr.contact_rows(rec, i, j, load(i), None if j is None else load(j), h, solver)
    return out


def solve_by_levels(st, island, h, static=None, mesh=None, body=None, solver=sr.SOLVER, gravity=sr.GRAVITY,
                    within=reversed):
    """The solve executed level after level, the rows of a level in the order `within` puts them (reversed by default:
    as far from canonical as a level allows).  Returns dict(lvel, avel, row_lambda, schedule); schedule: per island the
    list of levels, each a list of ordinals in canonical order."""
    h = f64(h)
    rows = solver_rows(st, island, h, static, mesh, body, solver, gravity)
    bodies, key = row_bodies(st, island, static, mesh, body)
    assert len(rows) == len(bodies)
    lv = levels(key, bodies)
    schedule = {}
    for k in range(len(rows)):
        per = schedule.setdefault(int(key[k]) >> 32, {})
        per.setdefault(int(lv[k]), []).append(k)
    schedule = {isl: [per[q] for q in sorted(per)] for isl, per in schedule.items()}
    lam = [f64(0)] * len(rows)
    a = {b: [f64(0)] * 6 for pair in bodies for b in pair if b is not None}
    with np.errstate(all="ignore"):
        for isl in sorted(schedule):
            for _ in range(int(solver["iterations"])):
                for level in schedule[isl]:
                    for k in within(level):
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
                        if r.two:
                            a[r.b2] = [x[6 + q] + r.iMJ[6 + q] * dl for q in range(6)]
                        lam[k] = nl
        fl = np.asarray(st["bflags"]).astype(np.uint32)
        lvel, avel = np.array(st["lvel"], f64), np.array(st["avel"], f64)
        for b, ab in a.items():
            if int(fl[b]) & (sr.DISABLED | sr.KINEMATIC):
                continue
            for q in range(3):
                lvel[b][q] = lvel[b][q] + h * ab[q]
                avel[b][q] = avel[b][q] + h * ab[3 + q]
    return dict(lvel=lvel, avel=avel, row_lambda=np.array(lam, f64).reshape(-1), schedule=schedule, row_level=lv, row_key=key)
