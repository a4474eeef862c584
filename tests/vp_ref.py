"""numpy restatement of the vanishing-point estimator (csrc/uvs_vanishing_points.hip), after the reference's
feature_tracker/src/line_feature_tracker.cpp:1977-2299 (getVPHypVia2Lines, getSphereGrids, getBestVpsHyp, lines2Vps) and :379-385.

Every function takes a dtype: float64 is the pin of the device, numpy.longdouble the yardstick the tolerances of
tests/test_vanishing_points.py are measured with (same constants -- CV_PI is a double in the reference -- only the rounding differs).
Two things are ours, not the reference's: the counter-based sample generator with a bounded number of attempts, and the snap of
the cell rule."""
import math

import numpy as np

N_SAMPLES = int(math.log(1 - 0.9999) / math.log(1.0 - 1.0 / 3.0 * (1.0 - 0.5) ** 2))      # :1981-1985
N_ROT = 360
N_HYP = N_SAMPLES * N_ROT
LA, LO = 90, 360
MAX_ATTEMPTS = 64
PI = 3.1415926535897932384626433832795       # CV_PI
DEG = 1.0 / 180.0 * PI
TOL60 = 60.0 / 180.0 * PI
SNAP = 1e-9
OK, TOO_FEW_LINES, NO_HYPOTHESIS = 0, 1, 2
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, s, t, n):
    """Attempt t of sample s: two line indices (they may be equal: the caller redraws)."""
    c = 1 + (s << 20) + 2 * t
    return mix64(seed + GOLDEN * c) % n, mix64(seed + GOLDEN * (c + 1)) % n


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def line_params(segs, dt=np.float64):
    s = np.asarray(segs, dtype=np.float64).reshape(-1, 4).astype(dt)
    x1, y1, x2, y2 = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    para = np.stack([y1 - y2, x2 - x1, x1 * y2 - y1 * x2], axis=1)      # (x1, y1, 1) x (x2, y2, 1)
    dx, dy = x2 - x1, y2 - y1
    length = np.sqrt(dx * dx + dy * dy)
    ori = np.arctan2(dy, dx)
    ori = np.where(ori < 0, ori + dt(PI), ori)
    return para, length, ori


def samples(seed, para):
    """[N_SAMPLES, 2] line pairs, or None when a sample runs out of attempts.  The z == 0 test is taken in float64 (the device's)."""
    p = np.asarray(para, dtype=np.float64)
    n = len(p)
    out = np.zeros((N_SAMPLES, 2), np.int64)
    for s in range(N_SAMPLES):
        for t in range(MAX_ATTEMPTS):
            a, b = draw(seed, s, t, n)
            if a == b or p[a, 0] * p[b, 1] - p[a, 1] * p[b, 0] == 0:
                continue
            out[s] = a, b
            break
        else:
            return None
    return out


def _unit(v, dt):
    """v(2) == 0 -> 0.0011; v *= 1 / N (:2034-2036)"""
    v = v.copy()
    v[..., 2] = np.where(v[..., 2] == 0, dt(0.0011), v[..., 2])
    n = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
    return v * (dt(1.0) / n)[..., None]


def hypotheses(para, smp, cam, dt=np.float64):
    """[N_HYP, 3, 3]: hypothesis 360 s + j = (vp1, vp2, vp3) of sample s, rotation j (:2024-2071)."""
    fx, fy, cx, cy = (dt(v) for v in cam)
    pa, pb = para[smp[:, 0]], para[smp[:, 1]]
    v = cross(pa, pb)
    vp1 = _unit(np.stack([v[:, 0] / v[:, 2] - cx, v[:, 1] / v[:, 2] - cy, np.full(len(v), fx, dtype=dt)], axis=1), dt)      # [S, 3]
    lam = (np.arange(N_ROT).astype(dt) * dt(2.0 * PI / N_ROT))[None, :]
    sl, cl = np.sin(lam), np.cos(lam)
    k1 = vp1[:, 0:1] * sl + vp1[:, 1:2] * cl
    k2 = vp1[:, 2:3]
    with np.errstate(divide="ignore"):
        phi = np.arctan(-k2 / k1)
    sp = np.sin(phi)
    vp2 = _unit(np.stack([sp * sl, sp * cl, np.cos(phi)], axis=-1), dt)
    vp2 = np.where((vp2[..., 2] < 0)[..., None], vp2 * dt(-1.0), vp2)
    vp3 = _unit(cross(np.broadcast_to(vp1[:, None, :], vp2.shape), vp2), dt)
    vp3 = np.where((vp3[..., 2] < 0)[..., None], vp3 * dt(-1.0), vp3)
    hyp = np.stack([np.broadcast_to(vp1[:, None, :], vp2.shape), vp2, vp3], axis=2)
    return hyp.reshape(N_HYP, 3, 3)


def snap_cell(angle, n):
    """-> (cell, q): q = angle / DEG; within SNAP of an integer -> that integer, otherwise truncated; clamped to n - 1.  Not q >= 0 -> cell 0."""
    dt = angle.dtype.type
    q = angle / dt(DEG)
    bad = ~(q >= 0)
    qq = np.where(bad, dt(0), q)
    r = np.rint(qq)
    c = np.where(np.abs(qq - r) <= dt(SNAP), r, np.trunc(qq)).astype(np.int64)
    return np.minimum(c, n - 1), q


def edge_distance(q):
    """Distance (in cells) of a quotient from the edge of the cell rule: the edges lie SNAP below the integers."""
    q = np.asarray(q, dtype=np.float64)
    return np.abs(q - (np.rint(q) - SNAP))


def vote(para, length, ori, cam, dt=np.float64):
    """-> raw grid [LA, LO], pair_cell [n (n - 1) / 2] (-1: did not vote), q_la, q_lo of every pair (nan where z == 0)  (:2104-2148)."""
    fx, fy, cx, cy = (dt(v) for v in cam)
    n = len(para)
    ii, jj = np.triu_indices(n, 1)
    pt = cross(para[ii], para[jj])
    nz = pt[:, 2] != 0
    z = np.where(nz, pt[:, 2], dt(1))
    X, Y, Z = pt[:, 0] / z - cx, pt[:, 1] / z - cy, fx
    N = np.sqrt(X * X + Y * Y + Z * Z)
    la, q_la = snap_cell(np.arccos(np.minimum(Z / N, dt(1.0))), LA)
    lo, q_lo = snap_cell(np.arctan2(X, Y) + dt(PI), LO)
    dev = np.abs(ori[ii] - ori[jj])
    dev = np.minimum(dt(PI) - dev, dev)
    keep = nz & ~(dev > dt(TOL60))
    w = np.sqrt(length[ii] * length[jj]) * (np.sin(dt(2.0) * dev) + dt(0.2))
    cell = la * LO + lo
    grid = np.zeros(LA * LO, dtype=dt)
    np.add.at(grid, cell[keep], w[keep])                 # unbuffered: added one by one in pair order, as the reference's loop does
    pair_cell = np.where(keep, cell, -1)
    return grid.reshape(LA, LO), pair_cell, np.where(nz, q_la, np.nan), np.where(nz, q_lo, np.nan)


def smooth(grid):
    """:2151-2173: g + (3 x 3 sum, row by row) / 9; border rows and columns zero."""
    dt = grid.dtype.type
    total = np.zeros((LA - 2, LO - 2), dtype=grid.dtype)
    for m in range(3):
        for k in range(3):
            total = total + grid[m:m + LA - 2, k:k + LO - 2]
    out = np.zeros_like(grid)
    out[1:-1, 1:-1] = grid[1:-1, 1:-1] + total / dt(9)
    return out


def score(hyp, g):
    """-> cells [N_HYP, 3] (-1: z == 0, skipped), scores, q_la, q_lo  (:2183-2214)."""
    dt = hyp.dtype.type
    z = hyp[..., 2]
    la, q_la = snap_cell(np.arccos(np.minimum(z, dt(1.0))), LA)
    lo, q_lo = snap_cell(np.arctan2(hyp[..., 0], hyp[..., 1]) + dt(PI), LO)
    cells = np.where(z != 0, la * LO + lo, -1)
    gv = np.where(cells >= 0, g.ravel()[np.maximum(cells, 0)], dt(0))
    sc = ((dt(0) + gv[:, 0]) + gv[:, 1]) + gv[:, 2]
    return cells, sc, q_la, q_lo


def tags(segs, vps, cam, th, dt=np.float64):
    """lines2Vps (:2232-2299) and the per-line vector (:379-385) -> tag, line_vp, angles [n, 3]."""
    fx, fy, cx, cy = (dt(v) for v in cam)
    s = np.asarray(segs, dtype=np.float64).reshape(-1, 4).astype(dt)
    x1, y1, x2, y2 = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    px = vps[:, 0] * fx / vps[:, 2] + cx
    py = vps[:, 1] * fy / vps[:, 2] + cy
    xm, ym = (x1 + x2) / dt(2.0), (y1 + y2) / dt(2.0)
    ax, ay = x1 - x2, y1 - y2
    n1 = np.sqrt(ax * ax + ay * ay)
    ax, ay = ax / n1, ay / n1
    ang = np.zeros((len(s), 3), dtype=dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(3):
            bx, by = px[j] - xm, py[j] - ym
            n2 = np.sqrt(bx * bx + by * by)
            bx, by = bx / n2, by / n2
            cv = ax * bx + ay * by
            cv = np.where(cv > 1, dt(1.0), cv)
            cv = np.where(cv < -1, dt(-1.0), cv)
            a = np.arccos(cv)
            ang[:, j] = np.where(a < dt(PI) - a, a, dt(PI) - a)
    tag = np.full(len(s), 3, np.int32)
    mn = np.full(len(s), dt(1000.0))
    bi = np.zeros(len(s), np.int32)
    for j in range(3):
        lt = ang[:, j] < mn
        mn = np.where(lt, ang[:, j], mn); bi = np.where(lt, j, bi)
    tag = np.where(mn < dt(th), bi, 3).astype(np.int32)
    unit = vps / vps[:, 2:3]
    line_vp = np.where((tag < 3)[:, None], unit[np.minimum(tag, 2)], dt(0))
    return tag, line_vp, ang


def estimate(segs, seed, cam, th=DEG, dt=np.float64, samples_from=None):
    """One frame.  -> dict: status, best_hypothesis, score, vps, n_tagged, tag, line_vp, and the intermediates (hyp, cells, scores, raw, smooth,
    pair_cell, the quotients, the tag angles).  `samples_from`: line parameters the z == 0 tests of the generator are taken with (float64)."""
    segs = np.asarray(segs, dtype=np.float64).reshape(-1, 4)
    n = len(segs)
    out = dict(status=OK, best_hypothesis=-1, score=0.0, vps=np.zeros((3, 3)), n_tagged=np.zeros(3, np.int32), tag=np.full(n, 3, np.int32),
               line_vp=np.zeros((n, 3)))
    if n < 2:
        out["status"] = TOO_FEW_LINES
        return out
    para, length, ori = line_params(segs, dt)
    smp = samples(seed, line_params(segs)[0])
    if smp is None:
        out["status"] = NO_HYPOTHESIS
        return out
    hyp = hypotheses(para, smp, cam, dt)
    raw, pair_cell, pq_la, pq_lo = vote(para, length, ori, cam, dt)
    g = smooth(raw)
    cells, sc, hq_la, hq_lo = score(hyp, g)
    best = int(np.argmax(sc))                   # the lowest index of the maximum; 0 when every score is 0
    vps = hyp[best]
    tag, line_vp, ang = tags(segs, vps, cam, th, dt)
    out.update(best_hypothesis=best, score=sc[best], vps=vps, tag=tag, line_vp=line_vp, n_tagged=np.bincount(tag, minlength=4)[:3].astype(np.int32),
               hyp=hyp, cells=cells, scores=sc, raw=raw, smooth=g, pair_cell=pair_cell, samples=smp, pair_q=(pq_la, pq_lo), hyp_q=(hq_la, hq_lo),
               angles=ang)
    return out


def best_margin(r):
    """How decided the argmax is.  -> (set_margin, triple_margin): the relative gap between the best score and the best score of a hypothesis
    whose SET of non-empty cells differs / whose ordered cell triple differs (inf when there is none)."""
    sc = np.asarray(r["scores"], dtype=np.float64); cells = r["cells"]; g = np.asarray(r["smooth"], dtype=np.float64).ravel()
    b = r["best_hypothesis"]
    if not sc[b] > 0:
        return 0.0, 0.0
    ne = np.where((cells >= 0) & (g[np.maximum(cells, 0)] != 0), cells, -1)
    key = np.sort(ne, axis=1)
    # a set, not a multiset: collapse repeats
    key[:, 1] = np.where(key[:, 1] == key[:, 0], -1, key[:, 1]); key[:, 2] = np.where((key[:, 2] == key[:, 1]) | (key[:, 2] == key[:, 0]), -1, key[:, 2])
    key = np.sort(key, axis=1)
    other_set = ~(key == key[b]).all(axis=1)
    other_triple = ~(cells == cells[b]).all(axis=1)
    f = lambda m: float((sc[b] - sc[m].max()) / sc[b]) if m.any() else float("inf")
    return f(other_set), f(other_triple)


def tag_margin(r, th=DEG):
    """Per line: min(|smallest angle - th|, gap between the two smallest angles), radians."""
    a = np.sort(np.asarray(r["angles"], dtype=np.float64), axis=1)
    return np.minimum(np.abs(a[:, 0] - th), a[:, 1] - a[:, 0])
