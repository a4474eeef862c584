"""The numpy restatement of uvs_ft_reject (include/uvs_solver.h states the rule; csrc/uvs_feature_reject.hip is held to this file bit for bit):
FeatureTracker::rejectWithF (reference feature_tracker/src/feature_tracker.cpp:149-182), i.e. cv::findFundamentalMat(.., FM_RANSAC, F_THRESHOLD,
0.99, status) on the normalized points, with the threshold F_THRESHOLD / FOCAL_LENGTH.

TEST INFRASTRUCTURE ONLY.  OpenCV is not a dependency, so this file is the pin, as tests/lc_ref.py is for the PnP-RANSAC.  Every FP64 operation
is one of + - * / sqrt in the order written here (numpy does not contract), the one log is in update_num_iters.

  sample     hypothesis h = 0 .. 999: z = mix64(seed + 0x9E3779B97F4A7C15 (1 + (h << 20) + a)), index z % n, a = 0, 1, ..; a duplicate is
             skipped; 7 distinct indices within 64 draws or the hypothesis is invalid (tests/lc_ref.py: draw, with 7)
  null space row [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1]; Gauss-Jordan on the 7 x 9 matrix with complete pivoting, no row or column is
             moved: step k takes the largest |a| over the rows and columns that hold no pivot yet (strict >, rows ascending, then columns
             ascending: ties go to the lowest row, then the lowest column); not |p| > 1e-10 |first pivot| -> invalid; the pivot row's other
             free-column entries are divided by p, then f = a[r][pc] times the pivot row is subtracted from each of the other six rows r, over
             the same columns.  With c1 < c2 the two columns left: F1 has 1 at c1, 0 at c2 and -a[row][c1] at each row's pivot column; F2 the same
             with c2
  cubic      det(F1 + l F2) = c0 + c1 l + c2 l^2 + c3 l^3 from the eight determinants of columns taken from F1 (A) or F2 (B):
             det3(u, v, w) = (u0 (v1 w2 - v2 w1) - u1 (v0 w2 - v2 w0)) + u2 (v0 w1 - v1 w0);  c0 = AAA, c1 = (BAA + ABA) + AAB,
             c2 = (BBA + BAB) + ABB, c3 = BBB;  p(x) = ((c3 x + c2) x + c1) x + c0
  roots      invalid unless c0 .. c3 are finite, c3 != 0 and R = 1 + max(|c0|, |c1|, |c2|) / |c3| is finite.  D = c2 c2 - (3 c3) c1; D > 0:
             s = sqrt(D), e = (-c2 -+ s) / (3 c3), both clamped to [-R, R], lo = min, hi = max, intervals [-R, lo], [lo, hi], [hi, R];
             otherwise [-R, R] alone.  An interval [a, b] holds a root iff (p(a) <= 0 and p(b) > 0) or (p(a) >= 0 and p(b) < 0).  60 times:
             m = 0.5 a + 0.5 b; b = m if p(m) is strictly on b's side of 0, else a = m.  x = 0.5 a + 0.5 b, then 4 times
             x' = x - p(x) / (((3 c3) x + 2 c2) x + c1), taken iff a <= x' <= b.  Roots are numbered in ascending interval order
  error      F = F1 + l F2 entry by entry; a = (F0 x1 + F1 y1) + F2, b, c alike from rows 1, 2; s2 = (x2 a + y2 b) + c; d2 = s2 s2 / (a a + b b);
             d1 the same with the transpose and the points swapped; inlier iff d1 <= t t and d2 <= t t (a NaN is an outlier)
  selection  OpenCV's sequential rule, h-major then r: h >= niters ends the loop; count > max(best, 6) makes (h, r) the best and
             niters = RANSACUpdateNumIters(confidence, (n - count) / n, 7, niters) with (1 - ep)^7 by six multiplications
"""
import numpy as np

N_HYP = 1000
MODEL_POINTS = 7
MAX_ATTEMPTS = 64
PIVOT_REL = 1e-10
BISECTIONS = 60
NEWTON = 4
GOLD = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
OK, SKIPPED, NO_MODEL = 0, 1, 2
TINY = float(np.finfo(np.float64).tiny)


# ---------------------------------------------------------------- sample
def mix64(z):
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 & M64
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB & M64
    return z ^ (z >> 31)


def draw(seed, h, n):
    """The 7 track indices of hypothesis h, or None (invalid)."""
    idx = []
    if n < 1:
        return None
    for a in range(MAX_ATTEMPTS):
        v = mix64((seed + GOLD * (1 + (h << 20) + a)) & M64) % n
        if v not in idx:
            idx.append(v)
            if len(idx) == MODEL_POINTS:
                return idx
    return None


def samples(seed, n):
    """-> [1000, 7] int32, a row of -1 where the hypothesis is invalid."""
    S = -np.ones((N_HYP, MODEL_POINTS), np.int32)
    for h in range(N_HYP):
        d = draw(seed & M64, h, n)
        if d is not None:
            S[h] = d
    return S


# ---------------------------------------------------------------- null space
def rows(prev, nxt, S):
    """prev, nxt [n, 2], S [H, 7] -> A [H, 7, 9]."""
    x1, y1 = prev[S, 0], prev[S, 1]
    x2, y2 = nxt[S, 0], nxt[S, 1]
    return np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], -1)


def null_space(A):
    """A [H, 7, 9] -> F1 [H, 9], F2 [H, 9], valid [H]."""
    A = np.array(A, np.float64)
    H = A.shape[0]
    hh = np.arange(H)
    row_free = np.ones((H, 7), bool); col_free = np.ones((H, 9), bool)
    prow = np.zeros((H, 7), np.int64); pcol = np.zeros((H, 7), np.int64)
    valid = np.ones(H, bool)
    first = np.zeros(H)
    with np.errstate(all="ignore"):
        for k in range(7):
            mag = np.where(row_free[:, :, None] & col_free[:, None, :], np.abs(A), -1.0)
            mag = np.where(np.isnan(mag), -1.0, mag)                     # a strict > never takes a NaN
            flat = np.argmax(mag.reshape(H, 63), 1)                      # the first maximum in row-major order
            pr, pc = flat // 9, flat % 9
            p = A[hh, pr, pc]
            if k == 0:
                first = np.abs(p)
            valid &= np.abs(p) > PIVOT_REL * first
            row_free[hh, pr] = False; col_free[hh, pc] = False
            prow[:, k] = pr; pcol[:, k] = pc
            piv = np.where(col_free, A[hh, pr, :] / p[:, None], A[hh, pr, :])      # the pivot row over the columns still free
            A[hh, pr, :] = piv
            A[hh, pr, pc] = 1.0
            f = A[hh, :, pc].copy()                                      # [H, 7]
            upd = A - f[:, :, None] * piv[:, None, :]
            other = np.ones((H, 7), bool); other[hh, pr] = False
            A = np.where(other[:, :, None] & col_free[:, None, :], upd, A)
            z = A[hh, :, pc]; z = np.where(other, 0.0, z); A[hh, :, pc] = z
        free = np.argsort(~col_free, 1, kind="stable")[:, :2]            # the two columns left, ascending
        c1, c2 = free[:, 0], free[:, 1]
        F1 = np.zeros((H, 9)); F2 = np.zeros((H, 9))
        for k in range(7):
            F1[hh, pcol[:, k]] = -A[hh, prow[:, k], c1]
            F2[hh, pcol[:, k]] = -A[hh, prow[:, k], c2]
        F1[hh, c1] = 1.0; F1[hh, c2] = 0.0; F2[hh, c1] = 0.0; F2[hh, c2] = 1.0
    return F1, F2, valid


# ---------------------------------------------------------------- cubic
def det3(u, v, w):
    return (u[0] * (v[1] * w[2] - v[2] * w[1]) - u[1] * (v[0] * w[2] - v[2] * w[0])) + u[2] * (v[0] * w[1] - v[1] * w[0])


def cubic(F1, F2):
    """-> c [H, 4]: c0 .. c3."""
    A = [[F1[:, 0 + j], F1[:, 3 + j], F1[:, 6 + j]] for j in range(3)]       # the columns
    B = [[F2[:, 0 + j], F2[:, 3 + j], F2[:, 6 + j]] for j in range(3)]
    with np.errstate(all="ignore"):
        c0 = det3(A[0], A[1], A[2])
        c1 = (det3(B[0], A[1], A[2]) + det3(A[0], B[1], A[2])) + det3(A[0], A[1], B[2])
        c2 = (det3(B[0], B[1], A[2]) + det3(B[0], A[1], B[2])) + det3(A[0], B[1], B[2])
        c3 = det3(B[0], B[1], B[2])
    return np.stack([c0, c1, c2, c3], -1)


def poly(c, x):
    return ((c[..., 3] * x + c[..., 2]) * x + c[..., 1]) * x + c[..., 0]


def roots(c):
    """c [H, 4] -> lam [H, 3] (0 where there is none), n_roots [H], valid [H]: the roots fill lam from the front."""
    H = c.shape[0]
    with np.errstate(all="ignore"):
        c0, c1, c2, c3 = (c[:, i] for i in range(4))
        m = np.abs(c0); m = np.where(np.abs(c1) > m, np.abs(c1), m); m = np.where(np.abs(c2) > m, np.abs(c2), m)
        R = 1.0 + m / np.abs(c3)
        valid = np.isfinite(c).all(1) & (c3 != 0.0) & np.isfinite(R)
        D = c2 * c2 - (3.0 * c3) * c1
        three = D > 0.0
        s = np.sqrt(np.where(three, D, 0.0))
        e1 = (-c2 - s) / (3.0 * c3); e2 = (-c2 + s) / (3.0 * c3)
        e1 = np.where(e1 < -R, -R, e1); e1 = np.where(e1 > R, R, e1)
        e2 = np.where(e2 < -R, -R, e2); e2 = np.where(e2 > R, R, e2)
        lo = np.where(e2 < e1, e2, e1); hi = np.where(e2 < e1, e1, e2)
        a = np.stack([-R, np.where(three, lo, -R), np.where(three, hi, -R)], -1)      # [H, 3]
        b = np.stack([np.where(three, lo, R), np.where(three, hi, R), R], -1)
        live = np.stack([np.ones(H, bool), three, three], -1) & valid[:, None]
        cc = c[:, None, :]
        fa = poly(cc, a); fb = poly(cc, b)
        up = (fa <= 0.0) & (fb > 0.0); down = (fa >= 0.0) & (fb < 0.0)
        has = live & (up | down)
        for _ in range(BISECTIONS):
            mid = 0.5 * a + 0.5 * b
            fm = poly(cc, mid)
            to_b = np.where(up, fm > 0.0, fm < 0.0)
            b = np.where(to_b, mid, b); a = np.where(to_b, a, mid)
        x = 0.5 * a + 0.5 * b
        for _ in range(NEWTON):
            d = ((3.0 * cc[..., 3]) * x + 2.0 * cc[..., 2]) * x + cc[..., 1]
            xn = x - poly(cc, x) / d
            x = np.where((xn >= a) & (xn <= b), xn, x)
    lam = np.zeros((H, 3)); n_roots = has.sum(1)
    order = np.argsort(~has, 1, kind="stable")                               # the intervals with a root first, in ascending order
    xs = np.take_along_axis(x, order, 1)
    for r in range(3):
        lam[:, r] = np.where(r < n_roots, xs[:, r], 0.0)
    return lam, n_roots, valid


# ---------------------------------------------------------------- error
def errors(F, prev, nxt):
    """F [..., 9], prev, nxt [n, 2] -> d1, d2 [..., n]."""
    F = np.asarray(F, np.float64)[..., None, :]
    x1, y1, x2, y2 = prev[:, 0], prev[:, 1], nxt[:, 0], nxt[:, 1]
    with np.errstate(all="ignore"):
        a = (F[..., 0] * x1 + F[..., 1] * y1) + F[..., 2]
        b = (F[..., 3] * x1 + F[..., 4] * y1) + F[..., 5]
        c = (F[..., 6] * x1 + F[..., 7] * y1) + F[..., 8]
        s2 = (x2 * a + y2 * b) + c
        d2 = s2 * s2 / (a * a + b * b)
        a = (F[..., 0] * x2 + F[..., 3] * y2) + F[..., 6]
        b = (F[..., 1] * x2 + F[..., 4] * y2) + F[..., 7]
        c = (F[..., 2] * x2 + F[..., 5] * y2) + F[..., 8]
        s1 = (x1 * a + y1 * b) + c
        d1 = s1 * s1 / (a * a + b * b)
    return d1, d2


def inliers(F, prev, nxt, threshold):
    d1, d2 = errors(F, prev, nxt)
    t2 = np.float64(threshold) * np.float64(threshold)
    with np.errstate(all="ignore"):
        return (d1 <= t2) & (d2 <= t2)


# ---------------------------------------------------------------- selection
def num_over_denom(p, ep):
    """num / denom of RANSACUpdateNumIters, or None where the quotient is not formed."""
    p = min(max(p, 0.0), 1.0); ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, TINY)
    w = 1.0 - ep
    q = w
    for _ in range(MODEL_POINTS - 1):
        q = q * w
    denom = 1.0 - q
    if denom < TINY:
        return None, None
    return float(np.log(num)), float(np.log(denom))


def update_num_iters(p, ep, max_iters):
    """OpenCV RANSACUpdateNumIters (cvRound = round half to even), model_points = 7."""
    num, denom = num_over_denom(p, ep)
    if num is None:
        return 0
    return max_iters if (denom >= 0 or -num >= max_iters * (-denom)) else int(np.rint(num / denom))


def select(counts, n, confidence, half_margins=None):
    """counts [1000, 3] (-1: none), n tracks -> (best hypothesis or -1, its root or -1, its count, hypotheses examined).  half_margins: a list
    that receives |frac(num / denom) - 0.5| of every quotient formed (how close the rounding of the one log-dependent value lies to a tie)."""
    bh, br, best, niters, h = -1, -1, 0, N_HYP, 0
    while h < niters:
        for r in range(3):
            c = int(counts[h][r])
            if c > max(best, MODEL_POINTS - 1):
                bh, br, best = h, r, c
                ep = float(np.float64(n - c) / np.float64(n))
                if half_margins is not None:
                    num, denom = num_over_denom(confidence, ep)
                    if num is not None and denom < 0:
                        q = num / denom
                        half_margins.append(abs((q - np.floor(q)) - 0.5))
                niters = update_num_iters(confidence, ep, niters)
        h += 1
    return bh, br, best, h


# ---------------------------------------------------------------- one item
def reject(prev, nxt, seed, threshold, confidence=0.99):
    """prev, nxt [n, 2] float64 normalized points -> dict with the fields of uvs_ft_reject_result, keep [n] uint8, and what uvs_ft_debug_reject
    returns: samples [1000, 7] int32, models [1000, 3, 9] float64 (0 where there is none), counts [1000, 3] int32 (-1 where there is none);
    half_margin: the smallest distance of a num / denom of the stopping rule from a half-integer (inf if none was formed)."""
    prev = np.ascontiguousarray(prev, np.float64).reshape(-1, 2); nxt = np.ascontiguousarray(nxt, np.float64).reshape(-1, 2)
    n = len(prev)
    out = dict(status=SKIPPED, n_inliers=n, hypothesis=-1, root=-1, iterations=0, F=np.zeros(9), keep=np.ones(n, np.uint8),
               samples=-np.ones((N_HYP, MODEL_POINTS), np.int32), models=np.zeros((N_HYP, 3, 9)), counts=-np.ones((N_HYP, 3), np.int32),
               half_margin=np.inf, pivot_valid=np.zeros(N_HYP, bool))
    if n < 8:
        return out
    S = samples(int(seed), n)
    ok = S[:, 0] >= 0
    Sc = np.where(ok[:, None], S, 0)
    F1, F2, valid = null_space(rows(prev, nxt, Sc))
    out["pivot_valid"] = valid & ok
    lam, n_roots, cvalid = roots(cubic(F1, F2))
    valid = valid & cvalid & ok
    n_roots = np.where(valid, n_roots, 0)
    with np.errstate(all="ignore"):
        models = F1[:, None, :] + lam[:, :, None] * F2[:, None, :]
    has = np.arange(3)[None, :] < n_roots[:, None]
    models = np.where(has[:, :, None], models, 0.0)
    mask = inliers(models, prev, nxt, threshold) & has[:, :, None]           # [1000, 3, n]
    counts = np.where(has, mask.sum(-1), -1).astype(np.int32)
    margins = []
    bh, br, best, iters = select(counts, n, float(confidence), margins)
    out.update(samples=S, models=models, counts=counts, iterations=iters, half_margin=min(margins) if margins else np.inf)
    if bh < 0:
        out["status"] = NO_MODEL
        return out
    F = models[bh, br]
    k = int(np.argmax(np.abs(F)))                                            # the first entry of largest magnitude
    with np.errstate(all="ignore"):
        out.update(status=OK, n_inliers=best, hypothesis=bh, root=br, F=F / F[k], keep=mask[bh, br].astype(np.uint8))
    return out
