"""The relative pose of a frame pair (include/uvs_solver.h: uvs_rp_*, which states the rule; csrc/uvs_relative_pose.hip), twice:

  * the FP64 numpy restatement of steps 1, 2 and 4 to 6 of the rule (Estimator::relativePose, estimator.cpp:448-477; solveRelativeRT and the
    recoverPose / decomposeEssentialMat of initial/solve_5pts.cpp), with step 3, the RANSAC, through tests/fr_ref.py.  Steps 1 to 3 are the pin:
    the device is held to them bit for bit.  The SVDs of steps 4 and 5 are numpy.linalg.svd, as the reference's are OpenCV's;
  * a 60-digit mpmath evaluation of steps 4 to 6 on the same F and RANSAC mask (`recover_hp`): the truth the device and the restatement are both
    measured against, with the margin of every comparison it makes.  The restatement's largest error on a case is that case's E_ref.

The SVD of F is unique only up to signs, and the order of the four candidates -- hence good[] and `chosen` -- depends on them, so the rule fixes
them (`fix_signs`): each right singular vector has its entry of largest magnitude positive, u_k = F v_k / s_k for k = 0, 1, and u_2 = +-(u_0 x u_1)
with its entry of largest magnitude positive.  The `defect` arguments plant the wrong formulas of tests/test_rp_ref.py; nothing else passes them.

TEST INFRASTRUCTURE ONLY."""
import mpmath
import numpy as np

import fr_ref

mp = mpmath.mp
DPS = 60
EPS = 2.0 ** -53
OK, FEW_CORRES, LOW_PARALLAX, FEW_POINTS, NO_MODEL, FEW_INLIERS = range(6)
PARAMS = dict(focal_length=460.0, min_parallax_px=30.0, f_threshold=0.3 / 460, confidence=0.99, max_depth=50.0, min_corres=20,
              min_ransac_points=15, min_inliers=12)
DEFECTS = ("both_wt", "no_det_flip", "no_x_depth", "no_minus_t", "translation_rt", "strict_choice")
METRICS = ("R", "t", "Rotation", "Translation")


# ---------------------------------------------------------------- steps 1, 2
def gate(left, right, params=PARAMS):
    """-> (status, average_parallax): the sum runs in item order, one addition per track."""
    n = len(left)
    s = np.float64(0.0)
    for i in range(n):
        dx = left[i, 0] - right[i, 0]; dy = left[i, 1] - right[i, 1]
        s = s + np.sqrt(dx * dx + dy * dy)
    avg = s / np.float64(n) if n else np.float64(0.0)
    if not n > params["min_corres"]:
        return FEW_CORRES, float(avg)
    if not avg * np.float64(params["focal_length"]) > params["min_parallax_px"]:
        return LOW_PARALLAX, float(avg)
    if not n >= params["min_ransac_points"]:
        return FEW_POINTS, float(avg)
    return OK, float(avg)


def round32(a):
    """cv::Point2f: to float32 (nearest even) and back."""
    return np.ascontiguousarray(a, np.float64).astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------- step 4
def _sign_of_largest(v):
    return -1.0 if v[int(np.argmax(np.abs(v)))] < 0 else 1.0          # argmax: the first entry of largest magnitude


def fix_signs(U, Vt):
    """The rule's signs on an SVD F = U diag(s) Vt with s descending -> (U, Vt), copies."""
    U = np.array(U, np.float64); Vt = np.array(Vt, np.float64)
    for k in range(2):
        sg = _sign_of_largest(Vt[k])
        Vt[k] = sg * Vt[k]; U[:, k] = sg * U[:, k]
    Vt[2] = _sign_of_largest(Vt[2]) * Vt[2]
    c = np.cross(U[:, 0], U[:, 1])
    U[:, 2] = _sign_of_largest(c) * c
    return U, Vt


W = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def decompose(F, defect=None):
    """-> R1, R2, t of decomposeEssentialMat under the rule's signs."""
    U, _, Vt = np.linalg.svd(np.asarray(F, np.float64).reshape(3, 3))
    U, Vt = fix_signs(U, Vt)
    if defect != "no_det_flip":
        if np.linalg.det(U) < 0:
            U = -U
        if np.linalg.det(Vt) < 0:
            Vt = -Vt
    R1 = U @ (W.T if defect == "both_wt" else W) @ Vt
    R2 = U @ W.T @ Vt
    return R1, R2, U[:, 2].copy()


# ---------------------------------------------------------------- step 5
def triangulation_matrices(R, t, left, right):
    """[n, 4, 4]: OpenCV's triangulatePoints rows for P0 = [I | 0], P = [R | t]."""
    n = len(left)
    P = np.concatenate([R, t[:, None]], 1)
    A = np.zeros((n, 4, 4))
    A[:, 0, 0] = -1.0; A[:, 0, 2] = left[:, 0]
    A[:, 1, 1] = -1.0; A[:, 1, 2] = left[:, 1]
    A[:, 2] = right[:, 0:1] * P[2] - P[0]
    A[:, 3] = right[:, 1:2] * P[2] - P[1]
    return A


def cheirality(R, t, left, right, keep, max_depth, defect=None):
    """-> m [n] bool of one candidate."""
    if len(left) == 0:
        return np.zeros(0, bool)
    Q = np.linalg.svd(triangulation_matrices(R, t, left, right))[2][:, 3, :]
    with np.errstate(all="ignore"):
        m = Q[:, 2] * Q[:, 3] > 0
        X = Q[:, :3] / Q[:, 3:4]
        if defect != "no_x_depth":
            m &= X[:, 2] < max_depth
        Y2 = X @ R[2] + t[2]
        m &= (Y2 > 0) & (Y2 < max_depth)
    return m & (np.asarray(keep) != 0)


# ---------------------------------------------------------------- step 6
def choose(good, strict=False):
    """The chain of solve_5pts.cpp:152-181 (strict: the planted defect, > in place of >=)."""
    ge = (lambda a, b: a > b) if strict else (lambda a, b: a >= b)
    g = [int(v) for v in good]
    if ge(g[0], g[1]) and ge(g[0], g[2]) and ge(g[0], g[3]):
        return 0
    if ge(g[1], g[0]) and ge(g[1], g[2]) and ge(g[1], g[3]):
        return 1
    if ge(g[2], g[0]) and ge(g[2], g[1]) and ge(g[2], g[3]):
        return 2
    return 3


def candidates(R1, R2, t, defect=None):
    return [(R1, t), (R2, t), (R1, t if defect == "no_minus_t" else -t), (R2, t if defect == "no_minus_t" else -t)]


def recover(F, keep, left, right, params=PARAMS, defect=None):
    """Steps 4 to 6 on the rounded points -> dict(good [4], chosen, inlier_cnt, ok, mask [n] uint8, R, t, Rotation, Translation)."""
    R1, R2, t = decompose(F, defect)
    cand = candidates(R1, R2, t, defect)
    masks = [cheirality(R, tt, left, right, keep, params["max_depth"], defect) for R, tt in cand]
    good = np.array([int(m.sum()) for m in masks], np.int32)
    k = choose(good, strict=defect == "strict_choice")
    R, tt = cand[k]
    cnt = int(good[k])
    return dict(good=good, chosen=k, inlier_cnt=cnt, ok=int(cnt > params["min_inliers"]), mask=masks[k].astype(np.uint8), R=R.copy(), t=tt.copy(),
                Rotation=R.T.copy(), Translation=(-(R @ tt) if defect == "translation_rt" else -(R.T @ tt)))


def _nothing(n):
    return dict(good=np.zeros(4, np.int32), chosen=-1, inlier_cnt=0, ok=0, mask=np.zeros(n, np.uint8), R=np.zeros((3, 3)), t=np.zeros(3),
                Rotation=np.zeros((3, 3)), Translation=np.zeros(3))


def relative_pose(left, right, seed, params=PARAMS, defect=None, recover_fn=recover):
    """One item through the whole rule -> dict with the fields of uvs_rp_item_result (the RANSAC's under their uvs_ft_reject_result names, its
    mask as `keep`) and `mask`.  recover_fn: `recover` or `recover_hp`."""
    left = np.ascontiguousarray(left, np.float64).reshape(-1, 2); right = np.ascontiguousarray(right, np.float64).reshape(-1, 2)
    n = len(left)
    status, avg = gate(left, right, params)
    out = dict(status=status, n=n, average_parallax=avg, ransac_status=fr_ref.SKIPPED, n_inliers=0, hypothesis=-1, root=-1, iterations=0, F=np.zeros(9),
               keep=np.zeros(n, np.uint8), **_nothing(n))
    if status != OK:
        return out
    l32, r32 = round32(left), round32(right)
    fr = fr_ref.reject(l32, r32, seed, params["f_threshold"], params["confidence"])
    out.update(ransac_status=fr["status"], n_inliers=fr["n_inliers"], hypothesis=fr["hypothesis"], root=fr["root"], iterations=fr["iterations"], F=fr["F"],
               keep=fr["keep"], half_margin=fr["half_margin"])
    if fr["status"] != fr_ref.OK or not np.linalg.svd(fr["F"].reshape(3, 3), compute_uv=False)[1] > 0:      # no model, or one of rank < 2
        out["status"] = NO_MODEL
        return out
    rec = recover_fn(fr["F"], fr["keep"], l32, r32, params) if defect is None else recover_fn(fr["F"], fr["keep"], l32, r32, params, defect)
    out.update(rec)
    out["status"] = OK if rec["ok"] else FEW_INLIERS
    return out


def window_l(frame_l, ok):
    """The window-level answer: frame_l of the first item with ok, or -1."""
    for f, o in zip(frame_l, ok):
        if o:
            return int(f)
    return -1


# ---------------------------------------------------------------- 60 digits
def _M(a):
    return mp.matrix(np.asarray(a, float).tolist())


def _sign_hp(v):
    k = max(range(len(v)), key=lambda i: (abs(v[i]), -i))
    return -1 if v[k] < 0 else 1


def _sign_margin(v):
    """How far the sign choice of a vector is from flipping: (largest - second largest magnitude) / largest, or 1 where both have one sign."""
    a = sorted(range(len(v)), key=lambda i: -abs(v[i]))
    if (v[a[0]] < 0) == (v[a[1]] < 0):
        return 1.0
    return float((abs(v[a[0]]) - abs(v[a[1]])) / abs(v[a[0]]))


def decompose_hp(F):
    """-> R1, R2, t as mp matrices, info dict(sv [3] floats, sign_margin)."""
    U, S, Vt = mp.svd_r(_M(np.asarray(F, float).reshape(3, 3)))
    order = sorted(range(3), key=lambda i: -S[i])
    u = [[U[r, k] for r in range(3)] for k in order]; v = [[Vt[k, c] for c in range(3)] for k in order]
    margins = []
    for k in range(2):
        margins.append(_sign_margin(v[k]))
        sg = _sign_hp(v[k])
        v[k] = [sg * x for x in v[k]]; u[k] = [sg * x for x in u[k]]
    margins.append(_sign_margin(v[2]))
    sg = _sign_hp(v[2]); v[2] = [sg * x for x in v[2]]
    c = [u[0][1] * u[1][2] - u[0][2] * u[1][1], u[0][2] * u[1][0] - u[0][0] * u[1][2], u[0][0] * u[1][1] - u[0][1] * u[1][0]]
    margins.append(_sign_margin(c))
    sg = _sign_hp(c); u[2] = [sg * x for x in c]
    Um = mp.matrix(3, 3); Vm = mp.matrix(3, 3)
    for k in range(3):
        for r in range(3):
            Um[r, k] = u[k][r]; Vm[k, r] = v[k][r]
    if mp.det(Um) < 0:
        Um = -Um
    if mp.det(Vm) < 0:
        Vm = -Vm
    Wm = _M(W)
    return Um * Wm * Vm, Um * Wm.T * Vm, mp.matrix([Um[0, 2], Um[1, 2], Um[2, 2]]), dict(sv=[float(S[i]) for i in order], sign_margin=min(margins))


def cheirality_hp(R, t, left, right, keep, max_depth):
    """-> (m [n] bool, margin [n]: the smallest relative margin of the point's four comparisons, gap [n]: the distance of the two smallest
    singular values of its matrix relative to the largest)."""
    n = len(left)
    m = np.zeros(n, bool); margin = np.zeros(n); gap = np.zeros(n)
    md = mp.mpf(max_depth)
    P = [[R[r, 0], R[r, 1], R[r, 2], t[r]] for r in range(3)]
    for i in range(n):
        x1, y1, x2, y2 = (mp.mpf(float(v)) for v in (left[i, 0], left[i, 1], right[i, 0], right[i, 1]))
        A = mp.matrix(4, 4)
        A[0, 0] = -1; A[0, 2] = x1; A[1, 1] = -1; A[1, 2] = y1
        for c in range(4):
            A[2, c] = x2 * P[2][c] - P[0][c]; A[3, c] = y2 * P[2][c] - P[1][c]
        _, S, Vt = mp.svd_r(A)
        order = sorted(range(4), key=lambda j: S[j])
        k = order[0]
        Q = [Vt[k, c] for c in range(4)]
        gap[i] = float((S[order[1]] - S[order[0]]) / S[order[3]])
        if Q[3] == 0:
            m[i] = False; margin[i] = 0.0
            continue
        X = [Q[c] / Q[3] for c in range(3)]
        Y = [R[r, 0] * X[0] + R[r, 1] * X[1] + R[r, 2] * X[2] + t[r] for r in range(3)]
        m[i] = (Q[2] * Q[3] > 0) and (X[2] < md) and (Y[2] > 0) and (Y[2] < md)
        ny = mp.sqrt(Y[0] * Y[0] + Y[1] * Y[1] + Y[2] * Y[2])
        margin[i] = float(min(abs(Q[2] * Q[3]), abs(md - X[2]) / max(md, abs(X[2])), abs(Y[2]) / ny, abs(md - Y[2]) / max(md, abs(Y[2]))))
    return m & (np.asarray(keep) != 0), margin, gap


def recover_hp(F, keep, left, right, params=PARAMS):
    """Steps 4 to 6 at 60 digits -> the dict of `recover` (R, t, Rotation, Translation rounded to float64 at the end) plus sv [3], sign_margin,
    margin (the smallest comparison margin over every point and candidate), gap (the smallest singular-value gap alike)."""
    with mp.workdps(DPS):
        R1, R2, t, info = decompose_hp(F)
        cand = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
        res = [cheirality_hp(R, tt, left, right, keep, params["max_depth"]) for R, tt in cand]
        good = np.array([int(r[0].sum()) for r in res], np.int32)
        k = choose(good)
        R, tt = cand[k]
        f = lambda M: np.array([[float(M[r, c]) for c in range(M.cols)] for r in range(M.rows)])
        cnt = int(good[k])
        return dict(good=good, chosen=k, inlier_cnt=cnt, ok=int(cnt > params["min_inliers"]), mask=res[k][0].astype(np.uint8), R=f(R), t=f(tt).reshape(3),
                    Rotation=f(R.T), Translation=f(-(R.T * tt)).reshape(3), sv=info["sv"], sign_margin=info["sign_margin"],
                    margin=float(min(r[1].min() for r in res)) if len(left) else np.inf, gap=float(min(r[2].min() for r in res)) if len(left) else np.inf)


# ---------------------------------------------------------------- the error measures of the tests
def errors(got, hp):
    """The largest |entry| difference of R, t, Rotation and Translation."""
    return {k: float(np.abs(np.asarray(got[k], np.float64).reshape(-1) - np.asarray(hp[k]).reshape(-1)).max()) for k in METRICS}


def exact_mismatches(got, hp):
    """The exact quantities of steps 5 and 6 that differ (names), empty when all agree."""
    bad = [k for k in ("chosen", "inlier_cnt", "ok") if int(got[k]) != int(hp[k])]
    if not np.array_equal(np.asarray(got["good"]), hp["good"]):
        bad.append("good")
    if not np.array_equal(np.asarray(got["mask"], np.uint8), hp["mask"]):
        bad.append("mask")
    return bad


def within(err, e_ref):
    """The metrics that exceed 8 max(E_ref, 2^-53) (names), empty when all hold."""
    return [k for k in METRICS if not err[k] <= 8.0 * max(e_ref[k], EPS)]
