"""Independent numpy restatement of loop verification: KeyFrame::findConnection (reference pose_graph/src/keyframe.cpp:121-170,
200-256, 259-521) as uvs_lc_verify (csrc/uvs_loop_verify.hip) computes it.

TEST INFRASTRUCTURE ONLY.  The reference's cv::solvePnPRansac is restated with the numerics include/uvs_solver.h pins down (OpenCV is not a
dependency, so this file is the pin, as tests/pg_ref.py is for the pose graph):

  matching   per query i in order: the old keypoint of smallest Hamming distance over 256 bits, bestDist starting at 128, updated on a
             strict <, so ties keep the first index; kept when bestDist < 80.  Matches are numbered in query order.
  generator  z = mix64(seed + 0x9E3779B97F4A7C15 * (1 + (h << 20) + a)) (mod 2^64) with mix64 the splitmix64 finalizer; draw a = 0, 1, ..
             gives the match index z % n; a duplicate of an earlier draw of the same hypothesis is skipped; 5 distinct indices within
             64 draws or the hypothesis is invalid.
  LM         6-DoF, residual (x / z, y / z) - uv of p = R X + t, analytic Jacobian, left perturbation R <- Exp(dtheta) R, t <- t + dt;
             M = J^T J + lambda diag(J^T J), lambda0 = 1e-3, / 10 on a step that lowers the cost (strict <), x 10 otherwise; at most
             20 iterations; stops after a step with |delta| < FLT_EPSILON max(1, |t|).  A Cholesky pivot that is not > 0 and finite
             makes a hypothesis invalid (in the refinement it ends the iterations, keeping the pose).  A hypothesis whose initial cost is
             not finite is invalid.
  inlier     z > 0 and dx^2 + dy^2 <= (10 / 460)^2 (FP64).
  selection  OpenCV's sequential rule over the 100 counts in hypothesis order: h >= niters ends the loop; count > max(best, 4)
             makes h the best and niters = RANSACUpdateNumIters(0.99, (n - count) / n, 5, niters).  ransac_iters = hypotheses the loop
             examined.
  refine     the same LM on the chosen hypothesis's inliers from its pose; the reported inlier mask stays that hypothesis's mask.
"""
import numpy as np

MIN_LOOP_NUM = 25
N_HYP = 100
MODEL_POINTS = 5
MAX_ATTEMPTS = 64
LM_ITERS = 20
LAMBDA0 = 1e-3
FLT_EPSILON = float(np.finfo(np.float32).eps)
THRESH = 10.0 / 460.0
CONFIDENCE = 0.99
GOLD = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1

# the trace of uvs_lc_debug_pair (UVS_LC_TRACE_* of include/uvs_solver.h), which verify(trace=True) fills from this file's own FP64 run
TRACE_HEAD, TRACE_ITER = 32, 64
TRACE_REC = TRACE_HEAD + LM_ITERS * TRACE_ITER
TRACE_STAGE = (N_HYP + 1) * TRACE_REC
MAX_QUERY = 1024
TRACE_LEN = TRACE_STAGE + 1 + 6 * MAX_QUERY
_IU = np.triu_indices(6)

REASON = dict(ACCEPTED=0, NO_MATCHES=1, FEW_MATCHES=2, RANSAC_FAILED=3, FEW_INLIERS=4, YAW_GATE=5, T_GATE=6)


# ---------------------------------------------------------------- matching
def hamming(a, b):
    """a [..., 4], b [..., 4] uint64 -> popcount(a ^ b) summed over the 4 words."""
    return np.bitwise_count(np.bitwise_xor(a, b)).sum(-1).astype(np.int64)


def match(qdesc, odesc):
    """-> match_old [nq] int32: the old index of the first minimum distance if that distance < 80, else -1."""
    qdesc = np.asarray(qdesc, np.uint64).reshape(-1, 4); odesc = np.asarray(odesc, np.uint64).reshape(-1, 4)
    out = -np.ones(len(qdesc), np.int32)
    if len(qdesc) == 0 or len(odesc) == 0:
        return out
    d = hamming(qdesc[:, None, :], odesc[None, :, :])            # [nq, no]
    j = np.argmin(d, 1)                                          # first index of the minimum
    best = d[np.arange(len(qdesc)), j]
    out[best < 80] = j[best < 80]                                # (< 128 is implied)
    return out


# ---------------------------------------------------------------- generator
def mix64(z):
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 & M64
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB & M64
    return z ^ (z >> 31)


def draw(seed, h, n):
    """The 5 match indices of hypothesis h, or None (invalid)."""
    idx = []
    for a in range(MAX_ATTEMPTS):
        v = mix64((seed + GOLD * (1 + (h << 20) + a)) & M64) % n
        if v not in idx:
            idx.append(v)
            if len(idx) == MODEL_POINTS:
                return idx
    return None


# ---------------------------------------------------------------- geometry
def skew(w):
    w = np.asarray(w)
    S = np.zeros(w.shape[:-1] + (3, 3))
    S[..., 0, 1] = -w[..., 2]; S[..., 0, 2] = w[..., 1]
    S[..., 1, 0] = w[..., 2]; S[..., 1, 2] = -w[..., 0]
    S[..., 2, 0] = -w[..., 1]; S[..., 2, 1] = w[..., 0]
    return S


def exp_so3(w):
    """Rodrigues; w [..., 3].  th^2 < 1e-20 takes the second-order series."""
    w = np.asarray(w, np.float64)
    th2 = (w * w).sum(-1)
    small = th2 < 1e-20
    th = np.sqrt(np.where(small, 1.0, th2))
    A = np.where(small, 1.0 - th2 / 6.0, np.sin(th) / th)
    B = np.where(small, 0.5 - th2 / 24.0, (1.0 - np.cos(th)) / np.where(small, 1.0, th2))
    K = skew(w)
    return np.eye(3) + A[..., None, None] * K + B[..., None, None] * (K @ K)


def residual_jacobian(R, t, X, uv):
    """R [H,3,3], t [H,3], X [H,m,3], uv [H,m,2] -> r [H,m,2], J [H,m,2,6] (columns dtheta, dt), z [H,m]."""
    RX = np.einsum("hij,hmj->hmi", R, X)
    p = RX + t[:, None, :]
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    iz = 1.0 / z
    r = np.stack([x * iz - uv[..., 0], y * iz - uv[..., 1]], -1)
    Dp = np.zeros(p.shape[:-1] + (2, 3))
    Dp[..., 0, 0] = iz; Dp[..., 0, 2] = -x * iz * iz
    Dp[..., 1, 1] = iz; Dp[..., 1, 2] = -y * iz * iz
    J = np.concatenate([-Dp @ skew(RX), Dp], -1)             # d p / d dtheta = -[R X]x
    return r, J, z


def cost_of(R, t, X, uv):
    with np.errstate(all="ignore"):
        r, _, _ = residual_jacobian(R, t, X, uv)
        return (r * r).sum((-1, -2))


def cholesky_solve(M, g):
    """Batched 6 x 6 Cholesky solve of M d = -g.  -> (d [H, 6], ok [H])."""
    H = M.shape[0]
    L = np.zeros_like(M); ok = np.ones(H, bool)
    for j in range(6):
        s = M[:, j, j] - (L[:, j, :j] ** 2).sum(-1)
        ok &= np.isfinite(s) & (s > 0)
        d = np.sqrt(np.where(s > 0, s, 1.0))
        L[:, j, j] = d
        for i in range(j + 1, 6):
            L[:, i, j] = (M[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(-1)) / d
    y = np.zeros((H, 6))
    for i in range(6):
        y[:, i] = (-g[:, i] - (L[:, i, :i] * y[:, :i]).sum(-1)) / L[:, i, i]
    x = np.zeros((H, 6))
    for i in reversed(range(6)):
        x[:, i] = (y[:, i] - (L[:, i + 1:, i] * x[:, i + 1:]).sum(-1)) / L[:, i, i]
    return x, ok


def lm(R0, t0, X, uv, refine=False, rec=None):
    """The LM of the header, batched over H problems of m points each.  -> (R [H,3,3], t [H,3], valid [H]).
    rec [H, TRACE_REC] (optional): the trace records of the H problems, filled as uvs_lc_debug_pair fills them (iterations, initial cost,
    iteration records; the caller writes samples, validity and poses)."""
    R = np.array(R0, np.float64); t = np.array(t0, np.float64)
    H = R.shape[0]
    with np.errstate(all="ignore"):
        cost = cost_of(R, t, X, uv)
        valid = np.isfinite(cost) if not refine else np.ones(H, bool)
        active = valid.copy()
        lam = np.full(H, LAMBDA0)
        if rec is not None:
            rec[:, 7] = cost
            its = rec[:, TRACE_HEAD:].reshape(H, LM_ITERS, TRACE_ITER)
        for it in range(LM_ITERS):
            if not active.any():
                break
            r, J, _ = residual_jacobian(R, t, X, uv)
            A = np.einsum("hmki,hmkj->hij", J, J)
            g = np.einsum("hmki,hmk->hi", J, r)
            M = A + lam[:, None, None] * (np.eye(6) * np.diagonal(A, 0, 1, 2)[:, None, :])
            d, ok = cholesky_solve(M, g)
            if rec is not None:
                a = np.flatnonzero(active)
                rec[a, 6] = it + 1
                its[a, it, 0:9] = R[a].reshape(-1, 9); its[a, it, 9:12] = t[a]; its[a, it, 12] = lam[a]
                its[a, it, 13:34] = A[a][:, _IU[0], _IU[1]]; its[a, it, 34:40] = g[a]; its[a, it, 40] = (r[a] * r[a]).sum((-1, -2))
                its[a, it, 41] = ok[a]
            fail = active & ~ok
            if refine:
                active &= ~fail
            else:
                valid &= ~fail; active &= ~fail
            Rc = exp_so3(d[:, :3]) @ R
            tc = t + d[:, 3:]
            cc = cost_of(Rc, tc, X, uv)
            acc = active & (cc < cost)
            if rec is not None:
                a = np.flatnonzero(active)
                its[a, it, 42:48] = d[a]; its[a, it, 48:57] = Rc[a].reshape(-1, 9); its[a, it, 57:60] = tc[a]
                its[a, it, 60] = cc[a]; its[a, it, 61] = cost[a]; its[a, it, 62] = acc[a]
            R = np.where(acc[:, None, None], Rc, R); t = np.where(acc[:, None], tc, t)
            cost = np.where(acc, cc, cost)
            lam = np.where(active, np.where(acc, lam / 10.0, lam * 10.0), lam)
            small = np.sqrt((d * d).sum(-1)) < FLT_EPSILON * np.maximum(1.0, np.sqrt((t * t).sum(-1)))
            if rec is not None:
                its[a, it, 63] = small[a]
            active &= ~small
    return R, t, valid


def inlier_mask(R, t, X, uv):
    """R [3,3], t [3] -> bool [m]."""
    with np.errstate(all="ignore"):
        p = X @ R.T + t
        dx = p[:, 0] / p[:, 2] - uv[:, 0]; dy = p[:, 1] / p[:, 2] - uv[:, 1]
        return (p[:, 2] > 0) & (dx * dx + dy * dy <= THRESH * THRESH)


def threshold_margin(R, t, X, uv):
    """min over matches of |err / thr^2 - 1|: how close any match lies to the inlier threshold."""
    with np.errstate(all="ignore"):
        p = X @ R.T + t
        dx = p[:, 0] / p[:, 2] - uv[:, 0]; dy = p[:, 1] / p[:, 2] - uv[:, 1]
        e = (dx * dx + dy * dy) / (THRESH * THRESH)
        e = e[np.isfinite(e) & (p[:, 2] > 0)]
        return float(np.abs(e - 1.0).min()) if len(e) else np.inf


# ---------------------------------------------------------------- selection
def update_num_iters(p, ep, model_points, max_iters):
    """OpenCV RANSACUpdateNumIters (cvRound = round half to even)."""
    p = min(max(p, 0.0), 1.0); ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, np.finfo(np.float64).tiny)
    denom = 1.0 - (1.0 - ep) ** model_points
    if denom < np.finfo(np.float64).tiny:
        return 0
    num = np.log(num); denom = np.log(denom)
    return max_iters if (denom >= 0 or -num >= max_iters * (-denom)) else int(np.rint(num / denom))


def select(counts, n):
    """counts [100] (-1 invalid), n matches -> (best hypothesis or -1, hypotheses examined)."""
    best, best_count, niters, h = -1, 0, N_HYP, 0
    while h < niters:
        c = int(counts[h])
        if c > max(best_count, MODEL_POINTS - 1):
            best, best_count = h, c
            niters = update_num_iters(CONFIDENCE, (n - c) / n, MODEL_POINTS, niters)
        h += 1
    return best, h


# ---------------------------------------------------------------- rotations (Eigen / Utility conventions)
def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def R_to_quat_eigen(m):
    """Eigen's Quaternion(Matrix3d) without any sign normalization -> (w, x, y, z)."""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0); w = 0.5 * t; t = 0.5 / t
        return np.array([w, (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t])
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    j = (i + 1) % 3; k = (j + 1) % 3
    t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
    v = np.zeros(3); v[i] = 0.5 * t; t = 0.5 / t
    w = (m[k, j] - m[j, k]) * t; v[j] = (m[j, i] + m[i, j]) * t; v[k] = (m[k, i] + m[i, k]) * t
    return np.array([w, v[0], v[1], v[2]])


def yaw_deg(R):
    return np.degrees(np.arctan2(R[1, 0], R[0, 0]))


def normalize_angle(a):
    """Utility::normalizeAngle of the pose_graph package (floor form)."""
    if a > 0:
        return a - 360.0 * np.floor((a + 180.0) / 360.0)
    return a + 360.0 * np.floor((-a + 180.0) / 360.0)


# ---------------------------------------------------------------- one pair
def verify(pair, tic, qic, trace=False):
    """pair: dict(p3d [nq,3], qdesc [nq,4] u64, vio_t [3], vio_q [4] xyzw, uv [no,2], odesc [no,4] u64, seed).
    -> dict with the fields of uvs_lc_result plus match_old [nq], inlier [nq] (uint8), margin (threshold_margin over every hypothesis).
    trace=True: -> (that dict, raw [TRACE_LEN]): the trace of uvs_lc_debug_pair from this FP64 run, in the header's layout."""
    if trace:
        raw = np.zeros(TRACE_LEN)
        return _verify(pair, tic, qic, raw), raw
    return _verify(pair, tic, qic, None)


def _verify(pair, tic, qic, raw):
    p3d = np.asarray(pair["p3d"], np.float64).reshape(-1, 3); uvo = np.asarray(pair["uv"], np.float64).reshape(-1, 2)
    nq = len(p3d)
    out = dict(accepted=0, reason=REASON["NO_MATCHES"], n_matches=0, n_inliers=0, best_hypothesis=-1, ransac_iters=0,
               loop_info=np.zeros(8), PnP_T_old=np.zeros(3), PnP_q_old=np.array([0.0, 0.0, 0.0, 1.0]), hyp_inliers=-np.ones(N_HYP, np.int32),
               match_old=match(pair["qdesc"], pair["odesc"]), inlier=np.zeros(nq, np.uint8), margin=np.inf)
    mi = np.flatnonzero(out["match_old"] >= 0)
    n = len(mi)
    out["n_matches"] = n
    rec = None
    if raw is not None:
        rec = raw[:TRACE_STAGE].reshape(N_HYP + 1, TRACE_REC)
        st = raw[TRACE_STAGE:]
        st[0] = n
        st[1:1 + 3 * n] = p3d[mi].ravel(); st[1 + 3 * MAX_QUERY:1 + 3 * MAX_QUERY + 2 * n] = uvo[out["match_old"][mi]].ravel()
        st[1 + 5 * MAX_QUERY:1 + 5 * MAX_QUERY + n] = mi
    if n == 0:
        return out
    if n <= MIN_LOOP_NUM:
        out["reason"] = REASON["FEW_MATCHES"]; return out
    X = p3d[mi]; uv = uvo[out["match_old"][mi]]
    tic = np.asarray(tic, np.float64); ric = quat_to_R(qic)
    vio_T = np.asarray(pair["vio_t"], np.float64); vio_R = quat_to_R(pair["vio_q"])
    R_w_c = vio_R @ ric; T_w_c = vio_T + vio_R @ tic
    R0 = R_w_c.T; t0 = -(R0 @ T_w_c)
    seed = int(pair["seed"]) & M64
    samples = [draw(seed, h, n) for h in range(N_HYP)]
    ok = np.array([s is not None for s in samples])
    S = np.array([s if s is not None else [0] * MODEL_POINTS for s in samples])
    if rec is not None:       # a failed draw runs no LM on the device: this file's batched LM runs it on the stand-in sample, so its record is cleared below
        Rh, th, valid = lm(np.broadcast_to(R0, (N_HYP, 3, 3)), np.broadcast_to(t0, (N_HYP, 3)), X[S], uv[S], rec=rec[:N_HYP])
        rec[:N_HYP][~ok] = 0.0
        Rh[~ok] = R0; th[~ok] = t0
        valid &= ok
        rec[:N_HYP, 0:5] = np.where(ok[:, None], S, -1); rec[:N_HYP, 5] = valid; rec[:N_HYP, 20] = ok
        rec[:N_HYP, 8:17] = Rh.reshape(N_HYP, 9); rec[:N_HYP, 17:20] = th
    else:
        Rh, th, valid = lm(np.broadcast_to(R0, (N_HYP, 3, 3)), np.broadcast_to(t0, (N_HYP, 3)), X[S], uv[S])
        valid &= ok
    counts = -np.ones(N_HYP, np.int32)
    for h in np.flatnonzero(valid):
        counts[h] = int(inlier_mask(Rh[h], th[h], X, uv).sum())
        out["margin"] = min(out["margin"], threshold_margin(Rh[h], th[h], X, uv))
    out["hyp_inliers"] = counts
    best, iters = select(counts, n)
    out["best_hypothesis"] = best; out["ransac_iters"] = iters
    if best < 0:
        out["reason"] = REASON["RANSAC_FAILED"]; return out
    mask = inlier_mask(Rh[best], th[best], X, uv)
    out["inlier"][mi[mask]] = 1
    out["n_inliers"] = int(mask.sum())
    Rr, tr, _ = lm(Rh[best][None], th[best][None], X[mask][None], uv[mask][None], refine=True, rec=None if rec is None else rec[N_HYP:])
    R_pnp, T_pnp = Rr[0], tr[0]
    if rec is not None:
        rec[N_HYP, 5] = 1.0
        rec[N_HYP, 8:17] = R_pnp.ravel(); rec[N_HYP, 17:20] = T_pnp
        rec[N_HYP, 20:29] = Rh[best].ravel(); rec[N_HYP, 29:32] = th[best]
    R_w_c_old = R_pnp.T; T_w_c_old = R_w_c_old @ (-T_pnp)
    PnP_R_old = R_w_c_old @ ric.T; PnP_T_old = T_w_c_old - PnP_R_old @ tic
    qw = R_to_quat_eigen(PnP_R_old)
    out["PnP_T_old"] = PnP_T_old; out["PnP_q_old"] = np.array([qw[1], qw[2], qw[3], qw[0]])
    if out["n_inliers"] <= MIN_LOOP_NUM:
        out["reason"] = REASON["FEW_INLIERS"]; return out
    rel_t = PnP_R_old.T @ (vio_T - PnP_T_old)
    rel_q = R_to_quat_eigen(PnP_R_old.T @ vio_R)
    rel_yaw = normalize_angle(yaw_deg(vio_R) - yaw_deg(PnP_R_old))
    out["loop_info"] = np.r_[rel_t, rel_q, rel_yaw]
    if not abs(rel_yaw) < 30.0:
        out["reason"] = REASON["YAW_GATE"]
    elif not np.linalg.norm(rel_t) < 20.0:
        out["reason"] = REASON["T_GATE"]
    else:
        out["reason"] = REASON["ACCEPTED"]; out["accepted"] = 1
    return out
