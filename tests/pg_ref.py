"""Independent numpy restatement of PoseGraph::optimize4DoF (reference pose_graph/src/pose_graph.cpp:403-579, pose_graph.h:90-248).

TEST INFRASTRUCTURE ONLY.  Written from the reference, not from csrc/uvs_pose_graph.hip: dense normal equations over every free variable
(no band, no Woodbury), `numpy.linalg.solve`, and the Levenberg-Marquardt controller of SURVEY.md Appendix B as tests/pyref_lm.py reads it
(Jacobi scaling computed once, the clamped Marquardt diagonal reused after a rejected step, tolerance tests before accept / reject, the
radius rules) with the pose graph's options: max_num_iterations = 5, everything else a Ceres default.

Conventions (those of include/uvs_solver.h, uvs_pg_*): keyframes in list order, x[i] = (yaw deg, tx, ty, tz); q as (x, y, z, w); a loop is
(cur, old, rel_t[3], rel_yaw deg) with old < cur.  Edges whose two keyframes are constant are left out (Ceres removes them from the reduced
program), so the costs are those of the other edges.
"""
import numpy as np

MAX_ITER = 5
HUBER_A = 0.1
D2R = np.pi / 180.0
TERM = dict(NO_CONVERGENCE=0, GRADIENT_TOL=1, PARAMETER_TOL=2, FUNCTION_TOL=3, MIN_RADIUS=4, INVALID_STEPS=5)


def normalize_angle(a):
    """pose_graph.h NormalizeAngle: a single wrap (not Utility::normalizeAngle)."""
    a = np.asarray(a, dtype=np.float64)
    return np.where(a > 180.0, a - 360.0, np.where(a < -180.0, a + 360.0, a))


def quat_to_R(q):
    """q [..., 4] (x, y, z, w) -> R [..., 3, 3] (Eigen's toRotationMatrix)."""
    q = np.asarray(q, dtype=np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - z * w); R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w); R[..., 2, 1] = 2 * (y * z + x * w); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def R_to_quat(R):
    """R [..., 3, 3] -> q (x, y, z, w), w >= 0."""
    R = np.asarray(R, dtype=np.float64)
    out = np.empty(R.shape[:-2] + (4,))
    for idx in np.ndindex(R.shape[:-2]):
        m = R[idx]
        tr = np.trace(m)
        if tr > 0:
            s = 2.0 * np.sqrt(tr + 1.0); w = 0.25 * s
            x = (m[2, 1] - m[1, 2]) / s; y = (m[0, 2] - m[2, 0]) / s; z = (m[1, 0] - m[0, 1]) / s
        else:
            i = int(np.argmax(np.diag(m))); j, k = (i + 1) % 3, (i + 2) % 3
            s = 2.0 * np.sqrt(1.0 + m[i, i] - m[j, j] - m[k, k])
            v = np.empty(3); v[i] = 0.25 * s; v[j] = (m[j, i] + m[i, j]) / s; v[k] = (m[k, i] + m[i, k]) / s
            w = (m[k, j] - m[j, k]) / s; x, y, z = v
        qq = np.array([x, y, z, w]); qq = qq if qq[3] >= 0 else -qq
        out[idx] = qq / np.linalg.norm(qq)
    return out


def R2ypr(R):
    """Utility::R2ypr, degrees; R [..., 3, 3] -> [..., 3]."""
    R = np.asarray(R, dtype=np.float64)
    yaw = np.arctan2(R[..., 1, 0], R[..., 0, 0]); cy, sy = np.cos(yaw), np.sin(yaw)
    pitch = np.arctan2(-R[..., 2, 0], R[..., 0, 0] * cy + R[..., 1, 0] * sy)
    roll = np.arctan2(R[..., 0, 2] * sy - R[..., 1, 2] * cy, R[..., 1, 1] * cy - R[..., 0, 1] * sy)
    return np.stack([yaw, pitch, roll], -1) / np.pi * 180.0


def ypr2R(yaw, pitch, roll):
    """YawPitchRollToRotationMatrix (pose_graph.h) = Utility::ypr2R, degrees; broadcasts."""
    y, p, r = (np.asarray(v, dtype=np.float64) * D2R for v in (yaw, pitch, roll))
    cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    R = np.empty(np.broadcast(y, p, r).shape + (3, 3))
    R[..., 0, 0] = cy * cp; R[..., 0, 1] = -sy * cr + cy * sp * sr; R[..., 0, 2] = sy * sr + cy * sp * cr
    R[..., 1, 0] = sy * cp; R[..., 1, 1] = cy * cr + sy * sp * sr; R[..., 1, 2] = -cy * sr + sy * sp * cr
    R[..., 2, 0] = -sp; R[..., 2, 1] = cp * sr; R[..., 2, 2] = cp * cr
    return R


class Problem:
    """Edges of optimize4DoF: arrays a, b (keyframe indices; a = the end whose yaw rotates the residual), rel_t, rel_yaw, pitch, roll, loop flag."""

    def __init__(self, t, q, sequence, constant, loops):
        t = np.asarray(t, dtype=np.float64).reshape(-1, 3); q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
        n = len(t)
        self.n = n
        self.constant = np.asarray(constant).astype(bool)
        seq = np.asarray(sequence)
        ypr = R2ypr(quat_to_R(q))
        self.x0 = np.concatenate([ypr[:, :1], t], 1)
        Rq = quat_to_R(q)
        A, B, RT, RY, P, RO, LP = [], [], [], [], [], [], []
        for i in range(n):                                    # pose_graph.cpp:497-512
            for j in range(1, 5):
                if i - j >= 0 and seq[i] == seq[i - j] and not (self.constant[i] and self.constant[i - j]):
                    A.append(i - j); B.append(i); RT.append(Rq[i - j].T @ (t[i] - t[i - j])); RY.append(ypr[i, 0] - ypr[i - j, 0])
                    P.append(ypr[i - j, 1]); RO.append(ypr[i - j, 2]); LP.append(False)
        for cur, old, rel_t, rel_yaw in loops:                # pose_graph.cpp:516-530
            if self.constant[cur] and self.constant[old]:
                continue
            A.append(old); B.append(cur); RT.append(np.asarray(rel_t, dtype=np.float64)); RY.append(float(rel_yaw))
            P.append(ypr[old, 1]); RO.append(ypr[old, 2]); LP.append(True)
        self.a = np.array(A, dtype=np.int64); self.b = np.array(B, dtype=np.int64)
        self.rel_t = np.array(RT, dtype=np.float64).reshape(-1, 3); self.rel_yaw = np.array(RY, dtype=np.float64)
        self.pitch = np.array(P, dtype=np.float64); self.roll = np.array(RO, dtype=np.float64); self.loop = np.array(LP, dtype=bool)
        self.free = np.flatnonzero(~self.constant)
        self.col = -np.ones(n, dtype=np.int64); self.col[self.free] = np.arange(len(self.free))


def residuals(pb, x, jacobian=True, robust=True):
    """Per edge: corrected residual r [E, 4], corrected J [E, 4, 8] (columns yaw_a, t_a, yaw_b, t_b), cost 0.5 rho(|r|^2) [E].
    robust=False: the raw residual and Jacobian of the cost functor (same cost)."""
    ya, yb = x[pb.a, 0], x[pb.b, 0]
    R = ypr2R(ya, pb.pitch, pb.roll)                              # w_R_i of the a end
    d = x[pb.b, 1:] - x[pb.a, 1:]
    w = np.where(pb.loop, 0.1, 1.0)                               # FourDOFWeightError: yaw / 10
    r = np.empty((len(pb.a), 4))
    r[:, :3] = np.einsum("eji,ej->ei", R, d) - pb.rel_t
    r[:, 3] = normalize_angle(yb - ya - pb.rel_yaw) * w
    s = (r * r).sum(1)
    outer = pb.loop & (s > HUBER_A ** 2)                          # HuberLoss(0.1) on loop edges only
    sr = np.sqrt(s)
    rho0 = np.where(outer, 2.0 * HUBER_A * sr - HUBER_A ** 2, s)
    rho1 = np.where(outer, np.maximum(np.finfo(float).tiny, HUBER_A / np.where(sr > 0, sr, 1.0)), 1.0)
    sc = np.sqrt(rho1) if robust else np.ones(len(s))             # Ceres corrector with rho'' <= 0: plain sqrt(rho') scaling
    cost = 0.5 * rho0
    if not jacobian:
        return r * sc[:, None], None, cost
    J = np.zeros((len(pb.a), 4, 8))
    # d(R^T d)/d yaw = dR/dyaw^T d, dR/dyaw = [e_z]x R (per radian), yaw in degrees
    K = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    dR = np.einsum("ij,ejk->eik", K, R) * D2R
    J[:, :3, 0] = np.einsum("eji,ej->ei", dR, d)
    J[:, :3, 1:4] = -np.transpose(R, (0, 2, 1))
    J[:, :3, 5:8] = np.transpose(R, (0, 2, 1))
    J[:, 3, 0] = -w; J[:, 3, 4] = w
    return r * sc[:, None], J * sc[:, None, None], cost


def normal_equations(pb, r, J):
    """Dense H = J^T J, g = J^T r over the free variables (4 per free keyframe)."""
    m = 4 * len(pb.free)
    H = np.zeros((m, m)); g = np.zeros(m)
    cols = np.full((len(pb.a), 8), -1, dtype=np.int64)
    for side, idx in ((0, pb.a), (1, pb.b)):
        c = pb.col[idx]
        for k in range(4):
            cols[:, 4 * side + k] = np.where(c >= 0, 4 * c + k, -1)
    for e in range(len(pb.a)):
        keep = cols[e] >= 0
        ce, Je = cols[e][keep], J[e][:, keep]
        H[np.ix_(ce, ce)] += Je.T @ Je
        g[ce] += Je.T @ r[e]
    return H, g, cols


def plus(pb, x, delta):
    """AngleLocalParameterization on yaw (x + d, then NormalizeAngle), Euclidean t; constant keyframes unchanged."""
    xc = x.copy()
    d = delta.reshape(-1, 4)
    xc[pb.free, 0] = normalize_angle(x[pb.free, 0] + d[:, 0])
    xc[pb.free, 1:] = x[pb.free, 1:] + d[:, 1:]
    return xc


def model_cost_change(r, J, cols, delta):
    """Ceres: -(J delta) . (r + J delta / 2), with the corrected r, J."""
    dg = np.where(cols >= 0, delta[np.maximum(cols, 0)], 0.0)
    Jd = np.einsum("eik,ek->ei", J, dg)
    return -(Jd * (r + 0.5 * Jd)).sum()


class Trace:
    def __init__(self):
        self.accepted, self.cost, self.radius, self.candidate_cost, self.model_cost_change = [1], [], [], [0.0], [0.0]
        self.termination, self.num_iterations = TERM["NO_CONVERGENCE"], 0
        self.initial_cost = self.final_cost = None


def optimize(t, q, sequence, constant, loops, max_num_iterations=MAX_ITER):
    """-> (x [n, 4] = (yaw deg, t) after the solve, Trace)."""
    pb = Problem(t, q, sequence, constant, loops)
    x = pb.x0.copy()
    tr = Trace()
    r, J, ce = residuals(pb, x)
    cost = ce.sum()
    tr.initial_cost = cost; tr.cost.append(cost)
    radius, decrease_factor = 1e4, 2.0
    tr.radius.append(radius)
    if len(pb.free) == 0:                                         # Ceres: no free parameter block, converged without an iteration
        tr.termination = TERM["FUNCTION_TOL"]; tr.final_cost = cost
        return x, tr
    H, g, cols = normal_equations(pb, r, J)
    s = 1.0 / (1.0 + np.sqrt(np.diag(H)))                         # Jacobi scaling, once
    free = pb.free

    def gmax_of(x, g):
        gy = g.reshape(-1, 4)
        yaw = x[free, 0]
        return max(np.abs(yaw - normalize_angle(yaw - gy[:, 0])).max(), np.abs(gy[:, 1:]).max())

    gmax = gmax_of(x, g)
    x_norm = np.linalg.norm(x[free])
    diag, fresh, invalid, it = None, True, 0, 0
    while True:
        if it >= max_num_iterations: tr.termination = TERM["NO_CONVERGENCE"]; break
        if gmax <= 1e-10: tr.termination = TERM["GRADIENT_TOL"]; break
        if radius <= 1e-32: tr.termination = TERM["MIN_RADIUS"]; break
        it += 1
        Hs, gs = H * np.outer(s, s), g * s
        if fresh:
            diag = np.clip(np.diag(Hs), 1e-6, 1e32); fresh = False
        y = np.linalg.solve(Hs + np.diag(diag / radius), -gs)
        delta = s * y
        mcc = model_cost_change(r, J, cols, delta)
        tr.model_cost_change.append(mcc)
        if not (np.all(np.isfinite(y)) and mcc > 0.0):
            invalid += 1
            radius /= decrease_factor; decrease_factor *= 2.0
            tr.accepted.append(-1); tr.radius.append(radius); tr.cost.append(cost); tr.candidate_cost.append(cost)
            if invalid >= 5: tr.termination = TERM["INVALID_STEPS"]; break
            continue
        invalid = 0
        xc = plus(pb, x, delta)
        cand = residuals(pb, xc, jacobian=False)[2].sum()
        cand = cand if np.isfinite(cand) else np.finfo(float).max
        tr.candidate_cost.append(cand)
        step_norm = np.linalg.norm(xc[free] - x[free])
        rho = (cost - cand) / mcc
        stop = None
        if step_norm <= 1e-8 * (x_norm + 1e-8): stop = TERM["PARAMETER_TOL"]
        elif abs(cost - cand) <= 1e-6 * cost: stop = TERM["FUNCTION_TOL"]
        if stop is not None:
            tr.accepted.append(0); tr.radius.append(radius); tr.cost.append(cost); tr.termination = stop; break
        if rho > 1e-3:
            x, cost = xc, cand
            r, J, _ = residuals(pb, x)
            H, g, cols = normal_equations(pb, r, J)
            gmax = gmax_of(x, g); x_norm = np.linalg.norm(x[free])
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            decrease_factor = 2.0; fresh = True
            tr.accepted.append(1)
        else:
            radius /= decrease_factor; decrease_factor *= 2.0
            tr.accepted.append(0)
        tr.radius.append(radius); tr.cost.append(cost)
    tr.num_iterations = it; tr.final_cost = cost
    return x, tr


# ---------------------------------------------------------------- one damped solve in extended precision
def damped_system(pb, radius):
    """The scaled damped system of the FIRST LM iteration at radius, formed exactly as `optimize` forms it:
    -> (M = S H S + diag(clip(diag(S H S), 1e-6, 1e32)) / radius, b = -S g, s = diag(S)), FP64."""
    r, J, _ = residuals(pb, pb.x0)
    H, g, _ = normal_equations(pb, r, J)
    s = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    Hs = H * np.outer(s, s)
    diag = np.clip(np.diag(Hs), 1e-6, 1e32)
    return Hs + np.diag(diag / radius), -(g * s), s


def cholesky_ld(M, nb=32):
    """Lower Cholesky factor of the symmetric positive definite M in np.longdouble (blocked right-looking, numpy only)."""
    A = np.array(M, dtype=np.longdouble)
    m = len(A)
    for k0 in range(0, m, nb):
        k1 = min(m, k0 + nb)
        for k in range(k0, k1):
            if not A[k, k] > 0:
                raise np.linalg.LinAlgError(f"cholesky_ld: pivot {k} is {A[k, k]}")
            A[k:, k] /= np.sqrt(A[k, k])
            c = A[k + 1:, k]
            A[k + 1:, k + 1:k1] -= c[:, None] * c[None, :k1 - k - 1]
        P = A[k1:, k0:k1]
        A[k1:, k1:] -= P @ P.T
    return np.tril(A)


def solve_ld(M, b):
    """M y = b through cholesky_ld and two triangular sweeps, all in np.longdouble.  -> y (np.longdouble)."""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not an extended type here: the reference would be plain FP64"
    L = cholesky_ld(M)
    m = len(L)
    y = np.array(b, dtype=np.longdouble)
    for k in range(m):
        y[k] = (y[k] - L[k, :k] @ y[:k]) / L[k, k]
    for k in range(m - 1, -1, -1):
        y[k] = (y[k] - L[k + 1:, k] @ y[k + 1:]) / L[k, k]
    return y


def damped_step(pb, radius):
    """The unscaled step delta = S y of the first LM iteration at `radius` (free-keyframe order, [4 nf]), y solved in np.longdouble:
    the reference of uvs_pg_debug_step.  -> delta (np.longdouble)."""
    M, b, s = damped_system(pb, radius)
    return s.astype(np.longdouble) * solve_ld(M, b)
