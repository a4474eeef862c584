"""60-digit reference of loop verification's PnP (uvs_lc_verify, csrc/uvs_loop_verify.hip) and the stage checker of its trace.

TEST INFRASTRUCTURE ONLY.  mpmath at 60 digits, as tests/factor_ref.py.  The mathematics is restated from its definitions: the projection
residual (x / z, y / z) - uv of p = R X + t, its Jacobian under the left perturbation p(dtheta, dt) = Exp(dtheta) R X + t + dt (d p / d dtheta =
-[R X]x, d p / d dt = I, chained through d (x / z, y / z) / d p), the damped normal equations (J^T J + lambda diag J^T J) d = -J^T r, Rodrigues'
Exp, the inlier rule z > 0 and |r|^2 <= (10 / 460)^2, and the body-pose / loop_info algebra of KeyFrame::findConnection.

check_trace verifies a trace of uvs_lc_debug_pair (or of lc_ref.verify(trace=True), which has the same layout) stage by stage.  No stage follows
an LM trajectory at two precisions: every stage takes the recorded FP64 inputs of that stage as exact, evaluates the stage at 60 digits and
compares the recorded FP64 outputs with a bound that is derived from the code's rounding count (u = 2^-53):

  0 prior      iteration 0 of every hypothesis starts at the camera pose of origin_vio through the extrinsic.  R0 = (R(vio_q) ric)^T:
               R(vio_q) entry 4 roundings (two products, their sum, the subtraction; the doubling is exact), x ric 1, the 3-term sum 2: C = 7.
               t0 = -R0 (vio_t + R(vio_q) tic): Twc 4 + 1 + 2 + 1 = 8, R0 7, product 1, sum 2: C = 18.  Scale: the same expressions with every
               operand replaced by its absolute value.
  1 samples    equal lc_ref.draw; invalid exactly when the draw fails, the initial cost is not finite or a pivot fails.
  2 normal eq. every acc entry, cc and the initial cost within C u S.  S: the entry with |.| taken of every term down to the operands (|R||X| +
               |t| for p, |z|-amplified 1 / z: izb = (pb_z / |z|) / |z|), so cancellation anywhere is covered.  C from accum_point: p 4 (3-term
               dot 3, + t 1), iz 5, dxz = -x iz iz 4 + 5 + 5 + 2 = 16, a J entry iz a2 - dxz a0 = max(5 + 3 + 1, 16 + 3 + 1) + 1 = 21, a
               product of two 43, J0 J0 + J1 J1 44: C_POINT = 44, then the sum: 5 serial adds for a hypothesis (C = 49); in the refinement the
               lane partial (ceil(n / 256) adds), 6 shuffle levels and 3 wave adds (C = 44 + ceil(n / 256) + 9).  point_cost: x / z 4 + 4 + 1,
               - uv 10, squares and their sum 22: C = 22 + the same sums.
  3 step       the componentwise backward error |(A + lambda diag A) d + g| <= gamma_19 |L||L^T||d| + u (1 + lambda) diag(A) |d| on the
               device's own matrix (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 10.4, gamma_{3n+1}, n = 6; L the 60-digit
               factor).  The success flag equals the 60-digit verdict unless a 60-digit pivot lies within gamma_19 (|L||L^T|)_jj of 0 (excused).
  4 candidate  Exp(d[0:3]) R and t + d[3:6] entrywise within K4 u scale (scale: sum_k S_ik |R_kj| with S = exp_so3_scale(d[0:3]); |t| + |d|).  sin, cos and sqrt come from
               the device's math library, so K4 is measured: K4 = 4 x K4_LC_REF, the worst error / (u scale) of lc_ref's own candidate poses
               over the committed cases (tests/test_lc_hp.py asserts that lc_ref stays within K4_LC_REF).
  5 decisions  replayed exactly from the recorded values: accepted == (cc < cost); lambda / 10 or x 10; the next start pose, the next cost, the
               final pose, the iteration count, bit for bit.  stop == (|d| < FLT_EPSILON max(1, |t|)) at 60 digits unless |d| is within 4 u
               relative of the threshold (excused).
  6 orthonorm. ||R^T R - I||_max of every recorded rotation <= that of the record's first start pose (an input) + K4 u x the sum over the
               accepted steps of the step's scale 2 max_ij sum_k |Rc_ki| S_kj, which is what stage 4's entrywise bound K4 u S allows R^T R to move.
  7 counts     hyp_inliers[h] equals the 60-digit inlier count at the recorded final pose of h, the mask the 60-digit mask at the best pose;
               a match may differ only if its 60-digit |e / thr^2 - 1| <= 1e-12 (excused).
  8 selection  best_hypothesis and ransac_iters equal lc_ref.select on the device's counts.
  9 finish     PnP_T_old, PnP_q_old, loop_info against the 60-digit closed form from the recorded refined pose, entrywise; the bound is the
               first-order propagation of one u per operation written next to each step in _finish (the quaternion in the branch Eigen's rule
               takes at 60 digits); yaw carries K_ATAN2 = 4 x K_ATAN2_LC_REF for atan2.  Gate verdicts exact unless within the bound of 30 / 20.
  10 minimiser the 60-digit Gauss-Newton fixed point (the stationary point of the cost over the reported inlier set) from the recorded refined
               pose; the recorded pose's distance to it is reported and must be <= max(2 x lc_ref's distance to its own minimiser on the same
               pair, FLT_EPSILON max(1, |t|)).

The excuses of stages 3, 5, 7 and 9 are counted; the tests assert the count is 0.  The worst error / bound per stage goes to the file UVS_LC_LOG
names."""
import math
import multiprocessing
import os
from concurrent.futures import ProcessPoolExecutor

import mpmath as mp
import numpy as np

import lc_ref

DPS = 60
mp.mp.dps = DPS
F = mp.mpf
U = F(2) ** -53
GAMMA19 = 19 * U / (1 - 19 * U)
MAX_WORKERS = 16
C_POINT, C_COST = 44, 22
K4_LC_REF = 1.96           # measured: lc_ref's worst stage-4 error / (u scale) over the committed cases is 1.950
K4 = 4 * K4_LC_REF
K_ATAN2_LC_REF = 1.90      # measured: lc_ref's worst yaw error / (u |yaw|) over the committed cases is 1.894
K_ATAN2 = 4 * K_ATAN2_LC_REF
THR2 = (F(10) / 460) ** 2
FLT_EPS = F(2) ** -23
BORDER = F(10) ** -12
STAGES = ["0 prior", "1 samples", "2 normal eq", "3 step", "4 candidate", "5 decisions", "6 orthonormal", "7 counts", "8 selection", "9 finish",
          "10 minimiser"]
IT = dict(start=slice(0, 12), lam=12, acc=slice(13, 41), chol=41, d=slice(42, 48), cand=slice(48, 60), cc=60, cost=61, acc_flag=62, stop=63)


# ---------------------------------------------------------------- 60-digit mathematics, from the definitions
def V(a):
    return [F(float(x)) for x in np.asarray(a, np.float64).ravel()]


def M3(v):
    return [list(v[0:3]), list(v[3:6]), list(v[6:9])]


def matmul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def transpose(A):
    return [list(r) for r in zip(*A)]


def mabs(A):
    return [[abs(x) for x in r] for r in A]


def matvec(A, v):
    return [sum(A[i][k] * v[k] for k in range(len(v))) for i in range(len(A))]


def skew(w):
    return [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]


def exp_so3(w):
    """Rodrigues: I + sin(th) / th K + (1 - cos th) / th^2 K^2, the second factor as 2 sin^2(th / 2) / th^2 (no cancellation)."""
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if th2 < F(10) ** -40:
        A = 1 - th2 / 6 + th2 * th2 / 120; B = F(1) / 2 - th2 / 24 + th2 * th2 / 720
    else:
        th = mp.sqrt(th2); A = mp.sin(th) / th; s = mp.sin(th / 2); B = 2 * s * s / th2
    K = skew(w); K2 = matmul(K, K)
    return [[(1 if i == j else 0) + A * K[i][j] + B * K2[i][j] for j in range(3)] for i in range(3)]


def exp_so3_scale(w):
    """The scale of Exp's rounding error, entrywise: (1 + th) (I + |A||K| + Bb |K|^2) with Bb = (1 + |cos th|) / th^2, the absolute values of
    both terms of B = (1 - cos th) / th^2 as the FP64 code forms it (its subtraction cancels for a small angle: the error of B K^2 stays near
    u whatever the angle).  The factor 1 + th is the conditioning of the FP64 evaluation itself: the angle th = sqrt(w . w) carries a relative
    rounding u, which moves sin th and cos th by th u.  Below th^2 = 1e-20 the code takes the series (Bb = 1 / 2)."""
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    th = mp.sqrt(th2)
    if th2 < F(10) ** -20:
        A = F(1); B = F(1) / 2
    else:
        A = abs(mp.sin(th) / th); B = (1 + abs(mp.cos(th))) / th2
    K = mabs(skew(w)); K2 = matmul(K, K)
    return [[(1 + th) * ((1 if i == j else 0) + A * K[i][j] + B * K2[i][j]) for j in range(3)] for i in range(3)]


def quat_to_R(q):
    """Unit quaternion (x, y, z, w) -> rotation (the definition; Eigen's toRotationMatrix)."""
    x, y, z, w = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def quat_to_R_abs(q):
    x, y, z, w = [abs(v) for v in q]
    return [[1 + 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 + 2 * (x * x + z * z), 2 * (y * z + x * w)],
            [2 * (x * z + y * w), 2 * (y * z + x * w), 1 + 2 * (x * x + y * y)]]


def residual_jacobian(R, t, X, uv):
    """One point.  -> (r [2], J [2][6], rb [2], Jb [2][6], z): the residual, its Jacobian (columns dtheta, dt), and both with absolute values
    taken of every term (the scale S of stage 2); None when z = 0."""
    a = matvec(R, X); ab = matvec(mabs(R), [abs(v) for v in X])
    p = [a[i] + t[i] for i in range(3)]; pb = [ab[i] + abs(t[i]) for i in range(3)]
    x, y, z = p
    if z == 0:
        return None
    iz = 1 / z
    izb = (pb[2] / abs(z)) / abs(z)              # |1 / z| with the amplification of z's own rounding (pb_z / |z| >= 1)
    r = [x * iz - uv[0], y * iz - uv[1]]
    rb = [pb[0] * izb + abs(uv[0]), pb[1] * izb + abs(uv[1])]
    Dp = [[iz, 0, -x * iz * iz], [0, iz, -y * iz * iz]]                      # d (x / z, y / z) / d p
    Dpb = [[izb, 0, pb[0] * izb * izb], [0, izb, pb[1] * izb * izb]]
    G = [[-v for v in row] for row in skew(a)]                               # d p / d dtheta = -[R X]x
    Gb = mabs(skew(ab))
    J = [matvec(transpose(G), Dp[k]) + Dp[k] for k in range(2)]
    Jb = [matvec(transpose(Gb), Dpb[k]) + Dpb[k] for k in range(2)]
    return r, J, rb, Jb, z


def normal_equations(R, t, Xs, uvs):
    """-> (acc [28], S [28]): packed upper J^T J (row by row), J^T r, r^T r summed over the points, and the sums of absolute values."""
    acc = [F(0)] * 28; S = [F(0)] * 28
    for X, uv in zip(Xs, uvs):
        rj = residual_jacobian(R, t, X, uv)
        if rj is None:
            return None, None
        r, J, rb, Jb, _ = rj
        k = 0
        for i in range(6):
            for j in range(i, 6):
                acc[k] += J[0][i] * J[0][j] + J[1][i] * J[1][j]; S[k] += Jb[0][i] * Jb[0][j] + Jb[1][i] * Jb[1][j]; k += 1
        for i in range(6):
            acc[21 + i] += J[0][i] * r[0] + J[1][i] * r[1]; S[21 + i] += Jb[0][i] * rb[0] + Jb[1][i] * rb[1]
        acc[27] += r[0] * r[0] + r[1] * r[1]; S[27] += rb[0] * rb[0] + rb[1] * rb[1]
    return acc, S


def cost(R, t, Xs, uvs):
    """-> (sum |r|^2, the same with absolute values of every term); (None, None) when a z = 0."""
    c = F(0); S = F(0)
    for X, uv in zip(Xs, uvs):
        a = matvec(R, X); ab = matvec(mabs(R), [abs(v) for v in X])
        p = [a[i] + t[i] for i in range(3)]; pb = [ab[i] + abs(t[i]) for i in range(3)]
        if p[2] == 0:
            return None, None
        k = pb[2] / abs(p[2])
        r0 = p[0] / p[2] - uv[0]; r1 = p[1] / p[2] - uv[1]
        b0 = pb[0] * k / abs(p[2]) + abs(uv[0]); b1 = pb[1] * k / abs(p[2]) + abs(uv[1])
        c += r0 * r0 + r1 * r1; S += b0 * b0 + b1 * b1
    return c, S


def inlier_error(R, t, X, uv):
    """-> (z, |r|^2 / thr^2) of one match (None for the second when z = 0)."""
    p = [sum(R[i][k] * X[k] for k in range(3)) + t[i] for i in range(3)]
    if p[2] == 0:
        return p[2], None
    dx = p[0] / p[2] - uv[0]; dy = p[1] / p[2] - uv[1]
    return p[2], (dx * dx + dy * dy) / THR2


def unpack_upper(acc):
    A = [[F(0)] * 6 for _ in range(6)]
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = acc[k]; k += 1
    return A


def cholesky(M):
    """-> (L or None, pivots [<= 6], partial |L||L^T| diagonal at the failing pivot)."""
    L = [[F(0)] * 6 for _ in range(6)]; piv = []
    for j in range(6):
        s = M[j][j] - sum(L[j][k] * L[j][k] for k in range(j))
        piv.append(s)
        if not s > 0:
            return None, piv, abs(M[j][j]) + sum(L[j][k] * L[j][k] for k in range(j))
        L[j][j] = mp.sqrt(s)
        for i in range(j + 1, 6):
            L[i][j] = (M[i][j] - sum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
    return L, piv, None


def solve6(M, b):
    return list(mp.lu_solve(mp.matrix(M), mp.matrix(b)))


def orthonormality(R):
    G = matmul(transpose(R), R)
    return max(abs(G[i][j] - (1 if i == j else 0)) for i in range(3) for j in range(3))


def R_to_quat_eigen(m, dm):
    """Eigen's Quaternion(Matrix3d) -> ((w, x, y, z), their error bounds) from m and the entrywise error bounds dm of the FP64 matrix it is
    taken of.  Propagation, one u per operation: the trace-like sum T (3 adds), s = sqrt(T), the half, f = 0.5 / s, each off-diagonal
    difference or sum and its product with f."""
    tr = m[0][0] + m[1][1] + m[2][2]
    if tr > 0:
        i = None
        T = tr + 1; Tb = abs(m[0][0]) + abs(m[1][1]) + abs(m[2][2]) + 1; dT = dm[0][0] + dm[1][1] + dm[2][2] + 3 * U * Tb
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        T = m[i][i] - m[j][j] - m[k][k] + 1; Tb = abs(m[0][0]) + abs(m[1][1]) + abs(m[2][2]) + 1; dT = dm[0][0] + dm[1][1] + dm[2][2] + 3 * U * Tb
    s = mp.sqrt(T); ds = dT / (2 * s) + U * s
    big = s / 2; dbig = ds / 2
    f = F(1) / 2 / s; df = ds / (2 * s * s) + U * f

    def off(a, b, sign):
        v = m[a[0]][a[1]] + sign * m[b[0]][b[1]]
        dv = dm[a[0]][a[1]] + dm[b[0]][b[1]] + U * (abs(m[a[0]][a[1]]) + abs(m[b[0]][b[1]]))
        return v * f, dv * f + abs(v) * df + U * abs(v * f)
    if i is None:
        q = [(big, dbig), off((2, 1), (1, 2), -1), off((0, 2), (2, 0), -1), off((1, 0), (0, 1), -1)]
    else:
        v = [None] * 3
        v[i] = (big, dbig); v[j] = off((j, i), (i, j), 1); v[k] = off((k, i), (i, k), 1)
        q = [off((k, j), (j, k), -1)] + v
    return [a for a, _ in q], [b for _, b in q], i


def prior_pose(pair, tic, ric):
    """-> (R0 [3][3], t0 [3], their bounds): the camera pose of origin_vio through the extrinsic, inverted (stage 0)."""
    q = V(pair["vio_q"]); vt = V(pair["vio_t"])
    vR = quat_to_R(q); vRb = quat_to_R_abs(q)
    Rwc = matmul(vR, ric); Rwcb = matmul(vRb, mabs(ric))
    Twc = [vt[i] + sum(vR[i][k] * tic[k] for k in range(3)) for i in range(3)]
    Twcb = [abs(vt[i]) + sum(vRb[i][k] * abs(tic[k]) for k in range(3)) for i in range(3)]
    R0 = transpose(Rwc); R0b = transpose(Rwcb)
    t0 = [-sum(R0[i][k] * Twc[k] for k in range(3)) for i in range(3)]
    t0b = [sum(R0b[i][k] * Twcb[k] for k in range(3)) for i in range(3)]
    return R0, t0, [[7 * U * v for v in r] for r in R0b], [18 * U * v for v in t0b]


def yaw_deg(R):
    return mp.atan2(R[1][0], R[0][0]) / mp.pi * 180


def yaw_error_in_u(R):
    """|lc_ref.yaw_deg(R) - the 60-digit yaw of the same FP64 matrix| / (u |yaw|): the figure K_ATAN2_LC_REF is measured with."""
    y = yaw_deg(M3(V(R)))
    return float(abs(F(float(lc_ref.yaw_deg(np.asarray(R, np.float64)))) - y) / (U * abs(y))) if y != 0 else 0.0


def normalize_angle(a):
    if a > 0:
        return a - 360 * mp.floor((a + 180) / 360)
    return a + 360 * mp.floor((-a + 180) / 360)


def _finish(Rp, tp, pair, tic, ric, n_inliers):
    """The finish at 60 digits from the refined pose (Rp, tp) -> dict name -> (values, bounds), and the gate quantities."""
    out = {}
    Rw = transpose(Rp); Rwb = mabs(Rw)                                        # R_w_c_old = R_pnp^T: exact
    Tw = [-sum(Rw[i][k] * tp[k] for k in range(3)) for i in range(3)]         # 3 products, 2 adds on the longest path: 3 u x sum |R||t|
    dTw = [3 * U * sum(Rwb[i][k] * abs(tp[k]) for k in range(3)) for i in range(3)]
    ricT = transpose(ric)
    PR = matmul(Rw, ricT)                                                     # 3 u x sum |R||ric|
    PRb = matmul(Rwb, mabs(ricT)); dPR = [[3 * U * v for v in r] for r in PRb]
    # PT = Tw - PR tic: the dot's terms carry dPR |tic| + u |PR tic| each, its 2 adds 2 u, the subtraction u
    dot = [sum(PR[i][k] * tic[k] for k in range(3)) for i in range(3)]
    dotb = [sum(abs(PR[i][k] * tic[k]) for k in range(3)) for i in range(3)]
    ddot = [sum(dPR[i][k] * abs(tic[k]) for k in range(3)) + 3 * U * dotb[i] for i in range(3)]
    PT = [Tw[i] - dot[i] for i in range(3)]
    dPT = [dTw[i] + ddot[i] + U * (abs(Tw[i]) + abs(dot[i])) for i in range(3)]
    out["PnP_T_old"] = (PT, dPT)
    q, dq, branch = R_to_quat_eigen(PR, dPR)
    out["PnP_q_old"] = ([q[1], q[2], q[3], q[0]], [dq[1], dq[2], dq[3], dq[0]])
    out["branch"] = branch
    if n_inliers <= lc_ref.MIN_LOOP_NUM:
        return out
    vq = V(pair["vio_q"]); vt = V(pair["vio_t"])
    vR = quat_to_R(vq); dvR = [[4 * U * v for v in r] for r in quat_to_R_abs(vq)]
    d = [vt[i] - PT[i] for i in range(3)]; dd = [dPT[i] + U * (abs(vt[i]) + abs(PT[i])) for i in range(3)]
    rt = [sum(PR[k][i] * d[k] for k in range(3)) for i in range(3)]
    drt = [sum(dPR[k][i] * abs(d[k]) + abs(PR[k][i]) * dd[k] for k in range(3)) + 3 * U * sum(abs(PR[k][i] * d[k]) for k in range(3)) for i in range(3)]
    RQ = matmul(transpose(PR), vR)
    dRQ = [[sum(dPR[k][i] * abs(vR[k][j]) + abs(PR[k][i]) * dvR[k][j] for k in range(3)) + 3 * U * sum(abs(PR[k][i] * vR[k][j]) for k in range(3))
            for j in range(3)] for i in range(3)]
    rq, drq, _ = R_to_quat_eigen(RQ, dRQ)

    def yaw(R, dR):
        # atan2's own error K_ATAN2 u |atan2|; its inputs' errors through d atan2 <= (|dy| + |dx|) / hypot; / pi x 180: 3 u relative
        y, x = R[1][0], R[0][0]
        a = mp.atan2(y, x)
        da = K_ATAN2 * U * abs(a) + (dR[1][0] + dR[0][0]) / mp.sqrt(x * x + y * y)
        return a / mp.pi * 180, (da + 3 * U * abs(a)) / mp.pi * 180
    y1, dy1 = yaw(vR, dvR); y2, dy2 = yaw(PR, dPR)
    ry = normalize_angle(y1 - y2)
    dry = dy1 + dy2 + U * (abs(y1) + abs(y2)) + 3 * U * (abs(y1 - y2) + 360)     # the subtraction; + 180, / 360 (floor exact away from its steps), 360 x, the last add
    out["loop_info"] = (rt + rq + [ry], drt + drq + [dry])
    out["yaw_scale"] = abs(y1) + abs(y2)
    tn = mp.sqrt(sum(v * v for v in rt)); dtn = sum(abs(rt[i]) * drt[i] for i in range(3)) / tn + 4 * U * tn
    out["gates"] = (abs(ry), dry, tn, dtn)
    return out


def minimiser(R, t, Xs, uvs, tol=F(10) ** -30, max_iter=80):
    """Gauss-Newton at 60 digits to a step below tol: its fixed point is where J^T r = 0, the stationary point of the cost.
    -> (R*, t*, iterations, last step norm) or None when it does not converge."""
    for it in range(max_iter):
        acc, _ = normal_equations(R, t, Xs, uvs)
        if acc is None:
            return None
        d = solve6(unpack_upper(acc), [-v for v in acc[21:27]])
        R = matmul(exp_so3(d[0:3]), R); t = [t[i] + d[3 + i] for i in range(3)]
        dn = mp.sqrt(sum(v * v for v in d))
        if dn < tol:
            return R, t, it + 1, dn
    return None


def pose_distance(Ra, ta, Rb, tb):
    """|(rotation vector of Rb Ra^T, tb - ta)| for nearby poses (the vee of the skew part: exact to third order in the angle)."""
    D = matmul(Rb, transpose(Ra))
    w = [(D[2][1] - D[1][2]) / 2, (D[0][2] - D[2][0]) / 2, (D[1][0] - D[0][1]) / 2]
    return mp.sqrt(sum(v * v for v in w) + sum((tb[i] - ta[i]) ** 2 for i in range(3)))


# ---------------------------------------------------------------- the pool
_pool = None


def pool():
    """At most 16 'spawn' workers (a worker imports this module and nothing of the parent's state).  Start it before anything touches the GPU."""
    global _pool
    if _pool is None:
        env = os.environ.get("OMP_NUM_THREADS", "")
        n = min(MAX_WORKERS, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else MAX_WORKERS,
                int(env) if env.isdigit() and int(env) > 0 else MAX_WORKERS)
        _pool = ProcessPoolExecutor(max_workers=max(1, n), mp_context=multiprocessing.get_context("spawn"))
        list(_pool.map(abs, range(4 * n)))
    return _pool


def shutdown():
    global _pool
    if _pool is not None:
        _pool.shutdown(); _pool = None


# ---------------------------------------------------------------- the stage checker
class _Report:
    def __init__(self):
        self.ratio = {s: 0.0 for s in STAGES}; self.where = {s: "" for s in STAGES}
        self.failures = []; self.excused = 0; self.figures = {}

    def see(self, stage, err, bound, where):
        """err against bound: the ratio enters the stage's worst; a zero bound demands a zero error."""
        if bound == 0:
            r = 0.0 if err == 0 else math.inf
        else:
            r = float(err / bound)
        if not r <= self.ratio[stage]:               # (a NaN ratio is recorded as a failure)
            self.ratio[stage] = r if r == r else math.inf; self.where[stage] = where
        return r

    def fail(self, stage, msg):
        self.failures.append((stage, msg)); self.ratio[stage] = math.inf; self.where[stage] = msg

    def merge(self, o):
        for s in STAGES:
            if not o.ratio[s] <= self.ratio[s]:
                self.ratio[s] = o.ratio[s]; self.where[s] = o.where[s]
        self.failures += o.failures; self.excused += o.excused
        for k, v in o.figures.items():
            self.figures[k] = max(self.figures[k], v) if k in self.figures else v

    def stage_failed(self, stage, limit=1.0):
        return (not self.ratio[stage] <= limit) or any(s == stage for s, _ in self.failures)


def _f64(x):
    return np.float64(x)


def _check_lm(rep, rec, Xs, uvs, who, c_sum, refine, iters_mode):
    """Stages 2-6 on one trace record (a hypothesis or the refinement) whose points are Xs, uvs (60-digit copies of the staged FP64 values).
    c_sum: roundings of the summation (5 for a hypothesis).  iters_mode 'all' or 'ends' (iteration 0 and the last one)."""
    n_it = int(rec[6])
    its = rec[lc_ref.TRACE_HEAD:].reshape(lc_ref.LM_ITERS, lc_ref.TRACE_ITER)
    if n_it < 0 or n_it > lc_ref.LM_ITERS:
        rep.fail("5 decisions", f"{who}: {n_it} iteration records"); return
    if np.any(its[n_it:] != 0):
        rep.fail("5 decisions", f"{who}: records beyond iteration {n_it} are not zero")
    ortho0 = None; accepted = 0; budget = F(0)
    for it in range(n_it):
        r = its[it]
        tag = f"{who} it {it}"
        last = it == n_it - 1
        full = iters_mode == "all" or it == 0 or last
        Rs = M3(V(r[0:9])); ts = V(r[9:12]); lam = F(float(r[12]))
        if ortho0 is None:
            ortho0 = orthonormality(Rs)
        if full:
            if accepted:
                rep.see("6 orthonormal", orthonormality(Rs), ortho0 + K4 * U * budget, tag + " start")
            # ---- stage 2: the normal equations at the recorded start pose
            acc, S = normal_equations(Rs, ts, Xs, uvs)
            if acc is None or not np.all(np.isfinite(r[IT["acc"]])):
                rep.fail("2 normal eq", tag + ": a point with z = 0 or a non-finite entry"); return
            dev = V(r[IT["acc"]])
            for k in range(28):
                rep.see("2 normal eq", abs(dev[k] - acc[k]), ((C_POINT if k < 27 else C_COST) + c_sum) * U * S[k], f"{tag} acc[{k}]")
        # ---- stage 3: the damped solve on the device's own matrix
        A = unpack_upper(V(r[13:34])); g = V(r[34:40])
        M = [[A[i][j] * (1 + lam if i == j else 1) for j in range(6)] for i in range(6)]
        L, piv, part = cholesky(M)
        ok = bool(r[41])
        if r[41] not in (0.0, 1.0):
            rep.fail("3 step", tag + ": flag"); return
        if L is None:
            if ok:
                if abs(piv[-1]) <= GAMMA19 * part:
                    rep.excused += 1
                else:
                    rep.fail("3 step", f"{tag}: Cholesky succeeded where the 60-digit pivot {len(piv) - 1} is {mp.nstr(piv[-1], 5)}")
                    return
            elif not last:
                rep.fail("5 decisions", tag + ": iterations after a failed Cholesky"); return
            if not ok:
                if np.any(r[42:64] != 0):
                    rep.fail("5 decisions", tag + ": entries after a failed Cholesky are not zero")
                return
        LLt = matmul(mabs(L), mabs(transpose(L))) if L is not None else None
        if not ok:
            if any(piv[j] <= GAMMA19 * LLt[j][j] for j in range(6)):
                rep.excused += 1
            else:
                rep.fail("3 step", f"{tag}: Cholesky failed where every 60-digit pivot is clear of 0")
            if not last:
                rep.fail("5 decisions", tag + ": iterations after a failed Cholesky")
            return
        if not np.all(np.isfinite(r[42:62])):
            rep.fail("3 step", tag + ": non-finite step, candidate or cost"); return
        d = V(r[IT["d"]])
        if LLt is not None:
            for i in range(6):
                res = sum(M[i][j] * d[j] for j in range(6)) + g[i]
                bound = GAMMA19 * sum(LLt[i][j] * abs(d[j]) for j in range(6)) + U * abs(M[i][i] * d[i])
                rep.see("3 step", abs(res), bound, f"{tag} row {i}")
        # ---- stage 4: the candidate pose
        Rc = M3(V(r[48:57])); tc = V(r[57:60])
        Sc = matmul(exp_so3_scale(d[0:3]), mabs(Rs))
        if full:
            E = exp_so3(d[0:3]); Rx = matmul(E, Rs)
            for i in range(3):
                for j in range(3):
                    raw = rep.see("4 candidate", abs(Rc[i][j] - Rx[i][j]), K4 * U * Sc[i][j], f"{tag} Rc[{i}][{j}]") * K4
                    rep.figures["stage4_raw"] = max(rep.figures.get("stage4_raw", 0.0), raw)
                raw = rep.see("4 candidate", abs(tc[i] - (ts[i] + d[3 + i])), K4 * U * (abs(ts[i]) + abs(d[3 + i])), f"{tag} tc[{i}]") * K4
                rep.figures["stage4_raw"] = max(rep.figures.get("stage4_raw", 0.0), raw)
            # ---- stage 2 again: the candidate's cost
            cc, Sc_ = cost(Rc, tc, Xs, uvs)
            if cc is None:
                rep.fail("2 normal eq", tag + ": a candidate point with z = 0"); return
            rep.see("2 normal eq", abs(F(float(r[60])) - cc), (C_COST + c_sum) * U * Sc_, tag + " cc")
        # ---- stage 5: the decisions, replayed exactly
        acc_flag = bool(r[62])
        if r[62] not in (0.0, 1.0) or r[63] not in (0.0, 1.0):
            rep.fail("5 decisions", tag + ": flag"); return
        if acc_flag != bool(r[60] < r[61]):
            rep.fail("5 decisions", f"{tag}: accepted = {acc_flag} with cc = {r[60]!r}, cost = {r[61]!r}")
        accepted += acc_flag
        nxt_pose = r[48:60] if acc_flag else r[0:12]
        nxt_cost = r[60] if acc_flag else r[61]
        nxt_lam = _f64(r[12]) / _f64(10.0) if acc_flag else _f64(r[12]) * _f64(10.0)
        tn = V(nxt_pose[9:12])
        dn = mp.sqrt(sum(v * v for v in d)); thr = FLT_EPS * max(F(1), mp.sqrt(sum(v * v for v in tn)))
        if bool(r[63]) != bool(dn < thr):
            if abs(dn / thr - 1) <= 4 * U:
                rep.excused += 1
            else:
                rep.fail("5 decisions", f"{tag}: stop = {bool(r[63])} with |d| / threshold = {mp.nstr(dn / thr, 20)}")
        if acc_flag:      # an entrywise error e <= K4 u Sc of the candidate moves R^T R by 2 sum_k |R_ki| e_kj to first order: the step's scale
            budget += 2 * max(sum(abs(Rc[k][i]) * Sc[k][j] for k in range(3)) for i in range(3) for j in range(3))
            if full:
                rep.see("6 orthonormal", orthonormality(Rc), ortho0 + K4 * U * budget, tag + " candidate")
        if last:
            if not (bool(r[63]) or it == lc_ref.LM_ITERS - 1):
                rep.fail("5 decisions", tag + ": the last record neither stops nor is iteration 19")
            if not np.array_equal(rec[8:20].view(np.uint64), np.ascontiguousarray(nxt_pose).view(np.uint64)):
                rep.fail("5 decisions", who + ": the final pose is not the pose after the last decision")
        else:
            q = its[it + 1]
            if bool(r[63]):
                rep.fail("5 decisions", tag + ": iterations after a stop")
            if not np.array_equal(np.ascontiguousarray(q[0:12]).view(np.uint64), np.ascontiguousarray(nxt_pose).view(np.uint64)):
                rep.fail("5 decisions", tag + ": the next start pose is neither the candidate nor the old pose, bit for bit")
            if _f64(q[12]).tobytes() != nxt_lam.tobytes():
                rep.fail("5 decisions", f"{tag}: the next lambda is {q[12]!r}, not {nxt_lam!r}")
            if _f64(q[61]).tobytes() != _f64(nxt_cost).tobytes():
                rep.fail("5 decisions", tag + ": the next current cost")
    if n_it:
        if its[0][12] != lc_ref.LAMBDA0:
            rep.fail("5 decisions", who + ": lambda0")
        c0 = its[0][40] if refine else rec[7]
        if _f64(its[0][61]).tobytes() != _f64(c0).tobytes() or (refine and _f64(rec[7]).tobytes() != _f64(c0).tobytes()):
            rep.fail("5 decisions", who + ": the first current cost is not the initial cost")


def _work_hyps(task):
    """Stages 0-7 of a chunk of hypotheses."""
    mp.mp.dps = DPS
    rep = _Report()
    X = task["X"]; uv = task["uv"]; n = len(X)
    Xm = [V(x) for x in X]; uvm = [V(x) for x in uv]
    tic = V(task["tic"]); ric = M3(V(task["ric"]))
    R0, t0, dR0, dt0 = prior_pose(task["pair"], tic, ric)
    for h, rec, count in zip(task["hyps"], task["recs"], task["counts"]):
        who = f"hyp {h}"
        want = lc_ref.draw(task["seed"], h, n)
        s = [int(v) for v in rec[0:5]]
        drew = bool(rec[20])
        if (want is None) != (not drew) or (want is not None and s != list(want)) or (want is None and s != [-1] * 5):
            rep.fail("1 samples", f"{who}: samples {s}, lc_ref.draw gives {want}"); continue
        n_it = int(rec[6])
        its = rec[lc_ref.TRACE_HEAD:].reshape(lc_ref.LM_ITERS, lc_ref.TRACE_ITER)
        valid = bool(rec[5])
        chol_failed = n_it > 0 and its[n_it - 1][41] == 0.0
        if valid != (drew and bool(np.isfinite(rec[7])) and not chol_failed):
            rep.fail("1 samples", f"{who}: valid = {valid} with draw {drew}, initial cost {rec[7]!r}, pivot failure {chol_failed}")
        if (count >= 0) != valid:
            rep.fail("7 counts", f"{who}: count {count} with valid = {valid}")
        if not drew:
            if rec[6] != 0 or np.any(rec[lc_ref.TRACE_HEAD:] != 0):
                rep.fail("1 samples", who + ": iteration records after a failed draw")
            continue
        Xs = [Xm[i] for i in s]; us = [uvm[i] for i in s]
        if not np.isfinite(rec[7]):
            if n_it:
                rep.fail("1 samples", who + ": iterations after a non-finite initial cost")
            continue
        # ---- stage 0: the prior pose, where iteration 0 starts (or the final pose when no iteration ran)
        p0 = its[0][0:12] if n_it else rec[8:20]
        P = V(p0)
        for i in range(3):
            for j in range(3):
                rep.see("0 prior", abs(P[3 * i + j] - R0[i][j]), dR0[i][j], f"{who} R0[{i}][{j}]")
            rep.see("0 prior", abs(P[9 + i] - t0[i]), dt0[i], f"{who} t0[{i}]")
        # ---- stage 2: the initial cost
        c0, S0 = cost(M3(P[0:9]), P[9:12], Xs, us)
        if c0 is None:
            rep.fail("2 normal eq", who + ": finite initial cost with a z = 0")
        else:
            rep.see("2 normal eq", abs(F(float(rec[7])) - c0), (C_COST + 5) * U * S0, who + " initial cost")
        _check_lm(rep, rec, Xs, us, who, 5, False, task["iters_mode"])
        # ---- stage 7: the inlier count at the recorded final pose
        if valid:
            Rf = M3(V(rec[8:17])); tf = V(rec[17:20])
            c60 = 0; border = 0
            for j in range(n):
                z, e = inlier_error(Rf, tf, Xm[j], uvm[j])
                if e is None:
                    continue
                if z > 0 and e <= 1:
                    c60 += 1
                if abs(e - 1) <= BORDER or abs(z) <= BORDER:
                    border += 1
            if c60 != count:
                if abs(c60 - count) <= border:
                    rep.excused += abs(c60 - count)
                else:
                    rep.fail("7 counts", f"{who}: count {count}, 60-digit count {c60} ({border} borderline)")
    return rep


def _work_refine(task):
    """Stages 2-6 of the refinement, the mask (stage 7), the finish (stage 9) and the minimiser (stage 10)."""
    mp.mp.dps = DPS
    rep = _Report()
    X = task["X"]; uv = task["uv"]; n = len(X)
    Xm = [V(x) for x in X]; uvm = [V(x) for x in uv]
    rec = task["rec"]; best_pose = task["best_pose"]; mask = task["mask"]; res = task["result"]
    tic = V(task["tic"]); ric = M3(V(task["ric"]))
    if task["part"] == "mask":
        Rb = M3(V(best_pose[0:9])); tb = V(best_pose[9:12])
        for j in range(n):
            z, e = inlier_error(Rb, tb, Xm[j], uvm[j])
            want = e is not None and z > 0 and e <= 1
            if want != bool(mask[j]):
                if e is not None and (abs(e - 1) <= BORDER or abs(z) <= BORDER):
                    rep.excused += 1
                else:
                    rep.fail("7 counts", f"mask: match {j} is {int(mask[j])}, 60-digit e / thr^2 = {mp.nstr(e, 20) if e is not None else None}, z = {mp.nstr(z, 5)}")
        if int(mask.sum()) != res["n_inliers"]:
            rep.fail("7 counts", f"n_inliers {res['n_inliers']} is not the mask's {int(mask.sum())}")
        return rep
    idx = np.flatnonzero(mask)
    Xs = [Xm[i] for i in idx]; us = [uvm[i] for i in idx]
    Rp = M3(V(rec[8:17])); tp = V(rec[17:20])
    if task["part"] == "lm":
        if not np.array_equal(np.ascontiguousarray(rec[20:32]).view(np.uint64), np.ascontiguousarray(best_pose).view(np.uint64)):
            rep.fail("5 decisions", "refinement: the start pose is not the chosen hypothesis's final pose, bit for bit")
        if int(rec[6]) and not np.array_equal(np.ascontiguousarray(rec[lc_ref.TRACE_HEAD:lc_ref.TRACE_HEAD + 12]).view(np.uint64),
                                              np.ascontiguousarray(rec[20:32]).view(np.uint64)):
            rep.fail("5 decisions", "refinement: iteration 0 does not start at the start pose")
        if rec[5] != 1.0 or int(rec[6]) < 1:
            rep.fail("5 decisions", "refinement: did not run")
        _check_lm(rep, rec, Xs, us, "refinement", -(-n // 256) + 9, True, task["iters_mode"])
        return rep
    if task["part"] == "finish":
        f = _finish(Rp, tp, task["pair"], tic, ric, res["n_inliers"])
        for name in ("PnP_T_old", "PnP_q_old", "loop_info"):
            dev = V(res[name])
            if name not in f:
                if np.any(np.asarray(res[name]) != 0):
                    rep.fail("9 finish", name + " is written although the inlier gate failed")
                continue
            val, bnd = f[name]
            for k in range(len(val)):
                rep.see("9 finish", abs(dev[k] - val[k]), bnd[k], f"{name}[{k}]")
            if name == "loop_info":
                rep.figures["yaw_raw"] = float(abs(dev[7] - val[7]) / (U * f["yaw_scale"]))
        want = lc_ref.REASON["FEW_INLIERS"]
        if "gates" in f:
            ay, dy, tn, dtn = f["gates"]
            if abs(ay - 30) <= dy or abs(tn - 20) <= dtn:
                rep.excused += 1; want = res["reason"]
            else:
                want = lc_ref.REASON["YAW_GATE"] if not ay < 30 else lc_ref.REASON["T_GATE"] if not tn < 20 else lc_ref.REASON["ACCEPTED"]
        if res["reason"] != want or res["accepted"] != int(want == lc_ref.REASON["ACCEPTED"]):
            rep.fail("9 finish", f"reason {res['reason']} / accepted {res['accepted']}, the 60-digit gates give {want}")
        return rep
    # part == "minimiser"
    m = minimiser(Rp, tp, Xs, us)
    if m is None:
        rep.fail("10 minimiser", "the 60-digit Gauss-Newton did not converge"); return rep
    Rm, tm, n_gn, _ = m
    rep.figures["distance"] = float(pose_distance(Rp, tp, Rm, tm))
    rep.figures["floor"] = float(FLT_EPS * max(F(1), mp.sqrt(sum(v * v for v in tp))))
    rep.figures["gn_iterations"] = n_gn
    return rep


def check_trace(trace, pair, extrinsic, iters_mode="all", hyps=None, ref=None, name="", use_pool=True):
    """trace: dict(raw [TRACE_LEN] doubles, result (the uvs_lc_result fields), match_old [nq], inlier [nq]) of uvs_lc_debug_pair or of
    lc_ref.verify(trace=True); pair and extrinsic (tic, qic) as given to the call.  iters_mode 'ends' checks stages 2, 4 and 6 only at iteration 0
    and the last iteration of every record (the decisions and the solve are checked at every iteration either way); hyps restricts stages 0-7 to
    some hypotheses (the planted-error tests).  ref: (result, raw) of lc_ref on the same pair, computed here when None.
    -> _Report: ratio / where per stage, failures [(stage, text)], excused, figures."""
    raw = np.asarray(trace["raw"], np.float64); res = trace["result"]
    tic, qic = extrinsic
    ric = lc_ref.quat_to_R(qic)                   # the extrinsic rotation as the call computes it on the host (the same FP64 formula)
    rep = _Report()
    recs = raw[:lc_ref.TRACE_STAGE].reshape(lc_ref.N_HYP + 1, lc_ref.TRACE_REC)
    st = raw[lc_ref.TRACE_STAGE:]
    n = int(st[0]); Q = lc_ref.MAX_QUERY
    X = st[1:1 + 3 * Q].reshape(Q, 3)[:n].copy(); uv = st[1 + 3 * Q:1 + 5 * Q].reshape(Q, 2)[:n].copy(); mq = st[1 + 5 * Q:1 + 6 * Q][:n].astype(np.int64)
    # the staged inputs are the call's own inputs: exact copies
    mo = np.asarray(trace["match_old"]); mi = np.flatnonzero(mo >= 0)
    p3d = np.asarray(pair["p3d"], np.float64).reshape(-1, 3); uvo = np.asarray(pair["uv"], np.float64).reshape(-1, 2)
    if n != res["n_matches"] or n != len(mi) or not np.array_equal(mq, mi) or not np.array_equal(X.view(np.uint64), p3d[mi].view(np.uint64)) \
            or not np.array_equal(uv.view(np.uint64), uvo[mo[mi]].view(np.uint64)):
        rep.fail("1 samples", "the staged matches are not the matched inputs in query order")
        return rep
    if np.any(st[1 + 3 * n:1 + 3 * Q] != 0) or np.any(st[1 + 3 * Q + 2 * n:1 + 5 * Q] != 0) or np.any(st[1 + 5 * Q + n:] != 0):
        rep.fail("1 samples", "staged entries beyond n are not zero")
    counts = np.asarray(res["hyp_inliers"])
    if n <= lc_ref.MIN_LOOP_NUM:
        if np.any(recs != 0) or np.any(counts != -1):
            rep.fail("1 samples", "trace entries written although gate 1 failed")
        return rep
    seed = int(pair["seed"]) & lc_ref.M64
    base = dict(X=X, uv=uv, tic=np.asarray(tic, np.float64), ric=ric, pair=dict(vio_t=np.asarray(pair["vio_t"], np.float64), vio_q=np.asarray(pair["vio_q"], np.float64)),
                seed=seed, iters_mode=iters_mode)
    hs = list(range(lc_ref.N_HYP)) if hyps is None else list(hyps)
    tasks = []
    chunk = 2
    for a in range(0, len(hs), chunk):
        hh = hs[a:a + chunk]
        tasks.append((_work_hyps, dict(base, hyps=hh, recs=[recs[h].copy() for h in hh], counts=[int(counts[h]) for h in hh])))
    # ---- stage 8: the selection on the device's counts
    best, iters = lc_ref.select(counts, n)
    if (res["best_hypothesis"], res["ransac_iters"]) != (best, iters):
        rep.fail("8 selection", f"best {res['best_hypothesis']} after {res['ransac_iters']}, lc_ref.select gives {best} after {iters}")
    inl = np.asarray(trace["inlier"])
    if np.any(inl[mo < 0] != 0):
        rep.fail("7 counts", "an unmatched query is in the mask")
    ref_rep = None
    if best < 0 or res["best_hypothesis"] != best:
        if np.any(recs[lc_ref.N_HYP] != 0) or np.any(inl != 0) or res["reason"] != lc_ref.REASON["RANSAC_FAILED"] or res["n_inliers"] != 0 \
                or np.any(np.asarray(res["loop_info"]) != 0) or np.any(np.asarray(res["PnP_T_old"]) != 0):
            rep.fail("8 selection", "entries after a failed selection are written")
    else:
        mask = inl[mq].astype(bool)
        rb = dict(base, rec=recs[lc_ref.N_HYP].copy(), best_pose=recs[best][8:20].copy(), mask=mask,
                  result={k: (np.asarray(v).copy() if isinstance(v, np.ndarray) else v) for k, v in res.items() if k != "margin"})
        for part in ("mask", "lm", "finish", "minimiser"):
            tasks.append((_work_refine, dict(rb, part=part)))
        if ref is None:
            r_out, r_raw = lc_ref.verify(pair, tic, qic, trace=True)
        else:
            r_out, r_raw = ref
        if r_out["best_hypothesis"] >= 0:
            r_recs = r_raw[:lc_ref.TRACE_STAGE].reshape(lc_ref.N_HYP + 1, lc_ref.TRACE_REC)
            r_mi = np.flatnonzero(r_out["match_old"] >= 0)
            ref_task = dict(base, X=p3d[r_mi], uv=uvo[r_out["match_old"][r_mi]], rec=r_recs[lc_ref.N_HYP].copy(), best_pose=None,
                            mask=r_out["inlier"][r_mi].astype(bool), result=None, part="minimiser")
            tasks.append((_work_refine, ref_task)); ref_rep = len(tasks) - 1
    if use_pool:
        futs = [pool().submit(fn, t) for fn, t in tasks]
        outs = [f.result() for f in futs]
    else:
        outs = [fn(t) for fn, t in tasks]
    for i, o in enumerate(outs):
        if i == ref_rep:
            if o.failures:
                rep.fail("10 minimiser", "lc_ref: " + o.failures[0][1])
            else:
                rep.figures["ref_distance"] = o.figures["distance"]
            continue
        rep.merge(o)
    # ---- stage 10: the distance to the minimiser against lc_ref's own
    if "distance" in rep.figures and "ref_distance" in rep.figures:
        bound = max(2 * rep.figures["ref_distance"], rep.figures["floor"])
        rep.see("10 minimiser", F(rep.figures["distance"]), F(bound), f"distance {rep.figures['distance']:.3e}, lc_ref's {rep.figures['ref_distance']:.3e}, floor {rep.figures['floor']:.3e}")
    if name:
        for s in STAGES:
            log(f"{name:28s} {s:14s} worst error / bound {rep.ratio[s]:.3e}  {rep.where[s]}")
        log(f"{name:28s} excused {rep.excused}; " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(rep.figures.items())))
    return rep


_log = []


def log(line):
    _log.append(line)


def write_log():
    """Every figure logged so far -> the file UVS_LC_LOG names (the test modules' fixtures call this at their end)."""
    path = os.environ.get("UVS_LC_LOG")
    if path and _log:
        with open(path, "a") as f:
            f.write("\n".join(_log) + "\n")
    del _log[:]
