"""60-digit reference of the residual blocks of the sliding-window solve (what uvs_evaluate dumps per block).

TEST INFRASTRUCTURE ONLY; mpmath + numpy, nothing else: it shares no code with csrc/uvs_factors.h, the oracle, pyref.py or
lm_step_ref.projection_block.  Every family is restated from its definition (vins_estimator/src/factor/*) at mp.dps = 60:

  point   projection_factor.cpp / projection_td_factor.cpp: p_cj = q_ic^-1 (Q_j^-1 (Q_i (q_ic p_i / lambda + t_ic) + P_i - P_j) - t_ic),
          r = sqrt_info (p_cj.xy / p_cj.z - p_j.xy); with a time offset the observations are first shifted by (td - td_k) velocity_k.
          Quaternions act as Eigen's do: q v is the (unnormalised) rotation polynomial, q^-1 = conjugate / squared norm.
  line    line_projection_factor.h: Pluecker line (n_w, d_w) = (cos phi U e_x, sin phi U e_y), U = Rx Ry Rz of the first three parameters,
          moved into the camera, r = line_factor (sp . n_c, ep . n_c) / sqrt(n_x^2 + n_y^2).  R(q) is the UNNORMALISED polynomial (Appendix D1).
  VP      vp_projection_factor.h: r = vp_factor acos(|d_c . v| / (|d_c| |v|)).  The angle is evaluated as atan2(|d_c x v|, |d_c . v|) and
          1 - c^2 as |d_c x v|^2 / (|d_c|^2 |v|^2): the same functions without the cancellation at c -> 1, so that the reference keeps its
          digits exactly where the FP64 formulation loses them.  1 - c^2 <= 1e-14: the documented deviation D8, zero Jacobian.
  IMU     integration_base.h:160-186 with the first-order bias correction, whitened by W = chol_lower(cov^-1)^T (imu_factor.h:64).
          synth's covariances are asymmetric by an ulp or so; the reference (Eigen: inverse() = PartialPivLU of the whole matrix, LLT reads
          the lower triangle), the oracle (inverse_lu of the whole matrix, chol_lower reads the lower triangle) and the kernel
          (imu_whiten_block: Gauss-Jordan on the whole matrix, the Cholesky lanes read the lower triangle of the inverse) all invert the
          FULL matrix and factor the LOWER triangle of the inverse; so does this module.
  loss    Cauchy, rho'' < 0: Ceres' corrector scales residual and Jacobian rows by sqrt(rho'(|r|^2)); cost = sum rho / 2.
  prior   marginalization_factor.cpp:333-381: r = r0 + J0 dx, dx of a pose block = (p - p0, 2 sign(e.w) e.xyz), e = q0^-1 q.

Jacobians are CENTRAL DIFFERENCES at 60 digits (h = 1e-25, truncation ~ 1e-50) in the convention each family is consumed in: tangent steps
P += dp, Q <- Q (x) (dtheta / 2, 1) for point and IMU blocks, raw (qx, qy, qz) with qw fixed for line and VP blocks.  No derivative formula
is written down here, with the exceptions that are not derivatives in the reference either:
  * the (O_R, O_BG) block of the IMU Jacobian (imu_factor.h:128: -Qleft(Q_j^-1 Q_i delta_q).bottomRight3x3 dq_dbg, with delta_q where the
    residual uses the corrected one): the reference's expression, evaluated at 60 digits; its distance from the derivative is recorded;
  * the (O_R, O_R) block of pose i (imu_factor.h:101): the corrected delta_q is not a unit quaternion (Utility::deltaQ does not normalise),
    the residual divides by its squared norm (Eigen inverse()) and the reference's expression does not, so that expression is EXACTLY
    |Q_j^-1 Q_i corrected_delta_q|^2 = 1 / |q_e|^2 times the derivative (|corrected_delta_q|^2 = 1 + |dq_dbg dbg|^2 / 4 for unit frame
    quaternions).  The reference value is the central difference times that factor (no formula needed); the factor - 1 is recorded;
  * the zero Jacobian inside the VP guard (D8).

`evaluate` returns per robust flag an object with the fields of abi.Eval (lm_step_ref.System / normal_equations accept it) plus, per array,
  level[name]  the largest deviation of the reference when every input double of the block is moved by +-1 ulp at random (`draws` draws):
               the conditioning of the block as a function;
  model[name]  where the reference's FORMULATION is worse conditioned than the function (derivations: DESIGN.md section 4):
               VP     dJ = |J| dc / (1 - c^2), dr = vp_factor dc / sqrt(1 - c^2), dc = 4 x 2^-53 (the dot product, the two norms, their product);
               point  J = reduce * jaco keeps POINT_G x 2^-53 of the absolute sum of the two terms of a row (far points, no parallax);
               IMU    the analytic blocks are derivatives for unit frame quaternions only: IMU_Q (| |Qi|^2 - 1 | + | |Qj|^2 - 1 |) |W| |J_raw|.
The metric and the bound of DESIGN.md section 4 (`check`) are computed from these alone: neither the oracle nor the device enters a number.

Residual-only mode (`jacobians=False` of tasks_of / block_task / evaluate; what tests/lm_accept_ref.py evaluates candidate costs with): no central differences; r, cost,
the level of r and the residual models are those of the full mode bit for bit (the +-1 ulp draws consume the generator identically), the Jacobians are zero, and
the blocks' costs are also summed at 60 digits (Ref.cost_mp).  `relo=True` adds the relocalization blocks (family 'relo': a point block on Pose[start frame of the
landmark], relo_Pose, Ex_Pose and the landmark, never a td factor), which uvs_evaluate and the default mode skip.  Measured on the canonical window with a
prior (750 point, 280 line / VP and 10 IMU blocks, n = 75): 1.5 s serially without levels, 2.5 s on 8 workers with four draws per block; the full mode takes 2.1 s
serially for a tenth of the blocks without levels.
"""
import os
from concurrent.futures import ProcessPoolExecutor
import multiprocessing

import numpy as np
import mpmath as mp
from mpmath import mpf

DPS = 60
H = "1e-25"
EPS = 2.0 ** -53
VP_DC = 4 * EPS
POINT_G = 8      # roundings on the path of one term of reduce * jaco: the reciprocal of z, two products of reduce, three of the matrix-vector product, two of the chain factor
IMU_Q = 2        # the IMU Jacobian's analytic blocks are derivatives on the unit sphere only: off by IMU_Q (| |Qi|^2 - 1 | + | |Qj|^2 - 1 |) of their size
VP_GUARD = 1e-14
FLOOR = 1e-13
MAX_WORKERS = 16

mp.mp.dps = DPS


# ---------------------------------------------------------------- small algebra on lists of mpf
def _v(a):
    return [mpf(float(x)) for x in np.asarray(a, np.float64).ravel()]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _add(a, b):
    return [x + y for x, y in zip(a, b)]


def _sub(a, b):
    return [x - y for x, y in zip(a, b)]


def _qmul(a, b):      # (x, y, z, w), Hamilton product
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
            aw * bw - ax * bx - ay * by - az * bz]


def _qinv(q):         # Eigen inverse(): conjugate / squared norm
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return [-q[0] / n2, -q[1] / n2, -q[2] / n2, q[3] / n2]


def _qrot(q, v):      # Eigen operator*: v + 2 w (u x v) + 2 u x (u x v), the rotation polynomial of an unnormalised quaternion
    u = q[:3]
    t = [2 * c for c in _cross(u, v)]
    c2 = _cross(u, t)
    return [v[i] + q[3] * t[i] + c2[i] for i in range(3)]


def _qmat(q):         # columns = images of the unit vectors
    cols = [_qrot(q, e) for e in ([mpf(1), mpf(0), mpf(0)], [mpf(0), mpf(1), mpf(0)], [mpf(0), mpf(0), mpf(1)])]
    return [[cols[j][i] for j in range(3)] for i in range(3)]


def _mtv(M, v):
    return [M[0][i] * v[0] + M[1][i] * v[1] + M[2][i] * v[2] for i in range(3)]


def _tangent(pose, k, s):
    """pose (7) with tangent coordinate k moved by s: P += dp (k < 3), Q <- Q (x) (dtheta / 2, 1)."""
    p = list(pose)
    if k < 3:
        p[k] = p[k] + s
    else:
        dq = [mpf(0), mpf(0), mpf(0), mpf(1)]; dq[k - 3] = s / 2
        p[3:7] = _qmul(pose[3:7], dq)
    return p


def _central(f, n, h):
    """J[row][k] of f(k, s) -> residual list (parameter k moved by s)."""
    cols = []
    for k in range(n):
        a, b = f(k, h), f(k, -h)
        cols.append([(x - y) / (2 * h) for x, y in zip(a, b)])
    return [[cols[k][i] for k in range(n)] for i in range(len(cols[0]))]


def _cauchy(a, r, J):
    """-> (rho, scaled r, scaled J) of CauchyLoss(a) under Ceres' corrector (rho'' < 0: rows scaled by sqrt(rho'))."""
    s = sum(x * x for x in r); b = a * a
    k = mp.sqrt(1 / (1 + s / b))
    return b * mp.log(1 + s / b), [k * x for x in r], [[k * x for x in row] for row in J], k


def _f(x):
    return np.array([[float(v) for v in row] for row in x]) if x and isinstance(x[0], list) else np.array([float(v) for v in x])


def _ulp(a, rng):
    """Every double of `a` moved by one ulp up or down at random."""
    a = np.asarray(a, np.float64)
    up = rng.integers(0, 2, a.shape).astype(bool)
    return np.where(up, np.nextafter(a, np.inf), np.nextafter(a, -np.inf))


def _perturb(d, keys, rng):
    o = dict(d)
    for k in keys:
        o[k] = _ulp(d[k], rng)
    return o


# ---------------------------------------------------------------- point
def _point_res(pi_, pj_, ex, lam, a, b, vi, vj, tdi, tdj, td, sq, use_td):
    if use_td:
        a = [a[0] - (td - tdi) * vi[0], a[1] - (td - tdi) * vi[1], a[2]]
        b = [b[0] - (td - tdj) * vj[0], b[1] - (td - tdj) * vj[1], b[2]]
    pci = [x / lam for x in a]
    pbi = _add(_qrot(ex[3:], pci), ex[:3])
    pw = _add(_qrot(pi_[3:], pbi), pi_[:3])
    pbj = _qrot(_qinv(pj_[3:]), _sub(pw, pj_[:3]))
    pcj = _qrot(_qinv(ex[3:]), _sub(pbj, ex[:3]))
    return [sq * (pcj[0] / pcj[2] - b[0]), sq * (pcj[1] / pcj[2] - b[1])], pcj


def _point_once(d, h, jac=True):
    pi_, pj_, ex = _v(d["pose_i"]), _v(d["pose_j"]), _v(d["ex"])
    lam = mpf(float(d["lam"])); a, b = _v(d["pi"]), _v(d["pj"])
    vi, vj = _v(d["vi"]), _v(d["vj"]); tdi, tdj, td = mpf(float(d["tdi"])), mpf(float(d["tdj"])), mpf(float(d["td"]))
    sq = mpf(d["sqrt_info"]); use_td = d["use_td"]
    if d.get("unit_q"):      # the three quaternions normalised at working precision (the comparison with lm_step_ref.projection_block, which normalises)
        for p in (pi_, pj_, ex):
            n = mp.sqrt(sum(c * c for c in p[3:]))
            p[3:] = [c / n for c in p[3:]]

    def f(k, s):      # residual (2) and the camera-frame point (3): one evaluation serves the Jacobian and the cancellation model
        if k < 6: o = _point_res(_tangent(pi_, k, s), pj_, ex, lam, a, b, vi, vj, tdi, tdj, td, sq, use_td)
        elif k < 12: o = _point_res(pi_, _tangent(pj_, k - 6, s), ex, lam, a, b, vi, vj, tdi, tdj, td, sq, use_td)
        elif k < 18: o = _point_res(pi_, pj_, _tangent(ex, k - 12, s), lam, a, b, vi, vj, tdi, tdj, td, sq, use_td)
        elif k == 18: o = _point_res(pi_, pj_, ex, lam + s, a, b, vi, vj, tdi, tdj, td, sq, use_td)
        else: o = _point_res(pi_, pj_, ex, lam, a, b, vi, vj, tdi, tdj, td + s, sq, use_td)
        return o[0] + o[1]
    r, pc = _point_res(pi_, pj_, ex, lam, a, b, vi, vj, tdi, tdj, td, sq, use_td)
    if not jac:      # residual-only: what the Jacobian does not enter (r, the loss, the cost) as in the full mode; J and its model stay zero
        rho, rr, _, ks = _cauchy(mpf(d["loss"]), r, [])
        z20 = np.zeros((2, 20))
        return dict(r=[_f(r), _f(rr)], J=[z20, z20], mJ=[z20, z20], cost=[float(sum(x * x for x in r)) / 2, float(rho) / 2], cost_mp=[sum(x * x for x in r) / 2, rho / 2],
                    aux=dict(depth_j=float(pc[2]), lam=float(lam)))
    J5 = _central(f, 20 if use_td else 19, h)
    if not use_td: J5 = [row + [mpf(0)] for row in J5]
    J = J5[:2]
    # model: the reference forms J = reduce * jaco with reduce = sqrt_info [1/z, 0, -x/z^2; 0, 1/z, -y/z^2] (projection_factor.cpp:90-93); where
    # the two terms of a row cancel (far points, p_cj nearly parallel to d p_cj) the product keeps POINT_G x eps of their absolute sum
    z = pc[2]
    mJ = [[POINT_G * EPS * float(sq * (abs(J5[2 + i][k] / z) + abs(pc[i] * J5[4][k] / (z * z)))) for k in range(20)] for i in range(2)]
    rho, rr, Jr, ks = _cauchy(mpf(d["loss"]), r, J)
    mJ = np.array(mJ)
    if d.get("keep_mp"): return dict(r=[r, rr], J=[J, Jr], mJ=[mJ, mJ * float(ks)])
    return dict(r=[_f(r), _f(rr)], J=[_f(J), _f(Jr)], mJ=[mJ, mJ * float(ks)], cost=[float(sum(x * x for x in r)) / 2, float(rho) / 2], aux=dict(depth_j=float(z), lam=float(lam)))


# ---------------------------------------------------------------- line + VP
def _line_cam(x, qw, ex):
    t, q = x[0:3], [x[3], x[4], x[5], qw]
    a, b, c, phi = x[6:10]
    ric = _qmat(ex[3:]); R = _qmat(q)
    Rwc = [[sum(R[i][k] * ric[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    twc = _add(_qrot(q, ex[:3]), t)
    sa, ca, sb, cb, sc, cc = mp.sin(a), mp.cos(a), mp.sin(b), mp.cos(b), mp.sin(c), mp.cos(c)
    # Rx(a) Ry(b) Rz(c): first and second column
    u0 = [cb * cc, sa * sb * cc + ca * sc, -ca * sb * cc + sa * sc]
    u1 = [-cb * sc, -sa * sb * sc + ca * cc, ca * sb * sc + sa * cc]
    nw = [mp.cos(phi) * v for v in u0]; dw = [mp.sin(phi) * v for v in u1]
    tcw = [-v for v in _mtv(Rwc, twc)]
    dc = _mtv(Rwc, dw)
    nc = _add(_mtv(Rwc, nw), _cross(tcw, dc))
    return nc, dc


def _line_vp_res(x, qw, ex, sp, ep, vp, lf, vf, has_vp):
    nc, dc = _line_cam(x, qw, ex)
    l = mp.sqrt(nc[0] * nc[0] + nc[1] * nc[1])
    out = [lf * _dot(sp, nc) / l, lf * _dot(ep, nc) / l]
    s2 = None
    if has_vp:
        cr = _cross(dc, vp); n2 = _dot(cr, cr); dv = abs(_dot(dc, vp))
        out.append(vf * mp.atan2(mp.sqrt(n2), dv))      # = vf acos(|d . v| / (|d| |v|))
        s2 = n2 / (_dot(dc, dc) * _dot(vp, vp))          # = 1 - c^2
    return out, s2


def _line_once(d, h, jac=True):
    x = _v(d["pose"][:6]) + _v(d["line"]); qw = mpf(float(d["pose"][6])); ex = _v(d["ex"])
    sp, ep, vp = _v(d["sp"]), _v(d["ep"]), _v(d["vp"])
    lf, vf, hv = mpf(d["line_factor"]), mpf(d["vp_factor"]), bool(d["has_vp"])

    def f(k, s):
        y = list(x); y[k] = y[k] + s
        return _line_vp_res(y, qw, ex, sp, ep, vp, lf, vf, hv)[0]
    r, s2 = _line_vp_res(x, qw, ex, sp, ep, vp, lf, vf, hv)
    J = _central(f, 10, h) if jac else [[mpf(0)] * 10 for _ in r]      # residual-only: zero Jacobians, everything else as in the full mode
    rho, rr, Jr, _ = _cauchy(mpf(d["loss_line"]), r[:2], J[:2])
    out = dict(r=[_f(r[:2]), _f(rr)], J=[_f(J[:2]), _f(Jr)], cost=[float(r[0] * r[0] + r[1] * r[1]) / 2, float(rho) / 2])
    if not jac: out["cost_mp"] = [(r[0] * r[0] + r[1] * r[1]) / 2, rho / 2]
    z1, z10 = np.zeros(1), np.zeros((1, 10))
    if hv:
        guarded = s2 <= mpf(VP_GUARD)
        Jv = [[mpf(0)] * 10] if guarded else [J[2]]
        rho, rv, Jvr, k = _cauchy(mpf(d["loss_vp"]), [r[2]], Jv)
        s2f = float(s2); k = float(k)
        mr = float(vf) * VP_DC / np.sqrt(s2f) if s2f > 0 else float(r[2])
        mJ = np.zeros((1, 10)) if guarded else np.abs(_f(Jv)) * (VP_DC / s2f)
        out.update(vr=[_f([r[2]]), _f(rv)], vJ=[_f(Jv), _f(Jvr)], vcost=[float(r[2] * r[2]) / 2, float(rho) / 2],
                   vmr=[np.array([mr]), np.array([mr * k])], vmJ=[mJ, mJ * k], aux=dict(s2=s2f, guarded=bool(guarded)))
        if not jac: out["vcost_mp"] = [r[2] * r[2] / 2, rho / 2]
    else:
        out.update(vr=[z1, z1], vJ=[z10, z10], vcost=[0.0, 0.0], vmr=[z1, z1], vmJ=[z10, z10], aux=dict(s2=float("nan"), guarded=False))
    return out


# ---------------------------------------------------------------- IMU
def _whiten(cov):
    """W = chol_lower(cov^-1)^T: the inverse of the FULL matrix (LU with partial pivoting), the Cholesky factor of its LOWER triangle."""
    A = mp.matrix(15, 15)
    for i in range(15):
        for j in range(15): A[i, j] = mpf(float(cov[i][j]))
    inv = mp.inverse(A)
    L = [[mpf(0)] * 15 for _ in range(15)]
    for j in range(15):
        dsum = inv[j, j] - sum(L[j][k] * L[j][k] for k in range(j))
        L[j][j] = mp.sqrt(dsum)
        for i in range(j + 1, 15):
            L[i][j] = (inv[i, j] - sum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
    return [[L[j][i] for j in range(15)] for i in range(15)]


def _m3(jac, r0, c0, v):
    return [jac[r0 + i][c0] * v[0] + jac[r0 + i][c0 + 1] * v[1] + jac[r0 + i][c0 + 2] * v[2] for i in range(3)]


def _imu_raw(B, G, pi_, sbi, pj_, sbj):
    dt = B["sum_dt"]; jac = B["jac"]
    dba = _sub(sbi[3:6], B["lin_ba"]); dbg = _sub(sbi[6:9], B["lin_bg"])
    th = _m3(jac, 3, 12, dbg)
    cq = _qmul(B["dq"], [th[0] / 2, th[1] / 2, th[2] / 2, mpf(1)])
    cv = _add(B["dv"], _add(_m3(jac, 6, 9, dba), _m3(jac, 6, 12, dbg)))
    cp = _add(B["dp"], _add(_m3(jac, 0, 9, dba), _m3(jac, 0, 12, dbg)))
    qi_inv = _qinv(pi_[3:])
    ap = [G[k] * dt * dt / 2 + pj_[k] - pi_[k] - sbi[k] * dt for k in range(3)]
    av = [G[k] * dt + sbj[k] - sbi[k] for k in range(3)]
    rp = _sub(_qrot(qi_inv, ap), cp)
    qe = _qmul(_qinv(cq), _qmul(qi_inv, pj_[3:]))
    rv = _sub(_qrot(qi_inv, av), cv)
    return rp + [2 * qe[0], 2 * qe[1], 2 * qe[2]] + rv + _sub(sbj[3:6], sbi[3:6]) + _sub(sbj[6:9], sbi[6:9]), cq, qe


def _imu_once(d, h, jac=True):
    B = dict(sum_dt=mpf(float(d["sum_dt"])), dp=_v(d["delta_p"]), dq=_v(d["delta_q"]), dv=_v(d["delta_v"]), lin_ba=_v(d["linearized_ba"]),
             lin_bg=_v(d["linearized_bg"]), jac=[_v(row) for row in np.asarray(d["jacobian"], np.float64).reshape(15, 15)])
    G = [mpf(float(g)) for g in d["G"]]
    pi_, sbi, pj_, sbj = _v(d["pose_i"]), _v(d["sb_i"]), _v(d["pose_j"]), _v(d["sb_j"])

    def f(k, s):
        if k < 6: return _imu_raw(B, G, _tangent(pi_, k, s), sbi, pj_, sbj)[0]
        if k < 15:
            y = list(sbi); y[k - 6] = y[k - 6] + s
            return _imu_raw(B, G, pi_, y, pj_, sbj)[0]
        if k < 21: return _imu_raw(B, G, pi_, sbi, _tangent(pj_, k - 15, s), sbj)[0]
        y = list(sbj); y[k - 21] = y[k - 21] + s
        return _imu_raw(B, G, pi_, sbi, pj_, y)[0]
    raw, cq, qe = _imu_raw(B, G, pi_, sbi, pj_, sbj)
    if not jac:      # residual-only: the whitened residual alone
        W = _whiten(np.asarray(d["covariance"], np.float64).reshape(15, 15))
        r = [sum(W[i][k] * raw[k] for k in range(i, 15)) for i in range(15)]
        z = np.zeros((15, 30)); c = sum(x * x for x in r) / 2
        return dict(r=[_f(r)] * 2, J=[z] * 2, mJ=[z] * 2, cost=[float(sum(x * x for x in r)) / 2] * 2, cost_mp=[c, c], aux=dict(sum_dt=float(B["sum_dt"])), W=_f(W))
    J = _central(f, 30, h)
    # (O_R, O_R) of pose i: the reference's expression is |Q_j^-1 Q_i corrected_delta_q|^2 = 1 / |q_e|^2 times the derivative (module docstring;
    # |corrected_delta_q|^2 when the frame quaternions are unit)
    n2 = 1 / sum(c * c for c in qe)
    for i in range(3, 6):
        for k in range(3, 6): J[i][k] = J[i][k] * n2
    # (O_R, O_BG) of speed/bias i: the reference's expression -Qleft(Qj^-1 Qi delta_q).bottomRight3x3 dq_dbg (imu_factor.h:128)
    qq = _qmul(_qmul(_qinv(pj_[3:]), pi_[3:]), B["dq"])
    La = [[qq[3], -qq[2], qq[1]], [qq[2], qq[3], -qq[0]], [-qq[1], qq[0], qq[3]]]
    true = [[J[3 + i][12 + k] for k in range(3)] for i in range(3)]
    for i in range(3):
        for k in range(3): J[3 + i][12 + k] = -sum(La[i][m] * B["jac"][3 + m][12 + k] for m in range(3))
    dist = max(abs(float(J[3 + i][12 + k] - true[i][k])) for i in range(3) for k in range(3)) / max(abs(float(true[i][k])) for i in range(3) for k in range(3))
    W = _whiten(np.asarray(d["covariance"], np.float64).reshape(15, 15))
    r = [sum(W[i][k] * raw[k] for k in range(i, 15)) for i in range(15)]
    Jw = [[sum(W[i][k] * J[k][c] for k in range(i, 15)) for c in range(30)] for i in range(15)]
    # model: R(q), the polynomial Eigen rotates with, is q v q* - (|q|^2 - 1) v, so it is multiplicative on the unit sphere only, and the reference's
    # blocks skew(Qi^-1 a), Qleft Qright, +-R(Qi^-1) equal the derivative of the residual up to O(|q|^2 - 1) of their size
    dq2 = abs(sum(c * c for c in pi_[3:]) - 1) + abs(sum(c * c for c in pj_[3:]) - 1)
    mJ = _f([[IMU_Q * dq2 * sum(abs(W[i][k] * J[k][c]) for k in range(i, 15)) for c in range(30)] for i in range(15)])
    dbg = _sub(sbi[6:9], B["lin_bg"]); dba = _sub(sbi[3:6], B["lin_ba"])
    aux = dict(dbg=float(mp.sqrt(_dot(dbg, dbg))), dba=float(mp.sqrt(_dot(dba, dba))), or_obg_dist=dist, cq_norm2_minus_1=float(n2 - 1), qe_w=float(qe[3]),
               sum_dt=float(B["sum_dt"]))
    aux["q_offnorm"] = float(dq2)
    return dict(r=[_f(r)] * 2, J=[_f(Jw)] * 2, mJ=[mJ] * 2, cost=[float(sum(x * x for x in r)) / 2] * 2, aux=aux, W=_f(W))


# ---------------------------------------------------------------- prior
def _prior_once(d, h, jac=True):
    n = int(d["n"]); x0 = _v(d["x0"]); r0 = _v(d["r0"]); J0 = np.asarray(d["J0"], np.float64).reshape(n, n)
    dx = [mpf(0)] * n
    neg = []
    for b in range(len(d["size"])):
        size, idx, off = int(d["size"][b]), int(d["idx"][b]), int(d["x0_off"][b])
        x = _v(d["x"][b])
        if size != 7:
            for k in range(size): dx[idx + k] = x[k] - x0[off + k]
        else:
            for k in range(3): dx[idx + k] = x[k] - x0[off + k]
            e = _qmul(_qinv(x0[off + 3:off + 7]), x[3:7])
            sg = 2 if e[3] >= 0 else -2
            neg.append(bool(e[3] < 0))
            for k in range(3): dx[idx + 3 + k] = sg * e[k]
    nz = [k for k in range(n) if dx[k] != 0]
    r = [r0[i] + sum(mpf(float(J0[i, k])) * dx[k] for k in nz) for i in range(n)]
    out = dict(r=[_f(r)] * 2, cost=[float(sum(x * x for x in r)) / 2] * 2, aux=dict(negative_w=neg))
    if not jac:
        # the absolute terms of the quadratic form c0 + g0 . dx + dx . (H0 dx) / 2 the solve evaluates the prior in (`quad`):
        # A = 1/2 sum_k (|r0_k| + sum_j |J0_kj| |dx_j|)^2; and dx itself, for the tests that look at its size
        A = sum((abs(r0[i]) + sum(abs(mpf(float(J0[i, k])) * dx[k]) for k in nz)) ** 2 for i in range(n)) / 2
        c = sum(x * x for x in r) / 2
        out["cost_mp"] = [c, c]; out["aux"] = dict(negative_w=neg, quad_A=float(A), dx=_f(dx), c0=float(sum(x * x for x in r0) / 2))
    return out


_ONCE = dict(pt=_point_once, ln=_line_once, imu=_imu_once, prior=_prior_once, relo=_point_once)
_INPUTS = dict(pt=("pose_i", "pose_j", "ex", "lam", "pi", "pj", "vi", "vj", "tdi", "tdj", "td"), relo=("pose_i", "pose_j", "ex", "lam", "pi", "pj"),
               ln=("pose", "line", "ex", "sp", "ep", "vp"),
               imu=("sum_dt", "delta_p", "delta_q", "delta_v", "linearized_ba", "linearized_bg", "jacobian", "covariance", "pose_i", "sb_i", "pose_j", "sb_j"),
               prior=("x0", "r0", "J0", "x"))
_ARRAYS = dict(pt=("r", "J"), ln=("r", "J", "vr", "vJ"), imu=("r", "J"), prior=("r",), relo=("r", "J"))
_FAMILY_STREAM = {"pt": 1, "ln": 2, "imu": 3, "prior": 4, "relo": 5}


def block_task(task):
    """One residual block: the reference at the inputs as given and, with task['draws'] > 0, the largest deviation over that many +-1 ulp
    re-evaluations.  Runs in a worker process (mpmath + numpy only).  Step task['h'], precision task['dps'].  task['jacobians'] = False: the
    residual-only mode (no central differences: r, cost, the level of r and the residual models as in the full mode, Jacobians zero)."""
    fam, d = task["family"], task["data"]
    mp.mp.dps = task.get("dps", DPS)
    h = mpf(task.get("h", H))
    jac = task.get("jacobians", True)
    base = _ONCE[fam](d, h) if jac else _ONCE[fam](d, h, False)
    names = _ARRAYS[fam] if jac else tuple(nm for nm in _ARRAYS[fam] if nm.endswith("r"))
    if task.get("draws", 0) > 0:
        rng = np.random.default_rng([task["seed"], task["index"], _FAMILY_STREAM[fam]])
        lvl = {nm: [np.zeros_like(base[nm][0]), np.zeros_like(base[nm][1])] for nm in _ARRAYS[fam]}
        for _ in range(task["draws"]):
            if fam == "prior":
                dd = _perturb(d, ("x0", "r0", "J0"), rng); dd["x"] = [_ulp(x, rng) for x in d["x"]]
            else:
                dd = _perturb(d, _INPUTS[fam], rng)
            o = _ONCE[fam](dd, h) if jac else _ONCE[fam](dd, h, False)
            for nm in names:
                for v in range(2): lvl[nm][v] = np.maximum(lvl[nm][v], np.abs(o[nm][v] - base[nm][v]))
        base["level"] = lvl
    mp.mp.dps = DPS
    return task["family"], task["index"], base


# ---------------------------------------------------------------- main process: windows -> tasks -> Eval-shaped results
_pool = None


def pool():
    """The process pool of the reference (at most 16 workers, 'spawn': a worker imports this module, i.e. mpmath and numpy, and nothing of
    the parent's state).  Start it before anything touches the GPU."""
    global _pool
    if _pool is None:
        env = os.environ.get("OMP_NUM_THREADS", "")
        n = min(MAX_WORKERS, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1), int(env) if env.isdigit() and int(env) > 0 else MAX_WORKERS)
        _pool = ProcessPoolExecutor(max_workers=max(1, n), mp_context=multiprocessing.get_context("spawn"))
    return _pool


def shutdown():
    global _pool
    if _pool is not None:
        _pool.shutdown(); _pool = None


class Ref:
    """Fields of abi.Eval (FP64 roundings of the 60-digit values) + level / model (absolute, per entry) + aux (per family, per block)."""

    def __init__(self, w):
        npo, nlo, ni = len(w.pt_lm), len(w.ln_lm), len(w.imu)
        n = w.prior.n if w.prior is not None else 0
        z = lambda *s: np.zeros(s)
        self.pt_r, self.pt_J, self.pt_Jtd = z(npo, 2), z(npo, 2, 19), z(npo, 2)
        self.ln_r, self.ln_J, self.vp_r, self.vp_J = z(nlo, 2), z(nlo, 2, 10), z(nlo, 1), z(nlo, 1, 10)
        self.imu_r, self.imu_J, self.prior_r = z(ni, 15), z(ni, 15, 30), z(max(n, 1))
        self.cost = 0.0
        self.cost_terms = dict(pt=z(npo), ln=z(nlo), vp=z(nlo), imu=z(ni), prior=0.0)
        names = ("pt_r", "pt_J", "pt_Jtd", "ln_r", "ln_J", "vp_r", "vp_J", "imu_r", "imu_J", "prior_r")
        self.level = {nm: np.full(getattr(self, nm).shape, np.nan) for nm in names}      # NaN: not sampled (check() fills in the family's largest)
        self.model = {nm: np.zeros(getattr(self, nm).shape) for nm in names}
        self.have = dict(pt=np.zeros(npo, bool), ln=np.zeros(nlo, bool), imu=np.zeros(ni, bool), prior=False)
        self.aux = dict(pt={}, ln={}, imu={}, prior={})
        self.W = {}


def _opts(o):
    return dict(sqrt_info=float(o.point_sqrt_info), line_factor=float(o.line_factor), vp_factor=float(o.vp_factor), loss=float(o.loss_point),
                loss_line=float(o.loss_line), loss_vp=float(o.loss_vp), G=[float(o.gravity[k]) for k in range(3)], use_td=bool(o.estimate_td))


def tasks_of(w, opts, subset=None, draws=4, level_stride=1, seed=0, dps=DPS, h=H, jacobians=True, relo=False):
    """The block tasks of window `w`.  subset: None (all) or dict(pt=[...], ln=[...], imu=[...], prior=bool).  Every level_stride-th block of a
    family gets its level; blocks named in subset['level'] (dict family -> indices) always do.  jacobians=False: the residual-only mode of
    block_task.  relo=True: the relocalization blocks of the window too (family 'relo'; solve-only blocks, estimator.cpp:944-978: the point block
    between Pose[frame of the landmark's first observation] and relo_Pose, the extrinsic and the landmark, never a td factor)."""
    o = _opts(opts); out = []
    want = lambda fam, n: range(n) if subset is None else subset.get(fam, [])
    force = (subset or {}).get("level", {})
    common = dict(seed=seed, dps=dps, h=h)
    if not jacobians: common["jacobians"] = False
    td_on = o["use_td"] and w.pt_vel_i is not None
    z2 = np.zeros(2)
    for k in want("pt", len(w.pt_lm)):
        fi, fj, lm = int(w.pt_fi[k]), int(w.pt_fj[k]), int(w.pt_lm[k])
        d = dict(pose_i=w.pose[fi], pose_j=w.pose[fj], ex=w.ex_pose, lam=w.inv_depth[lm], pi=w.pt_pi[k], pj=w.pt_pj[k],
                 vi=w.pt_vel_i[k] if td_on else z2, vj=w.pt_vel_j[k] if td_on else z2, tdi=w.pt_td_i[k] if td_on else 0.0, tdj=w.pt_td_j[k] if td_on else 0.0,
                 td=w.td, sqrt_info=o["sqrt_info"], loss=o["loss"], use_td=td_on)
        out.append(dict(family="pt", index=k, data=d, draws=draws if (k % level_stride == 0 or k in force.get("pt", ())) else 0, **common))
    for k in want("ln", len(w.ln_lm)):
        fj, lm = int(w.ln_fj[k]), int(w.ln_lm[k])
        d = dict(pose=w.pose[fj], line=w.line_orth[lm], ex=w.ex_pose, sp=w.ln_sp[k], ep=w.ln_ep[k], vp=w.ln_vp[k], has_vp=int(w.ln_has_vp[k]),
                 line_factor=o["line_factor"], vp_factor=o["vp_factor"], loss_line=o["loss_line"], loss_vp=o["loss_vp"])
        out.append(dict(family="ln", index=k, data=d, draws=draws if (k % level_stride == 0 or k in force.get("ln", ())) else 0, **common))
    for b in want("imu", len(w.imu)):
        blk = w.imu[b]
        if blk.get("skip", 0): continue
        i = int(blk["frame_i"])
        d = {k: np.asarray(blk[k], np.float64) for k in ("sum_dt", "delta_p", "delta_q", "delta_v", "linearized_ba", "linearized_bg", "jacobian", "covariance")}
        d.update(pose_i=w.pose[i], sb_i=w.speedbias[i], pose_j=w.pose[i + 1], sb_j=w.speedbias[i + 1], G=o["G"])
        out.append(dict(family="imu", index=b, data=d, draws=draws, **common))
    if relo and len(w.relo_lm):
        first = {}
        for k in range(len(w.pt_lm)): first.setdefault(int(w.pt_lm[k]), int(w.pt_fi[k]))
        for k in want("relo", len(w.relo_lm)):
            lm = int(w.relo_lm[k])
            d = dict(pose_i=w.pose[first[lm]], pose_j=w.relo_pose, ex=w.ex_pose, lam=w.inv_depth[lm], pi=w.relo_pi[k], pj=w.relo_pj[k], vi=z2, vj=z2, tdi=0.0, tdj=0.0,
                     td=0.0, sqrt_info=o["sqrt_info"], loss=o["loss"], use_td=False)
            out.append(dict(family="relo", index=k, data=d, draws=draws if (k % level_stride == 0 or k in force.get("relo", ())) else 0, **common))
    if w.prior is not None and w.prior.n > 0 and (subset is None or subset.get("prior", False)):
        p = w.prior; nb = p.n_blocks
        xs = []
        for b in range(nb):
            kind, fr = p.block_kind[b], p.block_frame[b]
            xs.append(np.array(w.pose[fr] if kind == 0 else w.speedbias[fr] if kind == 1 else w.ex_pose if kind == 2 else [w.td], np.float64))
        d = dict(n=p.n, size=list(p.block_size[:nb]), idx=list(p.block_idx[:nb]), x0_off=list(p.x0_off[:nb]), x0=np.array(p.x0[:]), r0=p.r0(), J0=p.J0(), x=xs)
        out.append(dict(family="prior", index=0, data=d, draws=draws, **common))
    return out


def run(tasks, parallel=True):
    if not parallel or len(tasks) < 4:
        return [block_task(t) for t in tasks]
    return list(pool().map(block_task, tasks, chunksize=max(1, min(8, len(tasks) // (4 * MAX_WORKERS) + 1))))


def evaluate_cached(key, w, opts, **kw):
    """evaluate(), kept in the directory UVS_FACTOR_REF_CACHE names (if any) under `key` and the hash of every input of the window: a GPU
    run can then start from references computed beforehand.  The cache holds reference values only."""
    import hashlib
    import pickle
    d = os.environ.get("UVS_FACTOR_REF_CACHE")
    if not d: return evaluate(w, opts, **kw)
    tasks = tasks_of(w, opts, kw.get("subset"), kw.get("draws", 4), kw.get("level_stride", 1), kw.get("seed", 0), kw.get("dps", DPS), kw.get("h", H),
                     kw.get("jacobians", True), kw.get("relo", False))
    tag = hashlib.sha1(pickle.dumps([(t["family"], t["index"], t["draws"]) + (() if t.get("jacobians", True) else ("r",)) + (sorted((k, np.asarray(v).tobytes() if not isinstance(v, list) else pickle.dumps([np.asarray(x).tobytes() for x in v])) for k, v in t["data"].items()),) for t in tasks])).hexdigest()[:16]
    path = os.path.join(d, f"{key}-{tag}.pkl")
    if os.path.exists(path):
        with open(path, "rb") as f: return pickle.load(f)
    out = evaluate(w, opts, **kw)
    os.makedirs(d, exist_ok=True)
    with open(path + ".tmp", "wb") as f: pickle.dump(out, f)
    os.replace(path + ".tmp", path)
    return out


def evaluate(w, opts, subset=None, draws=4, level_stride=1, seed=0, parallel=True, dps=DPS, h=H, jacobians=True, relo=False):
    """-> {False: Ref, True: Ref}: the reference of window `w` without and with the loss correction.  jacobians=False (residual-only mode): r,
    cost, the level of r and the residual models are those of the full mode, the Jacobians are zero, and the Ref also carries cost_mp, the sum of
    the blocks' costs taken at 60 digits (rounded by whoever uses it, once).  relo=True: the relocalization blocks too, as relo_r / cost_terms['relo'] /
    level['relo_r']; they enter cost_mp and NOT cost (uvs_evaluate does not evaluate them)."""
    res = run(tasks_of(w, opts, subset, draws, level_stride, seed, dps, h, jacobians, relo), parallel)
    out = {}
    for v, robust in enumerate((False, True)):
        R = Ref(w)
        cmp_ = mpf(0)
        if relo:
            nr = len(w.relo_lm)
            R.relo_r = np.zeros((nr, 2)); R.cost_terms["relo"] = np.zeros(nr); R.level["relo_r"] = np.full((nr, 2), np.nan); R.have["relo"] = np.zeros(nr, bool); R.aux["relo"] = {}
        for fam, k, b in res:
            lv = b.get("level")
            if "cost_mp" in b: cmp_ += b["cost_mp"][v] + (b["vcost_mp"][v] if "vcost_mp" in b else 0)
            if fam == "relo":
                R.relo_r[k] = b["r"][v]; R.cost_terms["relo"][k] = b["cost"][v]
                if lv: R.level["relo_r"][k] = lv["r"][v]
            elif fam == "pt":
                R.pt_r[k] = b["r"][v]; R.pt_J[k] = b["J"][v][:, :19]; R.pt_Jtd[k] = b["J"][v][:, 19]; R.cost_terms["pt"][k] = b["cost"][v]
                R.model["pt_J"][k] = b["mJ"][v][:, :19]; R.model["pt_Jtd"][k] = b["mJ"][v][:, 19]
                if lv: R.level["pt_r"][k] = lv["r"][v]; R.level["pt_J"][k] = lv["J"][v][:, :19]; R.level["pt_Jtd"][k] = lv["J"][v][:, 19]
            elif fam == "ln":
                R.ln_r[k] = b["r"][v]; R.ln_J[k] = b["J"][v]; R.vp_r[k] = b["vr"][v]; R.vp_J[k] = b["vJ"][v]
                R.cost_terms["ln"][k] = b["cost"][v]; R.cost_terms["vp"][k] = b["vcost"][v]
                R.model["vp_r"][k] = b["vmr"][v]; R.model["vp_J"][k] = b["vmJ"][v]
                if lv:
                    for nm, src in (("ln_r", "r"), ("ln_J", "J"), ("vp_r", "vr"), ("vp_J", "vJ")): R.level[nm][k] = lv[src][v]
            elif fam == "imu":
                R.imu_r[k] = b["r"][v]; R.imu_J[k] = b["J"][v]; R.cost_terms["imu"][k] = b["cost"][v]; R.W[k] = b["W"]; R.model["imu_J"][k] = b["mJ"][v]
                if lv: R.level["imu_r"][k] = lv["r"][v]; R.level["imu_J"][k] = lv["J"][v]
            else:
                n = len(b["r"][v]); R.prior_r[:n] = b["r"][v]; R.cost_terms["prior"] = b["cost"][v]
                if lv: R.level["prior_r"][:n] = lv["r"][v]
            if fam == "prior": R.have["prior"] = True
            else: R.have[fam][k] = True
            R.aux[fam][k] = b.get("aux", {})
        for b, blk in enumerate(w.imu):      # a skipped block is all zeros by definition (estimator.cpp:814)
            if blk.get("skip", 0) and (subset is None or b in subset.get("imu", [])):
                R.have["imu"][b] = True
                for nm in ("imu_r", "imu_J"): R.level[nm][b] = 0.0
        ct = R.cost_terms
        R.cost = float(ct["prior"] + ct["imu"].sum() + ct["pt"].sum() + ct["ln"].sum() + ct["vp"].sum())
        if not jacobians: R.cost_mp = cmp_
        out[robust] = R
    return out


# ---------------------------------------------------------------- the metric and the bound
_FRAME = (("p", 0, 3), ("th", 3, 6))
_SB = (("v", 0, 3), ("ba", 3, 6), ("bg", 6, 9))
COLS = dict(
    pt=[("i." + n, a, b) for n, a, b in _FRAME] + [("j." + n, 6 + a, 6 + b) for n, a, b in _FRAME] + [("ex." + n, 12 + a, 12 + b) for n, a, b in _FRAME] + [("lam", 18, 19), ("td", 19, 20)],
    ln=[("p", 0, 3), ("th", 3, 6), ("line", 6, 10)],
    vp=[("p", 0, 3), ("th", 3, 6), ("line", 6, 10)],
    imu=[("i." + n, a, b) for n, a, b in _FRAME] + [("i." + n, 6 + a, 6 + b) for n, a, b in _SB] + [("j." + n, 15 + a, 15 + b) for n, a, b in _FRAME] + [("j." + n, 21 + a, 21 + b) for n, a, b in _SB])
ROWS = dict(pt=[("r", 0, 2)], ln=[("r", 0, 2)], vp=[("r", 0, 1)], imu=[("r" + n, 3 * k, 3 * k + 3) for k, n in enumerate(("p", "q", "v", "ba", "bg"))])


def _family_arrays(x, fam):
    """(r [n, R], J [n, R, C]) of a family out of an Eval-shaped object or of a dict of arrays (level / model)."""
    g = (lambda nm: x[nm]) if isinstance(x, dict) else (lambda nm: getattr(x, nm))
    if fam == "pt":
        return np.asarray(g("pt_r")), np.concatenate([np.asarray(g("pt_J")), np.asarray(g("pt_Jtd"))[:, :, None]], axis=2)
    return np.asarray(g(fam + "_r")), np.asarray(g(fam + "_J"))


def _fill(level, have):
    """Blocks without a level of their own (level_stride) take the largest of the family's sampled blocks, entry by entry."""
    lv = level.copy()
    miss = np.isnan(lv.reshape(len(lv), -1)).any(axis=1) & have
    if miss.any():
        samp = ~np.isnan(lv.reshape(len(lv), -1)).any(axis=1)
        assert samp.any(), "no block of the family carries a level"
        lv[miss] = lv[samp].max(axis=0)
    return lv


def _abs_err(x, ref):
    """|x - ref|, infinite where x is not finite (a NaN must not compare as 'no error')."""
    e = np.abs(np.asarray(x, np.float64) - ref)
    return np.where(np.isfinite(e), e, np.inf)


def check(x, ref, C, families=("pt", "ln", "vp", "imu", "prior"), relative_levels=None):
    """Per residual block and, inside a block, per row group x parameter group: err = max |x - ref| / scale, scale = max |ref| over the sub-block (a
    sub-block that is zero in the reference is measured against the largest sub-block of the same rows; rows that are zero altogether must be
    zero in x), residuals absolutely; bound B = max(C level_in, C model, 1e-13 scale).  -> list of records
    (family, block, rows, cols or 'r', err, level_in, model, B, err / B, floor), all relative to `scale` for Jacobians and absolute for residuals."""
    out = []
    for fam in families:
        if fam == "prior":
            if not ref.have["prior"]: continue
            n = len(ref.level["prior_r"]); n = int(np.sum(~np.isnan(ref.level["prior_r"])))
            xr, rr, lv = np.asarray(x.prior_r)[:n], ref.prior_r[:n], ref.level["prior_r"][:n]
            scale = np.abs(rr).max()
            B = np.maximum(C * lv, FLOOR * scale); e = _abs_err(xr, rr)
            i = int(np.argmax(e / B))
            out.append(("prior", 0, "r", "r", float(e[i]), float(lv[i]), 0.0, float(B[i]), float(e[i] / B[i]), float(FLOOR * scale)))
            continue
        hv = ref.have["ln" if fam == "vp" else fam]
        if not hv.any(): continue
        xr, xJ = _family_arrays(x, fam); rr, rJ = _family_arrays(ref, fam)
        lr, lJ = _family_arrays(ref.level, fam); mr, mJ = _family_arrays(ref.model, fam)
        # level of unsampled blocks: the family's largest RELATIVE level per entry position (Jacobians), the largest absolute one (residuals)
        blockscale = np.maximum(np.abs(rJ).reshape(len(rJ), -1).max(axis=1), 1e-300)
        lJ = _fill(lJ / blockscale[:, None, None], hv) * blockscale[:, None, None]; lr = _fill(lr, hv)
        for rn, r0, r1 in ROWS[fam]:
            e = _abs_err(xr[:, r0:r1], rr[:, r0:r1]).max(axis=1)
            sc = np.abs(rr[:, r0:r1]).max(axis=1)
            lv = lr[:, r0:r1].max(axis=1); md = mr[:, r0:r1].max(axis=1)
            B = np.maximum(np.maximum(C * lv, C * md), FLOOR * sc)
            ratio = np.where(e > 0, e / np.maximum(B, 1e-300), 0.0)
            for k in np.nonzero(hv)[0]:
                out.append((fam, int(k), rn, "r", float(e[k]), float(lv[k]), float(md[k]), float(B[k]), float(ratio[k]), float(FLOOR * sc[k])))
            rowscale = np.abs(rJ[:, r0:r1, :]).reshape(len(rJ), -1).max(axis=1)
            for cn, c0, c1 in COLS[fam]:
                sub = lambda a: np.abs(a[:, r0:r1, c0:c1]).reshape(len(a), -1).max(axis=1)
                sc = sub(rJ); sc = np.where(sc > 0, sc, rowscale)
                e = sub(_abs_err(xJ, rJ)); lv = sub(lJ); md = sub(mJ)
                dead = sc == 0      # rows that are zero altogether in the reference: x must be zero
                scs = np.where(dead, 1.0, sc)
                e, lv, md = e / scs, lv / scs, md / scs
                B = np.where(dead, 0.0, np.maximum(np.maximum(C * lv, C * md), FLOOR))
                ratio = np.where(e > 0, e / np.maximum(B, 1e-300), 0.0)
                for k in np.nonzero(hv)[0]:
                    out.append((fam, int(k), rn, cn, float(e[k]), float(lv[k]), float(md[k]), float(B[k]), float(ratio[k]), FLOOR))
    return out


def cost_bound(ref, C):
    """First-order bound of |cost - cost*| from the residual bounds: sum |r| B_r (B_r as in check(), per row group), plus 1e-13 cost for the sum itself."""
    tot = 0.0
    for fam in ("pt", "ln", "vp", "imu"):
        hv = ref.have["ln" if fam == "vp" else fam]
        if not hv.any(): continue
        rr, _ = _family_arrays(ref, fam); lr, _ = _family_arrays(ref.level, fam); mr, _ = _family_arrays(ref.model, fam)
        lr = _fill(lr, hv)
        for rn, r0, r1 in ROWS[fam]:
            sc = np.abs(rr[:, r0:r1]).max(axis=1)
            B = np.maximum(np.maximum(C * lr[:, r0:r1].max(axis=1), C * mr[:, r0:r1].max(axis=1)), FLOOR * sc)
            tot += float((np.abs(rr[:, r0:r1]).sum(axis=1) * B)[hv].sum())
    if ref.have["prior"]:
        n = int(np.sum(~np.isnan(ref.level["prior_r"])))
        B = np.maximum(C * ref.level["prior_r"][:n], FLOOR * np.abs(ref.prior_r[:n]).max())
        tot += float((np.abs(ref.prior_r[:n]) * B).sum())
    return tot + FLOOR * abs(ref.cost)


def summarize(records):
    """{family: (worst record by ratio, median ratio of the records with err > 0)}."""
    out = {}
    for fam in sorted({r[0] for r in records}):
        rs = [r for r in records if r[0] == fam]
        pos = [r[8] for r in rs if r[4] > 0]
        out[fam] = (max(rs, key=lambda r: r[8]), float(np.median(pos)) if pos else 0.0)
    return out


def entry_bounds(ref, C):
    """The bound B of check(), per entry and absolute: {name: array} for the residual and Jacobian arrays of `ref` (an entry carries the bound
    of its sub-block times the sub-block's scale).  What the first-order propagation into g, diag H and the cost starts from."""
    out = {}
    for fam in ("pt", "ln", "vp", "imu"):
        hv = ref.have["ln" if fam == "vp" else fam]
        rr, rJ = _family_arrays(ref, fam); lr, lJ = _family_arrays(ref.level, fam); mr, mJ = _family_arrays(ref.model, fam)
        Br, BJ = np.zeros(rr.shape), np.zeros(rJ.shape)
        if hv.any():
            lr = _fill(lr, hv)
            blockscale = np.maximum(np.abs(rJ).reshape(len(rJ), -1).max(axis=1), 1e-300)
            lJ = _fill(lJ / blockscale[:, None, None], hv) * blockscale[:, None, None]
            for rn, r0, r1 in ROWS[fam]:
                sc = np.abs(rr[:, r0:r1]).max(axis=1)
                Br[:, r0:r1] = np.maximum(np.maximum(C * lr[:, r0:r1].max(axis=1), C * mr[:, r0:r1].max(axis=1)), FLOOR * sc)[:, None]
                rowscale = np.abs(rJ[:, r0:r1, :]).reshape(len(rJ), -1).max(axis=1)
                for cn, c0, c1 in COLS[fam]:
                    sub = lambda a: np.abs(a[:, r0:r1, c0:c1]).reshape(len(a), -1).max(axis=1)
                    sc = sub(rJ); sc = np.where(sc > 0, sc, rowscale)
                    BJ[:, r0:r1, c0:c1] = np.maximum(np.maximum(C * sub(lJ), C * sub(mJ)), FLOOR * sc)[:, None, None]
        if fam == "pt": out["pt_r"], out["pt_J"], out["pt_Jtd"] = Br, BJ[:, :, :19], BJ[:, :, 19]
        else: out[fam + "_r"], out[fam + "_J"] = Br, BJ
    n = int(np.sum(~np.isnan(ref.level["prior_r"]))) if ref.have["prior"] else 0
    out["prior_r"] = np.zeros(len(ref.prior_r))
    if n: out["prior_r"][:n] = np.maximum(C * ref.level["prior_r"][:n], FLOOR * np.abs(ref.prior_r[:n]).max())
    return out


_log = []


def log(line):
    _log.append(line)


def log_records(tag, records):
    """One line per family: the worst sub-block of `records` (by err / B) and the median ratio."""
    for fam, (w, med) in summarize(records).items():
        log(f"{tag:34s} {fam:5s} worst err {w[4]:.2e} (block {w[1]}, {w[2]} x {w[3]}) level_in {w[5]:.2e} model {w[6]:.2e} B {w[7]:.2e} err/B {w[8]:.3f}  median err/B {med:.2e}")


def write_log():
    """Every figure logged so far -> the file UVS_FACTOR_LOG names (each test module's fixture calls this at its end)."""
    path = os.environ.get("UVS_FACTOR_LOG")
    if path:
        with open(path, "a") as f: f.write("\n".join(_log) + "\n")
        del _log[:]
