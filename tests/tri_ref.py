"""Triangulation of landmarks (include/uvs_solver.h: uvs_tri_*; csrc/uvs_triangulate.hip), twice:

  * the FP64 numpy restatement in the reference's order of operations (feature_manager.cpp:427-481, 504-589, 827-902, 352-416, 627-634): for a
    point the 2n x 4 matrix svd_A and numpy.linalg.svd OF svd_A, as the reference's JacobiSVD -- not the eigenvectors of svd_A^T svd_A, which
    `point_depth_normal_equations` keeps as the planted defect the tests must catch;
  * a 60-digit mpmath evaluation of the same definitions on the same FP64 inputs (`*_hp`): the truth the device and the numpy restatement
    are both measured against.  The largest error of the restatement on a set of cases is that set's E_ref.

Cameras are (R_wc, t_wc) lists over the 11 frames of a window, built by `cameras` / `cameras_hp` from pose[11][7] = (p, q xyzw) and ex_pose[7].
The `defect` arguments plant the wrong formulas of tests/test_tri_ref.py; nothing else passes them.

TEST INFRASTRUCTURE ONLY."""
import mpmath
import numpy as np

mp = mpmath.mp
DPS = 60
PI = 3.14159265358979323846
THRESHOLD = 0.1          # feature_manager.cpp:475: a depth below it is replaced by INIT_DEPTH


# ---------------------------------------------------------------- FP64
def quat_R(q):
    """Eigen's Quaterniond(w, x, y, z).toRotationMatrix() of q = (x, y, z, w), not normalized."""
    qx, qy, qz, qw = q
    tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * qw, ty * qw, tz * qw, tx * qx, ty * qx, tz * qx, ty * qy, tz * qy, tz * qz
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def cameras(pose, ex_pose):
    ric, tic = quat_R(ex_pose[3:]), np.asarray(ex_pose[:3], float)
    R = [quat_R(p[3:]) @ ric for p in pose]
    t = [quat_R(p[3:]) @ tic + p[:3] for p in pose]
    return R, t


def svd_A(cams, start, obs):
    """The 2n x 4 matrix of feature_manager.cpp:437-466; obs[k] belongs to frame start + k."""
    R, t = cams
    R0, t0 = R[start], t[start]
    A = np.zeros((2 * len(obs), 4))
    for k, o in enumerate(obs):
        R1, t1 = R[start + k], t[start + k]
        tt = R0.T @ (t1 - t0)
        Rr = R0.T @ R1
        P = np.zeros((3, 4)); P[:, :3] = Rr.T; P[:, 3] = -(Rr.T @ tt)
        f = np.asarray(o, float) / np.linalg.norm(o)
        A[2 * k] = f[0] * P[2] - f[2] * P[0]
        A[2 * k + 1] = f[1] * P[2] - f[2] * P[1]
    return A


def point_depth(cams, start, obs):
    """V[2] / V[3] of the smallest right singular vector of svd_A (numpy.linalg.svd orders the singular values descending)."""
    v = np.linalg.svd(svd_A(cams, start, obs))[2][3]
    with np.errstate(all="ignore"):
        return v[2] / v[3]


def point_depth_normal_equations(cams, start, obs):
    """THE SHORTCUT: the eigenvector of the smallest eigenvalue of svd_A^T svd_A (the condition number squared)."""
    A = svd_A(cams, start, obs)
    v = np.linalg.eigh(A.T @ A)[1][:, 0]
    with np.errstate(all="ignore"):
        return v[2] / v[3]


def depth_flag(d, init_depth):
    """(returned depth, pt_flag) of a raw depth: the rule is the same for every precision, so d may be an mpf."""
    if not (abs(d) < float("inf")):          # NaN or infinite
        return float(init_depth), 2
    if d < THRESHOLD:
        return float(init_depth), 1
    return float(d), 0


def euler_xyz(U, other_branch=False):
    """Eigen 3.3 Matrix3d::eulerAngles(0, 1, 2): the first angle in [0, pi] (other_branch: the planted defect, the angle in (-pi, 0])."""
    r0 = np.arctan2(U[1, 2], U[2, 2])
    c2 = np.sqrt(U[0, 0] * U[0, 0] + U[0, 1] * U[0, 1])
    if (r0 > 0.0) != other_branch:
        r0 = r0 - PI if r0 > 0.0 else r0 + PI
        r1 = np.arctan2(-U[0, 2], -c2)
    else:
        r1 = np.arctan2(-U[0, 2], c2)
    s1, c1 = np.sin(r0), np.cos(r0)
    r2 = np.arctan2(s1 * U[2, 0] - c1 * U[1, 0], c1 * U[1, 1] - s1 * U[2, 1])
    return np.array([-r0, -r1, -r2])


def U_of_psi(psi):
    """Rx(a) Ry(b) Rz(c): the matrix the three angles stand for (what the tests compare instead of the angles)."""
    a, b, c = psi
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def plucker_world(cams, fi, fj, sp_i, ep_i, sp_j, ep_j, beta_sign=1.0):
    """(n_w, d_w) of feature_manager.cpp:525-585."""
    R, t = cams
    Rl, tl, Rr, tr = R[fi], t[fi], R[fj], t[fj]
    Rrel = Rl.T @ Rr
    trel = Rl.T @ (tr - tl)
    a = np.cross(sp_i, ep_i); b = np.cross(Rrel @ sp_j, Rrel @ ep_j)
    beta = -beta_sign * (b @ trel)
    d_l = np.cross(b, a); n_l = a * beta
    d_w = Rl @ d_l
    n_w = Rl @ n_l + np.cross(tl, d_w)
    return n_w, d_w


def orth_of_plucker(n_w, d_w, other_branch=False):
    """-> (orth[4], ln_flag, U or None)."""
    nxd = np.cross(n_w, d_w)
    nn, nd, nx = np.linalg.norm(n_w), np.linalg.norm(d_w), np.linalg.norm(nxd)
    if not all(0.0 < v < np.inf for v in (nn, nd, nx)):
        return np.zeros(4), 2, None
    U = np.stack([n_w / nn, d_w / nd, nxd / nx], axis=1)
    return np.r_[euler_xyz(U, other_branch), np.arctan2(nd, nn)], 0, U


def line_orth(cams, fi, fj, sp_i, ep_i, sp_j, ep_j, defect=None):
    n_w, d_w = plucker_world(cams, fi, fj, sp_i, ep_i, sp_j, ep_j, beta_sign=-1.0 if defect == "beta_sign" else 1.0)
    return orth_of_plucker(n_w, d_w, other_branch=defect == "euler_branch")[:2]


def check_line(cams, start, sp, ep, orth_old):
    """-> (flag 1 / 2, the two deciding depths D_s(2) / w_s, D_e(2) / w_e) of setLineOrtho, in the host mirror's statement."""
    a, b, c, phi = orth_old
    sa, ca, sb, cb, sc, cc = np.sin(a), np.cos(a), np.sin(b), np.cos(b), np.sin(c), np.cos(c)
    U0 = np.array([cb * cc, sa * sb * cc + ca * sc, -ca * sb * cc + sa * sc]); U1 = np.array([-cb * sc, -sa * sb * sc + ca * cc, ca * sb * sc + sa * cc])
    n_w, d_w = U0 * np.cos(phi), U1 * np.sin(phi)
    R, t = cams[0][start], cams[1][start]
    t_cw = -(R.T @ t)
    d_c = R.T @ d_w; n_c = R.T @ n_w + np.cross(t_cw, d_c)
    slope = -(ep[0] - sp[0]) / (ep[1] - sp[1])
    sp2 = np.array([sp[0] + 1.0, slope + sp[1], 1.0]); ep2 = np.array([ep[0] + 1.0, slope + ep[1], 1.0])
    pi_s, pi_e = np.cross(sp, sp2), np.cross(ep, ep2)
    Ds, De = np.cross(n_c, pi_s), np.cross(n_c, pi_e)
    ws, we = -(d_c @ pi_s), -(d_c @ pi_e)
    zs, ze = Ds[2] / ws, De[2] / we
    return (2 if zs < 0 or ze < 0 else 1), (zs, ze)


def shift_depth(uv0, depth, marg_R, marg_P, new_R, new_P, init_depth):
    """-> (depth_out[n], flag[n], the raw z[n])."""
    world = (np.asarray(uv0) * np.asarray(depth)[:, None]) @ marg_R.T + marg_P
    z = ((world - new_P) @ new_R)[:, 2]
    ok = z > 0
    return np.where(ok, z, init_depth), np.where(ok, 0, 1).astype(np.int32), z


def triangulate(batch, init_depth, point_fn=point_depth, line_defect=None):
    """A whole batch (the dict of tests/tri_cases.py, the fields of uvs_tri_batch) -> depth, pt_flag, orth, ln_flag."""
    cams = [cameras(p, e) for p, e in zip(batch["pose"], batch["ex_pose"])]
    n_pt, n_ln = len(batch["pt_window"]), len(batch["ln_window"])
    depth, pf = np.zeros(n_pt), np.zeros(n_pt, np.int32)
    for k in range(n_pt):
        obs = batch["pt_obs"][batch["pt_obs_begin"][k]:batch["pt_obs_begin"][k + 1]]
        depth[k], pf[k] = depth_flag(point_fn(cams[batch["pt_window"][k]], int(batch["pt_start"][k]), obs), init_depth)
    orth, lf = np.zeros((n_ln, 4)), np.zeros(n_ln, np.int32)
    for l in range(n_ln):
        orth[l], lf[l] = line_orth(cams[batch["ln_window"][l]], int(batch["ln_fi"][l]), int(batch["ln_fj"][l]), batch["ln_sp_i"][l], batch["ln_ep_i"][l],
                                   batch["ln_sp_j"][l], batch["ln_ep_j"][l], defect=line_defect)
    return depth, pf, orth, lf


# ---------------------------------------------------------------- 60 digits
def _M(a):
    return mp.matrix(np.asarray(a, float).tolist())


def _cross(a, b):
    return mp.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _norm(a):
    return mp.sqrt(_dot(a, a))


def quat_R_hp(q):
    qx, qy, qz, qw = [mp.mpf(float(v)) for v in q]
    tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * qw, ty * qw, tz * qw, tx * qx, ty * qx, tz * qx, ty * qy, tz * qy, tz * qz
    return mp.matrix([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def cameras_hp(pose, ex_pose):
    with mp.workdps(DPS):
        ric, tic = quat_R_hp(ex_pose[3:]), _M(ex_pose[:3])
        R = [quat_R_hp(p[3:]) * ric for p in pose]
        t = [quat_R_hp(p[3:]) * tic + _M(p[:3]) for p in pose]
        return R, t


def svd_A_hp(cams, start, obs):
    R, t = cams
    with mp.workdps(DPS):
        R0, t0 = R[start], t[start]
        A = mp.zeros(2 * len(obs), 4)
        for k, o in enumerate(obs):
            R1, t1 = R[start + k], t[start + k]
            tt = R0.T * (t1 - t0)
            Rt = (R0.T * R1).T
            mt = -(Rt * tt)
            f = _M(o); f = f / _norm(f)
            for c in range(4):
                p0, p1, p2 = (Rt[0, c], Rt[1, c], Rt[2, c]) if c < 3 else (mt[0], mt[1], mt[2])
                A[2 * k, c] = f[0] * p2 - f[2] * p0
                A[2 * k + 1, c] = f[1] * p2 - f[2] * p1
        return A


def point_depth_hp(cams, start, obs):
    """-> mpf (NaN when V[3] is zero and V[2] too)."""
    with mp.workdps(DPS):
        _, S, V = mp.svd_r(svd_A_hp(cams, start, obs))
        k = min(range(4), key=lambda i: S[i])
        v2, v3 = V[k, 2], V[k, 3]          # svd_r returns V^T: row k is the k-th right singular vector
        if v3 == 0:
            return mp.nan if v2 == 0 else mp.sign(v2) * mp.inf
        return v2 / v3


def plucker_world_hp(cams, fi, fj, sp_i, ep_i, sp_j, ep_j):
    R, t = cams
    with mp.workdps(DPS):
        Rl, tl, Rr, tr = R[fi], t[fi], R[fj], t[fj]
        Rrel = Rl.T * Rr
        trel = Rl.T * (tr - tl)
        a = _cross(_M(sp_i), _M(ep_i)); b = _cross(Rrel * _M(sp_j), Rrel * _M(ep_j))
        beta = -_dot(b, trel)
        d_l = _cross(b, a); n_l = a * beta
        d_w = Rl * d_l
        n_w = Rl * n_l + _cross(tl, d_w)
        return n_w, d_w


def line_hp(cams, fi, fj, sp_i, ep_i, sp_j, ep_j):
    """-> (U [3][3] as float64 rounded from 60 digits, phi, ln_flag); U and phi are None under flag 2."""
    with mp.workdps(DPS):
        n_w, d_w = plucker_world_hp(cams, fi, fj, sp_i, ep_i, sp_j, ep_j)
        nxd = _cross(n_w, d_w)
        nn, nd, nx = _norm(n_w), _norm(d_w), _norm(nxd)
        if nn == 0 or nd == 0 or nx == 0:
            return None, None, 2
        U = np.array([[float(n_w[r] / nn), float(d_w[r] / nd), float(nxd[r] / nx)] for r in range(3)])
        return U, float(mp.atan2(nd, nn)), 0


def check_line_hp(cams, start, sp, ep, orth_old):
    with mp.workdps(DPS):
        a, b, c, phi = [mp.mpf(float(v)) for v in orth_old]
        sa, ca, sb, cb, sc, cc = mp.sin(a), mp.cos(a), mp.sin(b), mp.cos(b), mp.sin(c), mp.cos(c)
        U0 = mp.matrix([cb * cc, sa * sb * cc + ca * sc, -ca * sb * cc + sa * sc]); U1 = mp.matrix([-cb * sc, -sa * sb * sc + ca * cc, ca * sb * sc + sa * cc])
        n_w, d_w = U0 * mp.cos(phi), U1 * mp.sin(phi)
        R, t = cams[0][start], cams[1][start]
        t_cw = -(R.T * t)
        d_c = R.T * d_w; n_c = R.T * n_w + _cross(t_cw, d_c)
        sp, ep = _M(sp), _M(ep)
        slope = -(ep[0] - sp[0]) / (ep[1] - sp[1])
        sp2 = mp.matrix([sp[0] + 1, slope + sp[1], 1]); ep2 = mp.matrix([ep[0] + 1, slope + ep[1], 1])
        pi_s, pi_e = _cross(sp, sp2), _cross(ep, ep2)
        Ds, De = _cross(n_c, pi_s), _cross(n_c, pi_e)
        zs, ze = Ds[2] / -_dot(d_c, pi_s), De[2] / -_dot(d_c, pi_e)
        return (2 if zs < 0 or ze < 0 else 1), (float(zs), float(ze))


def shift_depth_hp(uv0, depth, marg_R, marg_P, new_R, new_P):
    """-> the raw z[n] as mpf."""
    with mp.workdps(DPS):
        mR, mP, nR, nP = _M(marg_R), _M(marg_P), _M(new_R), _M(new_P)
        return [(nR.T * (mR * (_M(u) * mp.mpf(float(d))) + mP - nP))[2] for u, d in zip(uv0, depth)]


def triangulate_hp(batch, init_depth):
    """-> dict: depth[n] / pt_flag[n] after the flag rule, raw[n] (float of the 60-digit depth before it), U[n][3][3] / phi[n] (NaN under flag 2),
    ln_flag[n]."""
    cams = [cameras_hp(p, e) for p, e in zip(batch["pose"], batch["ex_pose"])]
    n_pt, n_ln = len(batch["pt_window"]), len(batch["ln_window"])
    depth, raw, pf = np.zeros(n_pt), np.zeros(n_pt), np.zeros(n_pt, np.int32)
    for k in range(n_pt):
        obs = batch["pt_obs"][batch["pt_obs_begin"][k]:batch["pt_obs_begin"][k + 1]]
        d = point_depth_hp(cams[batch["pt_window"][k]], int(batch["pt_start"][k]), obs)
        raw[k] = float(d); depth[k], pf[k] = depth_flag(d, init_depth)
    U, phi, lf = np.full((n_ln, 3, 3), np.nan), np.full(n_ln, np.nan), np.zeros(n_ln, np.int32)
    for l in range(n_ln):
        u, p, lf[l] = line_hp(cams[batch["ln_window"][l]], int(batch["ln_fi"][l]), int(batch["ln_fj"][l]), batch["ln_sp_i"][l], batch["ln_ep_i"][l],
                              batch["ln_sp_j"][l], batch["ln_ep_j"][l])
        if lf[l] == 0:
            U[l], phi[l] = u, p
    return dict(depth=depth, raw=raw, pt_flag=pf, U=U, phi=phi, ln_flag=lf)


# ---------------------------------------------------------------- the error measures of the tests
def depth_errors(got, hp):
    """Relative errors of returned depths against the 60-digit ones."""
    return np.abs(got - hp) / np.abs(hp)


def line_errors(orth, hp_U, hp_phi):
    """Per line: the largest entry of |U(psi) - U_hp| and |phi - phi_hp| (orth[n][4] of flag-0 lines)."""
    eu = np.array([np.abs(U_of_psi(o[:3]) - u).max() for o, u in zip(orth, hp_U)])
    return np.maximum(eu, np.abs(orth[:, 3] - hp_phi))
