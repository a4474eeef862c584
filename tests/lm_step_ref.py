"""Extended-precision reference of the sliding-window damped LM step (the reference of uvs_debug_step).

TEST INFRASTRUCTURE ONLY, numpy only: it shares no solver code with the product or the oracle.  From a per-block evaluation dump
(`abi.Eval`) it builds the Jacobi-scaled damped system over the FULL parameter vector in np.longdouble -- the layout of
include/uvs_solver.h: uvs_debug_step, [11 x 15 frame dofs | 6 extrinsic (estimate_extrinsic) | 1 td (estimate_td) | inverse depths |
4 x line parameters], with 6 relo_Pose dofs in front of the inverse depths when the window has relocalization blocks -- and solves it by eliminating the landmark blocks (exactly block-diagonal, so the elimination is exact at this
precision) and a longdouble Cholesky of the reduced system (pg_ref.cholesky_ld / solve_ld).  Scaling and damping follow pyref_lm.solve
(Ceres' LevenbergMarquardtStrategy): s = 1 / (1 + sqrt(diag H)) (ones without jacobi_scaling), D = clip(diag(s H s), min_lm_diagonal,
max_lm_diagonal) / radius, M = s H s + D, b = -s g, step = s y.

Relocalization blocks (estimator.cpp:944-978) are not in the evaluation dump (uvs_evaluate does not evaluate them): their rows are restated
here from the definition of the block -- the ordinary projection factor between Pose[start frame of the landmark] and relo_Pose, the extrinsic and
the landmark's inverse depth, under the visual blocks' Cauchy loss, never a td factor -- in np.longdouble with analytic tangent Jacobians
(relo_rows; checked against pyref's autograd in tests/test_lm_step_ref.py).  relo_Pose is a block of the layout, after td and before the landmarks.
"""
import numpy as np

from helpers import abi, NF
import pg_ref

LD = np.longdouble
FR = 15 * NF


def layout(w, opts):
    """-> dict of column offsets: ex / td (None when not free), points, lines, n."""
    ex = FR if opts.estimate_extrinsic else None
    td = FR + (6 if ex is not None else 0) if opts.estimate_td else None
    relo = FR + (6 if ex is not None else 0) + (1 if td is not None else 0) if len(w.relo_lm) else None
    pt = FR + (6 if ex is not None else 0) + (1 if td is not None else 0) + (6 if relo is not None else 0)
    ln = pt + len(w.inv_depth)
    return dict(ex=ex, td=td, relo=relo, pt=pt, ln=ln, n=ln + 4 * len(w.line_orth), frames=pt)


def groups(w, opts):
    """Block groups of the step: (name, index array).  Each frame's p, theta, v, ba, bg; extrinsic; td; all inverse depths; all lines."""
    L = layout(w, opts)
    out = []
    for f in range(NF):
        for nm, a, b in (("p", 0, 3), ("th", 3, 6), ("v", 6, 9), ("ba", 9, 12), ("bg", 12, 15)):
            out.append((f"f{f}.{nm}", np.arange(15 * f + a, 15 * f + b)))
    if L["ex"] is not None: out.append(("ex", np.arange(L["ex"], L["ex"] + 6)))
    if L["td"] is not None: out.append(("td", np.array([L["td"]])))
    if L["relo"] is not None: out += [("relo.p", np.arange(L["relo"], L["relo"] + 3)), ("relo.th", np.arange(L["relo"] + 3, L["relo"] + 6))]
    if len(w.inv_depth): out.append(("points", np.arange(L["pt"], L["ln"])))
    if len(w.line_orth): out.append(("lines", np.arange(L["ln"], L["n"])))
    return out


def _quat_R(q):
    """Rotation matrix of a quaternion (x, y, z, w), normalised, np.longdouble."""
    q = np.asarray(q, LD); x, y, z, s = q / np.sqrt(np.sum(q * q))
    one, two = LD(1), LD(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * s), two * (x * z + y * s)],
                     [two * (x * y + z * s), one - two * (x * x + z * z), two * (y * z - x * s)],
                     [two * (x * z - y * s), two * (y * z + x * s), one - two * (x * x + y * y)]])


def _skew(v):
    z = LD(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]])


def projection_block(pose_i, pose_j, ex, lam, pts_i, pts_j, sqrt_info, loss):
    """The projection factor of a point first seen in frame i and observed in frame j (normalised image points pts_i, pts_j = (x, y, 1), inverse
    depth lam in frame i), written out from its definition in np.longdouble:
        p_ci = pts_i / lam;  p_bi = R_ic p_ci + t_ic;  p_w = R_i p_bi + P_i;  p_bj = R_j^T (p_w - P_j);  p_cj = R_ic^T (p_bj - t_ic)
        r = sqrt_info (p_cj.xy / p_cj.z - pts_j.xy)
    with the Jacobians for the tangent steps P += dp, Q <- Q (x) (dtheta / 2, 1), and the robust correction of a loss with rho'' < 0 (Cauchy,
    rho(s) = a^2 log(1 + s / a^2), rho' = 1 / (1 + s / a^2)): Ceres' corrector then only scales residual and rows by sqrt(rho'(||r||^2)).
    loss <= 0: no loss.  -> (r[2], J[2, 19] = [pose_i 6 | pose_j 6 | extrinsic 6 | lam])."""
    pi_, pj_, pe = np.asarray(pose_i, LD), np.asarray(pose_j, LD), np.asarray(ex, LD)
    Ri, Rj, Ric = _quat_R(pi_[3:]), _quat_R(pj_[3:]), _quat_R(pe[3:])
    Pi, Pj, tic = pi_[:3], pj_[:3], pe[:3]
    lam = LD(lam); a = np.asarray(pts_i, LD); m = np.asarray(pts_j, LD)
    pci = a / lam
    pbi = Ric @ pci + tic
    pw = Ri @ pbi + Pi
    pbj = Rj.T @ (pw - Pj)
    pcj = Ric.T @ (pbj - tic)
    z = pcj[2]
    r = LD(sqrt_info) * (pcj[:2] / z - m[:2])
    red = LD(sqrt_info) * np.array([[1 / z, LD(0), -pcj[0] / (z * z)], [LD(0), 1 / z, -pcj[1] / (z * z)]])
    A = Ric.T @ Rj.T
    J = np.zeros((2, 19), LD)
    J[:, 0:3] = red @ A
    J[:, 3:6] = red @ (-(A @ Ri) @ _skew(pbi))
    J[:, 6:9] = red @ (-A)
    J[:, 9:12] = red @ (Ric.T @ _skew(pbj))
    T = A @ Ri @ Ric
    J[:, 12:15] = red @ (Ric.T @ (Rj.T @ Ri - np.eye(3, dtype=LD)))
    J[:, 15:18] = red @ (-T @ _skew(pci) + _skew(T @ pci) + _skew(Ric.T @ (Rj.T @ (Ri @ tic + Pi - Pj) - tic)))
    J[:, 18] = red @ (T @ a) * (-1 / (lam * lam))
    if loss > 0:
        s2 = np.sum(r * r); b = LD(loss) * LD(loss)
        k = np.sqrt(1 / (1 + s2 / b))
        r = k * r; J = k * J
    return r, J


def relo_rows(w, opts):
    """The relocalization blocks of `w` as (columns, J, r) in np.longdouble: frame i = the frame of the landmark's first observation, frame j = relo_Pose."""
    L = layout(w, opts)
    out = []
    first = {}
    for k in range(len(w.pt_lm)):
        first.setdefault(int(w.pt_lm[k]), int(w.pt_fi[k]))
    for k in range(len(w.relo_lm)):
        lm = int(w.relo_lm[k]); fi = first[lm]
        r, J = projection_block(w.pose[fi], w.relo_pose, w.ex_pose, w.inv_depth[lm], w.relo_pi[k], w.relo_pj[k], opts.point_sqrt_info, opts.loss_point)
        cols = list(range(15 * fi, 15 * fi + 6)) + list(range(L["relo"], L["relo"] + 6)); jc = list(range(12))
        if L["ex"] is not None: cols += list(range(L["ex"], L["ex"] + 6)); jc += list(range(12, 18))
        cols.append(L["pt"] + lm); jc.append(18)
        out.append((cols, J[:, jc], r))
    return out


def normal_equations(w, ev, opts):
    """H = J^T J, g = J^T r (np.longdouble) over the layout above, from an `abi.Eval` dump (robust, the Cauchy corrector applied) and, for the
    relocalization blocks the dump does not hold, from relo_rows."""
    L = layout(w, opts); P = L["n"]
    H = np.zeros((P, P), LD); g = np.zeros(P, LD)

    def add(cols, J, r):
        cols = np.asarray(cols); J = np.asarray(J, LD); r = np.asarray(r, LD)
        H[np.ix_(cols, cols)] += J.T @ J
        g[cols] += J.T @ r

    if w.prior is not None and w.prior.n > 0:
        p = w.prior; n = p.n; J0 = p.J0()
        cols, src = [], []
        for b in range(p.n_blocks):
            kind, fr, size, idx = p.block_kind[b], p.block_frame[b], p.block_size[b], p.block_idx[b]
            loc = 6 if size == 7 else size
            if kind == abi.BLOCK_POSE: base = 15 * fr
            elif kind == abi.BLOCK_SPEEDBIAS: base = 15 * fr + 6
            elif kind == abi.BLOCK_EX_POSE: base = L["ex"]
            else: base = L["td"]
            if base is None: continue          # a block the solve holds constant
            cols += [base + k for k in range(loc)]; src += [idx + k for k in range(loc)]
        add(cols, J0[:, src], ev.prior_r[:n])
    for b, blk in enumerate(w.imu):
        if blk.get("skip", 0): continue
        i = blk["frame_i"]
        add(list(range(15 * i, 15 * i + 30)), ev.imu_J[b], ev.imu_r[b])
    for k in range(len(w.pt_lm)):
        fi, fj, lm = int(w.pt_fi[k]), int(w.pt_fj[k]), int(w.pt_lm[k])
        cols = list(range(15 * fi, 15 * fi + 6)) + list(range(15 * fj, 15 * fj + 6)); jc = list(range(12))
        if L["ex"] is not None: cols += list(range(L["ex"], L["ex"] + 6)); jc += list(range(12, 18))
        cols.append(L["pt"] + lm); jc.append(18)
        J = np.asarray(ev.pt_J[k])[:, jc]
        if L["td"] is not None:
            cols.append(L["td"]); J = np.concatenate([J, np.asarray(ev.pt_Jtd[k]).reshape(2, 1)], axis=1)
        add(cols, J, ev.pt_r[k])
    for cols, J, r in relo_rows(w, opts):
        add(cols, J, r)
    for k in range(len(w.ln_lm)):
        fj, lm = int(w.ln_fj[k]), int(w.ln_lm[k])
        cols = list(range(15 * fj, 15 * fj + 6)) + list(range(L["ln"] + 4 * lm, L["ln"] + 4 * lm + 4))
        add(cols, ev.ln_J[k], ev.ln_r[k])
        if w.ln_has_vp[k]:
            add(cols, ev.vp_J[k], ev.vp_r[k])
    return H, g


class System:
    """The damped system of one linearization; only the diagonal changes with the radius, so build once and call at(radius)."""

    def __init__(self, w, ev, opts):
        self.w, self.opts, self.L = w, opts, layout(w, opts)
        self.H, self.g = normal_equations(w, ev, opts)
        hd = np.diag(self.H)
        self.s = (LD(1) / (LD(1) + np.sqrt(hd))) if opts.jacobi_scaling else np.ones(len(hd), LD)
        self.Hs = self.H * np.outer(self.s, self.s)
        self.b = -self.s * self.g
        self.diag = np.clip(np.diag(self.Hs), LD(opts.min_lm_diagonal), LD(opts.max_lm_diagonal))

    def M(self, radius):
        M = self.Hs.copy()
        M[np.diag_indices_from(M)] += self.diag / LD(radius)
        return M


def damped_system(w, ev, radius, opts):
    """(M, b, s) of the Jacobi-scaled damped system at `radius`, np.longdouble."""
    S = System(w, ev, opts)
    return S.M(radius), S.b, S.s


def _chol_batch(A):
    """Batched lower Cholesky of SPD k x k blocks A[n, k, k] (any dtype, numpy only)."""
    A = A.copy(); n, k, _ = A.shape
    Lf = np.zeros_like(A)
    for j in range(k):
        d = A[:, j, j] - np.einsum("ni,ni->n", Lf[:, j, :j], Lf[:, j, :j])
        Lf[:, j, j] = np.sqrt(d)
        for i in range(j + 1, k):
            Lf[:, i, j] = (A[:, i, j] - np.einsum("ni,ni->n", Lf[:, i, :j], Lf[:, j, :j])) / Lf[:, j, j]
    return Lf


def _chol_solve_batch(Lf, B):
    """Lf Lf^T X = B for lower factors Lf[n, k, k] and B[n, k, m]."""
    n, k, _ = Lf.shape
    Y = B.copy()
    for i in range(k):
        Y[:, i] = (Y[:, i] - np.einsum("nj,njm->nm", Lf[:, i, :i], Y[:, :i])) / Lf[:, i, i][:, None]
    X = Y
    for i in range(k - 1, -1, -1):
        X[:, i] = (X[:, i] - np.einsum("nj,njm->nm", Lf[:, i + 1:, i], X[:, i + 1:])) / Lf[:, i, i][:, None]
    return X


def schur_solve(M, b, nfr, n_pt, n_ln, dtype, frame_solve):
    """Eliminate the landmark blocks (points 1 x 1, lines 4 x 4, block-diagonal) of M y = b, solve the reduced frame system with
    `frame_solve(S, rhs)`, back-substitute.  All arithmetic in `dtype`."""
    M = np.asarray(M, dtype); b = np.asarray(b, dtype)
    pt = np.arange(nfr, nfr + n_pt); ln = nfr + n_pt
    A = M[:nfr, :nfr]; bf = b[:nfr]
    # points: 1 x 1
    Bp = M[:nfr, pt]; cp = np.diag(M)[pt] if n_pt else np.zeros(0, dtype)
    Xp = Bp / cp[None, :] if n_pt else np.zeros((nfr, 0), dtype)
    # lines: 4 x 4
    if n_ln:
        idx = ln + 4 * np.arange(n_ln)[:, None] + np.arange(4)[None, :]
        C = M[idx[:, :, None], idx[:, None, :]]                       # [n_ln, 4, 4]
        Bl = M[:nfr][:, idx].transpose(1, 2, 0)                       # [n_ln, 4, nfr] = B_l^T
        Lf = _chol_batch(C)
        Xl = _chol_solve_batch(Lf, np.concatenate([Bl, b[idx][:, :, None]], axis=2))      # C^-1 [B^T | b_l]
    S = A - Bp @ Xp.T if n_pt else A.copy()
    r = bf - (Bp @ (b[pt] / cp) if n_pt else 0)
    if n_ln:
        S = S - np.einsum("nkf,nkg->fg", Bl, Xl[:, :, :nfr])
        r = r - np.einsum("nkf,nk->f", Bl, Xl[:, :, nfr])
    yf = np.asarray(frame_solve(S, r), dtype)
    y = np.zeros(len(b), dtype); y[:nfr] = yf
    if n_pt: y[pt] = (b[pt] - Bp.T @ yf) / cp
    if n_ln:
        y[idx] = Xl[:, :, nfr] - np.einsum("nkf,f->nk", Xl[:, :, :nfr], yf)
    return y


def _sizes(sysm):
    w, L = sysm.w, sysm.L
    return L["frames"], len(w.inv_depth), len(w.line_orth)


def damped_step(sysm, radius):
    """-> (delta, y): the unscaled step s y and the scaled solution y of M y = b at `radius`, np.longdouble."""
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not an extended type here: the reference would be plain FP64"
    M = sysm.M(radius)
    y = schur_solve(M, sysm.b, *_sizes(sysm), LD, pg_ref.solve_ld)
    return sysm.s * y, y


def backward_error(M, b, y):
    """||M y - b|| / (||M|| ||y|| + ||b||), infinity norms, in np.longdouble."""
    M = np.asarray(M, LD); b = np.asarray(b, LD); y = np.asarray(y, LD)
    r = M @ y - b
    return float(np.abs(r).max() / (np.abs(M).sum(axis=1).max() * np.abs(y).max() + np.abs(b).max()))


def group_errors(delta, ref, grps):
    """{group: ||delta_G - ref_G|| / ||ref_G||} (2-norms; the reference in longdouble)."""
    d = np.asarray(delta, LD); r = np.asarray(ref, LD)
    out = {}
    for nm, ix in grps:
        den = np.sqrt(np.sum(r[ix] ** 2))
        out[nm] = float(np.sqrt(np.sum((d[ix] - r[ix]) ** 2)) / den) if den > 0 else float(np.sqrt(np.sum(d[ix] ** 2)))
    return out


def fp64_level(sysm, radius, ref_delta, grps, seed=0):
    """What careful FP64 solves reach on this system: per group the WORST forward error of dense np.linalg.solve in three orders of the
    unknowns and of a plain FP64 Schur path (landmark elimination, Cholesky of the reduced system, back-substitution); plus the backward
    error of the FP64 Schur path.  -> ({group: error}, backward error)."""
    M = np.asarray(sysm.M(radius), np.float64); b = np.asarray(sysm.b, np.float64); s = np.asarray(sysm.s, np.float64)
    n = len(b)
    worst = {nm: 0.0 for nm, _ in grps}
    perms = [np.arange(n), np.arange(n)[::-1], np.random.default_rng(seed).permutation(n)]
    for p in perms:
        y = np.empty(n); y[p] = np.linalg.solve(M[np.ix_(p, p)], b[p])
        for k, v in group_errors(s * y, ref_delta, grps).items(): worst[k] = max(worst[k], v)

    def chol64(S, r):
        Lc = np.linalg.cholesky(S)
        return np.linalg.solve(Lc.T, np.linalg.solve(Lc, r))
    ys = schur_solve(M, b, *_sizes(sysm), np.float64, chol64)
    for k, v in group_errors(s * ys, ref_delta, grps).items(): worst[k] = max(worst[k], v)
    return worst, backward_error(sysm.M(radius), sysm.b, ys)


def fp64_mcc_level(sysm, radius):
    """What careful FP64 reaches for model_cost_change on this system: the FP64 Schur path's own step y (fp64_level's), and relative to the
    longdouble value A(y) = y.b - y^T Hs y / 2 at that y the worse of (i) the sum 0.5 (y.Dy + y.b), which takes M y = b for exact (the kernels'
    form; its distance from A(y) is y.(M y - b) / 2, the solve's residual against the step, in any arithmetic) and (ii) A(y) itself evaluated in FP64.
    Both grow with ||y||^2: 1e-16 on the windows whose scaled step is 1e5 long, 4e-11 / 7e-11 on prior_td at radius 1e12, where it is 2e8 long."""
    M = np.asarray(sysm.M(radius), np.float64); b = np.asarray(sysm.b, np.float64); Hs = np.asarray(sysm.Hs, np.float64)
    D = np.asarray(sysm.diag / LD(radius), np.float64)

    def chol64(S, r):
        Lc = np.linalg.cholesky(S)
        return np.linalg.solve(Lc.T, np.linalg.solve(Lc, r))
    y = schur_solve(M, b, *_sizes(sysm), np.float64, chol64)
    yl = np.asarray(y, LD)
    A = yl @ sysm.b - LD(0.5) * (yl @ sysm.Hs @ yl)
    B = LD(0.5) * (yl @ ((sysm.diag / LD(radius)) * yl) + yl @ sysm.b)
    A64 = y @ b - 0.5 * (y @ Hs @ y)
    B64 = 0.5 * (y @ (D * y) + y @ b)
    return float(max(abs(B - A), abs(LD(A64) - A), abs(LD(B64) - A)) / abs(A))
