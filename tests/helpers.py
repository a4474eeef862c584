"""Shared test helpers: dense normal equations from a per-block evaluation dump, gauge-invariant pose comparison."""
import importlib
import numpy as np

uvs = importlib.import_module("uv-slam_amd")
abi = uvs.abi
synth = uvs.synth

NF = abi.NUM_FRAMES


def param_layout(w):
    F = 15 * NF
    Np, Nl = len(w.inv_depth), len(w.line_orth)
    return F, Np, Nl, F + Np + 4 * Nl


def dense_normal_equations(w, ev):
    """H = J^T J, g = J^T r over [frames(165) | points | lines] from an `abi.Eval` dump (Ex_Pose constant)."""
    F, Np, Nl, P = param_layout(w)
    H = np.zeros((P, P)); g = np.zeros(P)

    def add(cols, J, r):
        cols = np.asarray(cols)
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
            else: continue
            cols += [base + k for k in range(loc)]; src += [idx + k for k in range(loc)]
        add(cols, J0[:, src], ev.prior_r[:n])
    for b, blk in enumerate(w.imu):
        if blk.get("skip", 0): continue
        i = blk["frame_i"]
        add(list(range(15 * i, 15 * i + 30)), ev.imu_J[b], ev.imu_r[b])
    for k in range(len(w.pt_lm)):
        fi, fj, lm = int(w.pt_fi[k]), int(w.pt_fj[k]), int(w.pt_lm[k])
        cols = list(range(15 * fi, 15 * fi + 6)) + list(range(15 * fj, 15 * fj + 6)) + [F + lm]
        J = ev.pt_J[k][:, list(range(12)) + [18]]
        add(cols, J, ev.pt_r[k])
    for k in range(len(w.ln_lm)):
        fj, lm = int(w.ln_fj[k]), int(w.ln_lm[k])
        cols = list(range(15 * fj, 15 * fj + 6)) + list(range(F + Np + 4 * lm, F + Np + 4 * lm + 4))
        add(cols, ev.ln_J[k], ev.ln_r[k])
        if w.ln_has_vp[k]:
            add(cols, ev.vp_J[k], ev.vp_r[k])
    return H, g


def lm_reduced_system(w, ev, radius=1e4, dlo=1e-6, dhi=1e32):
    """First-iteration damped, Schur-reduced frame system in UNSCALED coordinates."""
    F, Np, Nl, P = param_layout(w)
    H, g = dense_normal_equations(w, ev)
    hd = np.diag(H).copy()
    s = 1.0 / (1.0 + np.sqrt(hd))
    dd = np.clip(s * s * hd, dlo, dhi) / (radius * s * s)
    Hd = H + np.diag(dd)
    Hff, Hfl, Hll = Hd[:F, :F], Hd[:F, F:], Hd[F:, F:]
    X = np.linalg.solve(Hll, Hfl.T)
    S = Hff - Hfl @ X
    gr = g[:F] - Hfl @ np.linalg.solve(Hll, g[F:])
    full_step = np.linalg.solve(Hd, -g)
    return dict(S=S, g=gr, hd=hd, dd=dd, step=full_step, H=H, gfull=g)


def unpad(v):
    """176-padded (16 per frame) -> 165."""
    idx = [16 * f + k for f in range(NF) for k in range(15)]
    v = np.asarray(v)
    if v.ndim == 1:
        return v[idx]
    return v[np.ix_(idx, idx)]


def quat_angle(qa, qb):
    """rotation angle (rad) between two unit quaternions (x,y,z,w)."""
    d = abs(float(np.dot(qa, qb)))
    return 2.0 * np.arccos(min(1.0, d))


def pose_deltas(A, B):
    """max position difference (m) and max rotation difference (rad) between two pose arrays [11][7]."""
    dp = np.abs(A[:, :3] - B[:, :3]).max()
    da = max(quat_angle(A[f, 3:], B[f, 3:]) for f in range(A.shape[0]))
    return dp, da


def marginalization_reference(w, ev):
    """MARGIN_OLD Schur complement in EXTENDED precision (numpy longdouble, plain Gaussian elimination with pivoting), from an `abi.Eval`
    dump of the post-solve window: the factors of estimator.cpp:1008-1129 (prior, IMU block 0, points anchored at frame 0, line / VP
    observations j != 0 of lines that start at frame 0), marginalised set = Pose[0], SpeedBias[0] and those landmarks.
    Returns (A_r, b_r, cols) over the kept columns `cols`: 0..164 = the frame layout (ORIGINAL frame numbering), -6..-1 = para_Ex_Pose
    (held constant by the solver but a parameter block of every point factor, so the reference's prior carries it)."""
    F, Np, Nl, P0 = param_layout(w)
    P = P0 + 6; EX = P0
    LD = np.longdouble
    H = np.zeros((P, P), LD); g = np.zeros(P, LD)

    def add(cols, J, r):
        cols = np.asarray(cols); J = np.asarray(J, LD); r = np.asarray(r, LD)
        H[np.ix_(cols, cols)] += J.T @ J
        g[cols] += J.T @ r

    drop = set(range(15))
    if w.prior is not None and w.prior.n > 0:
        p = w.prior; n = p.n; J0 = p.J0()
        cols, src = [], []
        for b in range(p.n_blocks):
            kind, fr, size, idx = p.block_kind[b], p.block_frame[b], p.block_size[b], p.block_idx[b]
            loc = 6 if size == 7 else size
            base = 15 * fr if kind == abi.BLOCK_POSE else 15 * fr + 6 if kind == abi.BLOCK_SPEEDBIAS else EX
            assert kind in (abi.BLOCK_POSE, abi.BLOCK_SPEEDBIAS, abi.BLOCK_EX_POSE)
            cols += [base + k for k in range(loc)]; src += [idx + k for k in range(loc)]
        add(cols, J0[:, src], ev.prior_r[:n])
    for b, blk in enumerate(w.imu):
        if blk["frame_i"] == 0 and not blk.get("skip", 0):
            add(list(range(0, 30)), ev.imu_J[b], ev.imu_r[b])
    for k in range(len(w.pt_lm)):
        fi, fj, lm = int(w.pt_fi[k]), int(w.pt_fj[k]), int(w.pt_lm[k])
        if fi != 0: continue
        add(list(range(0, 6)) + list(range(15 * fj, 15 * fj + 6)) + list(range(EX, EX + 6)) + [F + lm], ev.pt_J[k], ev.pt_r[k])
        drop.add(F + lm)
    start = {}
    for k in range(len(w.ln_lm)): start.setdefault(int(w.ln_lm[k]), int(w.ln_fj[k]))
    for k in range(len(w.ln_lm)):
        fj, lm = int(w.ln_fj[k]), int(w.ln_lm[k])
        if start[lm] != 0 or fj == 0: continue
        cols = list(range(15 * fj, 15 * fj + 6)) + list(range(F + Np + 4 * lm, F + Np + 4 * lm + 4))
        add(cols, ev.ln_J[k], ev.ln_r[k])
        if w.ln_has_vp[k]: add(cols, ev.vp_J[k], ev.vp_r[k])
        drop.update(range(F + Np + 4 * lm, F + Np + 4 * lm + 4))
    used = [c for c in range(P) if H[c, c] != 0]
    md = [c for c in used if c in drop]; kp = [c for c in used if c not in drop]
    assert all(c < F or c >= EX for c in kp)
    Amm = H[np.ix_(md, md)].copy(); R = np.concatenate([H[np.ix_(md, kp)], g[md][:, None]], axis=1).copy()
    m = len(md)
    for c in range(m):      # Gaussian elimination with partial pivoting in longdouble
        piv = c + int(np.argmax(np.abs(Amm[c:, c])))
        if piv != c: Amm[[c, piv]] = Amm[[piv, c]]; R[[c, piv]] = R[[piv, c]]
        f = Amm[c + 1:, c] / Amm[c, c]
        Amm[c + 1:] -= f[:, None] * Amm[c][None, :]; R[c + 1:] -= f[:, None] * R[c][None, :]
    X = np.zeros_like(R)
    for c in range(m - 1, -1, -1):
        X[c] = (R[c] - Amm[c, c + 1:] @ X[c + 1:]) / Amm[c, c]
    Ar = H[np.ix_(kp, kp)] - H[np.ix_(kp, md)] @ X[:, :-1]
    br = g[kp] - H[np.ix_(kp, md)] @ X[:, -1]
    return np.asarray(Ar, float), np.asarray(br, float), [c if c < F else c - P for c in kp]


def prior_information(p, n_frame_cols=165):
    """(H, b) = (J0^T J0, J0^T r0) of an `abi.Prior`, scattered to the 165-wide frame layout in ORIGINAL frame numbering for a MARGIN_OLD prior
    (block_frame is stored after the shift i -> i-1, estimator.cpp:1139-1152)."""
    J0, r0 = p.J0(), p.r0()
    cols, src = [], []
    for b in range(p.n_blocks):
        kind, fr, size, idx = p.block_kind[b], p.block_frame[b] + 1, p.block_size[b], p.block_idx[b]
        loc = 6 if size == 7 else size
        base = 15 * fr if kind == abi.BLOCK_POSE else 15 * fr + 6 if kind == abi.BLOCK_SPEEDBIAS else -6
        cols += [base + k for k in range(loc)]; src += [idx + k for k in range(loc)]
    Jc = J0[:, src]
    return Jc.T @ Jc, Jc.T @ r0, cols


def first_divergence(rg, ro, opts=None):
    """Where and how narrowly two LM traces (uvs_report of the HIP solver, of the oracle) part ways.
    Returns None when iteration count, accept / reject sequence and termination agree; otherwise a dict with the iteration `k` of the first
    differing DECISION, which test decided there and how close both sides were to its threshold:
      kind 'accept'   : the Ceres step test  rho = (cost - candidate) / model_cost_change > min_relative_decrease (estimator.cpp:982-994 -> trust_region_minimizer,
                        SURVEY.md Appendix B.5); margin = |rho - min_relative_decrease| on each side, rel_margin = margin / max(|rho|, min_relative_decrease)
      kind 'valid'    : model_cost_change > 0 (an invalid step); margin = |model_cost_change| relative to the cost
      kind 'terminate': same decisions up to the shorter trace, one side stopped (function / parameter tolerance, Appendix B.4); margin = distance of
                        |cost - candidate| / cost from function_tolerance on each side (the test that ends these windows)
    Up to iteration k both solvers made the same decisions, so their states there differ by round-off only and the quantities are comparable."""
    o = opts if opts is not None else abi.default_options()
    ng, no = int(rg.num_iterations), int(ro.num_iterations)
    ag, ao = list(rg.accepted[:ng + 1]), list(ro.accepted[:no + 1])
    if ng == no and ag == ao and rg.termination == ro.termination: return None
    n = min(ng, no)
    k = next((i for i in range(1, n + 1) if ag[i] != ao[i]), None)
    if k is None:
        k = n      # identical decisions; one side went on (or the two name different termination reasons at the same iteration)
        def ft(r):
            c, cand = r.cost[k], r.candidate_cost[k]
            return abs(abs(c - cand) / c - o.function_tolerance) if c > 0 else float("nan")
        return dict(k=k, kind="terminate", gpu=(ng, int(rg.termination)), oracle=(no, int(ro.termination)), margin_gpu=ft(rg), margin_oracle=ft(ro),
                    rel_margin=max(ft(rg), ft(ro)) / o.function_tolerance)
    if -1 in (ag[k], ao[k]):
        mg, mo = rg.model_cost_change[k], ro.model_cost_change[k]
        return dict(k=k, kind="valid", gpu=ag[k], oracle=ao[k], margin_gpu=abs(mg), margin_oracle=abs(mo), rel_margin=max(abs(mg), abs(mo)) / max(abs(rg.cost[k]), 1e-300))
    pg, po = rg.relative_decrease[k], ro.relative_decrease[k]
    thr = o.min_relative_decrease
    # conditioning of rho = (cost - candidate) / model_cost_change: both costs are sums of ~1e3 squared residuals, so their difference carries an absolute
    # round-off of a few 1e-16 * cost however it is summed; rho_noise = 4e-16 * cost / |model_cost_change| is the size of that noise in units of rho
    noise = lambda r: 4e-16 * abs(r.cost[k]) / max(abs(r.model_cost_change[k]), 1e-300)
    return dict(k=k, kind="accept", gpu=ag[k], oracle=ao[k], rho_gpu=pg, rho_oracle=po, margin_gpu=abs(pg - thr), margin_oracle=abs(po - thr),
                rel_margin=max(abs(pg - thr), abs(po - thr)) / max(abs(pg), abs(po), thr),
                mcc_over_cost=(abs(rg.model_cost_change[k]) / abs(rg.cost[k]), abs(ro.model_cost_change[k]) / abs(ro.cost[k])), rho_noise=(noise(rg), noise(ro)),
                cost_rel_diff=abs(rg.cost[k] - ro.cost[k]) / abs(ro.cost[k]), cand_rel_diff=abs(rg.candidate_cost[k] - ro.candidate_cost[k]) / abs(ro.candidate_cost[k]))


def prior_information_named(p, flag):
    """prior_information with the columns NAMED as tests/marg_ref.py names them (15 f + k in the window's ORIGINAL frame numbering, marg_ref.EX + k, marg_ref.TD),
    for both marginalization kinds: MARGIN_OLD stores block_frame after the shift i -> i - 1, MARGIN_SECOND_NEW after WINDOW_SIZE -> WINDOW_SIZE - 1 (estimator.cpp:1139-1152, 1203-1220)."""
    EX = 15 * NF; TD = EX + 6
    J0, r0 = p.J0(), p.r0()
    cols, src = [], []
    for b in range(p.n_blocks):
        kind, fr, size, idx = p.block_kind[b], p.block_frame[b], p.block_size[b], p.block_idx[b]
        fr = fr + 1 if flag == 0 or fr == abi.WINDOW_SIZE - 1 else fr
        loc = 6 if size == 7 else size
        base = {abi.BLOCK_POSE: 15 * fr, abi.BLOCK_SPEEDBIAS: 15 * fr + 6, abi.BLOCK_EX_POSE: EX, abi.BLOCK_TD: TD}[kind]
        cols += [base + k for k in range(loc)]; src += [idx + k for k in range(loc)]
    Jc = J0[:, src]
    return Jc.T @ Jc, Jc.T @ r0, cols


MARG_REF_CASES = {      # name: (option set, window index, where its prior comes from); every case with a prior runs under flags 0 and 1
    "70": ("default", 70, None), "71": ("default", 71, "own"), "72": ("default", 72, "own"), "41": ("default", 41, "own"), "73": ("default", 73, "own"), "74": ("default", 74, "own"),
    "td88": ("td", 88, None), "td89": ("td", 89, 88),      # 89 with 88's prior: the stiff foreign-prior construction of tests/test_td.py
    "ex80": ("ex", 80, None), "ex81": ("ex", 81, 80),
    "tdex83": ("tdex", 83, 183),
}


def marg_ref_options(optset):
    o = abi.default_options(); o.estimate_td = int("td" in optset); o.estimate_extrinsic = int("ex" in optset)
    return o


def marg_ref_case(name, solve, marginalize):
    """The post-solve window of a case of MARG_REF_CASES, built as tests/test_marginalization.py and tests/test_td.py build theirs: synth.make_window, the prior from
    `marginalize(window, flag)` of a predecessor (the previous window of the same trajectory, or the solved window `index` of the third field).
    `solve` and `marginalize` belong to ONE solver under marg_ref_options of the case's option set."""
    optset, index, prior = MARG_REF_CASES[name]
    td = "td" in optset
    mk = lambda i, **kw: synth.add_time_offset(synth.make_window(i, **kw), td_true=0.005) if td else synth.make_window(i, **kw)
    if prior == "own":
        w = synth.make_window(index, with_prior=True, marginalize_fn=marginalize)
    else:
        w = mk(index)
        if prior is not None:
            prev = mk(prior)
            st, _ = solve(prev)
            w.prior = marginalize(prev.with_state(st), 0)
    st, _ = solve(w)
    return w.with_state(st)


def marg_ref_weak_window(index=75, n_weak=2, offset=1e-9):
    """A window on which the reference's eps cut ACTS (marginalization_factor.cpp:234-243): `n_weak` points anchored at frame 0 keep ONE observation, in frame 1, of a point on
    the line through the two camera centres OF THE WINDOW'S STATE (relative offset `offset`: the epipole, no parallax); every other factor keeps its noise and the perturbed
    start state, so no residual block but those two is zero.  Their information is ~1e-14 <= 1e-8, the next eigenvalue of A_mm 1e-2.  Marginalized as it stands, without a
    solve: a solve would move the two cameras and give the points their parallax back."""
    o = synth.make_window(index).copy()
    keep = np.ones(len(o.pt_lm), bool)
    o.pt_pi = o.pt_pi.copy(); o.pt_pj = o.pt_pj.copy(); o.pt_fj = o.pt_fj.copy(); o.inv_depth = o.inv_depth.copy()
    Ri, ti = synth._cam(o.pose[0, :3], o.pose[0, 3:], o.ex_pose); Rj, tj = synth._cam(o.pose[1, :3], o.pose[1, 3:], o.ex_pose)
    d = (tj - ti) / np.linalg.norm(tj - ti)
    perp = np.cross(d, [0.3, -0.5, 0.8]); perp /= np.linalg.norm(perp)
    done = 0
    for lm in range(len(o.inv_depth)):
        rows = np.nonzero(o.pt_lm == lm)[0]
        if done == n_weak or int(o.pt_fi[rows[0]]) != 0: continue
        for sign in (1.0, -1.0):
            X = ti + sign * 6.0 * (d + offset * (done + 1) * perp)
            ci, cj = Ri.T @ (X - ti), Rj.T @ (X - tj)
            if ci[2] > 0.5 and cj[2] > 0.5: break
        else: continue
        k = rows[0]; keep[rows] = False; keep[k] = True
        o.pt_fj[k] = 1; o.pt_pi[k] = ci / ci[2]; o.pt_pj[k] = cj / cj[2]; o.inv_depth[lm] = 1.0 / ci[2]
        done += 1
    assert done == n_weak
    for nm in ("pt_lm", "pt_fi", "pt_fj", "pt_pi", "pt_pj"): setattr(o, nm, getattr(o, nm)[keep])
    return o
