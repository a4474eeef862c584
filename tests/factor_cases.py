"""Windows for the factor tests (tests/test_factor_ref.py, tests/test_gpu_factors.py): name -> (window, options).

Whole windows: the canonical windows 3, 4, 11 and 13, one with a time offset, one with a free extrinsic, one with the prior of marginalizing
the previous window, and that one moved 0.05 m / 0.05 m/s off the prior's linearization point with a frame quaternion stored as -q (prior_dx
takes e.w < 0).  Edge blocks are written into a copy of a smaller canonical window by editing its arrays (`edge`; the ABI validates the
structure of a window, not its values); `w.edge` maps a label to (family, block index) and `w.edge_note` holds what was realised.
`imu_offnorm` is an IMU-only window with one frame quaternion off unit norm by 1e-9: only the IMU factor divides by the squared norm
(Eigen's inverse()), the point and line kernels take a unit quaternion for granted as the reference's analytic Jacobians do, so the case
carries no landmark.
"""
import numpy as np
import mpmath as mp
from mpmath import mpf

from helpers import abi, synth
import factor_ref as fr

WHOLE = ["w3", "w4", "w11", "w13", "td", "extrinsic", "prior", "prior_moved"]
EDGE = ["edge", "imu_offnorm"]
NAMES = WHOLE + EDGE
SOLVE_NAMES = ["w3", "w4", "td", "extrinsic", "prior", "prior_moved", "edge"]      # the windows of the solver-instantiation checks
VP_TARGETS = [1e-15, 5e-15, 2e-14, 1e-13, 1e-12, 1e-10, 1e-8, 1e-4]


def options(name):
    o = abi.default_options()
    if name == "td": o.estimate_td = 1
    if name == "extrinsic": o.estimate_extrinsic = 1
    return o


def level_stride(name):
    """Every block gets its own input-rounding level: a whole window is twenty seconds on eight cores (factor_ref supports sampling, the cases do not need it)."""
    return 1


def _preintegrate(n_samples, seed, ba, bg):
    """A pre-integration of n_samples 200 Hz samples through synth.PreIntegration.push_back, so that delta_*, covariance and jacobian belong together."""
    rng = np.random.default_rng([seed, 41])
    gf, gph, gam = rng.uniform(0.2, 0.6, 3), rng.uniform(0, 2 * np.pi, 3), rng.uniform(0.1, 0.3, 3)
    af, aph, aam = rng.uniform(0.2, 0.6, 3), rng.uniform(0, 2 * np.pi, 3), rng.uniform(0.2, 0.6, 3)
    q = synth.exp_quat(rng.normal(0, 0.05, 3)); t = 0.0
    meas = lambda tt, qq: (synth.quat_to_R(qq).T @ (aam * np.sin(2 * np.pi * af * tt + aph) + synth.G) + ba, gam * np.sin(2 * np.pi * gf * tt + gph) + bg)
    a0, g0 = meas(t, q)
    pre = synth.PreIntegration(a0, g0, ba, bg)
    for _ in range(n_samples):
        q = synth.quat_mul(q, synth.exp_quat(gam * np.sin(2 * np.pi * gf * (t + 0.5 * synth.IMU_DT) + gph) * synth.IMU_DT)); q /= np.linalg.norm(q)
        t += synth.IMU_DT
        a1, g1 = meas(t, q)
        pre.push_back(synth.IMU_DT, a1, g1)
    return pre


def _unit(rng):
    d = rng.standard_normal(3)
    return d / np.linalg.norm(d)


def _mpv(a):
    return [mpf(float(x)) for x in a]


def _line_dc(w, k):
    """d_c (and n_c) of line observation k at the window's state, 60 digits."""
    fj, lm = int(w.ln_fj[k]), int(w.ln_lm[k])
    x = _mpv(w.pose[fj][:6]) + _mpv(w.line_orth[lm])
    return fr._line_cam(x, mpf(float(w.pose[fj][6])), _mpv(w.ex_pose))


def _edge(seed=21):
    mp.mp.dps = fr.DPS
    w = synth.make_window(seed, n_points=60, n_lines=32, n_tagged=20)
    rng = np.random.default_rng([seed, 5])
    w.imu = [dict(b) for b in w.imu]
    edge, note = {}, {}
    # ---- IMU: bias offsets of frames 0..2 (|dbg| 0 / 1e-3 / 1e-1 rad/s, |dba| 0 / 0.1 / 1 m/s^2)
    for f, (g, a) in enumerate(((0.0, 0.0), (1e-3, 0.1), (1e-1, 1.0))):
        w.speedbias[f, 6:9] = w.imu[f]["linearized_bg"] + g * _unit(rng); w.speedbias[f, 3:6] = w.imu[f]["linearized_ba"] + a * _unit(rng)
        edge[f"imu.dbg={g:g},dba={a:g}"] = ("imu", f)
    # ---- IMU: pre-integrations of two samples (0.01 s), 5 s and 9.9 s (blocks 3, 4, 5).  ONE sample (0.005 s) is singular in the reference's own
    # formulation and is therefore replaced: after one midpoint step the velocity rows of the noise map V are exactly 2 / dt times its position
    # rows (integration_base.h:108-121), so the covariance has rank 12, covariance.inverse() does not exist and the oracle's Cholesky refuses it.
    for b, n in ((3, 2), (4, 1000), (5, 1980)):
        pre = _preintegrate(n, b, w.imu[b]["linearized_ba"], w.imu[b]["linearized_bg"])
        blk = pre.as_block(b); assert blk["skip"] == 0
        w.imu[b] = blk; edge[f"imu.sum_dt={n * synth.IMU_DT:g}"] = ("imu", b)
    # ---- IMU: frames 170 degrees apart: q_e.w near zero and positive (block 6), near zero and negative (block 8: frame 9 stored as -q)
    for f, sign in ((7, 1.0), (9, -1.0)):
        q = synth.quat_mul(synth.quat_mul(w.pose[f - 1, 3:], w.imu[f - 1]["delta_q"]), synth.exp_quat(np.deg2rad(170.0) * _unit(rng)))
        w.pose[f, 3:] = sign * q / np.linalg.norm(q); edge[f"imu.170deg,sign={sign:+g}"] = ("imu", f - 1)
    # ---- lines: whole turns, phi near 0 and pi / 2, a line whose normal is (nearly) the optical axis in one observation, equal endpoints
    untag = [l for l in range(len(w.line_orth)) if not w.ln_has_vp[np.nonzero(w.ln_lm == l)[0][0]]]
    first = lambda l: int(np.nonzero(w.ln_lm == l)[0][0])
    for l, turns in zip(untag[0:3], (-8, 6, 2000)):
        w.line_orth[l, :3] += turns * np.pi; edge[f"line.angles{turns:+d}pi"] = ("ln", first(l))
    w.line_orth[untag[3], 3] = 1e-6; edge["line.phi=1e-6"] = ("ln", first(untag[3]))
    w.line_orth[untag[4], 3] = np.pi / 2 - 1e-6; edge["line.phi=pi/2-1e-6"] = ("ln", first(untag[4]))
    for l, ratio in zip(untag[5:7], (1e-6, 1e-12)):
        k = first(l) + 2; fj = int(w.ln_fj[k])
        Rc, tc = synth._cam(w.pose[fj, :3], w.pose[fj, 3:] / np.linalg.norm(w.pose[fj, 3:]), w.ex_pose)
        n_c = np.array([np.sqrt(ratio), 0.0, 1.0]); d_c = np.array([0.0, 1.0, 0.0])
        p0 = np.cross(d_c, n_c)                     # p0 x d_c = n_c
        w.line_orth[l] = synth.line_to_orth(Rc @ p0 + tc, Rc @ d_c)
        nc, _ = _line_dc(w, k)
        got = float((nc[0] ** 2 + nc[1] ** 2) / nc[2] ** 2)
        assert 0.25 * ratio < got < 4 * ratio, (ratio, got)
        edge[f"line.nxy2/nz2={ratio:g}"] = ("ln", k); note[f"line.nxy2/nz2={ratio:g}"] = got
    k = first(untag[7]) + 1; w.ln_ep[k] = w.ln_sp[k]; edge["line.equal_endpoints"] = ("ln", k)
    # ---- points: inverse depth 1e-4 and 50, depth 0.05 in frame j, observation = rounded projection, residual 1 (the knee), 1e2, 1e4 under the loss
    firstp = lambda lm: int(np.nonzero(w.pt_lm == lm)[0][0])
    w.inv_depth[0] = 1e-4; edge["point.lam=1e-4"] = ("pt", firstp(0))
    w.inv_depth[1] = 50.0; edge["point.lam=50"] = ("pt", firstp(1))
    done = False
    for lm in range(2, 20):
        for k in np.nonzero(w.pt_lm == lm)[0]:
            fi, fj = int(w.pt_fi[k]), int(w.pt_fj[k])
            Ri, ti = synth._cam(w.pose[fi, :3], w.pose[fi, 3:] / np.linalg.norm(w.pose[fi, 3:]), w.ex_pose); Rj, tj = synth._cam(w.pose[fj, :3], w.pose[fj, 3:] / np.linalg.norm(w.pose[fj, 3:]), w.ex_pose)
            a = (Rj.T @ (Ri @ w.pt_pi[k]))[2]; b = (Rj.T @ (ti - tj))[2]
            d = (0.05 - b) / a
            if d > 0.1:
                w.inv_depth[lm] = 1.0 / d; edge["point.depth_j=0.05"] = ("pt", int(k)); done = True; lm_depth = lm
                break
        if done: break
    assert done
    free = [lm for lm in range(2, 30) if lm != lm_depth][:4]
    o = abi.default_options()

    def project(k):
        fi, fj, lm = int(w.pt_fi[k]), int(w.pt_fj[k]), int(w.pt_lm[k])
        z2 = [mpf(0), mpf(0)]
        r, _ = fr._point_res(_mpv(w.pose[fi]), _mpv(w.pose[fj]), _mpv(w.ex_pose), mpf(float(w.inv_depth[lm])), _mpv(w.pt_pi[k]), [mpf(0), mpf(0), mpf(1)], z2, z2, mpf(0), mpf(0), mpf(0), mpf(1), False)
        return np.array([float(r[0]), float(r[1])])
    k = firstp(free[0]) + 1; w.pt_pj[k, :2] = project(k); edge["point.obs=projection"] = ("pt", k)
    for lm, mag in zip(free[1:], (1.0, 1e2, 1e4)):
        k = firstp(lm) + 1; w.pt_pj[k, :2] = project(k) - np.array([mag / o.point_sqrt_info, 0.0]); edge[f"point.r={mag:g}"] = ("pt", k)
    # ---- VP: the measured vanishing point at 1 - c^2 = target, built at 60 digits from the line's own d_c and rounded, both signs of c0
    tagged = np.nonzero(w.ln_has_vp == 1)[0]
    picks = tagged[np.linspace(0, len(tagged) - 1, 2 * len(VP_TARGETS)).astype(int)]
    assert len(set(picks.tolist())) == 2 * len(VP_TARGETS)
    for n, k in enumerate(picks):
        target, sign = VP_TARGETS[n // 2], (1.0 if n % 2 == 0 else -1.0)
        _, dc = _line_dc(w, int(k))
        nd = mp.sqrt(fr._dot(dc, dc)); dh = [c / nd for c in dc]
        a = fr._cross(dh, [mpf(0.3), mpf(-0.5), mpf(0.8)]); na = mp.sqrt(fr._dot(a, a)); a = [c / na for c in a]
        s = mp.sqrt(mpf(target)); c = mp.sqrt(1 - mpf(target))
        v = [sign * (c * dh[i] + s * a[i]) for i in range(3)]
        sc = 1 / abs(v[2]) if abs(v[2]) > mpf("0.05") else mpf(1)      # the usual (x, y, +-1) scaling where it exists; keeps the sign of c0
        w.ln_vp[k] = [float(sc * x) for x in v]
        vr = _mpv(w.ln_vp[k]); cr = fr._cross(dc, vr)
        got = float(fr._dot(cr, cr) / (fr._dot(dc, dc) * fr._dot(vr, vr)))
        assert not (0.9e-14 <= got <= 1.1e-14) and 0.99 * target < got < 1.01 * target, (target, got)
        lab = f"vp.s2={target:g},c0{'+' if sign > 0 else '-'}"
        edge[lab] = ("ln", int(k)); note[lab] = got
    w.edge, w.edge_note = edge, note
    return w


def _imu_offnorm(seed=23):
    w = synth.make_window(seed, n_points=0, n_lines=0, n_tagged=0)
    w.pose[4, 3:] *= 1.0 + 1e-9
    w.edge = {"imu.offnorm_qj": ("imu", 3), "imu.offnorm_qi": ("imu", 4)}; w.edge_note = {"|q|^2-1": float(np.sum(w.pose[4, 3:] ** 2) - 1.0)}
    return w


def build(name, marginalize_fn=None):
    """-> (window, options).  prior / prior_moved need marginalize_fn(window, flag) -> abi.Prior (the product's on the GPU, the oracle's on the CPU)."""
    if name in ("w3", "w4", "w11", "w13"): w = synth.make_window(int(name[1:]))
    elif name == "td": w = synth.add_time_offset(synth.make_window(8), seed=8)
    elif name == "extrinsic": w = synth.make_window(9)
    elif name in ("prior", "prior_moved"):
        w = synth.make_window(11, with_prior=True, marginalize_fn=marginalize_fn)
        if name == "prior_moved":
            p = w.prior; rng = np.random.default_rng(77); flipped = None
            for b in range(p.n_blocks):
                kind, fr_, off = p.block_kind[b], p.block_frame[b], p.x0_off[b]
                x0 = np.array(p.x0[off:off + p.block_size[b]])
                if kind == abi.BLOCK_POSE:
                    w.pose[fr_, :3] = x0[:3] + 0.05 * _unit(rng)
                    if flipped is None and fr_ >= 2: w.pose[fr_, 3:] = -w.pose[fr_, 3:]; flipped = fr_
                elif kind == abi.BLOCK_SPEEDBIAS:
                    w.speedbias[fr_, :3] = x0[:3] + 0.05 * _unit(rng)
            assert flipped is not None
            w.edge = {}; w.edge_note = {"frame stored as -q": flipped}
    elif name == "edge": w = _edge()
    elif name == "imu_offnorm": w = _imu_offnorm()
    else: raise KeyError(name)
    return w, options(name)


def check_structure(name, w, o):
    """The case is what its name promises."""
    if name in WHOLE:
        assert len(w.pt_lm) == 750 and len(w.ln_lm) == 280 and len(w.imu) == 10
    if name == "td": assert o.estimate_td and w.pt_vel_i is not None and np.abs(w.pt_vel_j).max() > 0
    if name == "extrinsic": assert o.estimate_extrinsic
    if name in ("prior", "prior_moved"): assert w.prior is not None and w.prior.n == 75
    if name == "edge":
        assert len(w.edge) == 3 + 3 + 2 + 8 + 7 + 2 * len(VP_TARGETS), len(w.edge)
        assert len(set(w.edge.values())) == len(w.edge)
    if name == "imu_offnorm": assert len(w.pt_lm) == 0 and len(w.ln_lm) == 0 and abs(np.sum(w.pose[4, 3:] ** 2) - 1.0) > 1e-9
