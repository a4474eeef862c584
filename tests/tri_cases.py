"""Seeded scenes for the triangulation of landmarks (tests/test_tri_ref.py on the CPU, tests/test_triangulate.py on the GPU), in the layout of
uvs_tri_batch, and their 60-digit values (computed once per process and shared: nothing modifies them).

Three baseline classes -- the camera moves 0.2 m, 0.02 m or 0.002 m per frame, with small random rotations -- of 3 windows each holding
1, 64 and 65 points and as many lines: a full wave and one lane more, the smallest shapes that still show a tail-lane, window-boundary or
indexing error.  Points lie 1.5 .. 12 m in front of their start camera, every observation carries 1e-3 of noise in the normalized plane;
track lengths cover 2 and 11 views, start frames 0 and 9; lines have their first and last view 1 .. 10 frames apart.  `edge()` is one more
window with the degenerate landmarks (exact arithmetic: identity rotations, so that a zero is a zero in every precision).

TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import tri_ref

INIT_DEPTH = 5.0
BASELINES = {"0.2": 0.2, "0.02": 0.02, "0.002": 0.002}
SEEDS = {"0.2": 9201, "0.02": 9202, "0.002": 9203}
COUNTS = (1, 64, 65)          # landmarks per window, points and lines alike
NOISE = 1e-3
NF = 11


def _quat(rng, sigma):
    q = np.r_[sigma * rng.standard_normal(3), 1.0]
    return q / np.linalg.norm(q)


def _window(rng, baseline):
    """pose[11][7], ex_pose[7]: a camera that moves `baseline` per frame, mostly sideways, with small random rotations."""
    pose = np.zeros((NF, 7))
    direction = np.array([1.0, 0.15, 0.1]); direction /= np.linalg.norm(direction)
    for i in range(NF):
        pose[i, :3] = baseline * (i * direction + 0.1 * rng.standard_normal(3))
        pose[i, 3:] = _quat(rng, 0.01)
    ex = np.r_[0.05, -0.02, 0.01, _quat(rng, 0.02)]
    return pose, ex


def _view(cams, f, X):
    c = cams[0][f].T @ (X - cams[1][f])
    return c / c[2]


def _noisy(rng, v, noise):
    return v + np.r_[noise * rng.standard_normal(2), 0.0]


def _point_track(rng, cams, k, noise):
    # the first three tracks of a window pin the extremes; the rest are drawn
    start, views = [(0, 11), (9, 2), (0, 2)][k] if k < 3 else (int(rng.integers(0, 10)), 0)
    if views == 0:
        views = int(rng.integers(2, NF - start + 1))
    X = cams[1][start] + cams[0][start] @ np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4), 1.0]) * rng.uniform(1.5, 12.0)
    true_depth = (cams[0][start].T @ (X - cams[1][start]))[2]
    return start, [_noisy(rng, _view(cams, start + j, X), noise) for j in range(views)], true_depth


def _line_track(rng, cams, l, noise):
    fi, fj = [(0, 10), (3, 4), (9, 10)][l] if l < 3 else (int(rng.integers(0, 10)), 0)
    if fj == 0:
        fj = int(rng.integers(fi + 1, NF))
    A = cams[1][fi] + cams[0][fi] @ np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(4.0, 9.0)])
    d = rng.standard_normal(3); d[2] *= 0.3; d /= np.linalg.norm(d)
    ends = []
    for f in (fi, fj):          # other end points in every frame, as a detector finds them
        ends.append(_noisy(rng, _view(cams, f, A + rng.uniform(-1.0, -0.3) * d), noise))
        ends.append(_noisy(rng, _view(cams, f, A + rng.uniform(0.3, 1.0) * d), noise))
    return fi, fj, ends, np.r_[np.cross(A, d), d]


def _pack(pose, ex, pts, lns):
    """pts: (window, start, [obs]); lns: (window, fi, fj, [sp_i, ep_i, sp_j, ep_j]) -> the batch dict (the fields of uvs_tri_batch)."""
    i32 = lambda v: np.asarray(v, np.int32)
    f3 = lambda v: np.asarray(v, np.float64).reshape(-1, 3)
    return dict(pose=np.asarray(pose, np.float64), ex_pose=np.asarray(ex, np.float64),
                pt_window=i32([p[0] for p in pts]), pt_start=i32([p[1] for p in pts]), pt_obs_begin=i32(np.r_[0, np.cumsum([len(p[2]) for p in pts])]),
                pt_obs=f3([o for p in pts for o in p[2]]),
                ln_window=i32([l[0] for l in lns]), ln_fi=i32([l[1] for l in lns]), ln_fj=i32([l[2] for l in lns]),
                ln_sp_i=f3([l[3][0] for l in lns]), ln_ep_i=f3([l[3][1] for l in lns]), ln_sp_j=f3([l[3][2] for l in lns]), ln_ep_j=f3([l[3][3] for l in lns]))


@functools.lru_cache(maxsize=None)
def scene(cls, noise=NOISE):
    """The batch of a baseline class ("0.2", "0.02", "0.002"), with `true_depth` [n_points] and `true_plucker` [n_lines][6] = (n, d) beside it."""
    rng = np.random.default_rng(SEEDS[cls])
    poses, exs, pts, lns, depth, plucker = [], [], [], [], [], []
    for w, count in enumerate(COUNTS):
        pose, ex = _window(rng, BASELINES[cls])
        cams = tri_ref.cameras(pose, ex)
        poses.append(pose); exs.append(ex)
        for k in range(count):
            start, obs, z = _point_track(rng, cams, k if count > 3 else 3, noise)
            pts.append((w, start, obs)); depth.append(z)
        for l in range(count):
            fi, fj, ends, L = _line_track(rng, cams, l if count > 3 else 3, noise)
            lns.append((w, fi, fj, ends)); plucker.append(L)
    b = _pack(poses, exs, pts, lns)
    b["true_depth"] = np.array(depth); b["true_plucker"] = np.array(plucker)
    return b


def window_of(batch, w):
    """The one-window batch of window w of a batch."""
    p = np.flatnonzero(batch["pt_window"] == w); l = np.flatnonzero(batch["ln_window"] == w)
    beg = batch["pt_obs_begin"]
    out = dict(pose=batch["pose"][w:w + 1], ex_pose=batch["ex_pose"][w:w + 1], pt_window=np.zeros(len(p), np.int32), pt_start=batch["pt_start"][p],
               pt_obs_begin=(beg[p[0]:p[-1] + 2] - beg[p[0]]).astype(np.int32), pt_obs=batch["pt_obs"][beg[p[0]]:beg[p[-1] + 1]],
               ln_window=np.zeros(len(l), np.int32))
    for k in ("ln_fi", "ln_fj", "ln_sp_i", "ln_ep_i", "ln_sp_j", "ln_ep_j"):
        out[k] = batch[k][l]
    return out, p, l


@functools.lru_cache(maxsize=None)
def edge():
    """One window in exact arithmetic: identity rotations, the camera in the body's origin, frames 0 .. 8 a step of 0.25 m along x apart and frames
    9 and 10 in the place of frame 8, turned.
      point 0   an ordinary track (flag 0)
      point 1   bearings mirrored through the start camera: it triangulates behind it (flag 1)
      point 2   seen from frames 8, 9, 10 only -- identical camera centres: the fourth column of svd_A is zero, V = e4, depth 0 (flag 1)
      line 0    an ordinary line (flag 0)
      line 1    in the plane y = 0 that also holds both camera centres: the two back-projected planes coincide, d_w = 0 (flag 2)"""
    rng = np.random.default_rng(9210)
    pose = np.zeros((NF, 7)); pose[:, 6] = 1.0
    for i in range(NF):
        pose[i, 0] = 0.25 * min(i, 8)
    pose[9, 3:] = _quat(rng, 0.02); pose[10, 3:] = _quat(rng, 0.02)
    ex = np.r_[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    cams = tri_ref.cameras(pose, ex)
    X = np.array([0.5, -0.25, 4.0])
    ordinary = [_noisy(rng, _view(cams, f, X), NOISE) for f in range(0, 5)]
    behind = [np.r_[-o[:2], 1.0] for o in ordinary]
    same_centre = [_noisy(rng, _view(cams, f, np.array([2.5, 0.5, 6.0])), NOISE) for f in (8, 9, 10)]
    pts = [(0, 0, ordinary), (0, 0, behind), (0, 8, same_centre)]
    _, _, ends, _ = _line_track(rng, cams, 0, NOISE)
    coincide = [np.array([-0.25, 0.0, 1.0]), np.array([0.5, 0.0, 1.0]), np.array([-0.5, 0.0, 1.0]), np.array([0.25, 0.0, 1.0])]
    lns = [(0, 0, 10, ends), (0, 0, 1, coincide)]
    b = _pack([pose], [ex], pts, lns)
    b["expect_pt_flag"] = np.array([0, 1, 1], np.int32); b["expect_ln_flag"] = np.array([0, 2], np.int32)
    return b


@functools.lru_cache(maxsize=None)
def refs(name, noise=NOISE):
    """-> (numpy restatement (depth, pt_flag, orth, ln_flag), 60-digit dict of tri_ref.triangulate_hp) of scene(name) or of "edge"."""
    b = edge() if name == "edge" else scene(name, noise)
    return tri_ref.triangulate(b, INIT_DEPTH), tri_ref.triangulate_hp(b, INIT_DEPTH)


def e_ref_points(name):
    """E_ref of a class: the largest relative depth error of the numpy SVD restatement against the 60-digit values, and the mask of the cases
    that are compared (left out: a 60-digit depth within 1e-9 of the threshold, or not finite)."""
    (depth, _, _, _), hp = refs(name)
    keep = np.isfinite(hp["raw"]) & (np.abs(hp["raw"] - tri_ref.THRESHOLD) > 1e-9)
    return float(tri_ref.depth_errors(depth[keep], hp["depth"][keep]).max()), keep


def e_ref_lines(name):
    (_, _, orth, _), hp = refs(name)
    ok = hp["ln_flag"] == 0
    return float(tri_ref.line_errors(orth[ok], hp["U"][ok], hp["phi"][ok]).max()), ok


# ---- uvs_tri_check_lines: lines in front of, behind and straddling the start camera
@functools.lru_cache(maxsize=None)
def check_scene():
    """-> dict(pose, ex_pose, ln_window, ln_start, ln_sp0, ln_ep0, orth_old, kind): over the 3 windows of class "0.2", 1 / 64 / 65 lines whose OLD
    parameters are those of the true line; kind 0: both end points in front of the start camera, 1: both behind, 2: one of each."""
    base = scene("0.2")
    rng = np.random.default_rng(9220)
    win, start, sp0, ep0, orth, kind = [], [], [], [], [], []
    for w, count in enumerate(COUNTS):
        cams = tri_ref.cameras(base["pose"][w], base["ex_pose"][w])
        for l in range(count):
            s = int(rng.integers(0, NF)); k = l % 3
            z1, z2 = {0: (rng.uniform(3, 8), rng.uniform(3, 8)), 1: (-rng.uniform(3, 8), -rng.uniform(3, 8)), 2: (rng.uniform(3, 8), -rng.uniform(3, 8))}[k]
            A = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), 1.0]) * z1; B = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), 1.0]) * z2
            Aw, Bw = cams[1][s] + cams[0][s] @ A, cams[1][s] + cams[0][s] @ B
            d = (Bw - Aw) / np.linalg.norm(Bw - Aw)
            o, flag, _ = tri_ref.orth_of_plucker(np.cross(Aw, d), d)
            assert flag == 0
            win.append(w); start.append(s); sp0.append(A / A[2]); ep0.append(B / B[2]); orth.append(o); kind.append(k)
    return dict(pose=base["pose"], ex_pose=base["ex_pose"], ln_window=np.array(win, np.int32), ln_start=np.array(start, np.int32),
                ln_sp0=np.array(sp0), ln_ep0=np.array(ep0), orth_old=np.array(orth), kind=np.array(kind))


@functools.lru_cache(maxsize=None)
def check_refs():
    """-> (numpy flags, 60-digit flags, 60-digit deciding depths [n][2])."""
    c = check_scene()
    cams = [tri_ref.cameras(p, e) for p, e in zip(c["pose"], c["ex_pose"])]
    hp_cams = [tri_ref.cameras_hp(p, e) for p, e in zip(c["pose"], c["ex_pose"])]
    n = len(c["ln_window"])
    f64 = np.array([tri_ref.check_line(cams[c["ln_window"][l]], int(c["ln_start"][l]), c["ln_sp0"][l], c["ln_ep0"][l], c["orth_old"][l])[0] for l in range(n)], np.int32)
    hp = [tri_ref.check_line_hp(hp_cams[c["ln_window"][l]], int(c["ln_start"][l]), c["ln_sp0"][l], c["ln_ep0"][l], c["orth_old"][l]) for l in range(n)]
    return f64, np.array([h[0] for h in hp], np.int32), np.array([h[1] for h in hp])


# ---- uvs_tri_shift_depth
@functools.lru_cache(maxsize=None)
def shift_scene():
    """130 points anchored in camera 0 of a window of class "0.2" and handed to camera 1; every fifth lies behind the new camera, which has
    turned away from it (flag 1)."""
    base = scene("0.2")
    rng = np.random.default_rng(9230)
    cams = tri_ref.cameras(base["pose"][1], base["ex_pose"][1])
    n = sum(COUNTS)
    uv0 = np.c_[rng.uniform(-0.5, 0.5, n), rng.uniform(-0.4, 0.4, n), np.ones(n)]
    depth = rng.uniform(1.5, 12.0, n)
    depth[::5] = -depth[::5]          # a depth the solve left negative: behind both cameras
    return dict(uv0=uv0, depth=depth, marg_R=cams[0][0], marg_P=cams[1][0], new_R=cams[0][1], new_P=cams[1][1])


@functools.lru_cache(maxsize=None)
def shift_refs():
    """-> (numpy (depth_out, flag, z), 60-digit z as float64, 60-digit (depth_out, flag))."""
    s = shift_scene()
    f64 = tri_ref.shift_depth(s["uv0"], s["depth"], s["marg_R"], s["marg_P"], s["new_R"], s["new_P"], INIT_DEPTH)
    z = np.array([float(v) for v in tri_ref.shift_depth_hp(s["uv0"], s["depth"], s["marg_R"], s["marg_P"], s["new_R"], s["new_P"])])
    return f64, z, (np.where(z > 0, z, INIT_DEPTH), np.where(z > 0, 0, 1).astype(np.int32))


# ---- tracks of abi.Window objects (what api.Triangulator.triangulate_windows derives), restated independently
def tracks_of_windows(windows):
    pose = [w.pose for w in windows]; ex = [w.ex_pose for w in windows]
    pts, lns = [], []
    for wi, w in enumerate(windows):
        for lm in range(len(w.inv_depth)):
            rows = np.flatnonzero(w.pt_lm == lm)
            pts.append((wi, int(w.pt_fi[rows[0]]), [w.pt_pi[rows[0]]] + [w.pt_pj[r] for r in rows]))
        for lm in range(len(w.line_orth)):
            rows = np.flatnonzero(w.ln_lm == lm)
            a, z = rows[0], rows[-1]
            lns.append((wi, int(w.ln_fj[a]), int(w.ln_fj[z]), [w.ln_sp[a], w.ln_ep[a], w.ln_sp[z], w.ln_ep[z]]))
    return _pack(pose, ex, pts, lns)
