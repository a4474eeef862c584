"""Synthetic two-view scenes for the relative pose (tests/test_rp_ref.py, tests/test_relative_pose.py, smoke()): a pinhole of unit focal length,
points 2 .. 40 m in front of the first camera, the second camera one metre away (recoverPose's t has unit length, so its max_depth of 50 is 50
baselines), Gaussian noise of 0.1 px / 460 on every coordinate.  Every case is one item of uvs_rp_relative_pose; `ref` is the numpy restatement's
result, `hp` the 60-digit evaluation of steps 4 to 6 on the restatement's F and RANSAC mask, `e_ref` the restatement's error against it.  All
three are computed on demand and cached.

The seeds are picked so that the 60-digit evaluation alone meets the conditions test_rp_ref.py asserts (MIN_MARGIN, MIN_LEAD, MIN_SV_RATIO and
the two that make the singular vectors themselves safe, MIN_SIGN_MARGIN and MIN_GAP).

TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import rp_ref

NOISE = 0.1 / 460
MIN_MARGIN = 1e-9         # no comparison of a point closer to its threshold than this, relative
MIN_LEAD = 2              # the best good[k] exceeds the second best by at least this
MIN_SV_RATIO = 1e-3       # F's second singular value over its first
MIN_SIGN_MARGIN = 1e-6    # the sign rule of a singular vector is this far from flipping: the vectors are known to eps / (relative gap of the
                          # singular values) ~ 1e-9 for an essential matrix, whose two large singular values differ by the noise only
MIN_GAP = 1e-6            # the two smallest singular values of a point's 4 x 4 matrix, relative: Q is known to eps / gap = 2e-10 < MIN_MARGIN


def rot(axis, deg):
    a = np.asarray(axis, float) / np.linalg.norm(axis); th = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def two_views(rng, n, R, t, zmin=2.0, zmax=40.0, far=0, zfar=(60.0, 200.0), outliers=0, noise=NOISE):
    """n points X in the first camera's frame; the second sees R X + t.  far: the last `far` points lie zfar away; outliers: the first
    `outliers` right points are replaced by random ones.  -> left [n, 2], right [n, 2], outlier [n] bool."""
    z = rng.uniform(zmin, zmax, n)
    if far:
        z[n - far:] = rng.uniform(zfar[0], zfar[1], far)
    X = np.stack([rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-0.45, 0.45, n) * z, z], 1)
    Y = X @ np.asarray(R).T + np.asarray(t, float)
    left = X[:, :2] / X[:, 2:3] + noise * rng.standard_normal((n, 2))
    right = Y[:, :2] / Y[:, 2:3] + noise * rng.standard_normal((n, 2))
    out = np.zeros(n, bool)
    if outliers:
        right[:outliers] = rng.uniform(-0.6, 0.6, (outliers, 2)); out[:outliers] = True
    return left, right, out


I3 = np.eye(3)
# name -> (n, generator seed, RANSAC seed, arguments of two_views)
SPEC = {
    "sideways_150": (150, 11, 101, dict(R=I3, t=(-1.0, 0.0, 0.0))),
    "sideways_64": (64, 12, 102, dict(R=I3, t=(-1.0, 0.0, 0.0))),
    "forward_64": (64, 13, 103, dict(R=I3, t=(0.0, 0.0, -1.0), zmax=12.0)),
    "rot20_65": (65, 14, 104, dict(R=rot((0, 1, 0), 20.0), t=(-0.9, 0.1, 0.2))),
    "rot20_150": (150, 15, 105, dict(R=rot((0.2, 1, 0.1), 20.0), t=(-0.9, 0.1, 0.2))),
    "outliers30_150": (150, 16, 106, dict(R=rot((0, 1, 0), 5.0), t=(-1.0, 0.05, 0.1), outliers=45)),
    # a fifth of the points beyond max_depth in the first camera; the turn puts some of them within it in the second (the X test alone drops them)
    "beyond_65": (65, 17, 107, dict(R=rot((0, 1, 0), 20.0), t=(-1.0, 0.0, 0.1), far=13, zfar=(53.0, 60.0))),
    "low_parallax_64": (64, 18, 108, dict(R=I3, t=(-0.02, 0.0, 0.0))),                       # fails gate 1's parallax test
    "few_corres_20": (20, 19, 109, dict(R=I3, t=(-1.0, 0.0, 0.0))),                          # fails n > 20
    "inliers_gt12_21": (21, 20, 110, dict(R=I3, t=(-1.0, 0.0, 0.0))),                        # ends with 12 < inlier_cnt
    "inliers_le12_21": (21, 21, 111, dict(R=I3, t=(-1.0, 0.0, 0.0), far=11, zmax=5.0)),      # 10 points within max_depth: inlier_cnt <= 12
}
NAMES = tuple(SPEC)
GATED = ("low_parallax_64", "few_corres_20")


@functools.lru_cache(maxsize=None)
def case(name):
    n, gen, seed, kw = SPEC[name]
    left, right, outlier = two_views(np.random.default_rng(gen), n, **kw)
    return dict(name=name, left=left, right=right, seed=seed, outlier=outlier)


def item(name, window=0, frame_l=0):
    c = case(name)
    return dict(window=window, frame_l=frame_l, seed=c["seed"], left=c["left"], right=c["right"])


@functools.lru_cache(maxsize=None)
def ref(name):
    """The numpy restatement's result."""
    c = case(name)
    return rp_ref.relative_pose(c["left"], c["right"], c["seed"])


@functools.lru_cache(maxsize=None)
def hp(name):
    """The restatement's steps 1 to 3 with the 60-digit steps 4 to 6 (None for a case that never gets there)."""
    r = ref(name)
    if r["ransac_status"] != 0:
        return None
    c = case(name)
    return rp_ref.recover_hp(r["F"], r["keep"], rp_ref.round32(c["left"]), rp_ref.round32(c["right"]))


@functools.lru_cache(maxsize=None)
def _e_ref(name):
    return tuple(sorted(rp_ref.errors(ref(name), hp(name)).items()))


def e_ref(name):
    """The restatement's own error against the 60-digit values, per metric."""
    return dict(_e_ref(name))


def expected(name):
    """What the device must give: steps 1 to 3 of `ref`, steps 4 to 6 of `hp`."""
    out = dict(ref(name))
    if hp(name) is not None:
        h = hp(name)
        out.update({k: h[k] for k in ("good", "chosen", "inlier_cnt", "ok", "mask", "R", "t", "Rotation", "Translation")})
        out["status"] = rp_ref.OK if h["ok"] else rp_ref.FEW_INLIERS
    return out


# ---- a window of ten pairs: the newest frame is a sideways step from frame 9 on; frames 0 .. 3 see (nearly) what the newest frame sees
def window_tracks(n=40, seed=31):
    """Tracks (start_frame, points [11 - start, 3]) of one window in feature order.  Camera f stands at x = step[f]; the newest at 1 m.  Frames
    0 .. 3 stand within 2 cm of the newest (low parallax against it), frames 4 .. 9 a metre or more away.  Every fifth track starts at frame 2,
    so the pairs (0, 10) and (1, 10) have fewer correspondences than the others."""
    rng = np.random.default_rng(seed)
    step = np.array([1.0, 1.005, 0.99, 1.01, 0.0, -0.2, -0.4, -0.1, 0.1, -0.05, 1.0])
    z = rng.uniform(2.0, 40.0, n)
    X = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], 1)
    tracks = []
    for k in range(n):
        start = 2 if k % 5 == 4 else 0
        pts = []
        for f in range(start, 11):
            Y = X[k] - np.array([step[f], 0.0, 0.0])
            pts.append([Y[0] / Y[2] + NOISE * rng.standard_normal(), Y[1] / Y[2] + NOISE * rng.standard_normal(), 1.0])
        tracks.append((start, np.array(pts)))
    return tracks
