"""Inputs of the keyframe-feature tests (tests/test_keyframe_features.py): seeded images, window points, cameras and the rendered two-view
scene of the image-to-loop-edge test.  Everything is generated from seeds with numpy alone; nothing is read but the BRIEF pattern fixture."""
import functools
import os

import numpy as np

import kf_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN_FILE = os.path.join(ROOT, "tests", "golden", "brief_pattern.yml")
W, H = 752, 480
CAM = (460.0, 460.0, 376.0, 240.0)                                        # the rendered views
CAM_DIST = (461.6, 460.3, 363.0, 248.1, -0.2917, 0.08228, 5.333e-05, -1.578e-04)      # EuRoC cam0
SCENE_SEEDS = (0, 1, 2, 3)
MAX_KEYPOINTS = 4096


def gaussian_filter(a, sigma):
    """Separable Gaussian of a float image, truncated at 4 sigma, border reflect-101."""
    r = int(4.0 * sigma + 0.5)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2); k /= k.sum()
    p = np.pad(np.asarray(a, np.float64), r, mode="reflect")
    h = sum(k[i] * p[:, i:i + a.shape[1]] for i in range(2 * r + 1))
    return sum(k[i] * h[i:i + a.shape[0], :] for i in range(2 * r + 1))


def texture(seed, width=W, height=H, n_rect=120):
    """The scene recipe: smooth noise scaled to 40..160, random grey rectangles, a slight blur, pixel noise."""
    rng = np.random.default_rng(1000 + seed)
    a = gaussian_filter(rng.normal(0.0, 1.0, (height, width)), 6.0)
    a = 40.0 + 120.0 * (a - a.min()) / (a.max() - a.min())
    for _ in range(n_rect):
        w, h = rng.integers(8, max(9, width // 6)), rng.integers(8, max(9, height // 6))
        x, y = rng.integers(0, width - 4), rng.integers(0, height - 4)
        a[y:y + h, x:x + w] = rng.uniform(0.0, 255.0)
    a = gaussian_filter(a, 0.8) + rng.normal(0.0, 2.0, a.shape)
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pattern():
    from helpers import abi
    return abi.load_brief_pattern(PATTERN_FILE)


def window_points(seed, n, width, height):
    """Sub-pixel window points inside the image."""
    rng = np.random.default_rng(2000 + seed)
    return np.stack([rng.uniform(0, width - 1, n), rng.uniform(0, height - 1, n)], 1).astype(np.float32)


def border_points(width, height):
    """Window points within 24 pixels of each border (the pattern reaches 24 pixels), at negative fractional coordinates, on the last row and
    column and just outside."""
    pts = []
    for t in (0.0, 0.25, 0.5, 3.75, 11.5, 23.0, 23.99):
        pts += [(t, height / 2 + t), (width - 1 - t, height / 3 + t), (width / 2 + t, t), (width / 3 - t, height - 1 - t), (t, t), (width - 1 - t, height - 1 - t)]
    pts += [(-0.5, -0.5), (-0.25, 10.75), (10.5, -0.99), (-0.999, -0.001), (-1.0, 5.0), (-3.5, -7.25), (width - 0.5, height - 0.5), (width + 5.25, 20.0),
            (30.0, height + 2.5), (-30.0, -30.0)]
    return np.array(pts, np.float32)


def checkerboard(width, height, cell):
    y, x = np.mgrid[0:height, 0:width]
    return (255 * (((x // cell) + (y // cell)) & 1)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> dict(image, window_uv, cam).  The scenes carry 150 sub-pixel window points plus the border points."""
    c = {}
    for s in SCENE_SEEDS:
        img = texture(s)
        uv = np.concatenate([window_points(s, 150, W, H), border_points(W, H)])
        c[f"scene_{s}"] = dict(image=img, window_uv=uv, cam=CAM_DIST if s % 2 else CAM)
        n = len(kf_ref.keypoints(kf_ref.score_map(img)[0])[0])
        assert 100 <= n <= MAX_KEYPOINTS, (s, n)             # a changed generator cannot slip out of range
    c["small_64x48"] = dict(image=texture(10, 64, 48, 12), window_uv=np.concatenate([window_points(10, 20, 64, 48), border_points(64, 48)]), cam=CAM_DIST)
    c["odd_131x97"] = dict(image=texture(11, 131, 97, 30), window_uv=np.concatenate([window_points(11, 40, 131, 97), border_points(131, 97)]), cam=CAM)
    c["odd_77x203"] = dict(image=texture(12, 77, 203, 30), window_uv=window_points(12, 33, 77, 203), cam=CAM_DIST)
    c["wide_1030x67"] = dict(image=texture(13, 1030, 67, 60), window_uv=window_points(13, 64, 1030, 67), cam=CAM)
    rng = np.random.default_rng(14)
    c["tiny_9x9"] = dict(image=rng.integers(0, 256, (9, 9)).astype(np.uint8), window_uv=border_points(9, 9), cam=CAM)
    spike = np.full((9, 9), 10, np.uint8); spike[4, 4] = 200
    c["tiny_9x9_spike"] = dict(image=spike, window_uv=np.zeros((0, 2), np.float32), cam=CAM)
    c["constant"] = dict(image=np.full((50, 70), 93, np.uint8), window_uv=window_points(15, 10, 70, 50), cam=CAM)
    c["checkerboard"] = dict(image=checkerboard(200, 120, 5), window_uv=window_points(16, 30, 200, 120), cam=CAM_DIST)
    c["checkerboard_1px"] = dict(image=checkerboard(96, 64, 1), window_uv=np.zeros((0, 2), np.float32), cam=CAM)
    c["noise"] = dict(image=rng.integers(0, 256, (90, 150)).astype(np.uint8), window_uv=window_points(17, 25, 150, 90), cam=CAM_DIST)
    c["no_window"] = dict(image=texture(18, 160, 120, 30), window_uv=np.zeros((0, 2), np.float32), cam=CAM)
    return c


# ---------------------------------------------------------------- image to loop edge: two rendered views of a textured plane
PLANE_Z, TEXEL = 4.0, 0.005
TEX_W, TEX_H = 1400, 1000
VIEW2_ROT_DEG = (4.0, 3.0)                     # about y, then about z
VIEW2_T = np.array([0.25, -0.1, 0.15])
N_WINDOW = 150


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def plane_texture(seed=7):
    return texture(100 + seed, TEX_W, TEX_H, 400).astype(np.float64)


def view_pose(k):
    """World-from-camera (R, t) of view k: view 0 at the origin, the plane z = PLANE_Z in front of it; view k > 0 the revisiting pose, scaled by
    k (k = 1: the issue's 4 / 3 degrees and (0.25, -0.1, 0.15) m)."""
    if k == 0:
        return np.eye(3), np.zeros(3)
    return rot_y(np.radians(VIEW2_ROT_DEG[0] * k)) @ rot_z(np.radians(VIEW2_ROT_DEG[1] * k)), VIEW2_T * k


def pixel_to_plane(R, t, uv, cam=CAM):
    """The 3-D points (world frame) where the rays of pixels uv [n, 2] of the camera (R, t) meet the plane."""
    fx, fy, cx, cy = cam[:4]
    d = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(len(uv))], 1) @ R.T
    lam = (PLANE_Z - t[2]) / d[:, 2]
    return t[None] + lam[:, None] * d


def project(R, t, X, cam=CAM):
    fx, fy, cx, cy = cam[:4]
    p = (X - t[None]) @ R
    return np.stack([fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy], 1)


def render(tex, R, t, seed, width=W, height=H, noise=1.5):
    """Bilinear rendering of the plane's texture (texel (i, j) at x = (i - TEX_W / 2) TEXEL, y = (j - TEX_H / 2) TEXEL) with pixel noise."""
    v, u = np.mgrid[0:height, 0:width]
    X = pixel_to_plane(R, t, np.stack([u.ravel(), v.ravel()], 1).astype(np.float64))
    i = X[:, 0] / TEXEL + TEX_W / 2; j = X[:, 1] / TEXEL + TEX_H / 2
    i0 = np.clip(np.floor(i).astype(int), 0, TEX_W - 2); j0 = np.clip(np.floor(j).astype(int), 0, TEX_H - 2)
    a = np.clip(i - i0, 0, 1); b = np.clip(j - j0, 0, 1)
    g = (1 - a) * (1 - b) * tex[j0, i0] + a * (1 - b) * tex[j0, i0 + 1] + (1 - a) * b * tex[j0 + 1, i0] + a * b * tex[j0 + 1, i0 + 1]
    inside = (i >= 0) & (i <= TEX_W - 1) & (j >= 0) & (j <= TEX_H - 1)
    g = np.where(inside, g, 0.0) + np.random.default_rng(3000 + seed).normal(0.0, noise, g.shape)
    return np.clip(np.rint(g), 0, 255).astype(np.uint8).reshape(height, width)


def strongest(ref, n=N_WINDOW):
    """The n strongest keypoints of a frame (kf_ref.extract's dict or the device's): ties by list order.  -> indices in list order."""
    order = np.argsort(-ref["score"].astype(int), kind="stable")[:n]
    return np.sort(order)


@functools.lru_cache(maxsize=None)
def views(n_views=2):
    """[(image, R, t)] of the first n_views view poses."""
    tex = plane_texture()
    return [(render(tex, *view_pose(k), seed=k),) + view_pose(k) for k in range(n_views)]
