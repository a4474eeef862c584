"""Independent numpy restatement of keyframe feature extraction: computeWindowBRIEFPoint / computeBRIEFPoint (reference
pose_graph/src/keyframe.cpp:75-113), DVision::BRIEF::compute (ThirdParty/DVision/BRIEF.cpp:39-106) and PinholeCamera::liftProjective
(camera_models/PinholeCamera.cc:450-510, 678-694) as uvs_kf_extract (csrc/uvs_keyframe_features.hip) computes them.

TEST INFRASTRUCTURE ONLY.  OpenCV is not a dependency, so this file is the pin (as tests/lc_ref.py is for loop verification); the numerics are
the ones include/uvs_solver.h spells out:

  blur    separable, taps {7, 17, 32, 46, 52, 46, 32, 17, 7} = round(256 exp(-k^2 / 8) / sum), border reflect-101 (numpy's pad mode "reflect"),
          rows then columns in integers, out = (sum + 32768) >> 16
  FAST    9 of 16, threshold 20, on the unblurred image; score max(A, B) - 1 where a corner, 0 elsewhere; kept iff strictly greater than its
          8 neighbours; keypoints in row-major order
  BRIEF   xa = int(float32(u) + float32(x1[i])) (truncation toward zero), bit i set iff the four coordinates are inside the image and
          blur[ya][xa] < blur[yb][xb]; bit i = bit (i & 63) of word (i >> 6)
  lift    FP64, every product and sum rounded as written (no fused multiply-add)
"""
import numpy as np

TAPS = np.array([7, 17, 32, 46, 52, 46, 32, 17, 7], np.int64)
FAST_THRESHOLD = 20
RING = [(0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3)]
OK, OVERFLOW = 0, 1
MIN_SIZE = 9
MAX_COORD = 1e6


def taps_from_formula():
    g = np.exp(-np.arange(-4, 5) ** 2 / 8.0)
    return np.rint(256.0 * g / g.sum()).astype(np.int64)


def blur(img):
    """[H, W] uint8 -> [H, W] uint8."""
    img = np.asarray(img)
    H, W = img.shape
    assert H >= MIN_SIZE and W >= MIN_SIZE
    p = np.pad(img.astype(np.int64), 4, mode="reflect")
    h = sum(TAPS[k] * p[:, k:k + W] for k in range(9))
    v = sum(TAPS[k] * h[k:k + H, :] for k in range(9))
    return ((v + 32768) >> 16).astype(np.uint8)


def score_map(img):
    """[H, W] uint8 -> ([H, W] uint8 score map, corners before suppression)."""
    img = np.asarray(img).astype(np.int16)
    H, W = img.shape
    out = np.zeros((H, W), np.uint8)
    if H < 7 or W < 7:
        return out, 0
    c = img[3:H - 3, 3:W - 3]
    d = np.stack([img[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] - c for dx, dy in RING])      # [16, H - 6, W - 6]
    d2 = np.concatenate([d, d[:8]])
    A = np.max(np.stack([d2[i:i + 9].min(0) for i in range(16)]), 0)
    B = np.max(np.stack([(-d2[i:i + 9]).min(0) for i in range(16)]), 0)
    s = np.maximum(A, B)
    corner = s > FAST_THRESHOLD
    out[3:H - 3, 3:W - 3] = np.where(corner, s - 1, 0).astype(np.uint8)
    return out, int(corner.sum())


def keypoints(smap):
    """Non-maximum suppression -> (xy [n, 2] int32 in row-major order, score [n] uint8)."""
    s = np.pad(np.asarray(smap).astype(np.int16), 1)
    H, W = smap.shape
    c = s[1:-1, 1:-1]
    keep = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= c > s[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    yx = np.argwhere(keep)                                    # sorted by y, then x
    return yx[:, ::-1].astype(np.int32).copy(), smap[keep].astype(np.uint8)


def pack_bits(bits):
    """[n, 256] bool -> [n, 4] uint64, bit i of a descriptor = bit (i & 63) of word (i >> 6)."""
    b = np.asarray(bits).astype(np.uint64).reshape(len(bits), 4, 64)
    return (b << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def brief(blurred, uv, pattern):
    """blurred [H, W] uint8, uv [n, 2] (cast to float32: cv::Point2f), pattern int32 [4, 256] -> [n, 4] uint64."""
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    H, W = blurred.shape
    pat = np.asarray(pattern).astype(np.float32)
    assert np.all(np.isfinite(uv)) and np.all(np.abs(uv) <= MAX_COORD)
    xa = (uv[:, :1] + pat[0][None]).astype(np.int32); ya = (uv[:, 1:] + pat[1][None]).astype(np.int32)
    xb = (uv[:, :1] + pat[2][None]).astype(np.int32); yb = (uv[:, 1:] + pat[3][None]).astype(np.int32)
    assert xa.dtype == np.int32 and (uv[:, :1] + pat[0][None]).dtype == np.float32
    inside = (xa >= 0) & (xa < W) & (ya >= 0) & (ya < H) & (xb >= 0) & (xb < W) & (yb >= 0) & (yb < H)
    cl = lambda a, n: np.clip(a, 0, n - 1)
    less = blurred[cl(ya, H), cl(xa, W)] < blurred[cl(yb, H), cl(xb, W)]
    return pack_bits(inside & less)


def distortion(cam, x, y):
    """PinholeCamera::distortion (:678-694), in the type of x."""
    k1, k2, p1, p2 = cam[4:8]
    mx2 = x * x; my2 = y * y; mxy = x * y
    rho2 = mx2 + my2
    rad = k1 * rho2 + k2 * rho2 * rho2
    return x * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2), y * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2)


def camera8(cam, dtype=np.float64):
    return np.array(list(cam) + [0.0] * (8 - len(cam)), dtype)


def lift(cam, uv, dtype=np.float64):
    """liftProjective of uv [n, 2] -> [n, 2] (mx_u, my_u); cam = (fx, fy, cx, cy[, k1, k2, p1, p2]).  dtype = numpy.longdouble evaluates the
    same expressions in extended precision."""
    cam = camera8(cam, dtype)
    uv = np.asarray(uv).astype(dtype).reshape(-1, 2)
    fx, fy, cx, cy = cam[:4]
    one = dtype(1.0)
    inv_K11 = one / fx; inv_K13 = -cx / fx; inv_K22 = one / fy; inv_K23 = -cy / fy
    mx_d = inv_K11 * uv[:, 0] + inv_K13
    my_d = inv_K22 * uv[:, 1] + inv_K23
    mx_u, my_u = mx_d, my_d
    if np.any(cam[4:8] != 0):
        for _ in range(8):
            dx, dy = distortion(cam, mx_u, my_u)
            mx_u = mx_d - dx; my_u = my_d - dy
    return np.stack([mx_u, my_u], 1)


def space_to_plane(cam, m):
    """PinholeCamera::spaceToPlane (:533-555) of normalized points m [n, 2] -> pixels."""
    cam = camera8(cam)
    m = np.asarray(m, np.float64).reshape(-1, 2)
    x, y = m[:, 0], m[:, 1]
    if np.any(cam[4:8] != 0):
        dx, dy = distortion(cam, x, y)
        x = x + dx; y = y + dy
    return np.stack([cam[0] * x + cam[2], cam[1] * y + cam[3]], 1)


def extract(img, window_uv, cam, pattern, max_keypoints=4096):
    """One frame as uvs_kf_extract returns it (plus the blurred image and the score map of uvs_kf_debug_frame)."""
    img = np.asarray(img, np.uint8)
    bl = blur(img)
    smap, n_corners = score_map(img)
    xy, sc = keypoints(smap)
    n = len(xy)
    xy, sc = xy[:max_keypoints], sc[:max_keypoints]
    return dict(status=OVERFLOW if n > max_keypoints else OK, n_keypoints=n, n_returned=len(xy), n_corners_before_nms=n_corners,
                xy=xy, score=sc, norm=lift(cam, xy), desc=brief(bl, xy, pattern),
                window_desc=brief(bl, np.asarray(window_uv, np.float32).reshape(-1, 2), pattern), blur=bl, score_map=smap)
