"""Independent numpy restatement of the point front end's tracking step: cv::calcOpticalFlowPyrLK(cur_img, forw_img, cur_pts, forw_pts, status,
err, cv::Size(21, 21), 3) followed by inBorder (reference feature_tracker/src/feature_tracker.cpp:86-95, utility.cpp:3-9) as uvs_ft_track
(csrc/uvs_feature_track.hip) computes them.

TEST INFRASTRUCTURE ONLY.  OpenCV is not a dependency, so this file is the pin (as tests/kf_ref.py is for the keyframe features); the numerics
are the ones include/uvs_solver.h spells out.  Integers are int64 arrays or Python ints, FP64 values are numpy.float64 scalars, and every FP64
expression is written in the order the header gives, one rounding per operation.

  refl      reflect-101: -i for i < 0, 2 n - 2 - i for i >= n
  pyramid   level l + 1 = ((W + 1) / 2, (H + 1) / 2); out = (sum k_i k_j in(refl(2 x + i), refl(2 y + j)) + 128) >> 8, k = {1, 4, 6, 4, 1}
  Scharr    Gx(x, y) = 3 (p(x+1, y-1) - p(x-1, y-1)) + 10 (p(x+1, y) - p(x-1, y)) + 3 (p(x+1, y+1) - p(x-1, y+1)), Gy the transpose, p read with
            refl; at a pixel outside the image the same formula holds (the gradient of the reflected image)
  sample    21 x 21 window around an FP64 position with 14-bit bilinear weights; grey levels keep 5 fractional bits
  track     levels from the coarsest down, at most 30 iterations each, integer window sums, a handful of FP64 operations per iteration
"""
import numpy as np

import kf_ref

KERNEL = np.array([1, 4, 6, 4, 1], np.int64)
WIN, HALF = 21, 10
MAX_ITER = 30
TRACKED, LOST_FLAT, LOST_OUTSIDE, LOST_BORDER = 0, 1, 2, 3
MAX_LEVELS = 4
MIN_EIG = np.float64(1e-4)
MIN_DET = np.float64(1.1920929e-7)
EPS2 = np.float64(1e-4)
OSC = np.float64(0.01)
SCALE = np.float64(2.0 ** -20)
MAX_COORD = 1e6
TRACE_HEADER, TRACE_ITER = 16, 10
TRACE_LEVEL = 320                      # doubles of one level's trace: header + 30 iterations, padded


def min_size(levels):
    return 24 << (levels - 1)


def refl(i, n):
    """reflect-101 of an int array (or int) into 0..n-1; exact for -n < i < 2 n - 1."""
    i = np.abs(np.asarray(i, np.int64))
    return np.where(i >= n, 2 * n - 2 - i, i)


def pyrdown(img):
    """[H, W] uint8 -> [(H + 1) / 2, (W + 1) / 2] uint8."""
    img = np.asarray(img)
    H, W = img.shape
    h, w = (H + 1) // 2, (W + 1) // 2
    a = img.astype(np.int64)
    cols = [refl(2 * np.arange(w) + i, W) for i in range(-2, 3)]
    rows = [refl(2 * np.arange(h) + j, H) for j in range(-2, 3)]
    hs = sum(KERNEL[i] * a[:, cols[i]] for i in range(5))            # [H, w]
    v = sum(KERNEL[j] * hs[rows[j], :] for j in range(5))            # [h, w]
    return ((v + 128) >> 8).astype(np.uint8)


def pyramid(img, levels):
    assert 1 <= levels <= MAX_LEVELS
    out = [np.ascontiguousarray(img, dtype=np.uint8)]
    for _ in range(levels - 1):
        out.append(pyrdown(out[-1]))
    return out


def _read(img, xs, ys):
    """img at the int64 index arrays xs [n] (columns) and ys [m] (rows) through refl -> [m, n] int64."""
    H, W = img.shape
    return img[np.ix_(refl(ys, H), refl(xs, W))].astype(np.int64)


def scharr_at(img, xs, ys):
    """(Gx, Gy) [m, n] int64 at the pixel columns xs and rows ys, which may lie outside the image."""
    xs = np.asarray(xs, np.int64); ys = np.asarray(ys, np.int64)
    p = lambda dx, dy: _read(img, xs + dx, ys + dy)
    gx = 3 * (p(1, -1) - p(-1, -1)) + 10 * (p(1, 0) - p(-1, 0)) + 3 * (p(1, 1) - p(-1, 1))
    gy = 3 * (p(-1, 1) - p(-1, -1)) + 10 * (p(0, 1) - p(0, -1)) + 3 * (p(1, 1) - p(1, -1))
    return gx, gy


def scharr(img):
    H, W = np.asarray(img).shape
    return scharr_at(np.asarray(img), np.arange(W), np.arange(H))


def weights(cx, cy):
    """-> (iu.x, iu.y, w00, w01, w10, w11) of the window around the FP64 position (cx, cy)."""
    cx = np.float64(cx); cy = np.float64(cy)
    ux = cx - np.float64(HALF); uy = cy - np.float64(HALF)
    fx = np.floor(ux); fy = np.floor(uy)
    a = ux - fx; b = uy - fy
    one = np.float64(1.0); s = np.float64(16384.0)
    w00 = int(np.rint((one - a) * (one - b) * s))
    w01 = int(np.rint(a * (one - b) * s))
    w10 = int(np.rint((one - a) * b * s))
    return int(fx), int(fy), w00, w01, w10, 16384 - w00 - w01 - w10


def _blend(P, w):
    """P [22, 22] int64 (rows iu.y .. iu.y + 21) -> S [21, 21]."""
    return w[0] * P[:-1, :-1] + w[1] * P[:-1, 1:] + w[2] * P[1:, :-1] + w[3] * P[1:, 1:]


def sample_grey(img, cx, cy):
    """[21, 21] int64 grey levels with 5 fractional bits."""
    ix, iy, *w = weights(cx, cy)
    P = _read(img, ix + np.arange(WIN + 1), iy + np.arange(WIN + 1))
    return (_blend(P, w) + 256) >> 9


def sample_grad(img, cx, cy):
    """(Dx, Dy) [21, 21] int64."""
    ix, iy, *w = weights(cx, cy)
    gx, gy = scharr_at(img, ix + np.arange(WIN + 1), iy + np.arange(WIN + 1))
    return (_blend(gx, w) + 8192) >> 14, (_blend(gy, w) + 8192) >> 14


def inside(x, y, W, H):
    return bool(x >= 0.0 and x <= np.float64(W - 1) and y >= 0.0 and y <= np.float64(H - 1))


def structure(A11i, A12i, A22i):
    """The int64 window sums -> (A11, A12, A22, D, minEig) as FP64."""
    A11 = np.float64(A11i) * SCALE; A12 = np.float64(A12i) * SCALE; A22 = np.float64(A22i) * SCALE
    D = A11 * A22 - A12 * A12
    t = A11 - A22
    min_eig = (A22 + A11 - np.sqrt(t * t + np.float64(4.0) * A12 * A12)) / np.float64(882.0)
    return A11, A12, A22, D, min_eig


def track_point(prev_pyr, next_pyr, px, py, trace=None):
    """One point from the pyramid prev_pyr into next_pyr -> (x, y, status, iterations at level 0).  `trace`, a list, receives one dict per
    visited level: the values uvs_ft_debug_point returns."""
    L = len(prev_pyr)
    px = np.float64(px); py = np.float64(py)
    qx = qy = None
    iters0 = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for l in range(L - 1, -1, -1):
            s = np.float64(2.0 ** -l); up = np.float64(2.0 ** l)
            plx = px * s; ply = py * s
            if qx is None:
                qx, qy = plx, ply
            else:
                qx = qx * np.float64(2.0); qy = qy * np.float64(2.0)
            H, W = prev_pyr[l].shape
            rec = dict(level=l, p=(plx, ply), iters=[], flat=0)
            if trace is not None:
                trace.append(rec)
            if not inside(plx, ply, W, H):
                rec["q"] = (qx, qy)
                return qx * up, qy * up, LOST_OUTSIDE, 0
            I = sample_grey(prev_pyr[l], plx, ply)
            Dx, Dy = sample_grad(prev_pyr[l], plx, ply)
            A11i = int((Dx * Dx).sum()); A12i = int((Dx * Dy).sum()); A22i = int((Dy * Dy).sum())
            A11, A12, A22, D, min_eig = structure(A11i, A12i, A22i)
            rec.update(w=weights(plx, ply)[2:], A=(A11i, A12i, A22i), D=D, min_eig=min_eig)
            if min_eig < MIN_EIG or D < MIN_DET:
                rec["flat"] = 1; rec["q"] = (qx, qy)
                if l > 0:
                    continue
                return qx, qy, LOST_FLAT, 0
            n = 0
            pdx = pdy = np.float64(0.0)
            for j in range(MAX_ITER):
                if not inside(qx, qy, W, H):
                    rec["q"] = (qx, qy)
                    return qx * up, qy * up, LOST_OUTSIDE, (n if l == 0 else 0)
                J = sample_grey(next_pyr[l], qx, qy)
                d = J - I
                b1i = int((d * Dx).sum()); b2i = int((d * Dy).sum())
                b1 = np.float64(b1i) * SCALE; b2 = np.float64(b2i) * SCALE
                dx = (A12 * b2 - A22 * b1) / D
                dy = (A12 * b1 - A11 * b2) / D
                it = dict(w=weights(qx, qy)[2:], b=(b1i, b2i), delta=(dx, dy))
                qx = qx + dx; qy = qy + dy
                n += 1
                stop = bool(dx * dx + dy * dy <= EPS2)
                if not stop and j > 0 and abs(dx + pdx) < OSC and abs(dy + pdy) < OSC:
                    qx = qx - np.float64(0.5) * dx; qy = qy - np.float64(0.5) * dy
                    stop = True
                it["q"] = (qx, qy)
                rec["iters"].append(it)
                if stop:
                    break
                pdx, pdy = dx, dy
            rec["q"] = (qx, qy)
            if l == 0:
                iters0 = n
    H, W = prev_pyr[0].shape
    if not inside(qx, qy, W, H):
        return qx, qy, LOST_OUTSIDE, iters0
    xr = np.rint(qx); yr = np.rint(qy)
    ok = 1.0 <= xr < np.float64(W - 1) and 1.0 <= yr < np.float64(H - 1)
    return qx, qy, (TRACKED if ok else LOST_BORDER), iters0


def track(prev_pyr, next_pyr, pts, cam=None):
    """pts [n, 2] float64 -> dict(next_xy [n, 2] float64, status [n] int32, iterations [n] int32, n_tracked[, next_norm [n, 2]: liftProjective of
    the tracked points, zero for the others])."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    n = len(pts)
    xy = np.zeros((n, 2)); st = np.zeros(n, np.int32); it = np.zeros(n, np.int32)
    for i, (x, y) in enumerate(pts):
        qx, qy, s, k = track_point(prev_pyr, next_pyr, x, y)
        xy[i] = (qx, qy); st[i] = s; it[i] = k
    out = dict(next_xy=xy, status=st, iterations=it, n_tracked=int((st == TRACKED).sum()))
    if cam is not None:
        nm = np.zeros((n, 2))
        ok = st == TRACKED
        if ok.any():
            nm[ok] = kf_ref.lift(cam, xy[ok])          # the keyframe unit's liftProjective: one statement of it
        out["next_norm"] = nm
    return out


def track_images(prev_img, next_img, pts, levels, cam=None):
    return track(pyramid(prev_img, levels), pyramid(next_img, levels), pts, cam)


def trace_array(trace, levels):
    """The list of level records of track_point -> the [4, 320] float64 array of uvs_ft_debug_point (unvisited entries zero)."""
    out = np.zeros((MAX_LEVELS, TRACE_LEVEL))
    for rec in trace:
        r = out[rec["level"]]
        r[0] = 1.0; r[1], r[2] = rec["p"]
        if "w" in rec:
            r[3:7] = rec["w"]; r[7:10] = rec["A"]; r[10] = rec["D"]; r[11] = rec["min_eig"]
        r[12] = rec["flat"]; r[13] = len(rec["iters"]); r[14], r[15] = rec["q"]
        for j, it in enumerate(rec["iters"]):
            o = TRACE_HEADER + TRACE_ITER * j
            r[o:o + 4] = it["w"]; r[o + 4:o + 6] = it["b"]; r[o + 6:o + 8] = it["delta"]; r[o + 8:o + 10] = it["q"]
    return out
