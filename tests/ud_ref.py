"""numpy restatement of the undistortion of the line front end's images (include/uvs_solver.h: uvs_lt_set_undistort, uvs_lt_set_remap,
uvs_lt_undistort; csrc/uvs_line_undistort.hip), which the device is held to word for word (the map) and byte for byte (the image).  The rule
is the project's own: a Q5 fixed-point map built in FP64, one rounding per operation in the order written (numpy evaluates an expression
operation by operation, never fused), a bilinear blend with exact integer weights and a zero border decided per tap.  Every function has a
vectorized form and a plain loop form.  `variant` plants one misreading of the rule (VARIANTS), for the tests that show they would be seen.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

LIMIT = 1 << 24
VARIANTS = ("truncate", "round_511", "border_per_pixel", "p1_p2_swapped", "margin_after_map")


def _fix(m, variant=None):
    """X = rint(32 m) clamped to -2^24 .. 2^24, -2^24 where not finite -> int32."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.float64(32.0) * np.asarray(m, np.float64)
        v = np.trunc(v) if variant == "truncate" else np.rint(v)
        v = np.where(np.isfinite(v), np.clip(v, -float(LIMIT), float(LIMIT)), -float(LIMIT))
    return v.astype(np.int32)


def _chain(cam, u, v, variant=None):
    """The header's FP64 chain for the doubles u, v (scalars or arrays) -> (mx, my)."""
    fx, fy, cx, cy, k1, k2, p1, p2 = [np.float64(c) for c in cam]
    if variant == "p1_p2_swapped":
        p1, p2 = p2, p1
    two = np.float64(2.0)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (u - cx) / fx
        y = (v - cy) / fy
        x2 = x * x; y2 = y * y; xy = x * y; r2 = x2 + y2
        kr = np.float64(1.0) + (k1 * r2 + k2 * (r2 * r2))
        xd = x * kr + ((two * p1) * xy + p2 * (r2 + two * x2))
        yd = y * kr + (p1 * (r2 + two * y2) + (two * p2) * xy)
        mx = fx * xd + cx
        my = fy * yd + cy
    return mx, my


def out_size(W, H, cm, rm):
    return W - 2 * cm, H - 2 * rm


def build_map(cam, W, H, cm=0, rm=0, variant=None):
    """cam = (fx, fy, cx, cy, k1, k2, p1, p2) of the raw image W x H -> map [Ho, Wo, 2] int32: (X, Y) in 1/32 px of the raw image."""
    Wo, Ho = out_size(W, H, cm, rm)
    vo, uo = np.mgrid[0:Ho, 0:Wo]
    late = variant == "margin_after_map"
    u = (uo + (0 if late else cm)).astype(np.float64); v = (vo + (0 if late else rm)).astype(np.float64)
    mx, my = _chain(cam, u, v, variant)
    if late:
        mx = mx + np.float64(cm); my = my + np.float64(rm)
    return np.stack([_fix(mx, variant), _fix(my, variant)], -1)


def build_map_loops(cam, W, H, cm=0, rm=0):
    Wo, Ho = out_size(W, H, cm, rm)
    m = np.zeros((Ho, Wo, 2), np.int32)
    for vo in range(Ho):
        for uo in range(Wo):
            mx, my = _chain(cam, np.float64(uo + cm), np.float64(vo + rm))
            m[vo, uo, 0] = _fix(mx); m[vo, uo, 1] = _fix(my)
    return m


def clamp_map(map_xy):
    """What uvs_lt_set_remap keeps of a caller's map."""
    return np.clip(np.asarray(map_xy, np.int64), -LIMIT, LIMIT).astype(np.int32)


def remap(src, map_xy, variant=None):
    """src [H, W] uint8, map [Ho, Wo, 2] int32 -> [Ho, Wo] uint8."""
    src = np.asarray(src, np.uint8)
    H, W = src.shape
    m = np.asarray(map_xy, np.int64)
    X, Y = m[..., 0], m[..., 1]
    xi, yi, ax, ay = X >> 5, Y >> 5, X & 31, Y & 31

    def tap(y, x):
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(ok, src[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.int64), 0), ok

    (p00, k00), (p01, k01), (p10, k10), (p11, k11) = tap(yi, xi), tap(yi, xi + 1), tap(yi + 1, xi), tap(yi + 1, xi + 1)
    s = (32 - ax) * (32 - ay) * p00 + ax * (32 - ay) * p01 + (32 - ax) * ay * p10 + ax * ay * p11
    out = (s + (511 if variant == "round_511" else 512)) >> 10
    if variant == "border_per_pixel":
        out = np.where(k00 & k01 & k10 & k11, out, 0)
    return out.astype(np.uint8)


def remap_loops(src, map_xy):
    src = np.asarray(src, np.uint8)
    H, W = src.shape
    Ho, Wo = map_xy.shape[:2]
    out = np.zeros((Ho, Wo), np.uint8)
    S = lambda y, x: int(src[y, x]) if 0 <= x < W and 0 <= y < H else 0
    for vo in range(Ho):
        for uo in range(Wo):
            X, Y = int(map_xy[vo, uo, 0]), int(map_xy[vo, uo, 1])
            xi, yi, ax, ay = X >> 5, Y >> 5, X & 31, Y & 31
            s = (32 - ax) * (32 - ay) * S(yi, xi) + ax * (32 - ay) * S(yi, xi + 1) + (32 - ax) * ay * S(yi + 1, xi) + ax * ay * S(yi + 1, xi + 1)
            out[vo, uo] = (s + 512) >> 10
    return out


def undistort(src, cam, cm=0, rm=0, variant=None):
    """The raw image src through the camera's map -> the undistorted, cropped image."""
    H, W = np.asarray(src).shape
    return remap(src, build_map(cam, W, H, cm, rm, variant), variant)
