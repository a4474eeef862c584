"""The cases of the tests of the line front end's undistortion (tests/test_line_undistort.py): small raw images of noise under cameras scaled
to them, the bars of ld_cases seen through the barrel camera, and a smooth analytic image for the accuracy of the rule.  Everything is
deterministic and computed once.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import kf_ref
import ld_cases
import ld_ref
import ud_ref

# the distortion of EuRoC's cam0 with k1 rounded as the issue states it, and a pincushion whose corner taps leave the source
BARREL = (-0.29, 0.07395907, 0.00019359, 1.76187114e-05)
PINCUSHION = (0.25, 0.0, 0.00019359, 1.76187114e-05)
SIZES = ((40, 32), (96, 80), (131, 97))          # 131 x 97 (and 121 x 91 under the margins): a pixel count that is no multiple of four
MARGINS = ((0, 0), (5, 3))


def camera(W, H, dist):
    """fx = fy = 0.6 W, the principal point off-centre and between pixels."""
    return (0.6 * W, 0.6 * W, 0.52 * W + 0.3, 0.47 * H - 0.2) + tuple(dist)


def _case(W, H, m, dname, seed):
    return dict(W=W, H=H, cm=m[0], rm=m[1], cam=camera(W, H, BARREL if dname == "barrel" else PINCUSHION), seed=seed)


CASES = {f"{W}x{H}_m{m[0]}_{d}": _case(W, H, m, d, 100 * i + 10 * j + k)
         for i, (W, H) in enumerate(SIZES) for j, m in enumerate(MARGINS) for k, d in enumerate(("barrel", "pincushion"))}
LARGE = "376x240_m5_barrel"
CASES[LARGE] = _case(376, 240, (5, 3), "barrel", 900)
SMALL = tuple(n for n in CASES if n != LARGE)
MAX_W, MAX_H = 131, 97                           # of the small cases' handle


@functools.lru_cache(maxsize=None)
def raw(name):
    c = CASES[name]
    return np.random.default_rng(c["seed"]).integers(0, 256, (c["H"], c["W"]), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def ref_map(name, variant=None):
    c = CASES[name]
    return ud_ref.build_map(c["cam"], c["W"], c["H"], c["cm"], c["rm"], variant)


@functools.lru_cache(maxsize=None)
def ref_image(name, variant=None):
    return ud_ref.remap(raw(name), ref_map(name, variant), variant)


def ideal_of_raw(cam, uv, extra=40):
    """The pixel of the distortion-free camera (same fx, fy, cx, cy) that a raw pixel uv [n, 2] shows: kf_ref's liftProjective, its fixed-point
    iteration continued `extra` rounds with kf_ref's own distortion, then the pinhole matrix.  -> ([n, 2], the largest distance in raw pixels
    between uv and the forward projection of the result: the inverse model's residual)."""
    cam = kf_ref.camera8(cam)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    m = kf_ref.lift(cam, uv)
    md = np.stack([(uv[:, 0] - cam[2]) / cam[0], (uv[:, 1] - cam[3]) / cam[1]], 1)
    for _ in range(extra):
        dx, dy = kf_ref.distortion(cam, m[:, 0], m[:, 1])
        m = np.stack([md[:, 0] - dx, md[:, 1] - dy], 1)
    back = kf_ref.space_to_plane(cam, m)
    return np.stack([cam[0] * m[:, 0] + cam[2], cam[1] * m[:, 1] + cam[3]], 1), float(np.abs(back - uv).max())


# ---- the bars of ld_cases through the barrel camera
BAR_SCENE = "131x97"


@functools.lru_cache(maxsize=None)
def bar_scene():
    """-> dict: raw [H, W] uint8 = frame B of ld_cases.scene(BAR_SCENE) as the barrel camera sees it (the bars rendered at the ideal position of
    every raw pixel, then the scene's noise), cam, edges [2 n, 4] in pixels of the undistorted image (ld_cases' edges_b), undistorted = ud_ref's
    image of raw."""
    W, H, _, seed = ld_cases.SCENES[BAR_SCENE]
    cam = camera(W, H, BARREL)
    b, level = ld_cases.bars(BAR_SCENE)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    ideal, _ = ideal_of_raw(cam, np.stack([u.ravel(), v.ravel()], 1))
    x = ideal[:, 0].reshape(H, W); y = ideal[:, 1].reshape(H, W)
    canvas = np.full((H, W), ld_cases.BACKGROUND)
    for i in range(len(b)):
        canvas[ld_cases._inside(x, y, b[i])] = level[i]
    canvas += np.random.default_rng(2000 + seed).normal(0.0, ld_cases.SIGMA, canvas.shape)
    img = np.clip(np.rint(canvas), 0, 255).astype(np.uint8)
    return dict(raw=img, cam=cam, W=W, H=H, edges=ld_cases.scene(BAR_SCENE)["edges_b"], undistorted=ud_ref.undistort(img, cam))


@functools.lru_cache(maxsize=None)
def bar_ref(which):
    """ld_ref.detect of the bar scene's 'undistorted' or 'raw' image with ld_cases' parameters."""
    P = ld_cases.PARAMS
    return ld_ref.detect(bar_scene()[which], P["grad_threshold"], P["min_pixels"], P["min_length"], ld_cases.MAX_LINES)


def edge_fits(segs, edges):
    """Per edge the best (offset, cover) among the segments within 1 px of its line, or None: test_line_detect's report."""
    out = []
    for e in edges:
        fits = [ld_cases.edge_report(s, e) for s in segs]
        fits = [f for f in fits if f[0] <= 1.0]
        out.append(max(fits, key=lambda f: f[1]) if fits else None)
    return out
