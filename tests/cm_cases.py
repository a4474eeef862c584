"""The cases of the camera-model tests (tests/test_camera_models.py): the five shipped fisheye configurations (tests/golden/cameras), their
edge-case variants, the points they are lifted at, and the bars of ld_cases seen through a 150-degree Kannala-Brandt camera.  Everything is
deterministic and computed once, the 60-digit references included.  TEST INFRASTRUCTURE ONLY."""
import functools
import os

import numpy as np

import cm_ref
import kf_cases
import ld_cases
import ld_ref
import ud_ref
from helpers import abi

CAMERAS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cameras")
FIXTURES = ("tum", "cla", "realsense_fisheye", "black_box", "3dm")
KB_FIXTURES = FIXTURES[:3]
PINHOLE, MEI, KB = cm_ref.PINHOLE, cm_ref.MEI, cm_ref.KB

# E_ref: the largest absolute error of a ray component of cm_ref's FP64 restatement against the 60-digit evaluation of the reference's
# definition, over every model and point below and over the grids of the five image rectangles (test_definition measures it and holds this
# record to the measurement; DESIGN.md 3.18 has the figures).  Measured 1.165e-15, at realsense_fisheye's pixel just above th = pi / 2: its
# branch ends at th_max = 1.618, r' is 0.23 there and divides the rounding of r; everywhere else, the grids of the five image rectangles
# included, the error is below 4.9e-16.  The device's Kannala-Brandt rays are allowed 4 E_ref, at least 8 * 2^-52.
E_REF = 1.2e-15
KB_ALLOWANCE = max(4.0 * E_REF, 8.0 * 2.0 ** -52)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return abi.load_camera_calibration(os.path.join(CAMERAS, name + "_config.yaml"))


def _with(name, **kw):
    f = fixture(name)
    names = abi.CAM_PARAMS[f["model"]]
    return f["model"], tuple(kw.get(k, v) for k, v in zip(names, f["params"])), f["width"], f["height"]


@functools.lru_cache(maxsize=None)
def models():
    """name -> (model id, params, image width, height)."""
    m = {n: _with(n) for n in FIXTURES}
    m["kb_k5_0"] = _with("tum", k5=0.0)
    m["kb_k45_0"] = _with("tum", k4=0.0, k5=0.0)
    m["kb_zero"] = _with("tum", k2=0.0, k3=0.0, k4=0.0, k5=0.0)
    m["mei_xi_1"] = _with("black_box", xi=1.0)
    m["mei_no_distortion"] = _with("black_box", k1=0.0, k2=0.0, p1=0.0, p2=0.0)
    m["pinhole"] = (PINHOLE, tuple(kf_cases.CAM_DIST), 752, 480)
    m["pinhole_no_distortion"] = (PINHOLE, tuple(kf_cases.CAM) + (0.0,) * 4, 752, 480)
    return m


MODEL_NAMES = FIXTURES + ("kb_k5_0", "kb_k45_0", "kb_zero", "mei_xi_1", "mei_no_distortion", "pinhole", "pinhole_no_distortion")
N_POINTS = 1000
# A pixel beyond the branch lifts to th = r.  Where r_max is large (cla: th_max = pi and r(pi) = 489) such a pixel lies hundreds of image widths
# out and sin / cos of th = r > 8 lose ulp(r) > 8 * 2^-52 before any model is involved, so those models get no such point
BEYOND_LIMIT = 8.0
N_HP = 65          # the points held to the 60-digit reference: the special ones and the first random ones (a polynomial's roots cost ~50 ms)
BATCHES = (1, 63, 64, 65, 1000)


def _pixel_at_theta(P, th):
    """The pixel on the row of the principal point whose ray makes the angle th with the axis."""
    return (float(P.sx * cm_ref._kb_r(P.c, np.float64(th)) + P.u0), float(P.v0))


@functools.lru_cache(maxsize=None)
def points(name):
    """[N_POINTS, 2] pixels: the principal point exactly, a point with r < 1e-10, the four corners, for Kannala-Brandt a pixel just below and one
    just above th = pi / 2 (z <= 0) and one beyond the branch (r = 1.1 r_max: the fallback th = r), then points spread over the image.  The
    batch of n points is the first n."""
    model, params, W, H = models()[name]
    P = cm_ref.pack(model, params)
    pts = [(float(P.u0), float(P.v0)), (float(P.u0) + 1e-9, float(P.v0)), (0.0, 0.0), (W - 1.0, 0.0), (0.0, H - 1.0), (W - 1.0, H - 1.0)]
    if model == KB:
        th_hi = min(np.pi / 2 + 0.01, 0.5 * (np.pi / 2 + float(P.c[4]))) if P.flag else np.pi / 2 + 0.01
        pts += [_pixel_at_theta(P, np.pi / 2 - 0.01), _pixel_at_theta(P, th_hi)]
        if P.flag and 1.1 * P.r_max < BEYOND_LIMIT:
            pts.append((float(P.sx * (1.1 * P.r_max) + P.u0), float(P.v0)))
    rng = np.random.default_rng(77)
    rest = np.stack([rng.uniform(0, W - 1, N_POINTS), rng.uniform(0, H - 1, N_POINTS)], 1)
    rest[::7] = np.rint(rest[::7])                  # some on the pixel grid, as the detector and the extractor lift them
    return np.concatenate([np.array(pts), rest])[:N_POINTS]


@functools.lru_cache(maxsize=None)
def lifted(name):
    """cm_ref.lift of points(name) -> (ray, norm)."""
    model, params, _, _ = models()[name]
    return cm_ref.lift(model, params, points(name))


@functools.lru_cache(maxsize=None)
def lifted_hp(name):
    """The 60-digit rays of the first N_HP points -> (rows of mpf, deviates)."""
    model, params, _, _ = models()[name]
    return cm_ref.lift_hp(model, params, points(name)[:N_HP])


@functools.lru_cache(maxsize=None)
def grid(name, nx=9, ny=7):
    """A grid over the image rectangle of a fixture, its four corners and its principal point."""
    model, params, W, H = models()[name]
    P = cm_ref.pack(model, params)
    g = [(x, y) for y in np.linspace(0, H - 1, ny) for x in np.linspace(0, W - 1, nx)]
    return np.array(g + [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (float(P.u0), float(P.v0))], np.float64)


# ---- the bars of ld_cases through a fisheye
BAR_SCENE = "131x97"
# a Kannala-Brandt camera of the scene's size: mu = mv = 62 px / rad puts the corners (81 px from the centre) at th = 75 degrees, a diagonal
# field of view of 150 degrees; the coefficients are TUM-VI's.  The output pinhole keeps the principal point and takes fx = fy = 52: the output
# corners then look 57 degrees off the axis, inside the raw image
BAR_KB = (KB, (0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182, 62.0, 62.0, 65.3, 47.8))
BAR_OUT = (52.0, 52.0, 65.3, 47.8)
BAR_MEI = "black_box"       # the MEI map case: the fixture's own camera scaled to the scene's size (bar_mei_model)


def bar_mei_model():
    """black_box's camera for an image of the bar scene's size: the scales and the centre shrunk by 131 / 752."""
    model, p, W, _ = models()[BAR_MEI]
    s = 131.0 / W
    return model, p[:5] + tuple(v * s for v in p[5:])


@functools.lru_cache(maxsize=None)
def bar_scene():
    """-> dict: raw [H, W] uint8 = frame B of ld_cases.scene(BAR_SCENE) as the fisheye sees it (the bars rendered where every raw pixel's ray
    meets the output pinhole's image plane, then the scene's noise), model, out_cam, edges in pixels of the undistorted image, map = cm_ref's,
    near = its words within the Kannala-Brandt slack of a half-integer, undistorted = ud_ref's remap of raw through the map."""
    W, H, _, seed = ld_cases.SCENES[BAR_SCENE]
    model, params = BAR_KB
    b, level = ld_cases.bars(BAR_SCENE)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    ray, _ = cm_ref.lift(model, params, np.stack([u.ravel(), v.ravel()], 1))
    front = ray[:, 2] > 1e-6
    z = np.where(front, ray[:, 2], 1.0)
    x = np.where(front, BAR_OUT[0] * ray[:, 0] / z + BAR_OUT[2], -1e9).reshape(H, W)
    y = np.where(front, BAR_OUT[1] * ray[:, 1] / z + BAR_OUT[3], -1e9).reshape(H, W)
    canvas = np.full((H, W), ld_cases.BACKGROUND)
    for i in range(len(b)):
        canvas[ld_cases._inside(x, y, b[i])] = level[i]
    canvas += np.random.default_rng(2000 + seed).normal(0.0, ld_cases.SIGMA, canvas.shape)
    img = np.clip(np.rint(canvas), 0, 255).astype(np.uint8)
    m, near = cm_ref.build_map(model, params, W, H, BAR_OUT, slack=params[4] * KB_ALLOWANCE)
    return dict(raw=img, model=model, params=params, out_cam=BAR_OUT, W=W, H=H, edges=ld_cases.scene(BAR_SCENE)["edges_b"], map=m, near=near,
                undistorted=ud_ref.remap(img, m))


@functools.lru_cache(maxsize=None)
def bar_ref(which):
    """ld_ref.detect of the bar scene's 'undistorted' or 'raw' image with ld_cases' parameters."""
    P = ld_cases.PARAMS
    return ld_ref.detect(bar_scene()[which], P["grad_threshold"], P["min_pixels"], P["min_length"], ld_cases.MAX_LINES)
