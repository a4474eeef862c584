"""The scenes and crafted images of the tests of uvs_lt_detect (tests/test_line_detect.py): small, deterministic.  A scene is a grey
background with randomly oriented filled bars that keep clear of each other and of the border, under Gaussian noise; it is rendered once on a
larger canvas and cropped twice, as lt_cases.scene does, so that frame B is frame A shifted by a whole number of pixels, noise and all.
TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import ld_ref
import lt_cases

# name: (width, height, bars asked for, seed)
SCENES = {"96x80": (96, 80, 3, 21), "131x97": (131, 97, 5, 12), "376x240": (376, 240, 24, 13)}
SMALL = ("96x80", "131x97")
SHIFT = lt_cases.SHIFT
PARAMS = dict(grad_threshold=40, min_pixels=10, min_length=12.0)
MAX_LINES = 128            # of the handles of the tests; the OVERFLOW case takes 4
LONG = 24.0                # a "long" segment: both long edges of a bar are (a bar's long edge is at least 28)
BACKGROUND, INFLATE, CLEAR, SIGMA = 110.0, 6.0, 8.0, 3.0
TRIES = 400               # placements tried per scene: a small scene ends with fewer bars than it asked for


def _inside(x, y, bar, grow=0.0):
    cx, cy, th, hl, wd = bar
    c, s = np.cos(th), np.sin(th)
    u = (x - cx) * c + (y - cy) * s; v = -(x - cx) * s + (y - cy) * c
    return (np.abs(u) <= hl + grow) & (np.abs(v) <= wd / 2 + grow)


@functools.lru_cache(maxsize=None)
def bars(name):
    """[n, 5]: centre x, y (canvas coordinates = frame B's), angle, half-length, width;  and the grey levels [n].  Placed by rejection: the
    rectangles inflated by INFLATE do not overlap, and a centre keeps half-length + CLEAR from every border of both crops.  TRIES placements
    are tried; the scene has the bars that fitted, at most the number asked for."""
    W, H, n, seed = SCENES[name]
    sx, sy = SHIFT
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H + sy, 0:W + sx].astype(np.float64)
    taken = np.zeros(x.shape, bool)
    out, level = [], []
    for _ in range(TRIES):
        if len(out) == n:
            break
        hl = rng.uniform(14, 30); wd = rng.uniform(8, 14); th = rng.uniform(0, np.pi)
        lv = BACKGROUND + rng.choice([-1.0, 1.0]) * rng.uniform(60, 100)
        lo_x, hi_x, lo_y, hi_y = sx + hl + CLEAR, W - hl - CLEAR, sy + hl + CLEAR, H - hl - CLEAR
        if lo_x > hi_x or lo_y > hi_y:
            continue
        bar = (rng.uniform(lo_x, hi_x), rng.uniform(lo_y, hi_y), th, hl, wd)
        m = _inside(x, y, bar, INFLATE)
        if (m & taken).any():
            continue
        taken |= m
        out.append(bar); level.append(lv)
    assert len(out) >= 2, name
    return np.array(out), np.array(level)


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict: A, B [H, W] uint8; edges_a, edges_b [2 n, 4]: the two long edges of every bar in each frame's coordinates (edge 2 i and
    2 i + 1 belong to bar i); W, H."""
    W, H, _, seed = SCENES[name]
    sx, sy = SHIFT
    b, level = bars(name)
    n = len(b)
    y, x = np.mgrid[0:H + sy, 0:W + sx].astype(np.float64)
    canvas = np.full((H + sy, W + sx), BACKGROUND)
    edges = np.zeros((2 * n, 4))
    for i in range(n):
        cx, cy, th, hl, wd = b[i]
        c, s = np.cos(th), np.sin(th)
        canvas[_inside(x, y, b[i])] = level[i]
        for k, sgn in enumerate((1.0, -1.0)):
            ex, ey = cx - sgn * s * wd / 2, cy + sgn * c * wd / 2
            edges[2 * i + k] = [ex - hl * c, ey - hl * s, ex + hl * c, ey + hl * s]
    canvas += np.random.default_rng(1000 + seed).normal(0.0, SIGMA, canvas.shape)
    img = np.clip(np.rint(canvas), 0, 255).astype(np.uint8)
    a = np.ascontiguousarray(img[sy:, sx:]); bb = np.ascontiguousarray(img[:H, :W])
    return dict(A=a, B=bb, edges_a=edges - np.array([sx, sy, sx, sy], np.float64), edges_b=edges.copy(), W=W, H=H)


# piece lengths (rows) of the bent edges.  "bent_half": the A region of the first two pieces has n = 270 and s = 135, exactly 2 s == n, so it is
# no candidate;  "bent_voters": the A region of the first two pieces is a candidate with s = 94 of n = 186, so its fit is over non-voters too
BENT = {"bent_half": (26, 21, 20), "bent_voters": (18, 14, 14)}


def bent(l1, l2, l3, W=72):
    """A bright half-plane right of an edge x = g(y) of three straight pieces whose gradient directions are about -10, -30 and -50 degrees:
    sectors (A, B) = (7, 0), (7, 7), (6, 7).  Partition A joins the first two pieces, partition B the last two, and the vote between them
    depends on the pieces' pixel counts.  Anti-aliased by the coverage of each pixel, no noise."""
    y = np.arange(l1 + l2 + l3)
    g = np.where(y < l1, 0.176 * y, np.where(y < l1 + l2, 0.176 * l1 + 0.577 * (y - l1), 0.176 * l1 + 0.577 * l2 + 1.2 * (y - l1 - l2))) + 8.0
    cov = np.clip(np.arange(W)[None, :] - g[:, None] + 0.5, 0, 1)
    return np.rint(60 + 130 * cov).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def crafted(name):
    """The crafted images by name -> [H, W] uint8."""
    if name == "constant":
        return np.full((40, 72), 93, np.uint8)
    if name == "ramp":                          # gx = 8 x 6 > T, gy = 0 everywhere but near the left and right border, where reflect-101 flattens the ramp
        return np.ascontiguousarray(np.broadcast_to((10 + 6 * np.arange(41))[None, :], (30, 41)).astype(np.uint8))
    if name == "step_vertical":                 # gy == 0
        a = np.full((48, 80), 60, np.uint8); a[:, 37:] = 190
        return a
    if name == "step_horizontal":               # gx == 0
        a = np.full((48, 80), 60, np.uint8); a[29:, :] = 190
        return a
    if name == "step_diagonal":                 # gx == gy along a 45 degree edge
        y, x = np.mgrid[0:64, 0:64]
        return np.where(x + y >= 64, 190, 60).astype(np.uint8)
    if name == "step_antidiagonal":             # gx == -gy
        y, x = np.mgrid[0:64, 0:64]
        return np.where(x - y >= 0, 190, 60).astype(np.uint8)
    if name == "corner_to_corner":              # one edge across every tile row and column of the 376 x 240 image
        y, x = np.mgrid[0:240, 0:376]
        return np.where(240 * x - 376 * y >= 0, 200, 50).astype(np.uint8)
    if name in ("checkerboard", "checkerboard_strong"):      # 2 px squares: very many regions of at most 3 pixels;  at the higher contrast more
        y, x = np.mgrid[0:60, 0:90]                           # pixels have support, and the regions chain along the diagonals
        lo, hi = (60, 190) if name == "checkerboard" else (30, 220)
        return np.where(((x // 2) + (y // 2)) % 2 == 0, lo, hi).astype(np.uint8)
    if name in BENT:                            # one edge of three straight pieces, see bent()
        return bent(*BENT[name])
    raise KeyError(name)


CRAFTED = ("constant", "ramp", "step_vertical", "step_horizontal", "step_diagonal", "step_antidiagonal", "corner_to_corner", "checkerboard",
           "checkerboard_strong", "bent_half", "bent_voters")
CRAFTED_SMALL = tuple(c for c in CRAFTED if c != "corner_to_corner")


@functools.lru_cache(maxsize=None)
def ref(name, which="A", max_lines=MAX_LINES, variant=None):
    """ld_ref.detect of frame 'A' or 'B' of a scene, or of a crafted image (computed once, shared by the tests)."""
    img = scene(name)[which] if name in SCENES else crafted(name)
    return ld_ref.detect(img, PARAMS["grad_threshold"], PARAMS["min_pixels"], PARAMS["min_length"], max_lines, variant)


@functools.lru_cache(maxsize=None)
def ref_stages(name, which="A"):
    img = scene(name)[which] if name in SCENES else crafted(name)
    return ld_ref.stages(img, PARAMS["grad_threshold"], PARAMS["min_pixels"], PARAMS["min_length"])


def edge_report(seg, edge):
    """(perpendicular offset of the segment's ends from the edge's line: the larger one;  the part of the edge's length the segment's
    projection covers)."""
    e0, e1 = np.array(edge[:2]), np.array(edge[2:])
    L = np.linalg.norm(e1 - e0); u = (e1 - e0) / L; nrm = np.array([-u[1], u[0]])
    p0, p1 = np.array(seg[:2]), np.array(seg[2:])
    off = max(abs((p0 - e0) @ nrm), abs((p1 - e0) @ nrm))
    t0, t1 = sorted([(p0 - e0) @ u, (p1 - e0) @ u])
    return off, max(0.0, min(t1, L) - max(t0, 0.0)) / L
