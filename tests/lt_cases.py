"""The scenes and cases of the tests of uvs_lt_* (tests/test_line_track.py): small, deterministic.  A scene is a grey background with randomly
oriented filled bars, one long edge of each being the bar's segment, under Gaussian noise; it is rendered once on a larger canvas and cropped
twice, so that frame B is frame A shifted by a whole number of pixels, noise and all.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import lt_ref

# name: (width, height, bars, seed)
SCENES = {"96x80": (96, 80, 8, 1), "131x97": (131, 97, 12, 2), "376x240": (376, 240, 40, 3)}
SMALL = ("96x80", "131x97")
SHIFT = (4, 3)
MAX_LENGTH = 80            # of the handles of the tests: a bar's edge is at most 70 long, the LONG extra is 90
CAM = (461.6, 460.3, 363.0, 248.1)


def bars(name):
    """[n, 5]: centre x, y (in frame A), angle, half-length, width;  and the grey levels [n]."""
    W, H, n, seed = SCENES[name]
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 5)); level = np.zeros(n)
    for i in range(n):
        out[i] = [rng.uniform(10, W - 10), rng.uniform(10, H - 10), rng.uniform(0, np.pi), rng.uniform(12, 35), rng.uniform(6, 14)]
        level[i] = rng.uniform(0, 255)
    return out, level


@functools.lru_cache(maxsize=None)
def scene(name, shift=SHIFT):
    """-> dict: A, B [H, W] uint8, segs_a, segs_b [n, 4] (segs_b = segs_a + shift: line i of A is line i of B)."""
    W, H, n, seed = SCENES[name]
    sx, sy = shift
    b, level = bars(name)
    y, x = np.mgrid[0:H + sy, 0:W + sx].astype(np.float64)
    canvas = np.full((H + sy, W + sx), 100.0)
    segs = np.zeros((n, 4))
    for i in range(n):
        cx, cy, th, hl, wd = b[i]
        cx += sx; cy += sy                                   # frame A is the crop at (sx, sy) of the canvas
        c, s = np.cos(th), np.sin(th)
        u = (x - cx) * c + (y - cy) * s; v = -(x - cx) * s + (y - cy) * c
        canvas[(np.abs(u) <= hl) & (np.abs(v) <= wd / 2)] = level[i]
        ex, ey = cx - s * wd / 2, cy + c * wd / 2             # the middle of the edge at v = + wd / 2
        segs[i] = [ex - hl * c, ey - hl * s, ex + hl * c, ey + hl * s]
    canvas += np.random.default_rng(1000 + seed).normal(0.0, 3.0, canvas.shape)
    img = np.clip(np.rint(canvas), 0, 255).astype(np.uint8)
    a = np.ascontiguousarray(img[sy:, sx:]); bb = np.ascontiguousarray(img[:H, :W])
    return dict(A=a, B=bb, segs_a=segs - np.array([sx, sy, sx, sy], np.float64), segs_b=segs.copy(), W=W, H=H)


def extras(name):
    """Hand-placed segments for the paths the bars do not reach, by name."""
    W, H = SCENES[name][:2]
    return {
        "vertical": [40.25, 12.5, 40.25, 47.0],                   # sx == ex: the tie keeps the ends
        "swapped": [70.5, 20.0, 30.0, 41.75],                     # sx > ex: the ends are swapped
        "corner": [-9.5, 6.25, 14.0, -7.5],                       # crosses the image corner: most samples clamp
        "far_corner": [W - 12.0, H + 5.0, W + 9.5, H - 14.0],
        "short": [20.0, 30.0, 21.2, 30.9],                        # length 1.5: SHORT
        "zero": [20.0, 30.0, 20.0, 30.0],                         # length 0: SHORT, nothing is divided
        "seventy": [10.0, 60.0, 77.0, 39.75],                     # length 70: more samples than a wave has lanes
        "long": [3.0, 5.0, 90.0, 28.0],                           # length 90 > MAX_LENGTH: LONG
    }


@functools.lru_cache(maxsize=None)
def ref_frame(name, which, shift=SHIFT, variant=None):
    """lt_ref.describe of frame 'A' or 'B' of a scene (computed once, shared by the tests)."""
    sc = scene(name, shift)
    return lt_ref.describe(sc[which], sc["segs_" + which.lower()], MAX_LENGTH, variant)


@functools.lru_cache(maxsize=None)
def ref_pair(name, shift=SHIFT, variant=None):
    """(match_of_prev, distance, prev_of_cur) of A's lines (previous) against B's (current)."""
    a = ref_frame(name, "A", shift, variant); b = ref_frame(name, "B", shift, variant)
    return lt_ref.match(a["desc"], a["ends"], b["desc"], b["ends"], a["status"], b["status"])


def crafted_match():
    """Descriptors and gate points for the match rule's corners -> dict(prev_desc, prev_ends, prev_status, cur_desc, cur_ends, cur_status,
    match_of_prev, distance, prev_of_cur): the expectation is written by hand."""
    z = np.zeros(32, np.uint8)

    def d(*bits_set):
        v = z.copy()
        for b in bits_set:
            v[b // 8] |= 1 << (b % 8)
        return v
    cur_desc = np.array([d(0, 1), d(0, 1), d(100, 101, 102, 103), d(200), d(*range(40, 56)), z])
    cur_ends = np.array([[10, 10, 50, 10], [10, 10, 50, 10], [100, 100, 140, 100], [200, 50, 230, 50], [60, 60, 90, 90], [5, 5, 9, 9]], np.int32)
    cur_status = np.array([0, 0, 0, 0, 0, lt_ref.SHORT], np.int32)
    prev_desc = np.array([d(0), d(100, 101, 102), d(100, 101, 103), d(200), d(200), d(*range(40, 56)), z, d(0, 1, 2)])
    prev_ends = np.array([[10, 10, 50, 10],            # 0: distance 1 to both t = 0 and t = 1: the tie goes to t = 0
                          [100, 100, 140, 100],        # 1: t = 2 at distance 1
                          [100, 100, 140, 100],        # 2: t = 2 at distance 1 as well: prev_of_cur[2] is the larger q = 2
                          [218, 74, 230, 20],          # 3: t = 3, start gate 18^2 + 24^2 = 900 and end gate 30^2 = 900: both pass
                          [230, 51, 230, 50],          # 4: t = 3 at distance 0, start gate 30^2 + 1^2 = 901 fails
                          [60, 60, 90, 121],           # 5: t = 4 at distance 0, end gate 31^2 = 961 fails
                          [5, 5, 9, 9],                # 6: a SHORT previous line is no query (its zero descriptor would match t = 5's)
                          [10, 10, 50, 10]], np.int32)  # 7: distance 1 to t = 0 and t = 1 again: t = 0, and prev_of_cur[0] = 7
    prev_status = np.array([0, 0, 0, 0, 0, 0, lt_ref.SHORT, 0], np.int32)
    return dict(prev_desc=prev_desc, prev_ends=prev_ends, prev_status=prev_status, cur_desc=cur_desc, cur_ends=cur_ends, cur_status=cur_status,
                match_of_prev=np.array([0, 2, 2, 3, -1, -1, -1, 0], np.int32), distance=np.array([1, 1, 1, 0, 0, 0, -1, 1], np.int32),
                prev_of_cur=np.array([7, -1, 2, 3, -1, -1], np.int32))


@functools.lru_cache(maxsize=None)
def random_match(n_prev=1024, n_cur=1024, seed=11):
    """Random descriptors, a quarter of the previous lines near copies of current ones, gate points within and beyond the gate."""
    rng = np.random.default_rng(seed)
    cur_desc = rng.integers(0, 256, (n_cur, 32)).astype(np.uint8)
    cur_ends = rng.integers(0, 700, (n_cur, 4)).astype(np.int32)
    src = rng.integers(0, n_cur, n_prev)
    prev_desc = rng.integers(0, 256, (n_prev, 32)).astype(np.uint8)
    near = rng.random(n_prev) < 0.5
    flip = np.zeros((n_prev, 32), np.uint8)
    flip[np.arange(n_prev), rng.integers(0, 32, n_prev)] = 1 << rng.integers(0, 8, n_prev)
    prev_desc[near] = cur_desc[src[near]] ^ flip[near]
    prev_ends = (cur_ends[src] + rng.integers(-24, 25, (n_prev, 4))).astype(np.int32)
    return dict(prev_desc=prev_desc, prev_ends=prev_ends, cur_desc=cur_desc, cur_ends=cur_ends)
