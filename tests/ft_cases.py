"""Inputs of the feature-tracking tests (tests/test_feature_track.py): smooth textures rendered with a known shift, rotation and pixel noise,
the point sets, the constructed images that reach each exit of the tracker, and the stateless replay of a sequence through ft_ref.
Everything is generated from seeds with numpy alone."""
import functools

import numpy as np

import ft_ref
import kf_cases

CAM = kf_cases.CAM_DIST
PAD = 40                                   # the canvas reaches this far beyond the image on every side


@functools.lru_cache(maxsize=None)
def canvas(seed, width, height):
    """A smooth float texture of (height + 2 PAD, width + 2 PAD): two scales of filtered noise, 30 .. 225."""
    rng = np.random.default_rng(5000 + seed)
    shape = (height + 2 * PAD, width + 2 * PAD)
    a = kf_cases.gaussian_filter(rng.normal(0.0, 1.0, shape), 2.0) * 2.0 + kf_cases.gaussian_filter(rng.normal(0.0, 1.0, shape), 5.0) * 5.0
    return 30.0 + 195.0 * (a - a.min()) / (a.max() - a.min())


def motion(p, width, height, shift=(0.0, 0.0), rot_deg=0.0):
    """Where the point p [n, 2] of the first image is in the second: a rotation about the image centre, then the shift."""
    c = np.array([(width - 1) / 2.0, (height - 1) / 2.0])
    a = np.radians(rot_deg)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return (np.asarray(p, np.float64) - c) @ R.T + c + np.asarray(shift, np.float64)


def render(seed, width, height, shift=(0.0, 0.0), rot_deg=0.0, noise=1.5, noise_seed=0):
    """The canvas seen after `motion`: pixel x of the result shows the canvas at motion^-1(x), bilinearly, plus pixel noise."""
    tex = canvas(seed, width, height)
    v, u = np.mgrid[0:height, 0:width]
    x = np.stack([u.ravel(), v.ravel()], 1).astype(np.float64)
    c = np.array([(width - 1) / 2.0, (height - 1) / 2.0])
    a = np.radians(rot_deg)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    src = (x - np.asarray(shift, np.float64) - c) @ R + c + PAD         # R^T applied: row vectors times R
    i0 = np.clip(np.floor(src[:, 0]).astype(int), 0, tex.shape[1] - 2); j0 = np.clip(np.floor(src[:, 1]).astype(int), 0, tex.shape[0] - 2)
    fa = np.clip(src[:, 0] - i0, 0, 1); fb = np.clip(src[:, 1] - j0, 0, 1)
    g = (1 - fa) * (1 - fb) * tex[j0, i0] + fa * (1 - fb) * tex[j0, i0 + 1] + (1 - fa) * fb * tex[j0 + 1, i0] + fa * fb * tex[j0 + 1, i0 + 1]
    if noise > 0:
        g = g + np.random.default_rng(6000 + 17 * seed + noise_seed).normal(0.0, noise, g.shape)
    return np.clip(np.rint(g), 0, 255).astype(np.uint8).reshape(height, width)


def grid_points(seed, width, height, n_random=24):
    """Points of every kind: a coarse grid that includes the borders and the corners (integer positions), points within 10 px of each border at
    sub-pixel positions, and random sub-pixel points."""
    rng = np.random.default_rng(7000 + seed)
    xs = np.linspace(0, width - 1, 5).round(); ys = np.linspace(0, height - 1, 5).round()
    pts = [(x, y) for y in ys for x in xs]
    for t in (0.25, 3.5, 9.75):
        pts += [(t, height / 2 + t), (width - 1 - t, height / 3 + t), (width / 2 + t, t), (width / 3 - t, height - 1 - t),
                (t, t), (width - 1 - t, t), (t, height - 1 - t), (width - 1 - t, height - 1 - t)]
    pts += list(zip(rng.uniform(0, width - 1, n_random), rng.uniform(0, height - 1, n_random)))
    return np.array(pts, np.float64)


def interior_mask(pts, width, height, shift):
    """The issue's interior: at least 25 px plus the shift from each border."""
    mx, my = 25.0 + abs(shift[0]), 25.0 + abs(shift[1])
    return (pts[:, 0] >= mx) & (pts[:, 0] <= width - 1 - mx) & (pts[:, 1] >= my) & (pts[:, 1] <= height - 1 - my)


# name: (seed, width, height, levels, shift, rotation in degrees, noise sigma)
SCENES = {
    "shift_200x192_L4": (1, 200, 192, 4, (13.25, -7.5), 0.0, 1.5),
    "shift_131x97_L3": (2, 131, 97, 3, (5.5, 3.25), 0.0, 1.5),
    "shift_96x80_L2": (3, 96, 80, 2, (2.75, -1.5), 0.0, 1.5),
    "shift_96x80_L1": (4, 96, 80, 1, (1.25, 0.75), 0.0, 1.5),
    "shift_48x40_L1": (5, 48, 40, 1, (1.25, 0.75), 0.0, 1.5),
    "rot_200x192_L4": (6, 200, 192, 4, (4.5, 2.25), 3.0, 1.5),
    "rot_131x97_L3": (7, 131, 97, 3, (-2.5, 1.75), -2.0, 2.5),
}
SHIFT_SCENES = ("shift_200x192_L4", "shift_131x97_L3", "shift_96x80_L2", "shift_96x80_L1")       # the accuracy test's: each has interior points
BIG_SHIFT = "shift_200x192_L4"             # above 8 px: one level cannot follow it, four do


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict(prev, next, pts, truth, interior, levels, shift)."""
    seed, W, H, levels, shift, rot, noise = SCENES[name]
    prev = render(seed, W, H, noise=noise, noise_seed=1)
    nxt = render(seed, W, H, shift=shift, rot_deg=rot, noise=noise, noise_seed=2)
    pts = grid_points(seed, W, H)
    return dict(prev=prev, next=nxt, pts=pts, truth=motion(pts, W, H, shift, rot), interior=interior_mask(pts, W, H, shift), levels=levels,
                shift=shift, width=W, height=H)


@functools.lru_cache(maxsize=None)
def scene_ref(name, levels=None):
    """ft_ref's result on a scene (computed once, shared by the tests)."""
    s = scene(name)
    return ft_ref.track_images(s["prev"], s["next"], s["pts"], levels or s["levels"], CAM)


def checkerboard(width, height, cell=1):
    return kf_cases.checkerboard(width, height, cell)


def fine_lattice(width, height):
    """128 + 50 s(x) + 50 s(y) with s = 0, 1, 0, -1, ...: textured at level 0, and the {1, 4, 6, 4, 1} kernel sampled at the even pixels cancels s,
    so that level 1 is the constant 128 away from the borders."""
    s = np.array([0, 1, 0, -1])
    y, x = np.mgrid[0:height, 0:width]
    return (128 + 50 * s[x % 4] + 50 * s[y % 4]).astype(np.uint8)


def contrast(seed, width, height, gain, shift=(0.0, 0.0)):
    """A noise-free rendering whose contrast about 128 is scaled by `gain`."""
    g = render(seed, width, height, shift=shift, noise=0.0).astype(np.float64)
    return np.clip(np.rint(128.0 + gain * (g - 128.0)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def exits():
    """name -> dict(prev, next, levels, pts, status [n], iterations [n]): images constructed so that each exit of the tracker is taken.
    The expected values are asserted against ft_ref by the CPU tests and against the device by the GPU tests."""
    T, F, O, B = ft_ref.TRACKED, ft_ref.LOST_FLAT, ft_ref.LOST_OUTSIDE, ft_ref.LOST_BORDER
    c = {}
    flat = np.full((48, 48), 93, np.uint8)
    c["flat"] = dict(prev=flat, next=flat, levels=2, pts=[(24.0, 24.0), (5.5, 40.25)], status=[F, F], iterations=[0, 0])
    lat = fine_lattice(64, 64)
    c["flat_level_skipped"] = dict(prev=lat, next=np.roll(lat, 1, axis=1), levels=2, pts=[(32.0, 32.0)], status=[T], iterations=[2])
    still = render(8, 48, 40, noise=0.0)
    c["border"] = dict(prev=still, next=still, levels=1, pts=[(0.3, 20.0), (0.7, 20.0), (47 - 0.3, 20.0), (47 - 0.7, 20.0), (20.0, 0.25), (20.0, 39 - 0.25)],
                       status=[B, T, B, T, B, B], iterations=[1] * 6)
    a = render(9, 48, 40, noise=0.0); b = render(9, 48, 40, shift=(-6.0, 0.0), noise=0.0)
    c["runs_off"] = dict(prev=a, next=b, levels=1, pts=[(3.0, 20.0)], status=[O], iterations=[3])
    # the second image has TWICE the contrast of the first: the step, which divides by the first image's gradients, overshoots by a factor of two,
    # so that the steps alternate in sign -- the oscillation stop takes half of the last one back, or the alternation goes on for 30 iterations
    lo = contrast(11, 64, 56, 0.25)
    c["oscillation"] = dict(prev=lo, next=contrast(11, 64, 56, 0.5, (0.25, 0.0)), levels=1, pts=[(32.0, 28.0)], status=[T], iterations=[2])
    c["thirty"] = dict(prev=lo, next=contrast(11, 64, 56, 0.5, (0.5, 0.25)), levels=1, pts=[(32.0, 28.0)], status=[T], iterations=[30])
    c["eps_stop"] = dict(prev=render(9, 48, 40, noise=0.0), next=render(9, 48, 40, shift=(1.25, 0.75), noise=0.0), levels=1, pts=[(24.5, 20.25)],
                         status=[T], iterations=[3])
    c["outside_start"] = dict(prev=a, next=b, levels=1, pts=[(-0.5, 20.0), (20.0, 39.5), (48.0, 3.0)], status=[O, O, O], iterations=[0, 0, 0])
    return c


def ref_sequence(images, pts, levels, cam=CAM):
    """The stateless replay of images[0] -> images[1] -> ...: every step tracks the points the step before it TRACKED.  -> [result of
    ft_ref.track_images per step]."""
    out = []
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    for a, b in zip(images[:-1], images[1:]):
        r = ft_ref.track_images(a, b, pts, levels, cam)
        out.append(r)
        pts = r["next_xy"][r["status"] == ft_ref.TRACKED]
    return out


@functools.lru_cache(maxsize=None)
def sequence(width=131, height=97):
    """Three frames of one canvas, the camera drifting and turning a little: [image]."""
    return [render(10, width, height, shift=s, rot_deg=r, noise=1.5, noise_seed=k) for k, (s, r) in enumerate((((0.0, 0.0), 0.0), ((3.25, -1.5), 0.5), ((6.0, -2.25), 1.0)))]
