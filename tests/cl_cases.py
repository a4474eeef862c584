"""The images and cases of the tests of uvs_ft_equalize (tests/test_feature_equalize.py): small, deterministic, each chosen for a path of the
rule in tests/cl_ref.py.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import cl_ref
import ft_cases


def noise(seed, width, height):
    """Uniform noise over all 256 levels."""
    return np.random.default_rng(9000 + seed).integers(0, 256, (height, width)).astype(np.uint8)


def low_contrast(seed, width, height):
    """A smooth texture squeezed into 120 .. 135: the frame CLAHE is for.  A tile's pixels fall into sixteen bins at most."""
    g = ft_cases.render(seed, width, height, noise=0.0).astype(np.float64)
    return np.clip(np.rint(120.0 + 15.0 * (g - g.min()) / (g.max() - g.min())), 0, 255).astype(np.uint8)


def checkerboard(width, height):
    """0 / 255 by the parity of x + y."""
    y, x = np.mgrid[0:height, 0:width]
    return (255 * ((x + y) & 1)).astype(np.uint8)


def constant(value, width, height):
    return np.full((height, width), value, np.uint8)


def grey_beside_noise(seed, width, height, tiles_x, tiles_y):
    """Uniform noise, except that the tile at (1, 1) of the padded grid is the single level 200: a histogram of one bin beside flat ones."""
    Wp, Hp, tw, th, _, _ = cl_ref.geometry(width, height, 3.0, tiles_x, tiles_y)
    img = noise(seed, width, height)
    img[th:2 * th, tw:2 * tw] = 200
    return img


# name: (width, height, tiles_x, tiles_y, clip_limit); the image is IMAGES[kind](seed, width, height) unless the case names its own
SHAPES = {
    "24x24_t8": (24, 24, 8, 8, 3.0),           # tile 3 x 3, N = 9, clip = max(0, 1) = 1
    "50x45_t8": (50, 45, 8, 8, 3.0),           # both dimensions padded: 56 x 48
    "48x45_t8": (48, 45, 8, 8, 3.0),           # the width divides and still gains 8 columns: 56 x 48
    "131x97_t16": (131, 97, 16, 16, 3.0),      # 144 x 112, tile 9 x 7
    "96x80_t1": (96, 80, 1, 1, 3.0),           # one tile: every pixel reads the one LUT four times
    "96x80_t8_clip0": (96, 80, 8, 8, 0.0),     # no clipping
    "96x80_t8_clip40": (96, 80, 8, 8, 40.0),   # tile 12 x 10, clip = 18
    "376x240_t8": (376, 240, 8, 8, 3.0),       # tile 47 x 30: an odd tile width, rows that are not dword-aligned
}
SHAPES_376_CLIP = 16


@functools.lru_cache(maxsize=None)
def image(kind, name):
    W, H, tx, ty, _ = SHAPES[name]
    seed = sorted(SHAPES).index(name)
    if kind == "noise":
        return noise(seed, W, H)
    if kind == "low_contrast":
        return low_contrast(seed, W, H)
    if kind == "checkerboard":
        return checkerboard(W, H)
    if kind == "zeros":
        return constant(0, W, H)
    if kind == "full":
        return constant(255, W, H)
    if kind == "grey_beside_noise":
        return grey_beside_noise(seed, W, H, tx, ty)
    raise KeyError(kind)


KINDS = ("noise", "low_contrast", "checkerboard", "zeros", "full", "grey_beside_noise")


@functools.lru_cache(maxsize=None)
def ref(kind, name):
    """cl_ref's result on a case (computed once, shared by the tests)."""
    _, _, tx, ty, clip = SHAPES[name]
    return cl_ref.equalize(image(kind, name), clip, tx, ty)


def raw(img):
    """A camera's dim frame of a rendered image: the contrast about 128 cut to a quarter.  Equalized, it has texture for the tracker again."""
    return np.clip(np.rint(100.0 + 0.25 * (img.astype(np.float64) - 128.0)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def raw_sequence():
    """ft_cases' three drifting frames (131 x 97) as raw frames."""
    return [raw(im) for im in ft_cases.sequence()]


@functools.lru_cache(maxsize=None)
def equalized_sequence(clip=3.0, tiles=8):
    return [cl_ref.equalize(im, clip, tiles, tiles)["out"] for im in raw_sequence()]


POINTS = ft_cases.grid_points(10, 131, 97)[25:]      # sub-pixel points, some near the borders (the tracker's host test uses the same)


@functools.lru_cache(maxsize=None)
def sequence_refs(equalized):
    """ft_ref's stateless replay A -> B -> C with three levels (computed once, shared by the tests): of the equalized raw frames, or of
    ft_cases' frames as they are."""
    return ft_cases.ref_sequence(equalized_sequence() if equalized else ft_cases.sequence(), POINTS, 3)
