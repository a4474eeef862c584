"""Inputs of the detection tests (tests/test_feature_detect.py): the constructed images with known answers, the rendered scenes of ft_cases with
occupied points, and fd_ref's result on each case, computed once and shared."""
import functools

import numpy as np

import fd_ref
import ft_cases as fc
import kf_cases

CAM = fc.CAM


def rectangle():
    img = np.full((40, 48), 50, np.uint8)
    img[10:30, 12:36] = 200
    return img


def edge_points(width, height):
    """Occupied points in each corner and on each edge (sub-pixel, so that rint matters): their discs are clipped by the image."""
    w, h = width - 1.0, height - 1.0
    return np.array([(0.0, 0.0), (w, 0.0), (0.0, h), (w, h), (width / 2 + 0.5, 0.25), (width / 3 - 0.5, h - 0.4), (0.49, height / 2 + 0.5),
                     (w - 0.51, height / 3 + 1.5)])


def image(name):
    """rect | cb1 | cb2 | lattice_WxH | texture_WxH | a scene of ft_cases (its first image)."""
    if name == "rect":
        return rectangle()
    if name == "cb1":
        return fc.checkerboard(48, 40, 1)
    if name == "cb2":
        return fc.checkerboard(48, 40, 2)
    kind, _, size = name.partition("_")
    if kind in ("lattice", "texture"):
        W, H = (int(v) for v in size.split("x"))
        return fc.fine_lattice(W, H) if kind == "lattice" else kf_cases.texture(90 + W, W, H, 20)
    return fc.scene(name)["prev"]


# name: (image, occupied, R, max_new, mask seed or None)
CASES = {
    "rect": ("rect", [], 8, 10, None),
    "rect_occupied": ("rect", [(12.4, 10.5)], 8, 10, None),
    "rect_two": ("rect", [], 8, 2, None),
    "rect_none_allowed": ("rect", [(24.0, 20.0)], 60, 10, None),
    "rect_R23": ("rect", [], 23, 10, None),
    "rect_R24": ("rect", [], 24, 10, None),
    "cb1": ("cb1", [], 5, 10, None),
    "cb2": ("cb2", [], 5, 40, None),
    "scene_48x40": ("shift_48x40_L1", "grid5", 10, 50, None),
    "scene_200x192": ("shift_200x192_L4", "grid5", 10, 50, None),
    "tiny_24x24": ("texture_24x24", "edges", 4, 16, None),
    "scene_131x97_edges_mask": ("shift_131x97_L3", "edges", 9, 60, 3),
    "lattice_131x97": ("lattice_131x97", "edges", 7, 256, None),
    "lattice_200x192": ("lattice_200x192", "edges", 3, 256, None),       # more than 8192 candidates: the ranking merges sorted chunks
    "wide_1030x192": ("texture_1030x192", "edges", 30, 100, 4),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(image, occupied [n, 2], R, max_new, mask or None)."""
    im, occ, R, max_new, mseed = CASES[name]
    img = image(im)
    H, W = img.shape
    if isinstance(occ, str):
        occ = fc.scene(im)["pts"][:5] if occ == "grid5" else edge_points(W, H)
    mask = None
    if mseed is not None:                                      # blocks of allowed and forbidden pixels, and a forbidden frame on two sides
        rng = np.random.default_rng(8000 + mseed)
        mask = np.kron(rng.integers(0, 3, ((H + 7) // 8, (W + 7) // 8)) > 0, np.ones((8, 8), bool))[:H, :W].astype(np.uint8) * 255
        mask[:3, :] = 0; mask[:, -2:] = 0
    return dict(image=img, occupied=np.asarray(occ, np.float64).reshape(-1, 2), R=R, max_new=max_new, mask=mask)


@functools.lru_cache(maxsize=None)
def ref(name, max_candidates=fd_ref.DEFAULT_CANDIDATES, with_mask=True, max_new=None):
    c = case(name)
    return fd_ref.detect(c["image"], CAM, c["occupied"], c["max_new"] if max_new is None else max_new, 0.01, c["R"], c["mask"] if with_mask else None,
                         max_candidates)
