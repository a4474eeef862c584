"""Equalization of the front ends' images (uvs_ft_set_equalize, uvs_ft_equalize; csrc/uvs_feature_equalize.hip): CLAHE as the reference's readImage
runs it (feature_tracker.cpp:60-66), pinned to tests/cl_ref.py bit for bit.  OpenCV is not a dependency and could not be compared; what pins the
rule is the header's statement, the two forms of it in cl_ref (vectorized against plain loops), hand cases, invariants and planted defects.

CPU: the restatement against itself, the hand cases, the invariants, the defects, the header against abi.py, the host mirror's bookkeeping of the
setting.  GPU: uvs_ft_debug_equalize value by value, uvs_ft_equalize in batches, uvs_ft_track with an equalized slot (pyramid, tracks, detection,
mixed batches, reset, the untouched plain path), the argument checks, and uvs::FeatureTracker::readImage with equalize = true."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cl_cases as cc
import cl_ref
import fd_ref
import ft_cases as fc
import ft_ref
from helpers import abi, uvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQ_SYMBOLS = ["uvs_ft_set_equalize", "uvs_ft_equalize", "uvs_ft_last_equalize_device_ms", "uvs_ft_debug_equalize"]
HOST_SYMBOLS = ["uvs_host_ft_set_equalize", "uvs_host_ft_equalize_pending", "uvs_host_ft_equalize_told", "uvs_host_ft_reset"]
CAM = fc.CAM
LOOP_SHAPES = [n for n in sorted(cc.SHAPES) if n != "376x240_t8"]      # the per-pixel Python loops stay below 13 000 pixels


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want, what=""):
    for k in ("info", "bins", "luts", "out"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


# ================================================================ CPU: the restatement
@pytest.mark.parametrize("name", LOOP_SHAPES)
@pytest.mark.parametrize("kind", ["noise", "low_contrast"])
def test_vectorized_form_equals_loop_form(name, kind):
    W, H, tx, ty, clip = cc.SHAPES[name]
    img = cc.image(kind, name)
    _same(cc.ref(kind, name), cl_ref.equalize_loops(img, clip, tx, ty), name)


def test_geometry_of_the_cases():
    g = {n: cl_ref.geometry(*cc.SHAPES[n][:2], cc.SHAPES[n][4], *cc.SHAPES[n][2:4]) for n in cc.SHAPES}
    assert g["24x24_t8"] == (24, 24, 3, 3, 9, 1)                # 3.0 * 9 / 256 truncates to 0 and is raised to 1
    assert g["50x45_t8"] == (56, 48, 7, 6, 42, 1)
    assert g["48x45_t8"] == (56, 48, 7, 6, 42, 1)               # 48 divides by 8 and still gains 8 columns
    assert g["131x97_t16"] == (144, 112, 9, 7, 63, 1)
    assert g["96x80_t1"] == (96, 80, 96, 80, 7680, 90)
    assert g["96x80_t8_clip0"][4:] == (120, 0) and g["96x80_t8_clip40"][4:] == (120, 18)
    assert g["376x240_t8"] == (376, 240, 47, 30, 1410, cc.SHAPES_376_CLIP)
    assert cl_ref.geometry(752, 480, 3.0, 8, 8) == (752, 480, 94, 60, 5640, 66)


def test_hand_cases():
    # the constant 77 on 48 x 48: tile 6 x 6, clip = 1, 35 clipped, batch 0, residual 35, step 7: bins 0, 7, .., 238 gain one, bin 77 = 7 * 11 among
    # them beside the one it keeps; the sum up to 77 is 1 + 12 = 13 (the steps 0, 7, .., 77 are twelve), and rint(13 * 255 / 36) = rint(92.08) = 92
    r = cl_ref.equalize(cc.constant(77, 48, 48), 3.0, 8, 8)
    assert r["info"].tolist() == [48, 48, 36, 1]
    want = np.zeros(256, np.int32); want[0:245:7] = 1; want[77] += 1
    assert np.array_equal(r["bins"][3, 4], want) and want.sum() == 36 and want[77] == 2
    assert int(r["luts"][0, 0, 77]) == 92 and np.all(r["out"] == 92)
    # all 0: bin 0 holds the clip, so every sum is at least 1 + 1 (its step) and level 0 maps to rint(2 * 255 / 36) = 14
    r0 = cl_ref.equalize(cc.constant(0, 48, 48), 3.0, 8, 8)
    assert np.all(r0["out"] == 14) and r0["bins"][0, 0, 0] == 2
    # all 255: whatever happens below, the sum at 255 is N
    r255 = cl_ref.equalize(cc.constant(255, 48, 48), 3.0, 8, 8)
    assert np.all(r255["out"] == 255)
    # the 0 / 255 checkerboard with clip 0: half the pixels at 0 -> rint(127.5) = 128 (half to even), the others 255
    cb = cc.checkerboard(48, 48)
    rc = cl_ref.equalize(cb, 0.0, 8, 8)
    assert np.array_equal(rc["out"], np.where(cb == 0, 128, 255))
    # ... and with clip 1 both bins are cut to 1 and 34 are handed back, step 7: bins 0 .. 231; level 0 -> rint(2 * 255 / 36) = 14
    rc1 = cl_ref.equalize(cb, 3.0, 8, 8)
    assert np.array_equal(rc1["out"], np.where(cb == 0, 14, 255))


@pytest.mark.parametrize("name", sorted(cc.SHAPES))
@pytest.mark.parametrize("kind", cc.KINDS)
def test_invariants(name, kind):
    r = cc.ref(kind, name)
    assert np.all(r["bins"].sum(axis=2) == r["info"][2]) and r["bins"].min() >= 0
    assert np.all(np.diff(r["luts"].astype(np.int64), axis=2) >= 0) and np.all(r["luts"][:, :, 255] == 255)
    assert r["out"].shape == cc.image(kind, name).shape


@pytest.mark.parametrize("kind", ["noise", "low_contrast", "checkerboard"])
def test_clip_0_with_one_tile_is_plain_histogram_equalization(kind):
    img = cc.image(kind, "96x80_t1")
    r = cl_ref.equalize(img, 0.0, 1, 1)
    want, lut = cl_ref.plain_equalization(img)
    assert np.array_equal(r["luts"][0, 0], lut) and np.array_equal(r["out"], want)


@pytest.mark.parametrize("defect", cl_ref.DEFECTS)
def test_each_planted_defect_changes_an_output(defect):
    changed = []
    for name in sorted(cc.SHAPES):
        W, H, tx, ty, clip = cc.SHAPES[name]
        for kind in ("noise", "low_contrast"):
            bad = cl_ref.equalize(cc.image(kind, name), clip, tx, ty, defect=defect)["out"]
            if not np.array_equal(bad, cc.ref(kind, name)["out"]):
                changed.append((name, kind))
    assert changed, defect
    if defect == "no_full_tile_padding":       # only the case whose width divides and is padded all the same can tell
        assert {n for n, _ in changed} == {"48x45_t8"}


# ================================================================ CPU: layout, symbols, the host mirror's setting
def test_eq_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "uvs_solver.h")).read()
    for s in EQ_SYMBOLS:
        assert s + "(" in hdr, s
        assert s in uvs.api.EXPORTS, s
    assert "#define UVS_ABI_VERSION 7" in hdr
    L = uvs.api.lib()
    for s in EQ_SYMBOLS:
        assert hasattr(L, s), s
    assert L.uvs_abi_version() == 7
    Hst = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
    for s in HOST_SYMBOLS:
        assert hasattr(Hst, s), s


def test_eq_struct_layout_matches_header():
    code = r'''
#include <stdio.h>
#include <stddef.h>
#include "uvs_solver.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(uvs_ft_image), offsetof(uvs_ft_image, image), offsetof(uvs_ft_image, width), offsetof(uvs_ft_image, height));
  printf("%d %d\n", UVS_FT_CLAHE_MAX_TILES, UVS_FT_MIN_SIZE);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c"); exe = os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    F = abi.FtImage
    assert out[:4] == [C.sizeof(F), F.image.offset, F.width.offset, F.height.offset]
    assert out[4:] == [abi.FT_CLAHE_MAX_TILES, abi.FT_MIN_SIZE] and cl_ref.MAX_TILES == abi.FT_CLAHE_MAX_TILES
    arr, keep = abi.ft_images([np.zeros((30, 40), np.uint8)])
    assert (arr[0].width, arr[0].height) == (40, 30)


class HostTracker:
    """ctypes face of uvs::FeatureTracker behind feature_tracker_capi.cpp with the calls of the equalization; device < 0: the bookkeeping alone."""

    def __init__(self, device, cam=CAM, max_width=752, max_height=480, levels=4, max_points=1024):
        L = self.L = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
        L.uvs_host_ft_create.restype = C.c_void_p
        L.uvs_host_ft_create.argtypes = [C.c_int, abi.c_double_p] + [C.c_int] * 4
        L.uvs_host_ft_destroy.argtypes = [C.c_void_p]; L.uvs_host_ft_destroy.restype = None
        L.uvs_host_ft_read_image.argtypes = [C.c_void_p, abi.c_u8_p, C.c_int, C.c_int, C.c_double, C.c_int, abi.c_double_p]
        L.uvs_host_ft_update_ids.argtypes = [C.c_void_p]
        L.uvs_host_ft_get.argtypes = [C.c_void_p, C.c_int, abi.c_double_p, abi.c_i32_p, abi.c_i32_p, abi.c_double_p, abi.c_double_p]
        L.uvs_host_ft_set_equalize.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int]
        L.uvs_host_ft_equalize_pending.argtypes = [C.c_void_p]
        L.uvs_host_ft_equalize_told.argtypes = [C.c_void_p, C.c_int]
        L.uvs_host_ft_reset.argtypes = [C.c_void_p]
        c = np.array(list(cam) + [0.0] * (8 - len(cam)))
        self.h = L.uvs_host_ft_create(device, abi._dp(c), max_width, max_height, levels, max_points)
        assert self.h, "uvs_host_ft_create"

    def close(self):
        self.L.uvs_host_ft_destroy(self.h); self.h = None

    def read_image(self, img, time, new=()):
        img = np.ascontiguousarray(img, np.uint8); new = np.ascontiguousarray(new, np.float64).reshape(-1, 2)
        return self.L.uvs_host_ft_read_image(self.h, img.ctypes.data_as(abi.c_u8_p), img.shape[1], img.shape[0], time, len(new), abi._dp(new) if len(new) else None)

    def set_equalize(self, on, clip=3.0, tiles=8):
        return self.L.uvs_host_ft_set_equalize(self.h, int(on), clip, tiles)

    def pending(self):
        return self.L.uvs_host_ft_equalize_pending(self.h)

    def told(self, told):
        return self.L.uvs_host_ft_equalize_told(self.h, int(told))

    def reset(self):
        return self.L.uvs_host_ft_reset(self.h)

    def update_ids(self):
        return self.L.uvs_host_ft_update_ids(self.h)

    def get(self):
        n = self.L.uvs_host_ft_get(self.h, 0, None, None, None, None, None)
        o = dict(cur_pts=np.zeros((n, 2)), ids=np.zeros(n, np.int32), track_cnt=np.zeros(n, np.int32), cur_un_pts=np.zeros((n, 2)), pts_velocity=np.zeros((n, 2)))
        if n:
            self.L.uvs_host_ft_get(self.h, n, abi._dp(o["cur_pts"]), o["ids"].ctypes.data_as(abi.c_i32_p), o["track_cnt"].ctypes.data_as(abi.c_i32_p),
                                   abi._dp(o["cur_un_pts"]), abi._dp(o["pts_velocity"]))
        return o


def test_host_mirror_sends_the_setting_when_it_changed_or_after_a_reset():
    """The bookkeeping of the setting fed by hand (no device is touched): what readImage asks before a frame."""
    t = HostTracker(-1)
    assert t.pending() == 0                                  # a fresh slot is plain, and so is the setting
    assert t.set_equalize(True) == 0 and t.pending() == 1
    assert t.told(True) == 0 and t.pending() == 0            # sent once, not with every frame
    assert t.set_equalize(True, clip=3.0, tiles=8) == 0 and t.pending() == 0
    t.set_equalize(True, clip=2.0); assert t.pending() == 1  # the clip limit changed
    t.told(True); assert t.pending() == 0
    t.set_equalize(True, clip=2.0, tiles=4); assert t.pending() == 1
    t.told(True)
    t.told(False); assert t.pending() == 1                   # the slot was reset: it is plain again, the setting is not
    t.told(True)
    t.set_equalize(False, clip=9.0, tiles=2); assert t.pending() == 1      # switched off: sent ...
    t.told(True)
    t.set_equalize(False, clip=1.0, tiles=3); assert t.pending() == 0      # ... and the parameters of an equalization that is off do not matter
    t.told(False); assert t.pending() == 0                   # reset while off: nothing to send
    assert t.reset() != 0                                    # a handle without a device has no slot to reset
    t.close()


# ================================================================ GPU
def _tracker(**kw):
    kw.setdefault("max_width", 400); kw.setdefault("max_height", 256); kw.setdefault("max_streams", 4); kw.setdefault("max_points", 256)
    kw.setdefault("levels", 1)
    return uvs.api.FeatureTracker(**kw)


@pytest.fixture(scope="module")
def eq_tracker():
    ft = _tracker()
    yield ft
    ft.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(cc.SHAPES))
@pytest.mark.parametrize("kind", cc.KINDS)
def test_gpu_debug_equalize_equals_the_restatement_value_by_value(eq_tracker, name, kind):
    W, H, tx, ty, clip = cc.SHAPES[name]
    got = eq_tracker.debug_equalize(cc.image(kind, name), clip, tx, ty)
    _same(got, cc.ref(kind, name), (name, kind))


@pytest.mark.gpu
def test_gpu_hand_cases(eq_tracker):
    assert np.all(eq_tracker.equalize([cc.constant(77, 48, 48)])[0] == 92)
    cb = cc.checkerboard(48, 48)
    assert np.array_equal(eq_tracker.equalize([cb], clip_limit=0.0)[0], np.where(cb == 0, 128, 255))
    img = cc.image("noise", "96x80_t1")
    assert np.array_equal(eq_tracker.equalize([img], 0.0, 1, 1)[0], cl_ref.plain_equalization(img)[0])


@pytest.mark.gpu
def test_gpu_a_batch_of_four_sizes_equals_one_at_a_time_and_a_second_run(eq_tracker):
    names = ["50x45_t8", "376x240_t8", "24x24_t8", "131x97_t16"]
    imgs = [cc.image("low_contrast", names[0]), cc.image("noise", names[1]), cc.image("grey_beside_noise", names[2]), cc.image("noise", names[3])]
    batch = eq_tracker.equalize(imgs, 3.0, 8, 8)
    assert eq_tracker.last_equalize_device_ms() > 0.0
    solo = _tracker(max_streams=1)
    for k, im in enumerate(imgs):
        want = cl_ref.equalize(im, 3.0, 8, 8)["out"]
        assert np.array_equal(batch[k], want), names[k]
        assert np.array_equal(solo.equalize([im], 3.0, 8, 8)[0], want), names[k]
    solo.close()
    again = eq_tracker.equalize(imgs, 3.0, 8, 8)
    for k in range(4):
        assert np.array_equal(again[k], batch[k]), names[k]
    # tiles_x != tiles_y
    im = imgs[0]
    assert np.array_equal(eq_tracker.equalize([im], 2.0, 5, 3)[0], cl_ref.equalize(im, 2.0, 5, 3)["out"])


def _assert_tracks(got, want, what=""):
    assert np.array_equal(got["status"], want["status"]), (what, got["status"], want["status"])
    assert np.array_equal(got["iterations"], want["iterations"]), what
    assert np.array_equal(bits(got["next_xy"]), bits(want["next_xy"])), what
    assert np.array_equal(bits(got["next_norm"]), bits(want["next_norm"])), what
    assert got["n_tracked"] == want["n_tracked"], what


@pytest.mark.gpu
def test_gpu_an_equalized_slot_holds_the_equalized_pyramid_and_tracks_and_detects_in_it():
    raw = cc.raw_sequence(); eq = cc.equalized_sequence()
    pts = cc.POINTS
    ft = _tracker(levels=3, max_width=131, max_height=97, max_streams=2)
    ft.set_equalize(1, 3.0, 8)
    a = ft.track([dict(stream=1, image=raw[0])], CAM)[0]
    assert a["n_tracked"] == 0
    pyr = ft.debug_pyramid(1)
    want = ft_ref.pyramid(eq[0], 3)
    assert np.array_equal(pyr[0], eq[0]) and not np.array_equal(pyr[0], raw[0])
    for l in range(3):
        assert np.array_equal(pyr[l], want[l]), l
    seq = cc.sequence_refs(True)                                              # A -> B -> C on the equalized images
    b = ft.track([dict(stream=1, image=raw[1], points=pts)], CAM)[0]
    _assert_tracks(b, seq[0], "A -> B")
    assert 20 < b["n_tracked"] < len(pts)
    kept = b["next_xy"][b["status"] == 0]
    c = ft.track([dict(stream=1, image=raw[2], points=kept)], CAM)[0]
    _assert_tracks(c, seq[1], "B -> C")
    occ = c["next_xy"][c["status"] == 0]
    d = ft.detect([dict(stream=1, occupied=occ, max_new=40)], CAM, quality_level=0.01, min_distance=8)[0]
    ref = fd_ref.detect(eq[2], CAM, occ, 40, 0.01, 8)
    assert d["n_new"] == ref["n_new"] > 0 and d["n_candidates"] == ref["n_candidates"] and np.array_equal(d["xy"], ref["xy"])
    assert np.array_equal(bits(d["score"]), bits(ref["score"])) and d["max_score"] == ref["max_score"] and d["threshold"] == ref["threshold"]
    assert not np.array_equal(d["xy"], fd_ref.detect(raw[2], CAM, occ, 40, 0.01, 8)["xy"])       # the raw image would have given other points
    # uvs_ft_debug_point goes the same way
    ft.reset(0); ft.set_equalize(0, 3.0, 8)
    ft.track([dict(stream=0, image=raw[0])], CAM)
    one = ft.debug_point(dict(stream=0, image=raw[1], points=pts[40:41]), CAM)
    trace = []
    x, y, st, it = ft_ref.track_point(ft_ref.pyramid(eq[0], 3), ft_ref.pyramid(eq[1], 3), *pts[40], trace=trace)
    assert int(one["status"][0]) == st and int(one["iterations"][0]) == it and np.array_equal(bits(one["next_xy"][0]), bits([x, y]))
    assert np.array_equal(bits(one["trace"]), bits(ft_ref.trace_array(trace, 3)))
    ft.close()


@pytest.mark.gpu
def test_gpu_a_mixed_batch_gives_each_slot_what_it_gives_alone_and_reset_makes_a_slot_plain():
    raw = cc.raw_sequence(); eq = cc.equalized_sequence()
    plain_imgs = fc.sequence()
    pts = cc.POINTS
    ft = _tracker(levels=3, max_width=131, max_height=97, max_streams=2)
    ft.set_equalize(0, 3.0, 8)                                                # slot 0 equalized, slot 1 plain
    ft.track([dict(stream=0, image=raw[0]), dict(stream=1, image=plain_imgs[0])], CAM)
    got = ft.track([dict(stream=0, image=raw[1], points=pts), dict(stream=1, image=plain_imgs[1], points=pts)], CAM)
    _assert_tracks(got[0], cc.sequence_refs(True)[0], "the equalized slot")
    _assert_tracks(got[1], cc.sequence_refs(False)[0], "the plain slot")
    assert np.array_equal(ft.debug_pyramid(0)[0], eq[1]) and np.array_equal(ft.debug_pyramid(1)[0], plain_imgs[1])
    # the items in the other order, the equalized one last
    ft.reset(0); ft.reset(1); ft.set_equalize(0, 3.0, 8)
    ft.track([dict(stream=1, image=plain_imgs[0]), dict(stream=0, image=raw[0])], CAM)
    got = ft.track([dict(stream=1, image=plain_imgs[1], points=pts), dict(stream=0, image=raw[1], points=pts)], CAM)
    _assert_tracks(got[1], cc.sequence_refs(True)[0], "the equalized slot, second")
    _assert_tracks(got[0], cc.sequence_refs(False)[0], "the plain slot, first")
    # after uvs_ft_reset the slot is plain again: the raw image is stored as it is
    ft.reset(0)
    ft.track([dict(stream=0, image=raw[0])], CAM)
    assert np.array_equal(ft.debug_pyramid(0)[0], raw[0])
    # switched on, then off by tiles_x = 0
    ft.set_equalize(0, 3.0, 8); ft.set_equalize(0, 3.0, 0)
    ft.track([dict(stream=0, image=raw[1])], CAM)
    assert np.array_equal(ft.debug_pyramid(0)[0], raw[1])
    # other parameters per slot in one call
    ft.reset(0); ft.reset(1); ft.set_equalize(0, 2.0, 4, 6); ft.set_equalize(1, 40.0, 16)
    ft.track([dict(stream=0, image=raw[0]), dict(stream=1, image=raw[2])], CAM)
    assert np.array_equal(ft.debug_pyramid(0)[0], cl_ref.equalize(raw[0], 2.0, 4, 6)["out"])
    assert np.array_equal(ft.debug_pyramid(1)[0], cl_ref.equalize(raw[2], 40.0, 16, 16)["out"])
    ft.close()


@pytest.mark.gpu
def test_gpu_a_handle_that_never_equalizes_tracks_as_before():
    name = "shift_131x97_L3"
    s = fc.scene(name)
    ft = _tracker(levels=3, max_width=131, max_height=97, max_streams=1)
    ft.track([dict(stream=0, image=s["prev"])], CAM)
    got = ft.track([dict(stream=0, image=s["next"], points=s["pts"])], CAM)[0]
    _assert_tracks(got, fc.scene_ref(name), name)
    ft.close()


@pytest.mark.gpu
def test_gpu_argument_checks_leave_the_handle_usable():
    INV, CAP = abi.UVS_ERR_INVALID_ARG, abi.UVS_ERR_CAPACITY
    img = cc.image("noise", "50x45_t8")
    want = cl_ref.equalize(img, 3.0, 8, 8)["out"]
    ft = _tracker(levels=1, max_width=100, max_height=90, max_streams=2)
    L = uvs.api.lib()
    assert L.uvs_ft_set_equalize(None, 0, 3.0, 8, 8) == INV and L.uvs_ft_equalize(None, 1, None, 3.0, 8, 8, None) == INV
    assert L.uvs_ft_last_equalize_device_ms(None) == 0.0
    bad_settings = [(np.nan, 8, 8), (np.inf, 8, 8), (-0.5, 8, 8), (256.5, 8, 8), (3.0, 17, 8), (3.0, 8, 17), (3.0, -1, 8), (3.0, 8, 0), (3.0, 8, -2)]
    for stream in (-1, 2):
        assert ft.set_equalize_raw(stream, 3.0, 8, 8) == INV and ft.last_error()
        assert ft.set_equalize_raw(stream, 3.0, 0, 0) == INV                  # also when it would switch off
    for clip, tx, ty in bad_settings:
        assert ft.set_equalize_raw(0, clip, tx, ty) == INV and ft.last_error(), (clip, tx, ty)
        assert ft.equalize_raw([img], clip, tx, ty)[0] == INV and ft.last_error(), (clip, tx, ty)
    assert ft.equalize_raw([img], 3.0, 0, 8)[0] == INV                         # 0 tiles switch a slot off, they equalize nothing
    # no rejected uvs_ft_set_equalize switched slot 0 on
    ft.track([dict(stream=0, image=img)], CAM)
    assert np.array_equal(ft.debug_pyramid(0)[0], img)
    for clip, tx, ty in ((0.0, 1, 1), (256.0, 16, 16)):                       # the ends of the ranges are inside
        assert ft.set_equalize_raw(1, clip, tx, ty) == 0
    bad = [
        (dict(images=[img], null=("images",)), INV), (dict(images=[img], null=("out",)), INV), (dict(images=[img], n_images=0), INV),
        (dict(images=[img], n_images=-1), INV),
        (dict(images=[img[:23, :]]), INV), (dict(images=[img[:, :23]]), INV), (dict(images=[img, img[:20, :20]]), INV),
        (dict(images=[np.zeros((90, 101), np.uint8)]), CAP), (dict(images=[np.zeros((91, 100), np.uint8)]), CAP),
        (dict(images=[img, img, img]), CAP),                                  # more images than slots
    ]
    for kw, rc_want in bad:
        images = kw.pop("images")
        rc, out = ft.equalize_raw(images, 3.0, 8, 8, **kw)
        assert rc == rc_want and out == [] and ft.last_error(), (kw, rc, ft.last_error())
        rc, out = ft.equalize_raw([img], 3.0, 8, 8)                           # the handle still works after each
        assert rc == 0 and np.array_equal(out[0], want)
    arr, keep = abi.ft_images([img])
    null_image = abi.FtImage(None, 50, 45)
    assert L.uvs_ft_equalize(ft._h, 1, C.byref(null_image), 3.0, 8, 8, np.zeros(50 * 45, np.uint8).ctypes.data_as(abi.c_u8_p)) == INV
    b = np.zeros((64, 256), np.int32); l = np.zeros((64, 256), np.uint8); o = np.zeros(img.shape, np.uint8); info = np.zeros(4, np.int32)
    P = lambda a, t: a.ctypes.data_as(t)
    for args in ((None, P(b, abi.c_i32_p), P(l, abi.c_u8_p), P(o, abi.c_u8_p), P(info, abi.c_i32_p)),
                 (arr, None, P(l, abi.c_u8_p), P(o, abi.c_u8_p), P(info, abi.c_i32_p)),
                 (arr, P(b, abi.c_i32_p), None, P(o, abi.c_u8_p), P(info, abi.c_i32_p)),
                 (arr, P(b, abi.c_i32_p), P(l, abi.c_u8_p), None, P(info, abi.c_i32_p)),
                 (arr, P(b, abi.c_i32_p), P(l, abi.c_u8_p), P(o, abi.c_u8_p), None)):
        assert L.uvs_ft_debug_equalize(ft._h, args[0], 3.0, 8, 8, *args[1:]) == INV
    with pytest.raises(RuntimeError):
        ft.debug_equalize(img, 3.0, 17)
    with pytest.raises(RuntimeError):
        ft.set_equalize(0, 300.0)
    # the smallest and the largest image the handle takes, and the slot state is as it was: slot 0 plain, slot 1 equalized 16 x 16 at clip 256
    small = cc.noise(3, 24, 24); large = cc.noise(4, 100, 90)
    out = ft.equalize([small, large], 3.0, 8)
    assert np.array_equal(out[0], cl_ref.equalize(small, 3.0, 8, 8)["out"]) and np.array_equal(out[1], cl_ref.equalize(large, 3.0, 8, 8)["out"])
    ft.reset(0)                                                               # slot 0 holds the 50 x 45 image; slot 1 holds nothing and keeps its setting
    ft.track([dict(stream=0, image=large), dict(stream=1, image=large)], CAM)
    assert np.array_equal(ft.debug_pyramid(0)[0], large)
    assert np.array_equal(ft.debug_pyramid(1)[0], cl_ref.equalize(large, 256.0, 16, 16)["out"])
    ft.close()


@pytest.mark.gpu
def test_gpu_host_mirror_reads_three_raw_frames():
    """Three raw frames through uvs::FeatureTracker::readImage with equalize = true against the same frames equalized by cl_ref and read with
    equalize = false: ids, track_cnt, points and pts_velocity bit for bit."""
    raw = cc.raw_sequence(); eq = cc.equalized_sequence()
    pts = cc.POINTS
    times = [10.0, 10.05, 10.125]
    new2 = np.array([[65.5, 48.25]])
    runs = []
    for on, imgs in ((True, raw), (False, eq)):
        t = HostTracker(0, max_width=131, max_height=97, levels=3, max_points=128)
        assert t.set_equalize(on) == 0 and t.pending() == int(on)
        frames = []
        for k in range(3):
            assert t.read_image(imgs[k], times[k], new=pts if k == 0 else (new2 if k == 2 else ())) == 0
            assert t.pending() == 0
            t.update_ids()
            frames.append(t.get())
        runs.append(frames)
        if on:                                                                # after a reset the setting is sent again with the next frame
            assert t.reset() == 0 and t.pending() == 1 and len(t.get()["ids"]) == 0
            assert t.read_image(imgs[0], 11.0, new=pts) == 0 and t.pending() == 0
            t.update_ids()
            g = t.get()
            assert t.read_image(imgs[1], 11.05) == 0
            t.update_ids()
            again = t.get()
            assert np.array_equal(bits(again["cur_pts"]), bits(frames[1]["cur_pts"]))
        t.close()
    n = [len(f["ids"]) for f in runs[0]]
    assert n[0] == len(pts) and 20 < n[1] < n[0] and runs[0][2]["pts_velocity"][:-1].all()
    for k in range(3):
        a, b = runs[0][k], runs[1][k]
        assert a["ids"].tolist() == b["ids"].tolist() and a["track_cnt"].tolist() == b["track_cnt"].tolist(), k
        for key in ("cur_pts", "cur_un_pts", "pts_velocity"):
            assert np.array_equal(bits(a[key]), bits(b[key])), (k, key)
    # and the raw frames read plain give something else: the equalization is what made the runs agree
    t = HostTracker(0, max_width=131, max_height=97, levels=3, max_points=128)
    t.read_image(raw[0], times[0], new=pts); t.update_ids(); t.read_image(raw[1], times[1]); t.update_ids()
    g = t.get()
    t.close()
    assert not (len(g["ids"]) == n[1] and np.array_equal(bits(g["cur_pts"]), bits(runs[0][1]["cur_pts"])))
