"""Keyframe features of loop closure (uvs_kf_*, csrc/uvs_keyframe_features.hip): the 9 x 9 blur, FAST 9-16 with non-maximum suppression, BRIEF at
the corners and at the window points, liftProjective -- the reference's KeyFrame constructor (keyframe.cpp:14-41, 75-113) on the GPU, against
the numpy restatement tests/kf_ref.py.

CPU tests pin kf_ref itself (the tap table against its formula, the blur against a double loop and hand-computed values, FAST against per-pixel
per-arc loops and hand-made corners, the suppression's ties, BRIEF against a scalar loop, the truncation quirk, patches that leave the image,
liftProjective against numpy.longdouble and spaceToPlane), the pattern loader, the ctypes layouts and the symbols, and calibrate the
image-to-loop-edge case.  GPU tests compare the device with kf_ref EXACTLY: integers and descriptors with ==, the normalized keypoints bit for
bit; there is no tolerance and no excused case in them.  Only the pose of the image-to-loop-edge test has tolerances, and they are lc_ref's."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import kf_cases as kc
import kf_ref
import lc_ref
from helpers import abi, uvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KF_SYMBOLS = ["uvs_kf_create", "uvs_kf_destroy", "uvs_kf_last_error", "uvs_kf_last_device_ms", "uvs_kf_extract", "uvs_kf_debug_frame"]


# ================================================================ CPU: the restatement
def test_tap_table_is_its_formula():
    assert kf_ref.taps_from_formula().tolist() == [7, 17, 32, 46, 52, 46, 32, 17, 7] == kf_ref.TAPS.tolist()
    assert kf_ref.TAPS.sum() == 256


def test_blur_equals_a_direct_double_loop():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (13, 17)).astype(np.uint8)
    H, W = img.shape
    refl = lambda i, n: -i if i < 0 else (2 * n - 2 - i if i >= n else i)          # cv::BORDER_REFLECT_101
    want = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            v = 0
            for j in range(-4, 5):
                h = 0
                for i in range(-4, 5):
                    h += int(kf_ref.TAPS[i + 4]) * int(img[refl(y + j, H), refl(x + i, W)])
                assert h <= 255 * 256
                v += int(kf_ref.TAPS[j + 4]) * h
            assert v < 2 ** 24
            want[y, x] = (v + 32768) >> 16
    assert np.array_equal(kf_ref.blur(img), want)


def test_blur_keeps_a_constant_and_spreads_a_step_by_the_cumulated_taps():
    for g in (0, 1, 93, 254, 255):
        assert np.all(kf_ref.blur(np.full((11, 19), g, np.uint8)) == g)
    img = np.zeros((12, 30), np.uint8); img[:, 15:] = 255
    # 255 c / 256 rounded half up, c = the taps that reach the bright side: 0, 7, 24, 56, 102, 154, 200, 232, 249, 256
    want = [0, 7, 24, 56, 102, 153, 199, 231, 248, 255]
    assert kf_ref.blur(img)[6, 10:20].tolist() == want
    assert np.all(kf_ref.blur(img) == kf_ref.blur(img)[6][None])
    assert np.array_equal(kf_ref.blur(img.T.copy()), kf_ref.blur(img).T)


def _fast_brute(img):
    H, W = img.shape
    out = np.zeros((H, W), np.uint8); n = 0
    for y in range(3, H - 3):
        for x in range(3, W - 3):
            d = [int(img[y + dy, x + dx]) - int(img[y, x]) for dx, dy in kf_ref.RING]
            A = max(min(d[(i + k) % 16] for k in range(9)) for i in range(16))
            B = max(min(-d[(i + k) % 16] for k in range(9)) for i in range(16))
            if max(A, B) > 20:
                out[y, x] = max(A, B) - 1; n += 1
    return out, n


def test_fast_equals_per_pixel_per_arc_loops():
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 256, (14, 19)).astype(np.uint8), kc.texture(30, 40, 31, 10), kc.checkerboard(24, 20, 3),
            rng.integers(100, 140, (9, 9)).astype(np.uint8), kc.all_cases()["tiny_9x9"]["image"]]
    seen = 0
    for img in imgs:
        want, n = _fast_brute(img)
        got, m = kf_ref.score_map(img)
        assert np.array_equal(got, want) and n == m
        seen += n
    assert seen > 50


def test_score_is_the_largest_threshold_that_keeps_the_corner():
    """cornerScore<16>: with threshold t a pixel is a corner iff some arc of 9 has every |d| > t on one side; the score is the largest such t."""
    spike = kc.all_cases()["tiny_9x9_spike"]["image"]                       # 10 everywhere, 200 at the centre: every arc has d = -190
    s, n = kf_ref.score_map(spike)
    assert n == 1 and s[4, 4] == 189 and s.sum() == 189
    img = np.full((11, 11), 100, np.uint8)
    for k, (dx, dy) in enumerate(kf_ref.RING[2:11]):                        # 9 contiguous ring pixels brighter by 30 .. 38: the weakest decides
        img[5 + dy, 5 + dx] = 130 + k
    assert kf_ref.score_map(img)[0][5, 5] == 29
    img[5 + kf_ref.RING[6][1], 5 + kf_ref.RING[6][0]] = 100                 # break the arc: 4 + 4 contiguous only
    assert kf_ref.score_map(img)[0][5, 5] == 0
    img = np.full((11, 11), 100, np.uint8)
    for dx, dy in kf_ref.RING[10:] + kf_ref.RING[:3]:                       # an arc across the ring's start, brighter by exactly 21 / 20
        img[5 + dy, 5 + dx] = 121
    assert kf_ref.score_map(img)[0][5, 5] == 20
    img[img == 121] = 120
    assert kf_ref.score_map(img)[0][5, 5] == 0


def test_equal_neighbours_suppress_each_other():
    s = np.zeros((12, 12), np.uint8)
    s[3, 3] = 50; s[3, 4] = 50                   # a tie: neither survives
    s[7, 3] = 50; s[8, 4] = 49                   # diagonal neighbours: the stronger survives
    s[6, 9] = 30                                 # alone
    s[9, 9] = 30; s[9, 7] = 30                   # two apart: both
    xy, sc = kf_ref.keypoints(s)
    assert xy.tolist() == [[9, 6], [3, 7], [7, 9], [9, 9]] and sc.tolist() == [30, 50, 30, 30]       # row-major: y, then x
    r = kf_ref.extract(kc.checkerboard(200, 120, 5), np.zeros((0, 2)), kc.CAM, kc.pattern())
    assert 0 < r["n_keypoints"] < r["n_corners_before_nms"]


def _brief_scalar(blurred, uv, pat):
    H, W = blurred.shape
    out = np.zeros((len(uv), 4), np.uint64)
    for n, (u, v) in enumerate(np.asarray(uv, np.float32)):
        for i in range(256):
            c = [int(np.float32(a) + np.float32(pat[k][i])) for k, a in ((0, u), (1, v), (2, u), (3, v))]      # int(): toward zero
            if 0 <= c[0] < W and 0 <= c[1] < H and 0 <= c[2] < W and 0 <= c[3] < H and blurred[c[1], c[0]] < blurred[c[3], c[2]]:
                out[n, i >> 6] |= np.uint64(1 << (i & 63))
    return out


def test_brief_equals_a_scalar_loop_also_where_the_patch_leaves_the_image():
    pat = kc.pattern()
    assert pat.shape == (4, 256) and np.abs(pat).max() == 24
    for name in ("small_64x48", "odd_131x97"):
        c = kc.all_cases()[name]
        bl = kf_ref.blur(c["image"])
        got = kf_ref.brief(bl, c["window_uv"], pat)
        assert np.array_equal(got, _brief_scalar(bl, c["window_uv"], pat)), name
        assert len(set(map(bytes, got))) > len(got) // 2
    # each edge: a test whose end leaves the image is 0 whatever the image holds
    bl = np.arange(60 * 80, dtype=np.int64).reshape(60, 80) % 251
    bl = bl.astype(np.uint8)
    bits = lambda d: np.array([[(int(w) >> b) & 1 for w in d for b in range(64)]], bool)[0]
    for (u, v), leaves in (((0.0, 30.0), (pat[0] < 0) | (pat[2] < 0)), ((79.0, 30.0), (pat[0] > 0) | (pat[2] > 0)),
                           ((40.0, 0.0), (pat[1] < 0) | (pat[3] < 0)), ((40.0, 59.0), (pat[1] > 0) | (pat[3] > 0))):
        d = kf_ref.brief(bl, np.array([[u, v]], np.float32), pat)[0]
        assert leaves.sum() > 100 and not bits(d)[leaves].any() and bits(d)[~leaves].any()
    assert not kf_ref.brief(bl, np.array([[-30.0, -30.0]], np.float32), pat).any()


def test_truncation_toward_zero_lets_minus_a_half_pass_the_bounds_test():
    """(int)(-0.5f + 0) is 0, not -1: the reference's cast keeps a point half a pixel outside the image inside it."""
    pat = np.zeros((4, 256), np.int32); pat[2, :] = 2            # every test: (u, v) against (u + 2, v)
    bl = np.zeros((9, 9), np.uint8); bl[:, 1] = 9                # column 0 is darker than column 1
    full, none = [[2 ** 64 - 1] * 4], [[0] * 4]
    assert kf_ref.brief(bl, [[-0.5, -0.5]], pat).tolist() == full          # (0, 0) against (1, 0): a floor would have put the first end at -1
    assert kf_ref.brief(bl, [[-0.999, 3.0]], pat).tolist() == full
    assert kf_ref.brief(bl, [[-1.0, 3.0]], pat).tolist() == none           # -1 is outside
    assert kf_ref.brief(bl, [[-0.5, 8.999]], pat).tolist() == full and kf_ref.brief(bl, [[-0.5, 9.0]], pat).tolist() == none
    assert kf_ref.brief(bl, [[1.0, 3.0]], pat).tolist() == none            # (1, 3) against (3, 3): 9 < 0 fails


def test_lift_projective_against_longdouble_and_space_to_plane():
    rng = np.random.default_rng(3)
    uv = np.stack([rng.integers(0, 752, 4000), rng.integers(0, 480, 4000)], 1)
    for cam in (kc.CAM, kc.CAM_DIST):
        m = kf_ref.lift(cam, uv)
        ml = kf_ref.lift(cam, uv, np.longdouble)
        dev = float(np.abs(m - ml.astype(np.float64)).max())
        print(f"liftProjective float64 against longdouble, distortion {'on' if len(cam) > 4 else 'off'}: max |dev| {dev:.2e}")      # for information
        assert dev < 1e-14
        back = kf_ref.space_to_plane(cam, m)
        # Without distortion the round trip is exact to rounding.  With it, the 8 evaluations are a fixed-point iteration that is short of
        # convergence in the corners: there |d distortion / d m| is about |k1| (rho^2 + 2 x^2) = 0.29 (0.93 + 1.3) = 0.65 per evaluation, so
        # 0.65^8 = 0.03 of the distortion (up to 100 px) may remain: 3 px.  A wrong sign or a wrong order of the terms is off by tens of pixels.
        err = float(np.abs(back - uv).max())
        print(f"    spaceToPlane(liftProjective(p)) - p: max {err:.3e} px")
        assert err < (3.0 if len(cam) > 4 else 1e-9), err
    centre = np.abs(uv - np.array([363.0, 248.1])).max(1) < 150
    assert np.abs(kf_ref.space_to_plane(kc.CAM_DIST, kf_ref.lift(kc.CAM_DIST, uv[centre])) - uv[centre]).max() < 1e-4
    assert np.array_equal(kf_ref.lift(kc.CAM, uv), kf_ref.lift(kc.CAM + (0.0, 0.0, 0.0, 0.0), uv))


def test_pattern_loader_reads_the_fixture_and_rejects_a_short_list():
    pat = abi.load_brief_pattern(kc.PATTERN_FILE)
    assert pat.dtype == np.int32 and pat.shape == (4, abi.KF_PATTERN_BITS) and pat.min() == -24 and pat.max() == 24
    assert pat[:, 0].tolist() == [0, -10, 0, -6] and pat[:, -1].tolist()[3] == -2
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "p.yml")
        open(p, "w").write("%YAML:1.0\nx1: [1, 2,\n  3]\ny1:\n  - 4\n  - 5\n  - 6\nx2: [7, 8, 9]\ny2: [1, 1, 1]\n")
        with pytest.raises(ValueError):
            abi.load_brief_pattern(p)                            # 3 tests, not 256: but parsed, inline and block lists alike
        open(p, "w").write("x1: [1]\ny1: [1]\nx2: [1]\n")
        with pytest.raises(ValueError):
            abi.load_brief_pattern(p)


def test_scene_generator_stays_in_range():
    for s in kc.SCENE_SEEDS:
        c = kc.all_cases()[f"scene_{s}"]
        r = kf_ref.extract(c["image"], c["window_uv"], c["cam"], kc.pattern())
        assert c["image"].shape == (480, 752) and 100 <= r["n_keypoints"] <= 4096 and r["status"] == kf_ref.OK
        assert r["blur"].min() < 10 and r["blur"].max() > 245
        assert np.all(np.diff(r["xy"][:, 1] * 752 + r["xy"][:, 0]) > 0)           # row-major order


# ================================================================ CPU: layout and symbols
def test_kf_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "uvs_solver.h")).read()
    for s in KF_SYMBOLS:
        assert s + "(" in hdr, s
        assert s in uvs.api.EXPORTS, s
    assert "#define UVS_ABI_VERSION 7" in hdr
    L = uvs.api.lib()
    for s in KF_SYMBOLS:
        assert hasattr(L, s), s
    assert L.uvs_abi_version() == 7
    Hst = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
    assert hasattr(Hst, "uvs_host_pose_graph_image_run") and hasattr(Hst, "uvs_host_pose_graph_verify_run")


def test_kf_struct_layout_matches_header():
    code = r'''
#include <stdio.h>
#include <stddef.h>
#include "uvs_solver.h"
int main(void) {
  printf("%zu %zu %zu\n", sizeof(uvs_kf_frame), sizeof(uvs_kf_camera), sizeof(uvs_kf_result));
  printf("%zu %zu %zu %zu %zu\n", offsetof(uvs_kf_frame, image), offsetof(uvs_kf_frame, width), offsetof(uvs_kf_frame, height),
         offsetof(uvs_kf_frame, n_window), offsetof(uvs_kf_frame, window_uv));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(uvs_kf_camera, fx), offsetof(uvs_kf_camera, fy), offsetof(uvs_kf_camera, cx),
         offsetof(uvs_kf_camera, cy), offsetof(uvs_kf_camera, k1), offsetof(uvs_kf_camera, k2), offsetof(uvs_kf_camera, p1), offsetof(uvs_kf_camera, p2));
  printf("%zu %zu %zu %zu\n", offsetof(uvs_kf_result, status), offsetof(uvs_kf_result, n_keypoints), offsetof(uvs_kf_result, n_returned),
         offsetof(uvs_kf_result, n_corners_before_nms));
  printf("%d %d %d %d %d %d %d %d\n", UVS_KF_MAX_FRAMES, UVS_KF_MIN_SIZE, UVS_KF_MAX_WIDTH, UVS_KF_MAX_HEIGHT, UVS_KF_PATTERN_BITS,
         UVS_KF_MAX_PATTERN_OFFSET, UVS_KF_OK, UVS_KF_OVERFLOW);
  printf("%d\n", (int)(UVS_KF_MAX_COORD == 1e6));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c"); exe = os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    F, K, R = abi.KfFrame, abi.KfCamera, abi.KfResult
    assert out[:3] == [C.sizeof(F), C.sizeof(K), C.sizeof(R)]
    assert out[3:8] == [F.image.offset, F.width.offset, F.height.offset, F.n_window.offset, F.window_uv.offset]
    assert out[8:16] == [getattr(K, n).offset for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")]
    assert out[16:20] == [R.status.offset, R.n_keypoints.offset, R.n_returned.offset, R.n_corners_before_nms.offset]
    assert out[20:28] == [abi.KF_MAX_FRAMES, abi.KF_MIN_SIZE, abi.KF_MAX_WIDTH, abi.KF_MAX_HEIGHT, abi.KF_PATTERN_BITS, abi.KF_MAX_PATTERN_OFFSET,
                          abi.KF_STATUS.index("OK"), abi.KF_STATUS.index("OVERFLOW")]
    assert out[28] == 1 and abi.KF_MAX_COORD == 1e6 == kf_ref.MAX_COORD
    assert (kf_ref.OK, kf_ref.OVERFLOW, kf_ref.MIN_SIZE) == (0, 1, abi.KF_MIN_SIZE)


def test_kf_extractor_create_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    pat = kc.pattern()
    p = [pat[k].ctypes.data_as(abi.c_i32_p) for k in range(4)]
    assert uvs.api.lib().uvs_kf_create(0, 1, 64, 64, 64, 16, *p, C.byref(h)) == abi.UVS_ERR_NO_DEVICE
    with pytest.raises(RuntimeError):
        uvs.api.KeyframeExtractor(pat)


# ================================================================ the image-to-loop-edge case (shared by the CPU calibration and the GPU test)
TIC, QIC = np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0])      # the camera is the body
# lc_ref's own error against the rendered pose of the old keyframe (test_image_to_loop_edge_numbers_with_the_numpy_references measures it):
LC_REF_T_ERR, LC_REF_ANGLE_ERR = 0.0061, 0.0763             # m, degrees
TRUTH_T_BOUND, TRUTH_ANGLE_BOUND = 2 * LC_REF_T_ERR, 2 * LC_REF_ANGLE_ERR
E2E_SEED = 11


def _quat_xyzw(R):
    q = lc_ref.R_to_quat_eigen(R)
    return np.array([q[1], q[2], q[3], q[0]])


def _loop_pair(cur, old, cur_view, old_view, seed):
    """cur / old: the frames' dicts (kf_ref.extract's or the device's; cur extracted WITH its window points); *_view = (image, R, t)."""
    _, R, t = cur_view
    return dict(p3d=cur["p3d"], qdesc=cur["window_desc"], vio_t=t, vio_q=_quat_xyzw(R), uv=old["norm"], odesc=old["desc"], seed=seed)


def _window_of(frame, view):
    """The 150 strongest keypoints of a frame as its window points: (uv float32 [150, 2], their 3-D points on the plane)."""
    _, R, t = view
    uv = frame["xy"][kc.strongest(frame)].astype(np.float32)
    return uv, kc.pixel_to_plane(R, t, uv.astype(np.float64))


def _pose_error(r, view):
    _, R, t = view
    Rp = lc_ref.quat_to_R(r["PnP_q_old"])
    return float(np.linalg.norm(np.asarray(r["PnP_T_old"]) - t)), float(np.degrees(np.arccos(np.clip((np.trace(Rp.T @ R) - 1) / 2, -1, 1))))


def test_image_to_loop_edge_numbers_with_the_numpy_references():
    """The calibration of the GPU test: two rendered views through kf_ref and lc_ref.  Measured here: 150 matches of 150 window points, 136 of
    them within 3 px of the true projection, 137 inliers; lc_ref's pose of the old keyframe is 0.0061 m and 0.0762 degrees from the rendered
    pose.  The constants LC_REF_T_ERR / LC_REF_ANGLE_ERR record that, and the GPU test's physical bound is twice them."""
    v = kc.views(2)
    pat = kc.pattern()
    first = kf_ref.extract(v[0][0], np.zeros((0, 2)), kc.CAM, pat)
    uv, X = _window_of(first, v[0])
    cur = kf_ref.extract(v[0][0], uv, kc.CAM, pat); cur["p3d"] = X
    old = kf_ref.extract(v[1][0], np.zeros((0, 2)), kc.CAM, pat)
    assert len(uv) == kc.N_WINDOW and np.array_equal(cur["window_desc"], cur["desc"][kc.strongest(first)])
    r = lc_ref.verify(_loop_pair(cur, old, v[0], v[1], E2E_SEED), TIC, QIC)
    m = r["match_old"] >= 0
    near = np.linalg.norm(kc.project(v[1][1], v[1][2], X[m]) - old["xy"][r["match_old"][m]], axis=1) < 3.0
    te, ae = _pose_error(r, v[1])
    print(f"image to loop edge (kf_ref + lc_ref): {r['n_matches']} matches, {int(near.sum())} within 3 px, {r['n_inliers']} inliers, "
          f"pose error {te:.4f} m / {ae:.4f} deg")
    assert r["accepted"] == 1 and r["n_matches"] >= 140 and near.sum() >= 120
    assert te <= LC_REF_T_ERR and ae <= LC_REF_ANGLE_ERR, (te, ae)             # the recorded figures still hold (rounded up)
    assert te > 0.5 * LC_REF_T_ERR and ae > 0.5 * LC_REF_ANGLE_ERR             # ... and are not stale


# ================================================================ GPU
def _extractor(**kw):
    kw.setdefault("max_width", 1100); kw.setdefault("max_height", 480); kw.setdefault("max_frames", 16); kw.setdefault("max_window", 512)
    return uvs.api.KeyframeExtractor(kc.pattern(), **kw)


def _frame(c):
    return dict(image=c["image"], window_uv=c["window_uv"])


def _same(name, dev, ref, debug=False):
    """Exact: integers and descriptors with ==, normalized keypoints bit for bit."""
    for k in ("status", "n_keypoints", "n_returned", "n_corners_before_nms"):
        assert dev[k] == ref[k], (name, k, dev[k], ref[k])
    for k in ("xy", "score", "desc", "window_desc") + (("blur", "score_map") if debug else ()):
        assert dev[k].shape == ref[k].shape and dev[k].dtype == ref[k].dtype, (name, k, dev[k].shape, ref[k].shape, dev[k].dtype)
        assert np.array_equal(dev[k], ref[k]), (name, k, np.argwhere(dev[k] != ref[k])[:5].tolist())
    assert dev["norm"].shape == ref["norm"].shape and dev["norm"].dtype == np.float64 == ref["norm"].dtype
    assert np.array_equal(dev["norm"].view(np.uint64), ref["norm"].view(np.uint64)), (name, "norm", np.abs(dev["norm"] - ref["norm"]).max())


def _bits(frames):
    return [tuple((k, np.asarray(v).tobytes()) for k, v in sorted(d.items())) for d in frames]


@pytest.mark.gpu
def test_gpu_every_case_equals_the_reference_exactly():
    x = _extractor()
    pat = kc.pattern()
    for name, c in kc.all_cases().items():
        ref = kf_ref.extract(c["image"], c["window_uv"], c["cam"], pat)
        _same(name + " (debug_frame)", x.debug_frame(_frame(c), c["cam"]), ref, debug=True)
        _same(name + " (extract)", x.extract([_frame(c)], c["cam"])[0], ref)
    assert kf_ref.extract(kc.all_cases()["constant"]["image"], [], kc.CAM, pat)["n_keypoints"] == 0
    x.close()


@pytest.mark.gpu
def test_gpu_batch_equals_one_at_a_time_and_runs_repeat():
    x = _extractor()
    cases = kc.all_cases()
    for cam, names in ((kc.CAM, [f"scene_{s}" for s in kc.SCENE_SEEDS]),
                       (kc.CAM_DIST, ["small_64x48", "scene_2", "tiny_9x9", "wide_1030x67", "no_window", "odd_77x203", "constant", "scene_0", "checkerboard", "noise"])):
        batch = [_frame(cases[n]) for n in names]
        a = x.extract(batch, cam)
        assert _bits(a) == _bits(x.extract(batch, cam))
        one = [x.extract([f], cam)[0] for f in batch]
        assert _bits(a) == _bits(one)
        for n, d in zip(names, a):
            _same(n + " (batch)", d, kf_ref.extract(cases[n]["image"], cases[n]["window_uv"], cam, kc.pattern()))
    assert x.last_device_ms > 0.0 and x.last_ms >= x.last_device_ms * 0.5
    x.close()


@pytest.mark.gpu
def test_gpu_overflow_reports_the_true_count_and_returns_the_first_64():
    x = _extractor(max_keypoints=64)
    c = kc.all_cases()["scene_1"]
    full = kf_ref.extract(c["image"], c["window_uv"], c["cam"], kc.pattern())
    ref = kf_ref.extract(c["image"], c["window_uv"], c["cam"], kc.pattern(), max_keypoints=64)
    assert full["n_keypoints"] > 64 and ref["status"] == kf_ref.OVERFLOW and ref["n_returned"] == 64 and ref["n_keypoints"] == full["n_keypoints"]
    assert np.array_equal(ref["xy"], full["xy"][:64]) and np.array_equal(ref["desc"], full["desc"][:64])
    small = kc.all_cases()["small_64x48"]                              # 24 keypoints: no overflow beside an overflowing frame
    out = x.extract([_frame(c), _frame(small), _frame(c)], c["cam"])
    _same("overflow", out[0], ref); _same("overflow again", out[2], ref)
    _same("beside it", out[1], kf_ref.extract(small["image"], small["window_uv"], c["cam"], kc.pattern(), max_keypoints=64))
    assert out[0]["status"] == abi.KF_STATUS.index("OVERFLOW") and out[1]["status"] == abi.KF_STATUS.index("OK")
    _same("overflow (debug_frame)", x.debug_frame(_frame(c), c["cam"]), ref, debug=True)
    x.close()


@pytest.mark.gpu
def test_gpu_argument_checks_and_status_codes():
    x = _extractor(max_frames=2, max_width=160, max_height=120, max_keypoints=256, max_window=64)
    L = uvs.api.lib()
    ok = _frame(kc.all_cases()["no_window"]); ok["window_uv"] = kc.window_points(1, 8, 160, 120)
    assert x.extract_raw([ok], kc.CAM)[0] == abi.UVS_OK
    for k in ("frames", "camera", "xy", "score", "norm", "desc", "wdesc", "results"):
        assert x.extract_raw([ok], kc.CAM, null=(k,))[0] == abi.UVS_ERR_INVALID_ARG, k
    assert x.extract_raw([ok], kc.CAM, n_frames=0)[0] == abi.UVS_ERR_INVALID_ARG
    assert x.extract_raw([ok], kc.CAM, n_frames=-1)[0] == abi.UVS_ERR_INVALID_ARG
    assert x.extract_raw([ok, ok, ok], kc.CAM)[0] == abi.UVS_ERR_CAPACITY
    assert "capacity" in L.uvs_kf_last_error(x._h).decode()
    img = lambda h, w: dict(image=np.zeros((h, w), np.uint8))
    assert x.extract_raw([img(120, 161)], kc.CAM)[0] == abi.UVS_ERR_CAPACITY          # too wide
    assert x.extract_raw([img(121, 160)], kc.CAM)[0] == abi.UVS_ERR_CAPACITY          # too tall
    assert x.extract_raw([img(120, 160)], kc.CAM)[0] == abi.UVS_OK
    assert x.extract_raw([img(8, 40)], kc.CAM)[0] == abi.UVS_ERR_INVALID_ARG          # below UVS_KF_MIN_SIZE
    assert x.extract_raw([img(40, 8)], kc.CAM)[0] == abi.UVS_ERR_INVALID_ARG
    assert "UVS_KF_MIN_SIZE" in L.uvs_kf_last_error(x._h).decode()
    assert x.extract_raw([img(9, 9)], kc.CAM)[0] == abi.UVS_OK
    many = dict(ok); many["window_uv"] = kc.window_points(2, 65, 160, 120)
    assert x.extract_raw([many], kc.CAM)[0] == abi.UVS_ERR_CAPACITY
    for bad in (np.nan, np.inf, -np.inf, 1.0001e6, -2e6):
        w = dict(ok); w["window_uv"] = ok["window_uv"].copy(); w["window_uv"][3, 1] = bad
        assert x.extract_raw([w], kc.CAM)[0] == abi.UVS_ERR_INVALID_ARG, bad
    assert "window point" in L.uvs_kf_last_error(x._h).decode()
    edge = dict(ok); edge["window_uv"] = np.array([[1e6, -1e6]], np.float32)           # the bound itself is taken
    rc, out = x.extract_raw([edge], kc.CAM)
    assert rc == abi.UVS_OK and not out[0]["window_desc"].any()
    for cam in ((0.0, 460.0, 1.0, 1.0), (460.0, -1.0, 1.0, 1.0), (np.nan, 460.0, 1.0, 1.0), (460.0, 460.0, np.inf, 1.0),
                (460.0, 460.0, 1.0, 1.0, np.nan, 0.0, 0.0, 0.0)):
        assert x.extract_raw([ok], cam)[0] == abi.UVS_ERR_INVALID_ARG, cam
    # a null image, a null window array behind a positive count, a negative count
    arr, keep = abi.kf_frames([ok])
    cam = abi.kf_camera(kc.CAM)
    o = x._outputs(1, 8); res = (abi.KfResult * 1)()
    call = lambda: L.uvs_kf_extract(x._h, 1, C.cast(arr, C.POINTER(abi.KfFrame)), C.byref(cam), o["xy"].ctypes.data_as(abi.c_i32_p),
                                    o["score"].ctypes.data_as(abi.c_u8_p), abi._dp(o["norm"]), o["desc"].ctypes.data_as(abi.c_u64_p),
                                    o["wdesc"].ctypes.data_as(abi.c_u64_p), C.cast(res, C.POINTER(abi.KfResult)))
    assert call() == abi.UVS_OK
    # (the addresses, not the field objects: a ctypes pointer read from a structure is a view of the field and turns NULL with it)
    uv_addr = C.cast(arr[0].window_uv, C.c_void_p).value; im_addr = C.cast(arr[0].image, C.c_void_p).value
    arr[0].window_uv = None
    assert call() == abi.UVS_ERR_INVALID_ARG
    arr[0].window_uv = C.cast(uv_addr, abi.c_float_p); arr[0].n_window = -1
    assert call() == abi.UVS_ERR_INVALID_ARG
    arr[0].n_window = 8; arr[0].image = None
    assert call() == abi.UVS_ERR_INVALID_ARG
    arr[0].image = C.cast(im_addr, abi.c_u8_p)
    assert uv_addr and im_addr and C.cast(arr[0].window_uv, C.c_void_p).value == uv_addr and C.cast(arr[0].image, C.c_void_p).value == im_addr
    assert call() == abi.UVS_OK                                   # the handle still works after every rejected call
    assert L.uvs_kf_extract(None, 1, C.cast(arr, C.POINTER(abi.KfFrame)), C.byref(cam), None, None, None, None, None, None) == abi.UVS_ERR_INVALID_ARG
    x.close()
    # create
    pat = kc.pattern(); p = [pat[k].ctypes.data_as(abi.c_i32_p) for k in range(4)]
    h = C.c_void_p()
    assert L.uvs_kf_create(0, 1, 64, 64, 64, 16, *p, None) == abi.UVS_ERR_INVALID_ARG
    assert L.uvs_kf_create(0, 0, 64, 64, 64, 16, *p, C.byref(h)) == abi.UVS_ERR_INVALID_ARG
    assert L.uvs_kf_create(0, 1, 8, 64, 64, 16, *p, C.byref(h)) == abi.UVS_ERR_INVALID_ARG
    assert L.uvs_kf_create(0, 1, 64, 64, 0, 16, *p, C.byref(h)) == abi.UVS_ERR_INVALID_ARG
    assert L.uvs_kf_create(0, 1, 64, 64, 64, 16, p[0], None, p[2], p[3], C.byref(h)) == abi.UVS_ERR_INVALID_ARG
    assert L.uvs_kf_create(0, abi.KF_MAX_FRAMES + 1, 64, 64, 64, 16, *p, C.byref(h)) == abi.UVS_ERR_CAPACITY
    assert L.uvs_kf_create(0, 1, abi.KF_MAX_WIDTH + 1, 64, 64, 16, *p, C.byref(h)) == abi.UVS_ERR_CAPACITY
    assert L.uvs_kf_create(0, 1, 64, abi.KF_MAX_HEIGHT + 1, 64, 16, *p, C.byref(h)) == abi.UVS_ERR_CAPACITY
    assert L.uvs_kf_create(0, 1, 64, 64, abi.LC_MAX_OLD + 1, 16, *p, C.byref(h)) == abi.UVS_ERR_CAPACITY
    assert L.uvs_kf_create(0, 1, 64, 64, 64, abi.LC_MAX_QUERY + 1, *p, C.byref(h)) == abi.UVS_ERR_CAPACITY
    far = pat.copy(); far[2, 17] = abi.KF_MAX_PATTERN_OFFSET + 1
    assert L.uvs_kf_create(0, 1, 64, 64, 64, 16, *[far[k].ctypes.data_as(abi.c_i32_p) for k in range(4)], C.byref(h)) == abi.UVS_ERR_INVALID_ARG
    assert L.uvs_kf_create(99, 1, 64, 64, 64, 16, *p, C.byref(h)) == abi.UVS_ERR_NO_DEVICE
    assert not h.value
    assert L.uvs_kf_last_device_ms(None) == 0.0 and b"null" in L.uvs_kf_last_error(None)


@pytest.mark.gpu
def test_gpu_image_to_loop_edge():
    """Two rendered views of a textured plane: the GPU's features of both go unchanged into uvs_lc_verify, which must accept the loop.  The
    device is held to lc_ref's own result on the same arrays within the 1e-7 of DESIGN.md 3.7 (integers exactly).  Against the rendered pose of
    the old keyframe only a loose physical bound holds: lc_ref itself is 0.0061 m / 0.0763 degrees from it (measured by
    test_image_to_loop_edge_numbers_with_the_numpy_references), and the bound is twice that: 0.0122 m, 0.1526 degrees."""
    v = kc.views(2)
    pat = kc.pattern()
    x = _extractor(max_frames=2, max_width=752)
    first = x.extract([dict(image=v[0][0])], kc.CAM)[0]
    uv, X = _window_of(first, v[0])
    cur, old = x.extract([dict(image=v[0][0], window_uv=uv), dict(image=v[1][0])], kc.CAM)
    x.close()
    _same("view 0", cur, kf_ref.extract(v[0][0], uv, kc.CAM, pat)); _same("view 1", old, kf_ref.extract(v[1][0], [], kc.CAM, pat))
    cur["p3d"] = X
    pair = _loop_pair(cur, old, v[0], v[1], E2E_SEED)
    lv = uvs.api.LoopVerifier(max_pairs=1, max_query=kc.N_WINDOW, max_old=4096)
    res, mo, inl = lv.verify([pair], TIC, QIC)
    lv.close()
    r, ref = res[0], lc_ref.verify(pair, TIC, QIC)
    assert r["accepted"] == 1 and r["reason"] == lc_ref.REASON["ACCEPTED"]
    assert np.array_equal(mo[0], ref["match_old"]) and np.array_equal(inl[0], ref["inlier"])
    for k in ("accepted", "reason", "n_matches", "n_inliers", "best_hypothesis", "ransac_iters"):
        assert r[k] == ref[k], (k, r[k], ref[k])
    for k in ("loop_info", "PnP_T_old", "PnP_q_old"):
        a, b = np.asarray(r[k]), np.asarray(ref[k])
        assert np.all(np.abs(a - b) <= 1e-7 * np.maximum(1.0, np.abs(b))), (k, a, b)
    te, ae = _pose_error(r, v[1])
    print(f"image to loop edge (GPU): {r['n_matches']} matches, {r['n_inliers']} inliers, pose error {te:.4f} m / {ae:.4f} deg")
    assert te < TRUTH_T_BOUND and ae < TRUTH_ANGLE_BOUND, (te, ae)


@pytest.mark.gpu
def test_gpu_host_mirror_builds_keyframes_from_images():
    """Three rendered views through uvs_host_pose_graph_image_run (the online KeyFrame constructor, addKeyFrameWithCandidate, optimize4DoF):
    the same descriptors and keypoints as the Python path bit for bit, and an accepted loop for the view that revisits the first one."""
    order = (1, 2, 0)                                             # the revisited pose first, the revisiting view last
    v = [kc.views(3)[k] for k in order]
    n, max_kp = len(v), 2048
    x = _extractor(max_frames=1, max_width=752, max_keypoints=max_kp)
    win = [_window_of(x.extract([dict(image=im)], kc.CAM)[0], (im, R, t)) for im, R, t in v]
    py = [x.extract([dict(image=v[k][0], window_uv=win[k][0])], kc.CAM)[0] for k in range(n)]
    x.close()
    Hst = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
    f = Hst.uvs_host_pose_graph_image_run
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int, abi.c_double_p, abi.c_double_p, abi.c_double_p, abi.c_int_p, abi.c_double_p, abi.c_double_p, C.POINTER(abi.KfCamera),
                  abi.c_i32_p, C.c_int, C.c_int, C.c_int, abi.c_u8_p, abi.c_int_p, abi.c_double_p, abi.c_float_p, abi.c_int_p, abi.c_int_p,
                  abi.c_double_p, abi.c_double_p, abi.c_int_p, abi.c_double_p, abi.c_u64_p, abi.c_u64_p]
    stamps = np.arange(n, dtype=np.float64); t = np.array([w[2] for w in v]); q = np.array([_quat_xyzw(w[1]) for w in v])
    seq = np.ones(n, np.int32); cand = np.array([-1, -1, 0], np.int32)
    images = np.ascontiguousarray(np.stack([w[0] for w in v])); nq = np.array([len(w[0]) for w in win], np.int32)
    p3d = np.ascontiguousarray(np.concatenate([w[1] for w in win])); uv = np.ascontiguousarray(np.concatenate([w[0] for w in win]), dtype=np.float32)
    pat = np.ascontiguousarray(kc.pattern()); cam = abi.kf_camera(kc.CAM)
    acc = np.zeros(n, np.int32); info = np.zeros((n, 8)); pose = np.zeros((n, 7)); n_kp = np.zeros(n, np.int32)
    norm = np.zeros((n, max_kp, 2)); desc = np.zeros((n, max_kp, 4), np.uint64); wdesc = np.zeros((int(nq.sum()), 4), np.uint64)
    ip = lambda a: a.ctypes.data_as(abi.c_int_p)
    rc = f(0, n, abi._dp(stamps), abi._dp(t), abi._dp(q), ip(seq), abi._dp(TIC), abi._dp(QIC), C.byref(cam), pat.ctypes.data_as(abi.c_i32_p), max_kp,
           kc.W, kc.H, images.ctypes.data_as(abi.c_u8_p), ip(nq), abi._dp(p3d), uv.ctypes.data_as(abi.c_float_p), ip(cand), ip(acc), abi._dp(info),
           abi._dp(pose), ip(n_kp), abi._dp(norm), desc.ctypes.data_as(abi.c_u64_p), wdesc.ctypes.data_as(abi.c_u64_p))
    assert rc == abi.UVS_OK
    off = np.r_[0, np.cumsum(nq)]
    for k in range(n):
        assert n_kp[k] == py[k]["n_returned"] > 100
        assert np.array_equal(desc[k, :n_kp[k]], py[k]["desc"]) and np.array_equal(norm[k, :n_kp[k]].view(np.uint64), py[k]["norm"].view(np.uint64))
        assert np.array_equal(wdesc[off[k]:off[k + 1]], py[k]["window_desc"])
    assert acc.tolist() == [0, 0, 1]
    # the loop edge of the revisiting view: the Python path on the same arrays, with the mirror's seed (index << 32) | old index
    cur = dict(py[2]); cur["p3d"] = win[2][1]
    lv = uvs.api.LoopVerifier(max_pairs=1, max_query=kc.N_WINDOW, max_old=4096)
    r = lv.verify([_loop_pair(cur, py[0], v[2], v[0], (2 << 32) | 0)], TIC, QIC)[0][0]
    lv.close()
    assert r["accepted"] == 1
    assert np.all(np.abs(info[2] - r["loop_info"]) <= 1e-7 * np.maximum(1.0, np.abs(r["loop_info"]))), (info[2], r["loop_info"])
    assert np.all(info[:2] == 0) and np.all(np.isfinite(pose)) and np.abs(np.linalg.norm(pose[:, 3:], axis=1) - 1).max() < 1e-9
