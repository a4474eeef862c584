"""Detection of new track points (uvs_ft_detect, uvs_ft_set_mask; csrc/uvs_feature_detect.hip): Shi-Tomasi corners of the image a tracker slot
holds, kept away from the occupied points and from each other -- the reference's setMask + cv::goodFeaturesToTrack + addPoints
(feature_tracker.cpp:9-52, 119-131) on the GPU, against the numpy restatement tests/fd_ref.py.

CPU tests pin fd_ref itself (the score map against a scalar loop with reflection, the sums against Python integers, the known answers of
constructed images, the cap, the distance rules, the invariants of every result), the ctypes layouts and the symbols, and the host mirror's
setMask without a device.  GPU tests compare the device with fd_ref EXACTLY: integers with ==, every FP64 value bit for bit; there is no
tolerance in them."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import fd_cases as dc
import fd_ref
import ft_cases as fc
import ft_ref
import kf_ref
from helpers import abi, uvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_SYMBOLS = ["uvs_ft_set_max_candidates", "uvs_ft_set_mask", "uvs_ft_detect", "uvs_ft_last_detect_device_ms", "uvs_ft_debug_detect"]
HOST_SYMBOLS = ["uvs_host_ft_set_detection", "uvs_host_ft_set_image_mask", "uvs_host_ft_read_image_detect", "uvs_host_ft_apply_set_mask"]
CAM = dc.CAM


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def refl(i, n):
    return -i if i < 0 else (2 * n - 2 - i if i >= n else i)


# ================================================================ CPU: the restatement
def _score_scalar(img):
    """The rules of include/uvs_solver.h pixel by pixel in Python integers: -> (A, B, C, S) lists of lists and the score map."""
    H, W = img.shape
    p = lambda x, y: int(img[refl(y, H), refl(x, W)])
    gx = [[(p(x + 1, y - 1) - p(x - 1, y - 1)) + 2 * (p(x + 1, y) - p(x - 1, y)) + (p(x + 1, y + 1) - p(x - 1, y + 1)) for x in range(W)] for y in range(H)]
    gy = [[(p(x - 1, y + 1) - p(x - 1, y - 1)) + 2 * (p(x, y + 1) - p(x, y - 1)) + (p(x + 1, y + 1) - p(x + 1, y - 1)) for x in range(W)] for y in range(H)]
    A = np.zeros((H, W), object); B = np.zeros((H, W), object); Cc = np.zeros((H, W), object); S = np.zeros((H, W), object)
    score = np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            a = b = c = 0
            for j in (-1, 0, 1):
                for i in (-1, 0, 1):
                    u, v = gx[refl(y + j, H)][refl(x + i, W)], gy[refl(y + j, H)][refl(x + i, W)]
                    a += u * u; b += u * v; c += v * v
            A[y, x], B[y, x], Cc[y, x] = a, b, c
            S[y, x] = (a - c) ** 2 + 4 * b * b
            score[y, x] = np.float64(a + c) - np.sqrt(np.float64(S[y, x]))
    return A, B, Cc, S, score


def test_score_map_equals_a_scalar_loop_with_reflection():
    rng = np.random.default_rng(11)
    for H, W in ((24, 24), (17, 13)):                           # 13 wide, 17 high: odd sizes; corners and edges are in the comparison
        img = rng.integers(0, 256, (H, W)).astype(np.uint8)
        A, B, Cc, S, want = _score_scalar(img)
        got = fd_ref.score_map(img)
        assert got.shape == (H, W) and np.array_equal(bits(got), bits(want))
        a, b, c = fd_ref.sums(img)
        assert np.array_equal(a, A.astype(np.int64)) and np.array_equal(b, B.astype(np.int64)) and np.array_equal(c, Cc.astype(np.int64))
        assert (got >= 0).all()
    gx, gy = fd_ref.sobel(np.tile((10 + 3 * np.arange(30)).astype(np.uint8), (12, 1)))
    assert np.all(gx[:, 1:-1] == 24) and np.all(gy == 0)        # a ramp of slope 3: 8 x 3


def test_sums_on_a_0_255_pattern_need_int64_for_S():
    img = np.zeros((24, 24), np.uint8)
    img[:, 12:] = 255                                           # a vertical step: |gx| = 1020 on both sides of it, gy = 0
    img[16:, :] = 255 - img[16:, :]                             # ... and a horizontal one that flips it
    A, B, Cc, S, want = _score_scalar(img)
    a, b, c = fd_ref.sums(img)
    assert np.abs(fd_ref.sobel(img)[0]).max() == 1020
    assert int(a.max()) == max(int(v) for v in A.ravel()) == 6 * 1020 ** 2 <= 9 * 1020 ** 2 < 2 ** 31
    s_max = max(int(v) for v in S.ravel())
    assert 2 ** 31 < s_max <= (9 * 1020 ** 2) ** 2 < 2 ** 53     # beyond int32, exact in FP64
    got = fd_ref.score_map(img)
    assert np.array_equal(bits(got), bits(want)) and (got >= 0).all()
    for name in ("cb2", "scene_48x40", "lattice_131x97"):
        assert (dc.ref(name)["score_map"] >= 0).all()


def _check_invariants(r, occupied, R, shape):
    H, W = shape
    xy = r["xy"].astype(np.int64)
    for i in range(len(xy)):
        d2 = ((xy[:i] - xy[i]) ** 2).sum(axis=1)
        assert (d2 >= R * R).all()                              # pairwise at least R apart
    for ox, oy in np.asarray(occupied).reshape(-1, 2):
        c = np.array([int(np.rint(ox)), int(np.rint(oy))])
        assert (((xy - c) ** 2).sum(axis=1) > R * R).all()      # more than R from every occupied centre
    if len(xy):
        assert xy[:, 0].min() >= 1 and xy[:, 0].max() <= W - 2 and xy[:, 1].min() >= 1 and xy[:, 1].max() <= H - 2
    assert (np.diff(r["score"]) <= 0).all() and (np.diff(r["cand_score"]) <= 0).all()
    assert np.array_equal(r["score"], r["score_map"][xy[:, 1], xy[:, 0]])
    assert np.array_equal(bits(r["norm"]), bits(kf_ref.lift(CAM, xy.astype(np.float64)) if len(xy) else np.zeros((0, 2))))


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_invariants_of_every_result(name):
    c, r = dc.case(name), dc.ref(name)
    _check_invariants(r, c["occupied"], c["R"], c["image"].shape)
    assert r["n_new"] <= c["max_new"] and r["n_new"] == len(r["xy"]) == len(r["score"]) == len(r["norm"])


def test_known_answers_of_the_rectangle():
    r = dc.ref("rect")
    assert r["n_candidates"] == 4 and r["xy"].tolist() == [[35, 29], [12, 29], [35, 10], [12, 10]] and r["max_score"] == 1620000.0
    assert r["threshold"] == 16200.0 and r["status"] == fd_ref.DETECT_OK
    r = dc.ref("rect_occupied")                                 # rint(12.4, 10.5) = (12, 10): the corner itself
    assert r["xy"].tolist() == [[35, 29], [12, 29], [35, 10]] and r["n_candidates"] == 3
    assert dc.ref("rect_two")["xy"].tolist() == [[35, 29], [12, 29]] and dc.ref("rect_two")["n_candidates"] == 4
    r = dc.ref("rect_none_allowed")
    assert not r["allowed"].any() and r["n_new"] == 0 and r["max_score"] == 0.0 and r["n_candidates"] == 0


def test_known_answers_of_the_checkerboards():
    r = dc.ref("cb1")
    assert not r["score_map"].any() and r["n_candidates"] == 0 and r["n_new"] == 0
    r = dc.ref("cb2")
    assert r["n_candidates"] == 1584 and r["max_score"] == 6242400.0
    # the board and its scores are symmetric under both flips, so the candidates that are not tied come in fours: the four outermost, at the
    # maximum; the other 1580 share one score, and the pixel index alone orders them
    v, n = np.unique(r["cand_score"], return_counts=True)
    assert v.tolist() == [4161600.0, 6242400.0] and n.tolist() == [1580, 4]
    assert r["cand_index"][:4].tolist() == [38 * 48 + 46, 38 * 48 + 1, 48 + 46, 48 + 1]
    assert (np.diff(r["cand_index"][4:]) < 0).all()


def test_the_cap_keeps_the_first_candidates_in_row_major_order():
    full, r = dc.ref("cb2"), dc.ref("cb2", 100)
    assert r["status"] == fd_ref.DETECT_OVERFLOW and r["n_candidates"] == 1584 and len(r["cand_index"]) == 100
    assert sorted(r["cand_index"].tolist()) == sorted(full["cand_index"].tolist())[:100]
    assert dc.ref("cb2", 1584)["status"] == fd_ref.DETECT_OK


def _upper_half_mask():
    m = np.zeros((40, 48), np.uint8)
    m[:20] = 255
    return m


def test_distance_rules():
    img = dc.rectangle()
    # the two upper corners alone (the lower half is masked out) are 23 px apart: both at 23, one at 24
    r23 = fd_ref.detect(img, CAM, [], 10, 0.01, 23, _upper_half_mask())
    r24 = fd_ref.detect(img, CAM, [], 10, 0.01, 24, _upper_half_mask())
    assert r23["xy"].tolist() == [[35, 10], [12, 10]] and r24["xy"].tolist() == [[35, 10]] and r23["n_candidates"] == r24["n_candidates"] == 2
    # without the mask the lower corners rank first: they are 23 apart as well, and 19 from the upper ones
    assert dc.ref("rect_R23")["xy"].tolist() == [[35, 29], [12, 29]] and dc.ref("rect_R24")["xy"].tolist() == [[35, 29], [12, 10]]
    # an occupied point exactly R from a corner masks it ((12, 10) - (6, 2) = (6, 8): 10), one a little farther does not
    assert [12, 10] not in fd_ref.detect(img, CAM, [(6.0, 2.0)], 10, 0.01, 10)["xy"].tolist()
    assert [12, 10] in fd_ref.detect(img, CAM, [(6.0, 1.0)], 10, 0.01, 10)["xy"].tolist()


def test_scene_numbers():
    r = dc.ref("scene_48x40")
    assert (r["n_candidates"], r["n_new"]) == (60, 11)
    r = dc.ref("scene_200x192")
    assert (r["n_candidates"], r["n_new"]) == (1616, 50)


# ================================================================ CPU: layout and symbols
def test_fd_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "uvs_solver.h")).read()
    for s in FD_SYMBOLS:
        assert s + "(" in hdr, s
        assert s in uvs.api.EXPORTS, s
    assert "#define UVS_ABI_VERSION 7" in hdr
    L = uvs.api.lib()
    for s in FD_SYMBOLS:
        assert hasattr(L, s), s
    assert L.uvs_abi_version() == 7
    Hst = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
    for s in HOST_SYMBOLS:
        assert hasattr(Hst, s), s
    for m in ("set_max_candidates", "set_mask", "detect_raw", "detect", "debug_detect", "last_detect_device_ms"):
        assert callable(getattr(uvs.api.FeatureTracker, m)), m


def test_fd_struct_layout_matches_header():
    code = r'''
#include <stdio.h>
#include <stddef.h>
#include "uvs_solver.h"
int main(void) {
  printf("%zu %zu\n", sizeof(uvs_ft_detect_item), sizeof(uvs_ft_detect_result));
  printf("%zu %zu %zu %zu %zu\n", offsetof(uvs_ft_detect_item, stream), offsetof(uvs_ft_detect_item, n_occupied), offsetof(uvs_ft_detect_item, max_new),
         offsetof(uvs_ft_detect_item, reserved), offsetof(uvs_ft_detect_item, occupied_xy));
  printf("%zu %zu %zu %zu %zu %zu\n", offsetof(uvs_ft_detect_result, status), offsetof(uvs_ft_detect_result, n_new),
         offsetof(uvs_ft_detect_result, n_candidates), offsetof(uvs_ft_detect_result, reserved), offsetof(uvs_ft_detect_result, max_score),
         offsetof(uvs_ft_detect_result, threshold));
  printf("%d %d %d %d %d\n", UVS_FT_DEFAULT_CANDIDATES, UVS_FT_MAX_CANDIDATES, UVS_FT_MAX_MIN_DISTANCE, UVS_FT_DETECT_OK, UVS_FT_DETECT_OVERFLOW);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c"); exe = os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    I, R = abi.FtDetectItem, abi.FtDetectResult
    assert out[:2] == [C.sizeof(I), C.sizeof(R)]
    assert out[2:7] == [I.stream.offset, I.n_occupied.offset, I.max_new.offset, I.reserved.offset, I.occupied_xy.offset]
    assert out[7:13] == [R.status.offset, R.n_new.offset, R.n_candidates.offset, R.reserved.offset, R.max_score.offset, R.threshold.offset]
    assert out[13:] == [abi.FT_DEFAULT_CANDIDATES, abi.FT_MAX_CANDIDATES, abi.FT_MAX_MIN_DISTANCE, abi.FT_DETECT_OK, abi.FT_DETECT_OVERFLOW]
    assert out[13:] == [fd_ref.DEFAULT_CANDIDATES, fd_ref.MAX_CANDIDATES, fd_ref.MAX_MIN_DISTANCE, fd_ref.DETECT_OK, fd_ref.DETECT_OVERFLOW]


# ================================================================ host mirror
class HostTracker:
    """ctypes face of uvs::FeatureTracker behind feature_tracker_capi.cpp, with the entry points of the detection; device < 0: the bookkeeping
    alone."""

    def __init__(self, device, cam=CAM, max_width=752, max_height=480, levels=4, max_points=1024):
        self.L = L = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
        L.uvs_host_ft_create.restype = C.c_void_p
        L.uvs_host_ft_create.argtypes = [C.c_int, abi.c_double_p] + [C.c_int] * 4
        L.uvs_host_ft_destroy.argtypes = [C.c_void_p]; L.uvs_host_ft_destroy.restype = None
        L.uvs_host_ft_read_flow.argtypes = [C.c_void_p, C.c_double, C.c_int, abi.c_double_p, abi.c_i32_p, abi.c_double_p, C.c_int, abi.c_double_p]
        L.uvs_host_ft_apply_set_mask.argtypes = [C.c_void_p, C.c_double, C.c_int, abi.c_double_p, abi.c_i32_p, abi.c_double_p, C.c_int, C.c_int, abi.c_double_p]
        L.uvs_host_ft_set_detection.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double]
        L.uvs_host_ft_set_image_mask.argtypes = [C.c_void_p, abi.c_u8_p, C.c_int, C.c_int]
        L.uvs_host_ft_read_image_detect.argtypes = [C.c_void_p, abi.c_u8_p, C.c_int, C.c_int, C.c_double]
        L.uvs_host_ft_update_ids.argtypes = [C.c_void_p]
        L.uvs_host_ft_get.argtypes = [C.c_void_p, C.c_int, abi.c_double_p, abi.c_i32_p, abi.c_i32_p, abi.c_double_p, abi.c_double_p]
        c = np.array(list(cam) + [0.0] * (8 - len(cam)))
        self.h = L.uvs_host_ft_create(device, abi._dp(c), max_width, max_height, levels, max_points)
        assert self.h, "uvs_host_ft_create"

    def close(self):
        self.L.uvs_host_ft_destroy(self.h); self.h = None

    @staticmethod
    def _pts(a):
        a = np.ascontiguousarray(a, np.float64).reshape(-1, 2)
        return a, (abi._dp(a) if len(a) else None)

    def read_flow(self, time, next_xy, status, next_norm, new=(), min_dist=None):
        nx, pnx = self._pts(next_xy); nm, pnm = self._pts(next_norm); new, pn = self._pts(new)
        st = np.ascontiguousarray(status, np.int32)
        pst = st.ctypes.data_as(abi.c_i32_p) if len(st) else None
        if min_dist is None:
            return self.L.uvs_host_ft_read_flow(self.h, time, len(nx), pnx, pst, pnm, len(new), pn)
        return self.L.uvs_host_ft_apply_set_mask(self.h, time, len(nx), pnx, pst, pnm, int(min_dist), len(new), pn)

    def set_detection(self, max_cnt, min_dist, quality_level=0.01):
        return self.L.uvs_host_ft_set_detection(self.h, max_cnt, min_dist, quality_level)

    def set_image_mask(self, mask):
        if mask is None:
            return self.L.uvs_host_ft_set_image_mask(self.h, None, 0, 0)
        m = np.ascontiguousarray(mask, np.uint8)
        return self.L.uvs_host_ft_set_image_mask(self.h, m.ctypes.data_as(abi.c_u8_p), m.shape[1], m.shape[0])

    def read_image_detect(self, img, time):
        img = np.ascontiguousarray(img, np.uint8)
        return self.L.uvs_host_ft_read_image_detect(self.h, img.ctypes.data_as(abi.c_u8_p), img.shape[1], img.shape[0], time)

    def update_ids(self):
        return self.L.uvs_host_ft_update_ids(self.h)

    def get(self):
        n = self.L.uvs_host_ft_get(self.h, 0, None, None, None, None, None)
        o = dict(cur_pts=np.zeros((n, 2)), ids=np.zeros(n, np.int32), track_cnt=np.zeros(n, np.int32), cur_un_pts=np.zeros((n, 2)), pts_velocity=np.zeros((n, 2)))
        if n:
            self.L.uvs_host_ft_get(self.h, n, abi._dp(o["cur_pts"]), o["ids"].ctypes.data_as(abi.c_i32_p), o["track_cnt"].ctypes.data_as(abi.c_i32_p),
                                   abi._dp(o["cur_un_pts"]), abi._dp(o["pts_velocity"]))
        return o


def test_host_mirror_set_mask_by_hand():
    """setMask without a device: the order by track_cnt, its stability on ties, a point within R of a longer-tracked one dropped, and ids, counts
    and normalized points permuted together."""
    T = ft_ref.TRACKED
    t = HostTracker(-1)
    a = np.array([[10.0, 10.0], [100.0, 100.0]])
    assert t.read_flow(0.0, [], [], [], new=a) == 0 and t.update_ids() == 2               # ids 0, 1: the oldest
    b = np.array([[13.4, 14.4], [50.0, 50.0]])                                           # rint (13, 14): (3, 4) from (10, 10), exactly 5
    assert t.read_flow(0.1, a, [T, T], kf_ref.lift(CAM, a), new=b) == 0 and t.update_ids() == 4
    c = np.array([[200.0, 50.0], [53.0, 54.5], [16.0, 10.0]])                            # (53, 54) is 5 from (50, 50); (16, 10) is 6 from (10, 10)
    cur = np.concatenate([a, b])
    assert t.read_flow(0.2, cur, [T] * 4, kf_ref.lift(CAM, cur), new=c) == 0 and t.update_ids() == 7
    g = t.get()
    assert g["track_cnt"].tolist() == [3, 3, 2, 2, 1, 1, 1] and g["ids"].tolist() == list(range(7))
    # the frame under test: the counts become 4 4 3 3 2 2 2
    cur = g["cur_pts"]; nrm = kf_ref.lift(CAM, cur) + 1e-3 * np.arange(7)[:, None]         # marked per point: the permutation is visible
    assert t.read_flow(0.3, cur, [T] * 7, nrm, new=[(300.0, 300.0)], min_dist=5) == 0
    g = t.get()
    # id 2 (13.4, 14.4) is within 5 of id 0 and dropped (<=); id 5 (53, 54.5) -> rint (53, 54): 5 from id 3, dropped; id 6 is 6 away, kept;
    # ties keep their order (0 before 1, 3 alone, 4 before 6): a stable sort
    assert g["ids"].tolist() == [0, 1, 3, 4, 6, -1] and g["track_cnt"].tolist() == [4, 4, 3, 2, 2, 1]
    keep = [0, 1, 3, 4, 6]
    assert np.array_equal(g["cur_pts"][:5], cur[keep]) and np.array_equal(bits(g["cur_un_pts"][:5]), bits(nrm[keep]))
    want = fd_ref.set_mask(cur, np.arange(7), [4, 4, 3, 3, 2, 2, 2], nrm, 5)
    assert want[1].tolist() == keep and np.array_equal(want[0], cur[keep]) and want[2].tolist() == [4, 4, 3, 2, 2]
    t.close()


def test_set_mask_orders_by_track_count():
    """The book's vectors are oldest first by construction (new points are appended, reduceVector and setMask keep the order), so the ordering
    itself shows only on vectors given in another order: the numpy setMask, which the chained GPU test holds the mirror to."""
    pts = np.array([[5.0, 5.0], [50.0, 50.0], [90.0, 90.0], [52.0, 50.0], [5.0, 7.5]])
    nrm = kf_ref.lift(CAM, pts)
    got = fd_ref.set_mask(pts, [7, 8, 9, 10, 11], [1, 2, 5, 3, 1], nrm, 2)
    # id 8 is 2 from the longer-tracked id 10: dropped; id 11 -> rint (5, 8), 3 from id 7: kept, after it (a tie keeps the order given)
    assert got[1].tolist() == [9, 10, 7, 11] and got[2].tolist() == [5, 3, 1, 1]
    assert np.array_equal(got[0], pts[[2, 3, 0, 4]]) and np.array_equal(bits(got[3]), bits(nrm[[2, 3, 0, 4]]))
    assert fd_ref.set_mask(pts, [7, 8, 9, 10, 11], [1, 2, 5, 3, 1], nrm, 3)[1].tolist() == [9, 10, 7]


# ================================================================ GPU
def _tracker(**kw):
    kw.setdefault("max_width", 1100); kw.setdefault("max_height", 200); kw.setdefault("max_streams", 4); kw.setdefault("max_points", 256)
    kw.setdefault("levels", 1)
    return uvs.api.FeatureTracker(**kw)


def _load(ft, img, stream=0):
    ft.reset(stream)
    ft.track([dict(stream=stream, image=img)], CAM)


def _assert_outputs(got, want, what=""):
    assert (got["n_new"], got["n_candidates"], got["status"]) == (want["n_new"], want["n_candidates"], want["status"]), (what, got["n_new"], got["n_candidates"])
    assert np.array_equal(bits([got["max_score"], got["threshold"]]), bits([want["max_score"], want["threshold"]])), what
    assert np.array_equal(got["xy"], want["xy"]), (what, got["xy"][:5], want["xy"][:5])
    assert np.array_equal(bits(got["score"]), bits(want["score"])) and np.array_equal(bits(got["norm"]), bits(want["norm"])), what


def _assert_debug(got, want, what=""):
    bad = np.argwhere(bits(got["score_map"]) != bits(want["score_map"]))
    assert len(bad) == 0, (what, len(bad), [(int(y), int(x), got["score_map"][y, x], want["score_map"][y, x]) for y, x in bad[:6]])
    bad = np.argwhere(got["allowed"] != want["allowed"])
    assert len(bad) == 0, (what, len(bad), bad[:6].tolist())
    assert np.array_equal(got["cand_index"], want["cand_index"]), what
    assert np.array_equal(bits(got["cand_score"]), bits(want["cand_score"])), what
    _assert_outputs(got, want, what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_gpu_debug_detect_equals_the_restatement_value_by_value(name):
    c = dc.case(name)
    ft = _tracker(max_streams=2)
    _load(ft, c["image"], 1)
    item = dict(stream=1, occupied=c["occupied"], max_new=c["max_new"])
    if c["mask"] is not None:
        ft.set_mask(1, c["mask"])
        _assert_debug(ft.debug_detect(item, CAM, c["image"].shape, 0.01, c["R"]), dc.ref(name), name + " masked")
        assert not dc.ref(name)["allowed"][c["mask"] == 0].any()
        ft.set_mask(1, None)                                    # cleared: the same call without it
    _assert_debug(ft.debug_detect(item, CAM, c["image"].shape, 0.01, c["R"]), dc.ref(name, with_mask=False), name)
    ft.close()


@pytest.mark.gpu
def test_gpu_detect_known_answers_and_distance_rules():
    ft = _tracker(max_width=64, max_height=64, max_streams=1)
    for name in ("rect", "rect_occupied", "rect_two", "rect_none_allowed", "rect_R23", "rect_R24", "cb1", "cb2", "scene_48x40"):
        c = dc.case(name)
        _load(ft, c["image"])
        got = ft.detect([dict(stream=0, occupied=c["occupied"], max_new=c["max_new"])], CAM, 0.01, c["R"])[0]
        _assert_outputs(got, dc.ref(name), name)
    _load(ft, dc.rectangle())
    r = ft.detect([dict(stream=0, max_new=10)], CAM, 0.01, 8)[0]
    assert r["xy"].tolist() == [[35, 29], [12, 29], [35, 10], [12, 10]] and r["n_candidates"] == 4 and r["max_score"] == 1620000.0
    none = ft.detect([dict(stream=0, occupied=[(24.0, 20.0)], max_new=10)], CAM, 0.01, 60)[0]
    assert (none["n_new"], none["n_candidates"], none["max_score"], none["threshold"]) == (0, 0, 0.0, 0.0)
    ft.set_mask(0, _upper_half_mask())                          # the two upper corners, 23 px apart
    assert ft.detect([dict(stream=0, max_new=10)], CAM, 0.01, 23)[0]["xy"].tolist() == [[35, 10], [12, 10]]
    assert ft.detect([dict(stream=0, max_new=10)], CAM, 0.01, 24)[0]["xy"].tolist() == [[35, 10]]
    ft.reset(0)                                                 # the reset drops the mask with the image
    ft.track([dict(stream=0, image=dc.rectangle())], CAM)
    assert ft.detect([dict(stream=0, max_new=10)], CAM, 0.01, 23)[0]["xy"].tolist() == [[35, 29], [12, 29]]
    assert [12, 10] not in ft.detect([dict(stream=0, occupied=[(6.0, 2.0)], max_new=10)], CAM, 0.01, 10)[0]["xy"].tolist()
    assert [12, 10] in ft.detect([dict(stream=0, occupied=[(6.0, 1.0)], max_new=10)], CAM, 0.01, 10)[0]["xy"].tolist()
    ft.close()


@pytest.mark.gpu
def test_gpu_max_new_counts_and_no_occupied_points():
    c = dc.case("scene_200x192")
    ft = _tracker(max_points=64, max_streams=1)
    _load(ft, c["image"])
    for max_new in (0, 1, 64):                                  # 64 = max_points
        got = ft.detect([dict(stream=0, occupied=c["occupied"], max_new=max_new)], CAM, 0.01, c["R"])[0]
        want = dc.ref("scene_200x192", max_new=max_new)
        _assert_outputs(got, want, max_new)
        assert got["n_new"] == max_new and got["n_candidates"] == 1616
    got = ft.detect([dict(stream=0, max_new=50)], CAM, 0.01, c["R"])[0]
    _assert_outputs(got, fd_ref.detect(c["image"], CAM, [], 50, 0.01, c["R"]), "no occupied points")
    assert ft.last_detect_device_ms() > 0.0
    ft.close()


@pytest.mark.gpu
def test_gpu_overflow_of_the_candidate_cap():
    c = dc.case("cb2")
    ft = _tracker(max_width=64, max_height=64, max_streams=1)
    _load(ft, c["image"])
    ft.set_max_candidates(100)
    item = dict(stream=0, max_new=c["max_new"])
    want = dc.ref("cb2", 100)
    got = ft.debug_detect(item, CAM, c["image"].shape, 0.01, c["R"])
    assert got["status"] == abi.FT_DETECT_OVERFLOW and got["n_candidates"] == 1584 and len(got["cand_index"]) == 100
    _assert_debug(got, want, "overflow")
    _assert_outputs(ft.detect([item], CAM, 0.01, c["R"])[0], want, "overflow")
    ft.set_max_candidates(1584)                                 # exactly enough
    _assert_outputs(ft.detect([item], CAM, 0.01, c["R"])[0], dc.ref("cb2"), "exact")
    ft.set_max_candidates(abi.FT_DEFAULT_CANDIDATES)
    _assert_outputs(ft.detect([item], CAM, 0.01, c["R"])[0], dc.ref("cb2"), "default")
    ft.close()


@pytest.mark.gpu
def test_gpu_a_batch_equals_its_items_one_at_a_time_and_a_second_run():
    names = ["scene_200x192", "scene_131x97_edges_mask", "scene_48x40", "wide_1030x192"]
    cs = [dc.case(n) for n in names]
    ft, solo = _tracker(), _tracker()
    for k, c in enumerate(cs):
        _load(ft, c["image"], k); _load(solo, c["image"], k)
    items = [dict(stream=k, occupied=c["occupied"], max_new=c["max_new"]) for k, c in enumerate(cs)]
    R = 10
    batch = ft.detect(items, CAM, 0.01, R)
    for k in (2, 0, 3, 1):
        _assert_outputs(batch[k], solo.detect([items[k]], CAM, 0.01, R)[0], names[k])
        c = cs[k]
        _assert_outputs(batch[k], fd_ref.detect(c["image"], CAM, c["occupied"], c["max_new"], 0.01, R), names[k])
    again = ft.detect(items, CAM, 0.01, R)
    for k in range(4):
        _assert_outputs(again[k], batch[k], "run against run")
    ft.close(); solo.close()


@pytest.mark.gpu
def test_gpu_detection_sees_the_slots_last_image_and_leaves_the_pyramid_alone():
    imgs = fc.sequence()
    pts = fc.grid_points(10, 131, 97)
    seq = fc.ref_sequence(imgs, pts, 3)
    ft, plain = _tracker(levels=3, max_streams=1), _tracker(levels=3, max_streams=1)
    for t in (ft, plain):
        t.track([dict(stream=0, image=imgs[0])], CAM)
    a = ft.track([dict(stream=0, image=imgs[1], points=pts)], CAM)[0]
    plain.track([dict(stream=0, image=imgs[1], points=pts)], CAM)
    occ = a["next_xy"][a["status"] == 0]
    got = ft.detect([dict(stream=0, occupied=occ, max_new=40)], CAM, 0.01, 8)[0]
    _assert_outputs(got, fd_ref.detect(imgs[1], CAM, occ, 40, 0.01, 8), "after A -> B: B")
    assert got["n_new"] > 0 and not np.array_equal(got["xy"], fd_ref.detect(imgs[0], CAM, occ, 40, 0.01, 8)["xy"])
    pyr = ft.debug_pyramid(0)
    for l, lvl in enumerate(ft_ref.pyramid(imgs[1], 3)):
        assert np.array_equal(pyr[l], lvl)
    c = ft.track([dict(stream=0, image=imgs[2], points=occ)], CAM)[0]
    d = plain.track([dict(stream=0, image=imgs[2], points=occ)], CAM)[0]
    for k in ("status", "iterations"):
        assert np.array_equal(c[k], d[k]) and np.array_equal(c[k], seq[1][k])
    for k in ("next_xy", "next_norm"):
        assert np.array_equal(bits(c[k]), bits(d[k])) and np.array_equal(bits(c[k]), bits(seq[1][k]))
    ft.close(); plain.close()


@pytest.mark.gpu
def test_gpu_detect_argument_checks_leave_the_handle_usable():
    c = dc.case("scene_48x40")
    ft = _tracker(max_width=64, max_height=64, max_streams=2, max_points=20)
    INV, CAP = abi.UVS_ERR_INVALID_ARG, abi.UVS_ERR_CAPACITY
    ok = lambda **kw: dict(stream=0, max_new=5, **kw)
    assert ft.detect_raw([ok()], CAM)[0] == INV and "holds no image" in ft.last_error()      # nothing stored yet
    with pytest.raises(RuntimeError):
        ft.set_mask(0, np.ones((40, 48), np.uint8))                                           # ... so no mask either
    _load(ft, c["image"])
    bad = [
        (dict(items=[ok()], null=("items",)), INV), (dict(items=[ok()], null=("camera",)), INV), (dict(items=[ok()], null=("new_xy",)), INV),
        (dict(items=[ok()], null=("new_score",)), INV), (dict(items=[ok()], null=("new_norm",)), INV), (dict(items=[ok()], null=("results",)), INV),
        (dict(items=[ok()], n_items=0), INV), (dict(items=[ok(), ok()]), INV),                 # a stream given twice
        (dict(items=[dict(stream=2, max_new=5)]), INV), (dict(items=[dict(stream=-1, max_new=5)]), INV),
        (dict(items=[dict(stream=1, max_new=5)]), INV),                                       # a slot that holds nothing
        (dict(items=[dict(stream=0, max_new=-1)]), INV), (dict(items=[ok(n_occupied=-1)]), INV),
        (dict(items=[ok(n_occupied=3)]), INV),                                                # a null array behind a positive count
        (dict(items=[ok(occupied=[(1.0, np.nan)])]), INV), (dict(items=[ok(occupied=[(np.inf, 1.0)])]), INV),
        (dict(items=[ok(occupied=[(1.0, 1.0e6 + 1)])]), INV),
        (dict(items=[ok()], quality_level=0.0), INV), (dict(items=[ok()], quality_level=1.5), INV), (dict(items=[ok()], quality_level=np.nan), INV),
        (dict(items=[ok()], min_distance=0), INV), (dict(items=[ok()], min_distance=abi.FT_MAX_MIN_DISTANCE + 1), INV),
        (dict(items=[ok(occupied=np.zeros((21, 2)))]), CAP), (dict(items=[dict(stream=0, max_new=21)]), CAP),
        (dict(items=[ok(), dict(stream=1, max_new=5), dict(stream=1, max_new=5)]), CAP),       # more items than slots
    ]
    for kw, want in bad:
        items = kw.pop("items")
        rc, out = ft.detect_raw(items, CAM, **kw)
        assert rc == want and out == [] and (kw.get("null") == ("items",) or ft.last_error()), (kw, rc, ft.last_error())
    for cam in ((np.nan, 460.0, 376.0, 240.0), (0.0, 460.0, 376.0, 240.0), (460.0, -1.0, 376.0, 240.0)):
        assert ft.detect_raw([ok()], cam)[0] == INV
    for m in (np.ones((40, 47), np.uint8), np.ones((41, 48), np.uint8)):                      # a mask whose size is not the slot's
        with pytest.raises(RuntimeError):
            ft.set_mask(0, m)
    with pytest.raises(RuntimeError):
        ft.set_mask(2, None)
    for n in (0, -3, abi.FT_MAX_CANDIDATES + 1):
        with pytest.raises(RuntimeError):
            ft.set_max_candidates(n)
    with pytest.raises(RuntimeError):
        ft.debug_detect(dict(stream=1, max_new=5), CAM, (40, 48))
    assert ft.detect_raw([ok()], CAM, quality_level=1.0, min_distance=abi.FT_MAX_MIN_DISTANCE)[0] == 0      # the ends of the ranges
    # no rejected call changed anything: the handle detects (no mask, the default cap) and tracks
    got = ft.detect([dict(stream=0, occupied=c["occupied"], max_new=20)], CAM, 0.01, c["R"])[0]      # max_points
    _assert_outputs(got, dc.ref("scene_48x40", max_new=20))
    s = fc.scene("shift_48x40_L1")
    trk = ft.track([dict(stream=0, image=s["next"], points=s["pts"][:20])], CAM)[0]
    want = ft_ref.track_images(s["prev"], s["next"], s["pts"][:20], 1, CAM)
    assert np.array_equal(trk["status"], want["status"]) and np.array_equal(bits(trk["next_xy"]), bits(want["next_xy"]))
    ft.close()


def _mirror_reference(imgs, times, levels, max_cnt, min_dist):
    """readImage with the tracker's own detection, replayed with ft_ref + fd_ref + the numpy setMask; update_ids after every frame.
    -> [dict(cur_pts, ids, track_cnt, cur_un_pts, pts_velocity) per frame, after update_ids], [n_new per frame]."""
    pts = np.zeros((0, 2)); ids = np.zeros(0, int); cnt = np.zeros(0, int)
    prev_map, n_id, out, added = {}, 0, [], []
    for k, img in enumerate(imgs):
        norm = np.zeros((0, 2))
        if len(pts):
            r = ft_ref.track_images(imgs[k - 1], img, pts, levels, CAM)
            ok = r["status"] == ft_ref.TRACKED
            pts, ids, cnt, norm = r["next_xy"][ok], ids[ok], cnt[ok], r["next_norm"][ok]
        cnt = cnt + 1
        pts, ids, cnt, norm = fd_ref.set_mask(pts, ids, cnt, norm, min_dist)
        n_new = 0
        if max_cnt - len(pts) > 0:
            d = fd_ref.detect(img, CAM, pts, max_cnt - len(pts), 0.01, min_dist)
            n_new = d["n_new"]
            pts = np.concatenate([pts, d["xy"].astype(np.float64)]); norm = np.concatenate([norm, d["norm"]])
            ids = np.concatenate([ids, -np.ones(n_new, int)]); cnt = np.concatenate([cnt, np.ones(n_new, int)])
        added.append(n_new)
        cur_map = {}
        for i, m in zip(ids, norm):
            cur_map.setdefault(int(i), m)                       # std::map::insert keeps the first entry of a key
        vel = np.zeros((len(pts), 2))
        if prev_map:
            dt = np.float64(times[k]) - np.float64(times[k - 1])
            for j, (i, m) in enumerate(zip(ids, norm)):
                if i != -1 and int(i) in prev_map:
                    vel[j] = (m - prev_map[int(i)]) / dt
        prev_map = cur_map
        ids = ids.copy()
        for j in range(len(ids)):
            if ids[j] == -1:
                ids[j] = n_id; n_id += 1
        out.append(dict(cur_pts=pts.copy(), ids=ids.copy(), track_cnt=cnt.copy(), cur_un_pts=norm.copy(), pts_velocity=vel))
    return out, added


@pytest.mark.gpu
def test_gpu_host_mirror_detects_tracks_and_replenishes():
    """Three rendered frames through uvs::FeatureTracker::readImage with max_cnt = 50 and no Detector: the first frame detects 50 points, the
    following ones track them, order and thin them with setMask and top the count back up, bit for bit."""
    imgs = fc.sequence()
    times = [10.0, 10.05, 10.125]
    want, added = _mirror_reference(imgs, times, 3, 50, 8)
    assert added[0] == 50 and added[1] > 0 and len(want[1]["ids"]) == 50 and want[1]["track_cnt"].max() == 2      # lost points were replaced
    t = HostTracker(0, max_width=131, max_height=97, levels=3, max_points=128)
    assert t.set_detection(50, 8, 0.01) == 0
    for k, img in enumerate(imgs):
        assert t.read_image_detect(img, times[k]) == 0
        t.update_ids()
        g = t.get()
        w = want[k]
        assert g["ids"].tolist() == w["ids"].tolist() and g["track_cnt"].tolist() == w["track_cnt"].tolist(), k
        for key in ("cur_pts", "cur_un_pts", "pts_velocity"):
            assert np.array_equal(bits(g[key]), bits(w[key])), (k, key)
    assert want[2]["pts_velocity"].any()
    t.close()


@pytest.mark.gpu
def test_gpu_host_mirror_image_mask():
    """The fisheye mask of the mirror reaches the device with the next image: no new point where it is zero."""
    img = fc.sequence()[0]
    mask = np.zeros(img.shape, np.uint8); mask[:, 60:] = 255
    t = HostTracker(0, max_width=131, max_height=97, levels=3, max_points=128)
    assert t.set_detection(30, 8, 0.01) == 0 and t.set_image_mask(mask) == 0
    assert t.read_image_detect(img, 1.0) == 0
    g = t.get()
    want = fd_ref.detect(img, CAM, [], 30, 0.01, 8, mask)
    assert np.array_equal(g["cur_pts"], want["xy"].astype(np.float64)) and g["cur_pts"][:, 0].min() >= 60 and len(g["cur_pts"]) == 30
    t.close()
