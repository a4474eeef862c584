"""Outlier rejection of the point front end (uvs_ft_reject; csrc/uvs_feature_reject.hip): a fundamental-matrix RANSAC over 7-point samples on
the normalized tracks of a frame -- the reference's rejectWithF (feature_tracker.cpp:149-182) on the GPU, against the numpy restatement
tests/fr_ref.py.

CPU tests pin fr_ref itself (one hypothesis against a scalar Python loop, the draw against lc_ref's, a known essential matrix, the residual of
every model on its own sample, the replay of the stopping rule by hand, the outcomes, what it keeps and drops on the scenes), the ctypes layouts
and the symbols, and the host mirror's applyReject without a device.  GPU tests compare the device with fr_ref EXACTLY: integers with ==, every
FP64 value bit for bit; there is no tolerance in them.  One excuse, stated as a condition: `iterations` may differ where num / denom of
RANSACUpdateNumIters lies within 1e-9 of a half-integer, the log being the library's; test_no_committed_case_is_near_a_rounding_tie asserts
that no committed case does, so the excused share is 0."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import fr_cases as rc
import fr_ref
import ft_cases as fc
import ft_ref
import kf_ref
import lc_ref
from helpers import abi, uvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FR_SYMBOLS = ["uvs_ft_reject", "uvs_ft_last_reject_device_ms", "uvs_ft_debug_reject"]
HOST_SYMBOLS = ["uvs_host_ft_set_rejection", "uvs_host_ft_apply_reject", "uvs_host_ft_last_reject"]
CAM = fc.CAM
THR, CONF = rc.THRESHOLD, rc.CONFIDENCE
ALL = sorted(rc.CASES)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ================================================================ CPU: the restatement
def _hypothesis_scalar(prev, nxt, idx, threshold):
    """The rule of include/uvs_solver.h for ONE sample in Python floats, entry by entry: -> (models [[9 floats]], counts) or None (invalid)."""
    A = []
    for i in idx:
        x1, y1 = float(prev[i][0]), float(prev[i][1]); x2, y2 = float(nxt[i][0]), float(nxt[i][1])
        A.append([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0])
    rows, cols, piv, first = list(range(7)), list(range(9)), [], 0.0
    for k in range(7):
        best, pr, pc = -1.0, 0, 0
        for r in rows:
            for c in cols:
                if abs(A[r][c]) > best:
                    best, pr, pc = abs(A[r][c]), r, c
        p = A[pr][pc]
        if k == 0:
            first = abs(p)
        if not abs(p) > 1e-10 * first:
            return None
        rows.remove(pr); cols.remove(pc); piv.append((pr, pc))
        for c in cols:
            A[pr][c] = A[pr][c] / p
        for r in range(7):
            if r != pr:
                f = A[r][pc]
                for c in cols:
                    A[r][c] = A[r][c] - f * A[pr][c]
    c1, c2 = cols
    F1, F2 = [0.0] * 9, [0.0] * 9
    for pr, pc in piv:
        F1[pc] = -A[pr][c1]; F2[pc] = -A[pr][c2]
    F1[c1], F1[c2], F2[c1], F2[c2] = 1.0, 0.0, 0.0, 1.0

    def det3(u, v, w):
        return (u[0] * (v[1] * w[2] - v[2] * w[1]) - u[1] * (v[0] * w[2] - v[2] * w[0])) + u[2] * (v[0] * w[1] - v[1] * w[0])
    a = [[F1[j], F1[3 + j], F1[6 + j]] for j in range(3)]; b = [[F2[j], F2[3 + j], F2[6 + j]] for j in range(3)]
    c0 = det3(a[0], a[1], a[2])
    k1 = (det3(b[0], a[1], a[2]) + det3(a[0], b[1], a[2])) + det3(a[0], a[1], b[2])
    k2 = (det3(b[0], b[1], a[2]) + det3(b[0], a[1], b[2])) + det3(a[0], b[1], b[2])
    c3 = det3(b[0], b[1], b[2])
    if not all(math.isfinite(v) for v in (c0, k1, k2, c3)) or c3 == 0.0:
        return None
    R = 1.0 + max(abs(c0), abs(k1), abs(k2)) / abs(c3)
    if not math.isfinite(R):
        return None
    poly = lambda x: ((c3 * x + k2) * x + k1) * x + c0
    D = k2 * k2 - (3.0 * c3) * k1
    if D > 0.0:
        s = math.sqrt(D)
        e1 = min(max((-k2 - s) / (3.0 * c3), -R), R); e2 = min(max((-k2 + s) / (3.0 * c3), -R), R)
        lo, hi = min(e1, e2), max(e1, e2)
        intervals = [(-R, lo), (lo, hi), (hi, R)]
    else:
        intervals = [(-R, R)]
    lams = []
    for lo_, hi_ in intervals:
        fa, fb = poly(lo_), poly(hi_)
        up = fa <= 0.0 and fb > 0.0
        if not (up or (fa >= 0.0 and fb < 0.0)):
            continue
        x0, x1 = lo_, hi_
        for _ in range(60):
            m = 0.5 * x0 + 0.5 * x1
            fm = poly(m)
            if (fm > 0.0) if up else (fm < 0.0):
                x1 = m
            else:
                x0 = m
        x = 0.5 * x0 + 0.5 * x1
        for _ in range(4):
            xn = x - poly(x) / (((3.0 * c3) * x + 2.0 * k2) * x + k1)
            if x0 <= xn <= x1:
                x = xn
        lams.append(x)
    models, counts = [], []
    t2 = threshold * threshold
    for lam in lams:
        F = [F1[j] + lam * F2[j] for j in range(9)]
        n_in = 0
        for i in range(len(prev)):
            x1, y1 = float(prev[i][0]), float(prev[i][1]); x2, y2 = float(nxt[i][0]), float(nxt[i][1])
            a_ = (F[0] * x1 + F[1] * y1) + F[2]; b_ = (F[3] * x1 + F[4] * y1) + F[5]; c_ = (F[6] * x1 + F[7] * y1) + F[8]
            s2 = (x2 * a_ + y2 * b_) + c_
            d2 = s2 * s2 / (a_ * a_ + b_ * b_)
            a_ = (F[0] * x2 + F[3] * y2) + F[6]; b_ = (F[1] * x2 + F[4] * y2) + F[7]; c_ = (F[2] * x2 + F[5] * y2) + F[8]
            s1 = (x1 * a_ + y1 * b_) + c_
            d1 = s1 * s1 / (a_ * a_ + b_ * b_)
            n_in += d1 <= t2 and d2 <= t2
        models.append(F); counts.append(n_in)
    return models, counts


@pytest.mark.parametrize("name", ["general_12", "forward_40", "general_150_o20", "rotation_150"])
def test_fr_ref_equals_a_scalar_restatement_of_one_hypothesis(name):
    """Elimination, cubic, roots and error of 40 hypotheses per case, bit for bit."""
    sc, r = rc.case(name), rc.ref(name)
    seen = set()
    for h in range(0, 1000, 25):
        got = _hypothesis_scalar(sc["prev"], sc["next"], r["samples"][h].tolist(), THR)
        assert got is not None and r["counts"][h, 0] >= 0, h
        models, counts = got
        seen.add(len(models))
        assert counts == [int(c) for c in r["counts"][h] if c >= 0], h
        assert np.array_equal(bits(models), bits(r["models"][h, :len(models)])) and not r["models"][h, len(models):].any(), h
    assert seen == {1, 3}                                      # both shapes of the cubic were met
    rest = rc.case("rest_150")
    assert _hypothesis_scalar(rest["prev"], rest["next"], rc.ref("rest_150")["samples"][0].tolist(), THR) is None


def test_the_draw_is_the_generator_of_loop_verification_with_seven(monkeypatch):
    monkeypatch.setattr(lc_ref, "MODEL_POINTS", 7)
    for seed, n in ((1, 8), (12345, 9), (2 ** 63 + 11, 150), (7, 7), (3, 5000)):
        for h in (0, 1, 17, 999):
            assert fr_ref.draw(seed, h, n) == lc_ref.draw(seed, h, n), (seed, n, h)
    assert fr_ref.draw(5, 0, 6) is None and lc_ref.draw(5, 0, 6) is None      # 7 distinct indices of 6 do not exist
    d = fr_ref.draw(1, 0, 8)
    assert len(set(d)) == 7 and all(0 <= v < 8 for v in d)
    S = fr_ref.samples(1008, 8)
    assert (S >= 0).all() and all(len(set(row)) == 7 for row in S.tolist())


def _unit(F):
    F = np.asarray(F, np.float64).ravel()
    return F / np.sqrt((F * F).sum())


def _distance_to(E, F):
    e, f = _unit(E), _unit(F)
    return min(np.abs(f - e).max(), np.abs(f + e).max())


# what fr_ref measures on the committed scenes (printed by the tests below); the bounds are twice these
KNOWN_ANSWER_ERROR = {"general_150": 5.9e-11, "forward_150_o20": 3.4e-12}
OWN_SAMPLE_RESIDUAL_PX = 2.6e-9


@pytest.mark.parametrize("name", sorted(KNOWN_ANSWER_ERROR))
def test_seven_exact_correspondences_of_a_known_essential_matrix(name):
    """Noise-free scene: every sample of true correspondences has the true E (up to scale and sign, unit Frobenius norm, largest entry difference)
    among its roots.  The bound is twice what fr_ref itself measures here (recorded in DESIGN.md 3.12)."""
    sc, r = rc.case(name), rc.ref(name)
    worst, n_samples = 0.0, 0
    for h in range(1000):
        if sc["outlier"][r["samples"][h]].any():
            continue
        assert r["counts"][h, 0] >= 0, h                       # an all-inlier sample is never invalid
        n_samples += 1
        worst = max(worst, min(_distance_to(sc["E"], r["models"][h, k]) for k in range(3) if r["counts"][h, k] >= 0))
    print(f"{name}: worst distance of the best root to the true E over {n_samples} samples: {worst:.3g}")
    assert n_samples >= 150 and worst <= 2 * KNOWN_ANSWER_ERROR[name]


def test_every_model_fits_its_own_sample():
    """sqrt(max(d1, d2)) of every model on its seven tracks, in pixels at focal length 460; the bound is twice fr_ref's worst over the committed
    scenes.  Every model is singular: |det| of the unit-norm F is at rounding level."""
    worst, worst_det = 0.0, 0.0
    for name in ALL:
        sc, r = rc.case(name), rc.ref(name)
        for h in range(1000):
            for k in range(3):
                if r["counts"][h, k] < 0:
                    continue
                idx = r["samples"][h]
                d1, d2 = fr_ref.errors(r["models"][h, k], sc["prev"][idx], sc["next"][idx])
                worst = max(worst, float(np.sqrt(max(d1.max(), d2.max()))) * rc.FOCAL)
                worst_det = max(worst_det, abs(np.linalg.det(_unit(r["models"][h, k]).reshape(3, 3))))
    print(f"worst residual of a model on its own sample: {worst:.3g} px; worst |det| of a unit-norm model: {worst_det:.3g}")
    assert worst <= 2 * OWN_SAMPLE_RESIDUAL_PX and worst_det < 1e-12


@pytest.mark.parametrize("name", ALL)
def test_the_mask_of_a_model_has_as_many_ones_as_its_count(name):
    sc, r = rc.case(name), rc.ref(name)
    assert int(r["keep"].sum()) == r["n_inliers"]
    if r["status"] == fr_ref.OK:
        assert r["n_inliers"] == r["counts"][r["hypothesis"], r["root"]]
        assert np.array_equal(r["keep"], fr_ref.inliers(r["models"][r["hypothesis"], r["root"]], sc["prev"], sc["next"], THR).astype(np.uint8))
        F = r["F"]
        assert np.abs(F).max() == 1.0 and 1.0 in F.tolist()


def test_the_replay_of_the_stopping_rule_by_hand():
    """RANSACUpdateNumIters(0.99, ep, 7, 1000): log(0.01) / log(1 - (1 - ep)^7) = 587.2, 162.2, 7.08, 3.84 for ep = 0.5, 0.4, 0.1, 0.05."""
    assert [fr_ref.update_num_iters(0.99, e, 1000) for e in (0.5, 0.4, 0.1, 0.05, 0.0)] == [587, 162, 7, 4, 0]
    assert fr_ref.update_num_iters(0.99, 0.5, 300) == 300                      # never above the budget it is given
    assert round(math.log(0.01) / math.log(1 - 0.5 ** 7), 1) == 587.2
    c = -np.ones((1000, 3), int)
    assert fr_ref.select(c, 100, 0.99) == (-1, -1, 0, 1000)                     # no model at all: the whole budget is examined
    c[1] = [5, 6, -1]                                                          # 6 inliers are not more than 6
    assert fr_ref.select(c, 100, 0.99) == (-1, -1, 0, 1000)
    c[2] = [50, 40, -1]                                                        # 50 -> 587 iterations; the second root is no better
    assert fr_ref.select(c, 100, 0.99) == (2, 0, 50, 587)
    c[3] = [50, 60, 90]                                                        # 50 is not more than 50; 60 -> 162; 90 -> 7
    assert fr_ref.select(c, 100, 0.99) == (3, 2, 90, 7)
    c[5] = [95, -1, -1]                                                        # -> 4 < 6: the loop ends after h = 5
    assert fr_ref.select(c, 100, 0.99) == (5, 0, 95, 6)
    c[7] = [99, -1, -1]                                                        # never examined
    assert fr_ref.select(c, 100, 0.99) == (5, 0, 95, 6)
    c = -np.ones((1000, 3), int); c[4] = [100, -1, -1]                         # every track an inlier: niters = 0
    assert fr_ref.select(c, 100, 0.99) == (4, 0, 100, 5)
    c = -np.ones((1000, 3), int); c[999] = [7, 8, -1]                          # the last hypothesis still counts, and both its roots in turn
    assert fr_ref.select(c, 100, 0.99) == (999, 1, 8, 1000)


def test_no_committed_case_is_near_a_rounding_tie():
    """The condition of the one excuse: no num / denom of the stopping rule within 1e-9 of a half-integer, in any committed case (the mirror
    test's frames assert the same of theirs)."""
    for name in ALL:
        assert rc.ref(name)["half_margin"] > 1e-9, name


def test_outcomes_skipped_and_no_model():
    sc = rc.case("general_150")
    r = fr_ref.reject(sc["prev"][:7], sc["next"][:7], 1, THR)
    assert r["status"] == fr_ref.SKIPPED and r["keep"].tolist() == [1] * 7 and (r["n_inliers"], r["hypothesis"], r["root"], r["iterations"]) == (7, -1, -1, 0)
    assert fr_ref.reject(sc["prev"][:0], sc["next"][:0], 1, THR)["status"] == fr_ref.SKIPPED
    assert fr_ref.reject(sc["prev"][:8], sc["next"][:8], 1, THR)["status"] == fr_ref.OK
    rest = rc.case("rest_150"); r = rc.ref("rest_150")
    assert np.array_equal(bits(rest["prev"]), bits(rest["next"]))               # a camera at exact rest
    assert r["status"] == fr_ref.NO_MODEL and r["keep"].all() and (r["n_inliers"], r["hypothesis"], r["root"], r["iterations"]) == (150, -1, -1, 1000)
    assert (r["counts"] == -1).all() and not r["pivot_valid"].any() and not r["F"].any()


def _epipolar_px(E, prev, nxt):
    d1, d2 = fr_ref.errors(np.asarray(E, np.float64).ravel(), prev, nxt)
    return np.sqrt(np.maximum(d1, d2)) * rc.FOCAL


# what fr_ref gives on the committed scenes (recorded, not fixed in advance): name -> (true tracks kept, true tracks, outliers kept, outliers, iterations)
RECORDED = {
    "general_150": (150, 150, 0, 0, 1),
    "general_150_o20_clean": (120, 120, 1, 30, 18),
    "forward_150_o20": (120, 120, 0, 30, 20),
    "general_150_o20": (110, 120, 1, 30, 36),
    "general_150_o50": (70, 75, 4, 75, 645),
    "general_150_o50_n05": (55, 75, 2, 75, 1000),
    "general_300_o20": (200, 240, 3, 60, 69),
}


def test_what_is_kept_and_dropped_on_the_scenes():
    """The behavioural conditions, on scenes and seeds for which fr_ref alone satisfies them (checked here: these assertions are on fr_ref).  On
    noise-free general and forward motion every true correspondence is kept and every outlier farther than twice the threshold from its true
    epipolar line is dropped (the outliers that stay lie along their line); no all-inlier sample of these scenes fails the pivot test."""
    for name in ("general_150", "general_150_o20_clean", "forward_150_o20"):
        sc, r = rc.case(name), rc.ref(name)
        assert r["status"] == fr_ref.OK and r["keep"][~sc["outlier"]].all(), name
        far = sc["outlier"] & (_epipolar_px(sc["E"], sc["prev"], sc["next"]) > 2.0)
        assert far.sum() >= 0.8 * sc["outlier"].sum() and not r["keep"][far].any(), name
    for name, want in RECORDED.items():
        sc, r = rc.case(name), rc.ref(name)
        got = (int(r["keep"][~sc["outlier"]].sum()), int((~sc["outlier"]).sum()), int(r["keep"][sc["outlier"]].sum()), int(sc["outlier"].sum()), r["iterations"])
        print(name, got)
        assert got == want, name
        clean = ~sc["outlier"][r["samples"]].any(1)
        assert clean.any() and r["pivot_valid"][clean].all(), name
    # the rounds of the device: the loop ends in the first round of 256, in a later one, and at 1 000
    its = [rc.ref(n)["iterations"] for n in ("general_150_o20", "general_150_o50", "general_150_o50_n05")]
    assert its[0] <= 256 < its[1] < 1000 == its[2]
    r = rc.ref("rotation_150")                                                 # a pure rotation has no epipolar geometry: whatever F the noise gives
    assert r["status"] == fr_ref.OK


# ================================================================ CPU: layout and symbols
def test_fr_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "uvs_solver.h")).read()
    for s in FR_SYMBOLS:
        assert s + "(" in hdr, s
        assert s in uvs.api.EXPORTS, s
    assert "#define UVS_ABI_VERSION 7" in hdr
    L = uvs.api.lib()
    for s in FR_SYMBOLS:
        assert hasattr(L, s), s
    assert L.uvs_abi_version() == 7
    Hst = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
    for s in HOST_SYMBOLS:
        assert hasattr(Hst, s), s
    for m in ("reject_raw", "reject", "debug_reject", "last_reject_device_ms"):
        assert callable(getattr(uvs.api.FeatureTracker, m)), m


def test_fr_struct_layout_matches_header():
    code = r'''
#include <stdio.h>
#include <stddef.h>
#include "uvs_solver.h"
int main(void) {
  printf("%zu %zu\n", sizeof(uvs_ft_reject_item), sizeof(uvs_ft_reject_result));
  printf("%zu %zu %zu %zu %zu\n", offsetof(uvs_ft_reject_item, n_points), offsetof(uvs_ft_reject_item, reserved), offsetof(uvs_ft_reject_item, seed),
         offsetof(uvs_ft_reject_item, prev_norm), offsetof(uvs_ft_reject_item, next_norm));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", offsetof(uvs_ft_reject_result, status), offsetof(uvs_ft_reject_result, n_inliers),
         offsetof(uvs_ft_reject_result, hypothesis), offsetof(uvs_ft_reject_result, root), offsetof(uvs_ft_reject_result, iterations),
         offsetof(uvs_ft_reject_result, reserved), offsetof(uvs_ft_reject_result, F));
  printf("%d %d %d %d\n", UVS_FT_REJECT_HYPOTHESES, UVS_FT_REJECT_OK, UVS_FT_REJECT_SKIPPED, UVS_FT_REJECT_NO_MODEL);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c"); exe = os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    I, R = abi.FtRejectItem, abi.FtRejectResult
    assert out[:2] == [C.sizeof(I), C.sizeof(R)] == [32, 96]
    assert out[2:7] == [I.n_points.offset, I.reserved.offset, I.seed.offset, I.prev_norm.offset, I.next_norm.offset]
    assert out[7:14] == [R.status.offset, R.n_inliers.offset, R.hypothesis.offset, R.root.offset, R.iterations.offset, R.reserved.offset, R.F.offset]
    assert out[14:] == [abi.FT_REJECT_HYPOTHESES, abi.FT_REJECT_OK, abi.FT_REJECT_SKIPPED, abi.FT_REJECT_NO_MODEL]
    assert out[14:] == [fr_ref.N_HYP, fr_ref.OK, fr_ref.SKIPPED, fr_ref.NO_MODEL]


# ================================================================ host mirror
class HostTracker:
    """ctypes face of uvs::FeatureTracker behind feature_tracker_capi.cpp, with the entry points of the rejection; device < 0: the bookkeeping
    alone."""

    def __init__(self, device, cam=CAM, max_width=752, max_height=480, levels=4, max_points=1024):
        self.L = L = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
        L.uvs_host_ft_create.restype = C.c_void_p
        L.uvs_host_ft_create.argtypes = [C.c_int, abi.c_double_p] + [C.c_int] * 4
        L.uvs_host_ft_destroy.argtypes = [C.c_void_p]; L.uvs_host_ft_destroy.restype = None
        L.uvs_host_ft_read_image.argtypes = [C.c_void_p, abi.c_u8_p, C.c_int, C.c_int, C.c_double, C.c_int, abi.c_double_p]
        L.uvs_host_ft_read_flow.argtypes = [C.c_void_p, C.c_double, C.c_int, abi.c_double_p, abi.c_i32_p, abi.c_double_p, C.c_int, abi.c_double_p]
        L.uvs_host_ft_apply_reject.argtypes = [C.c_void_p, C.c_double, C.c_int, abi.c_double_p, abi.c_i32_p, abi.c_double_p, C.c_int, abi.c_u8_p, C.c_int,
                                               abi.c_double_p]
        L.uvs_host_ft_set_rejection.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_uint64]
        L.uvs_host_ft_last_reject.argtypes = [C.c_void_p, abi.c_i32_p]
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

    def read_image(self, img, time, new=()):
        img = np.ascontiguousarray(img, np.uint8); new, pn = self._pts(new)
        return self.L.uvs_host_ft_read_image(self.h, img.ctypes.data_as(abi.c_u8_p), img.shape[1], img.shape[0], time, len(new), pn)

    def read_flow(self, time, next_xy, status, next_norm, new=(), keep=None):
        nx, pnx = self._pts(next_xy); nm, pnm = self._pts(next_norm); new, pn = self._pts(new)
        st = np.ascontiguousarray(status, np.int32)
        pst = st.ctypes.data_as(abi.c_i32_p) if len(st) else None
        if keep is None:
            return self.L.uvs_host_ft_read_flow(self.h, time, len(nx), pnx, pst, pnm, len(new), pn)
        kp = np.ascontiguousarray(keep, np.uint8)
        return self.L.uvs_host_ft_apply_reject(self.h, time, len(nx), pnx, pst, pnm, len(kp), kp.ctypes.data_as(abi.c_u8_p) if len(kp) else None, len(new), pn)

    def set_rejection(self, f_threshold, focal_length=460.0, seed=0):
        return self.L.uvs_host_ft_set_rejection(self.h, f_threshold, focal_length, seed)

    def last_reject(self):
        o = np.zeros(5, np.int32)
        assert self.L.uvs_host_ft_last_reject(self.h, o.ctypes.data_as(abi.c_i32_p)) == 0
        return tuple(int(v) for v in o)

    def update_ids(self):
        return self.L.uvs_host_ft_update_ids(self.h)

    def get(self):
        n = self.L.uvs_host_ft_get(self.h, 0, None, None, None, None, None)
        o = dict(cur_pts=np.zeros((n, 2)), ids=np.zeros(n, np.int32), track_cnt=np.zeros(n, np.int32), cur_un_pts=np.zeros((n, 2)), pts_velocity=np.zeros((n, 2)))
        if n:
            self.L.uvs_host_ft_get(self.h, n, abi._dp(o["cur_pts"]), o["ids"].ctypes.data_as(abi.c_i32_p), o["track_cnt"].ctypes.data_as(abi.c_i32_p),
                                   abi._dp(o["cur_un_pts"]), abi._dp(o["pts_velocity"]))
        return o


def test_host_mirror_apply_reject_by_hand():
    """applyReject without a device: the tracks the flow left are cut by the keep mask -- positions, ids, counts and the device's normalized points
    together -- and the next frame's velocity pairs the survivors with their own previous points."""
    T, O = ft_ref.TRACKED, ft_ref.LOST_OUTSIDE
    t = HostTracker(-1)
    a = np.array([[10.0, 10.0], [30.0, 12.0], [50.0, 14.0], [70.0, 16.0], [90.0, 18.0]])
    assert t.read_flow(0.0, [], [], [], new=a) == 0 and t.update_ids() == 5
    b = a + [1.5, 0.25]; nb = kf_ref.lift(CAM, b) + 1e-3 * np.arange(5)[:, None]          # marked per point
    # the flow loses track 1; of the four left (ids 0 2 3 4) the mask drops the second and the last (ids 2 and 4); one new point
    assert t.read_flow(0.1, b, [T, O, T, T, T], nb, new=[(200.0, 100.0)], keep=[1, 0, 1, 0]) == 0
    assert t.update_ids() == 3
    g = t.get()
    assert g["ids"].tolist() == [0, 3, 5] and g["track_cnt"].tolist() == [2, 2, 1]
    assert np.array_equal(g["cur_pts"], np.r_[b[[0, 3]], [[200.0, 100.0]]])
    assert np.array_equal(bits(g["cur_un_pts"][:2]), bits(nb[[0, 3]])) and np.array_equal(bits(g["cur_un_pts"][2:]), bits(kf_ref.lift(CAM, [[200.0, 100.0]])))
    # a mask of another length changes nothing and is refused; the frame goes on with every track
    cur = g["cur_pts"]; c = cur + [0.5, 0.5]; ncn = kf_ref.lift(CAM, c)
    assert t.read_flow(0.2, c, [T, T, T], ncn, keep=[1, 0]) == abi.UVS_ERR_INVALID_ARG
    g2 = t.get()
    assert g2["ids"].tolist() == [0, 3, 5] and g2["track_cnt"].tolist() == [3, 3, 2]
    want_v = (ncn - g["cur_un_pts"]) / (np.float64(0.2) - np.float64(0.1))
    assert np.array_equal(bits(g2["pts_velocity"][:2]), bits(want_v[:2]))
    # all ones keeps everything; all zeros leaves only the new point
    d = c + [0.5, 0.0]
    assert t.read_flow(0.3, d, [T, T, T], kf_ref.lift(CAM, d), keep=[1, 1, 1]) == 0 and t.get()["ids"].tolist() == [0, 3, 5]
    e = d + [0.5, 0.0]
    assert t.read_flow(0.4, e, [T, T, T], kf_ref.lift(CAM, e), new=[(5.0, 5.0)], keep=[0, 0, 0]) == 0
    g = t.get()
    assert g["ids"].tolist() == [-1] and g["track_cnt"].tolist() == [1] and g["cur_pts"].tolist() == [[5.0, 5.0]]
    t.close()


# ================================================================ GPU
def _tracker(**kw):
    kw.setdefault("max_width", 96); kw.setdefault("max_height", 80); kw.setdefault("max_streams", 4); kw.setdefault("max_points", 300)
    kw.setdefault("levels", 1)
    return uvs.api.FeatureTracker(**kw)


def _item(name):
    sc = rc.case(name)
    return dict(prev=sc["prev"], next=sc["next"], seed=sc["seed"])


def _assert_result(got, want, what=""):
    """The fields of uvs_ft_reject's answer: integers ==, F bit for bit, the mask byte for byte."""
    for k in ("status", "n_inliers", "hypothesis", "root", "iterations"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(bits(got["F"]), bits(want["F"])), (what, got["F"], want["F"])
    assert np.array_equal(got["keep"], want["keep"]), (what, np.flatnonzero(got["keep"] != want["keep"])[:8])
    assert int(got["keep"].sum()) == got["n_inliers"], what


def _assert_debug(got, want, what=""):
    assert np.array_equal(got["samples"], want["samples"]), (what, np.argwhere(got["samples"] != want["samples"])[:4].tolist())
    bad = np.argwhere(got["counts"] != want["counts"])
    assert len(bad) == 0, (what, len(bad), [(int(h), int(r), int(got["counts"][h, r]), int(want["counts"][h, r])) for h, r in bad[:6]])
    bad = np.argwhere((bits(got["models"]) != bits(want["models"])).any(2))
    assert len(bad) == 0, (what, len(bad), [(int(h), int(r), got["models"][h, r].tolist(), want["models"][h, r].tolist()) for h, r in bad[:2]])
    _assert_result(got, want, what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_gpu_debug_reject_equals_the_restatement_value_by_value(name):
    """Every sample, all 1 000 x 3 models and counts, the mask and the result; then uvs_ft_reject, which leaves its loop as soon as the stopping
    rule allows, gives the result of the full evaluation."""
    ft = _tracker(max_streams=1)
    want = rc.ref(name)
    _assert_debug(ft.debug_reject(_item(name), THR, CONF), want, name)
    _assert_result(ft.reject([_item(name)], THR, CONF)[0], want, name + " (early exit)")
    assert ft.last_reject_device_ms() > 0.0
    ft.close()


@pytest.mark.gpu
def test_gpu_skipped_and_no_model():
    ft = _tracker(max_streams=2)
    sc = rc.case("general_150")
    for n in (0, 1, 7):
        it = dict(prev=sc["prev"][:n], next=sc["next"][:n], seed=5)
        want = fr_ref.reject(sc["prev"][:n], sc["next"][:n], 5, THR)
        assert want["status"] == fr_ref.SKIPPED
        _assert_debug(ft.debug_reject(it, THR, CONF), want, n)
        _assert_result(ft.reject([it], THR, CONF)[0], want, n)
    got = ft.reject([_item("rest_150"), dict(prev=sc["prev"][:7], next=sc["next"][:7], seed=5)], THR, CONF)
    assert got[0]["status"] == abi.FT_REJECT_NO_MODEL and got[0]["keep"].all() and got[0]["iterations"] == 1000 and not got[0]["F"].any()
    assert got[1]["status"] == abi.FT_REJECT_SKIPPED and got[1]["keep"].tolist() == [1] * 7
    _assert_result(got[0], rc.ref("rest_150"))
    ft.close()


@pytest.mark.gpu
def test_gpu_a_batch_equals_its_items_one_at_a_time_and_a_second_run():
    names = ["general_8", "forward_40", "general_150_o50", "general_300_o20"]
    ft, solo = _tracker(), _tracker(max_streams=1)
    items = [_item(n) for n in names]
    batch = ft.reject(items, THR, CONF)
    for k in (2, 0, 3, 1):
        _assert_result(batch[k], solo.reject([items[k]], THR, CONF)[0], names[k])
        _assert_result(batch[k], rc.ref(names[k]), names[k])
    again = ft.reject(items, THR, CONF)
    for k in range(4):
        _assert_result(again[k], batch[k], "run against run")
    back = ft.reject(items[::-1], THR, CONF)                    # the place in the batch does not matter
    for k in range(4):
        _assert_result(back[3 - k], batch[k], "order")
    ft.close(); solo.close()


@pytest.mark.gpu
def test_gpu_max_points_tracks_in_one_item_and_another_threshold():
    ft = _tracker(max_streams=1, max_points=300)                 # general_300_o20 fills the capacity
    _assert_result(ft.reject([_item("general_300_o20")], THR, CONF)[0], rc.ref("general_300_o20"))
    sc = rc.case("general_150_o20")
    for thr, conf in ((3.0 / rc.FOCAL, 0.99), (THR, 0.5), (0.25 / rc.FOCAL, 0.999)):
        want = fr_ref.reject(sc["prev"], sc["next"], 77, thr, conf)
        assert want["half_margin"] > 1e-9
        _assert_result(ft.reject([dict(prev=sc["prev"], next=sc["next"], seed=77)], thr, conf)[0], want, (thr, conf))
    big = 2 ** 64 - 3                                           # the seed is 64 bits wide
    want = fr_ref.reject(sc["prev"], sc["next"], big, THR, CONF)
    assert want["half_margin"] > 1e-9
    _assert_result(ft.reject([dict(prev=sc["prev"], next=sc["next"], seed=big)], THR, CONF)[0], want, "seed")
    ft.close()


@pytest.mark.gpu
def test_gpu_reject_argument_checks_leave_the_handle_usable():
    ft = _tracker(max_streams=2, max_points=150)
    INV = abi.UVS_ERR_INVALID_ARG
    sc = rc.case("general_150_o20")
    ok = lambda **kw: dict(dict(prev=sc["prev"], next=sc["next"], seed=sc["seed"]), **kw)
    nan = sc["next"].copy(); nan[17, 1] = np.nan
    inf = sc["prev"].copy(); inf[149, 0] = np.inf
    more = np.zeros((151, 2))
    bad = [
        dict(items=[ok()], null=("items",)), dict(items=[ok()], null=("keep",)), dict(items=[ok()], null=("results",)),
        dict(items=[ok()], n_items=0), dict(items=[ok()], n_items=-1), dict(items=[ok(), ok(), ok()]),      # more items than slots
        dict(items=[ok(n_points=-1)]), dict(items=[dict(prev=more, next=more, seed=1)]),                   # more tracks than max_points
        dict(items=[dict(prev=np.zeros((0, 2)), next=np.zeros((0, 2)), n_points=9, seed=1)]),              # null arrays behind a positive count
        dict(items=[ok(next=nan)]), dict(items=[ok(prev=inf)]),
        dict(items=[ok()], threshold=0.0), dict(items=[ok()], threshold=-1.0), dict(items=[ok()], threshold=np.inf), dict(items=[ok()], threshold=np.nan),
        dict(items=[ok()], confidence=0.0), dict(items=[ok()], confidence=1.0), dict(items=[ok()], confidence=np.nan),
    ]
    for kw in bad:
        items = kw.pop("items")
        rcode, out = ft.reject_raw(items, kw.pop("threshold", THR), kw.pop("confidence", CONF), **kw)
        assert rcode == INV and out == [] and ft.last_error(), (kw, rcode, ft.last_error())
    with pytest.raises(RuntimeError):
        ft.debug_reject(ok(next=nan), THR, CONF)
    # no rejected call changed anything: the handle answers correctly, and tracks
    _assert_result(ft.reject([ok()], THR, CONF)[0], rc.ref("general_150_o20"))
    s = fc.scene("shift_48x40_L1")
    ft.track([dict(stream=0, image=s["prev"])], CAM)
    trk = ft.track([dict(stream=0, image=s["next"], points=s["pts"][:20])], CAM)[0]
    want = ft_ref.track_images(s["prev"], s["next"], s["pts"][:20], 1, CAM)
    assert np.array_equal(trk["status"], want["status"]) and np.array_equal(bits(trk["next_xy"]), bits(want["next_xy"]))
    ft.close()


@pytest.mark.gpu
def test_gpu_reject_between_track_and_detect_changes_neither():
    s = fc.scene("shift_96x80_L2")
    ft, plain = _tracker(levels=2, max_streams=1, max_points=150), _tracker(levels=2, max_streams=1, max_points=150)
    pts = s["pts"]
    ft.track([dict(stream=0, image=s["prev"])], CAM); plain.track([dict(stream=0, image=s["prev"])], CAM)
    _assert_result(ft.reject([_item("general_150_o20")], THR, CONF)[0], rc.ref("general_150_o20"))
    a = ft.track([dict(stream=0, image=s["next"], points=pts)], CAM)[0]
    b = plain.track([dict(stream=0, image=s["next"], points=pts)], CAM)[0]
    for k in ("status", "iterations"):
        assert np.array_equal(a[k], b[k])
    for k in ("next_xy", "next_norm"):
        assert np.array_equal(bits(a[k]), bits(b[k]))
    _assert_result(ft.reject([_item("forward_40")], THR, CONF)[0], rc.ref("forward_40"))
    occ = a["next_xy"][a["status"] == 0]
    da = ft.detect([dict(stream=0, occupied=occ, max_new=20)], CAM, 0.01, 8)[0]
    db = plain.detect([dict(stream=0, occupied=occ, max_new=20)], CAM, 0.01, 8)[0]
    assert da["n_new"] == db["n_new"] > 5 and np.array_equal(da["xy"], db["xy"]) and np.array_equal(bits(da["score"]), bits(db["score"]))
    _assert_result(ft.reject([_item("general_150_o20")], THR, CONF)[0], rc.ref("general_150_o20"))      # and the rejection is not disturbed either
    ft.close(); plain.close()


# ---- three rendered frames through the mirror
MIRROR_W, MIRROR_H, MIRROR_LEVELS = 131, 97, 3
MIRROR_SEED = 4242
MIRROR_DIR = np.array([1.0, -0.4])                                               # the camera slides: every track moves along this direction ...
MIRROR_STEPS = ((0.0, 0.0), (2.0, 4.5), (4.0, 9.0))                              # ... by this much per frame, the far layer and the near one
MIRROR_EDGE = 76                                                                 # columns from here on show the near layer
MIRROR_ODD = 7                                                                   # the track displaced by hand (far layer)
MIRROR_EXTRA = np.array([1.6, 4.0])                                              # ... across the epipolar lines, in frame 1


def _mirror_points():
    return np.array([(x + 0.25, y + 0.5) for y in (14, 38, 62, 84) for x in (14, 38, 62, 86, 110)], np.float64)


def _mirror_truth(k):
    """Where the points of frame 0 are in frame k."""
    p = _mirror_points()
    step = np.where(p[:, 0] >= MIRROR_EDGE, MIRROR_STEPS[k][1], MIRROR_STEPS[k][0])
    return p + step[:, None] * MIRROR_DIR


def _mirror_frames():
    """Two depth layers behind a fixed edge, so that the tracks have parallax and the epipolar geometry is determined (one plane alone would
    leave F two degrees of freedom, enough to explain any single outlier).  In frame 1 the 25 x 25 patch around track MIRROR_ODD shows its layer
    moved by MIRROR_EXTRA more than the rest."""
    imgs = []
    for k, (far, near) in enumerate(MIRROR_STEPS):
        a = fc.render(10, MIRROR_W, MIRROR_H, shift=tuple(far * MIRROR_DIR), noise=1.5, noise_seed=k)
        b = fc.render(12, MIRROR_W, MIRROR_H, shift=tuple(near * MIRROR_DIR), noise=1.5, noise_seed=k)
        img = a.copy(); img[:, MIRROR_EDGE:] = b[:, MIRROR_EDGE:]
        imgs.append(img)
    odd = fc.render(10, MIRROR_W, MIRROR_H, shift=tuple(MIRROR_STEPS[1][0] * MIRROR_DIR + MIRROR_EXTRA), noise=1.5, noise_seed=1)
    q = _mirror_truth(1)[MIRROR_ODD] + MIRROR_EXTRA
    x0, y0 = int(round(q[0])) - 12, int(round(q[1])) - 12
    imgs[1][y0:y0 + 25, x0:x0 + 25] = odd[y0:y0 + 25, x0:x0 + 25]
    return imgs


def _mirror_reference(imgs, times, pts0):
    """readImage with the caller's points in frame 0 and rejectWithF on, replayed with ft_ref + fr_ref + the numpy bookkeeping; update_ids after
    every frame.  -> [dict(cur_pts, ids, track_cnt, cur_un_pts, pts_velocity, reject) per frame]."""
    pts = np.zeros((0, 2)); ids = np.zeros(0, int); cnt = np.zeros(0, int); un = np.zeros((0, 2))
    prev_map, n_id, out = {}, 0, []
    for k, img in enumerate(imgs):
        norm = np.zeros((0, 2)); rej = None
        if len(pts):
            r = ft_ref.track_images(imgs[k - 1], img, pts, MIRROR_LEVELS, CAM)
            ok = r["status"] == ft_ref.TRACKED
            pts, ids, cnt, norm, un = r["next_xy"][ok], ids[ok], cnt[ok], r["next_norm"][ok], un[ok]
        cnt = cnt + 1
        if len(pts) >= 8:
            rej = fr_ref.reject(un, norm, MIRROR_SEED + k, 1.0 / 460.0, 0.99)
            kp = rej["keep"] != 0
            pts, ids, cnt, norm = pts[kp], ids[kp], cnt[kp], norm[kp]
        if k == 0:
            pts = np.concatenate([pts, pts0]); norm = np.concatenate([norm, kf_ref.lift(CAM, pts0)])
            ids = np.concatenate([ids, -np.ones(len(pts0), int)]); cnt = np.concatenate([cnt, np.ones(len(pts0), int)])
        cur_map = {}
        for i, m in zip(ids, norm):
            cur_map.setdefault(int(i), m)
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
        un = norm
        out.append(dict(cur_pts=pts.copy(), ids=ids.copy(), track_cnt=cnt.copy(), cur_un_pts=norm.copy(), pts_velocity=vel, reject=rej))
    return out


@pytest.mark.gpu
def test_gpu_host_mirror_rejects_the_displaced_track():
    """Three rendered frames through uvs::FeatureTracker::readImage with f_threshold = 1: the tracks the flow leaves go through uvs_ft_reject
    (seed + frame number) before the bookkeeping goes on, bit for bit with ft_ref + fr_ref; the track whose patch was moved by hand in frame 1 is
    followed by the flow and dropped by the rejection.  With f_threshold = 0 (the default) the same frames keep it."""
    imgs = _mirror_frames(); pts0 = _mirror_points()
    times = [10.0, 10.05, 10.125]
    want = _mirror_reference(imgs, times, pts0)
    r1 = want[1]["reject"]
    assert r1 is not None and r1["status"] == fr_ref.OK and want[2]["reject"]["status"] == fr_ref.OK
    assert r1["half_margin"] > 1e-9 and want[2]["reject"]["half_margin"] > 1e-9
    flow = ft_ref.track_images(imgs[0], imgs[1], pts0, MIRROR_LEVELS, CAM)
    assert flow["status"][MIRROR_ODD] == ft_ref.TRACKED                         # the flow follows the moved patch ...
    moved = flow["next_xy"] - _mirror_truth(1)
    assert np.abs(moved[MIRROR_ODD] - MIRROR_EXTRA).max() < 0.5 and np.abs(np.delete(moved, MIRROR_ODD, 0)).max() < 0.5
    assert MIRROR_ODD not in want[1]["ids"].tolist() and len(want[1]["ids"]) >= 15      # ... and the rejection drops it, and little else
    t = HostTracker(0, max_width=MIRROR_W, max_height=MIRROR_H, levels=MIRROR_LEVELS, max_points=64)
    plain = HostTracker(0, max_width=MIRROR_W, max_height=MIRROR_H, levels=MIRROR_LEVELS, max_points=64)
    assert t.set_rejection(1.0, 460.0, MIRROR_SEED) == 0
    for k, img in enumerate(imgs):
        assert t.read_image(img, times[k], new=pts0 if k == 0 else ()) == 0
        assert plain.read_image(img, times[k], new=pts0 if k == 0 else ()) == 0
        t.update_ids(); plain.update_ids()
        g, w = t.get(), want[k]
        assert g["ids"].tolist() == w["ids"].tolist() and g["track_cnt"].tolist() == w["track_cnt"].tolist(), k
        for key in ("cur_pts", "cur_un_pts", "pts_velocity"):
            assert np.array_equal(bits(g[key]), bits(w[key])), (k, key)
        if w["reject"] is not None:
            rj = w["reject"]
            assert t.last_reject() == (rj["status"], rj["n_inliers"], rj["hypothesis"], rj["root"], rj["iterations"]), k
        if k == 1:
            assert MIRROR_ODD in plain.get()["ids"].tolist() and MIRROR_ODD not in g["ids"].tolist()
    assert want[2]["pts_velocity"].any()
    t.close(); plain.close()
