"""Line tracking of the line front end (uvs_lt_*; csrc/uvs_line_track.hip): one LBD descriptor per caller-supplied segment and the Hamming match
with the 30 px endpoint gates, as the reference's lineExtraction / lineMatching use OpenCV's BinaryDescriptor, pinned to tests/lt_ref.py bit
for bit.  OpenCV is not a dependency and could not be compared; what pins the rule is the header's statement, the two forms of it in lt_ref
(vectorized against plain loops), hand cases, invariants, planted defects, and the scenes of lt_cases, in which every line finds itself again.

CPU: the restatement against itself, the hand cases, the invariants, the tables, the match rule, the shifted scenes, the defects, the header
against abi.py, the host mirror's bookkeeping with a stubbed match.  GPU: uvs_lt_debug_line value by value, uvs_lt_track in batches and alone,
reset, an empty frame, uvs_lt_match, the argument checks, and uvs::LineFeatureTracker::readImage4Line over three frames."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import lt_cases as lc
import lt_ref
from helpers import abi, uvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LT_SYMBOLS = ["uvs_lt_create", "uvs_lt_destroy", "uvs_lt_last_error", "uvs_lt_reset", "uvs_lt_track", "uvs_lt_match", "uvs_lt_last_device_ms",
              "uvs_lt_debug_line", "uvs_lt_gauss_tables"]
HOST_SYMBOLS = ["uvs_host_lt_book_create", "uvs_host_lt_create", "uvs_host_lt_destroy", "uvs_host_lt_apply_matches", "uvs_host_lt_read_image",
                "uvs_host_lt_update_ids", "uvs_host_lt_reset", "uvs_host_lt_get", "uvs_host_lt_last"]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def all_lines(name):
    """[(label, image, segment)]: every bar of both frames of a scene and every extra on frame A."""
    sc = lc.scene(name)
    out = [(f"A{i}", sc["A"], s) for i, s in enumerate(sc["segs_a"])] + [(f"B{i}", sc["B"], s) for i, s in enumerate(sc["segs_b"])]
    return out + [(k, sc["A"], np.array(s)) for k, s in lc.extras(name).items()]


# ================================================================ CPU: the restatement
@pytest.mark.parametrize("name", lc.SMALL)
def test_vectorized_form_equals_loop_form(name):
    grads = {}
    for label, img, seg in all_lines(name):
        g = grads.setdefault(id(img), lt_ref.gradient(img))
        v = lt_ref.describe_line(g, seg, lc.MAX_LENGTH); l = lt_ref.describe_line(g, seg, lc.MAX_LENGTH, loops=True)
        for k in ("geom", "ends", "row_sums", "desc"):
            assert np.array_equal(v[k], l[k]), (label, k)
        for k in ("desc_float", "clamped"):
            assert np.array_equal(bits(v[k]), bits(l[k])), (label, k)


def test_geometry_of_the_extras():
    g = {k: lt_ref.keyline(s, lc.MAX_LENGTH) for k, s in lc.extras("96x80").items()}
    assert g["vertical"][0].tolist() == [34, 0, 1024, 41216, 30464, 16, lt_ref.OK, 0] and g["vertical"][1].tolist() == [40, 12, 40, 47]
    assert g["swapped"][1].tolist() == [30, 41, 70, 20] and g["swapped"][0][1] > 0 > g["swapped"][0][2]      # the ends were swapped
    assert g["corner"][1].tolist() == [-9, 6, 14, -7]                                                       # truncation is towards zero
    assert g["short"][0].tolist() == [1, 0, 0, 21094, 31181, 0, lt_ref.SHORT, 0]
    assert g["zero"][0].tolist() == [0, 0, 0, 20480, 30720, 0, lt_ref.SHORT, 0]
    assert g["seventy"][0][0] == 69 and g["seventy"][0][5] == 34                                            # more samples than a wave has lanes
    assert g["long"][0].tolist()[:3] == [89, 0, 0] and g["long"][0][6] == lt_ref.LONG
    assert lt_ref.keyline([3.0, 5.0, 90.0, 28.0])[0][6] == lt_ref.OK                                        # ... under the default max_length
    for k in ("short", "zero", "long"):
        d = lt_ref.describe_line(lt_ref.gradient(lc.scene("96x80")["A"]), lc.extras("96x80")[k], lc.MAX_LENGTH)
        assert not d["desc"].any() and not d["desc_float"].any() and not d["row_sums"].any()


def test_hand_cases():
    # a constant image: no gradient, all-zero sums, desc_float = 0 and all bits 0 (every comparison is a tie)
    d = lt_ref.describe(np.full((40, 60), 93, np.uint8), [[10.0, 20.0, 50.0, 20.0]])
    assert d["status"].tolist() == [0] and not d["row_sums"].any() and not d["desc_float"].any() and not d["desc"].any()
    # a vertical step edge under a horizontal segment: dx > 0, so cq = 1024, sq = 0, gDL = 1024 gx and gDO = 1024 gy = 0 ... the step is
    # ALONG the line direction; turned by 90 degrees (a horizontal step, gy != 0, gx = 0) all the weight is in the orthogonal sums
    img = np.full((80, 100), 50, np.uint8); img[40:, :] = 200            # brighter below: gy > 0 at the rows 39, 40
    up = lt_ref.describe(img, [[20.0, 40.0, 80.0, 40.0]])
    S = up["row_sums"][0]
    assert up["geom"][0].tolist()[:3] == [60, 1024, 0]
    assert not S[:, 0].any() and not S[:, 1].any() and not S[:, 3].any() and S[:, 2].any()
    # row h samples y = 40 + (h - 31): the rows h = 30, 31 see gy = 4 x 150 = 600 at each of the 60 samples
    assert S[:, 2].tolist() == [60 * 600 * 1024 if h in (30, 31) else 0 for h in range(63)]
    down = lt_ref.describe(255 - img, [[20.0, 40.0, 80.0, 40.0]])["row_sums"][0]
    assert not down[:, 2].any() and np.array_equal(down[:, 3], S[:, 2])
    # the same edge vertical under a horizontal segment: gx != 0 only, so the weight is in S[.][0] (brighter to the right) or S[.][1]
    ver = lt_ref.describe(np.ascontiguousarray(img.T), [[10.0, 30.0, 70.0, 30.0]])["row_sums"][0]
    assert ver[:, 0].any() and not ver[:, 1:].any()


@pytest.mark.parametrize("name", lc.SMALL)
def test_invariants(name):
    sc = lc.scene(name)
    grad = lt_ref.gradient(sc["A"])
    assert max(np.abs(grad[0]).max(), np.abs(grad[1]).max()) <= 1020
    r = lc.ref_frame(name, "A")
    for i, seg in enumerate(sc["segs_a"]):
        dl, do, use = lt_ref.projections(grad, r["geom"][i])
        assert use.all() and max(np.abs(dl).max(), np.abs(do).max()) < 1.5e6
        S = r["row_sums"][i]
        assert np.array_equal(S[:, 0] - S[:, 1], dl.sum(1)) and np.array_equal(S[:, 2] - S[:, 3], do.sum(1))
        assert S.min() >= 0 and S.max() < 2 ** 32
        d, df = lt_ref.normalise(lt_ref.bands(S))
        assert d.max() <= 0.4 and d.min() >= 0.0
        assert abs(math.sqrt(float((df * df).sum())) - 1.0) < 1e-12
        assert np.array_equal(bits(df), bits(r["desc_float"][i]))
    z = lt_ref.normalise(np.zeros(72))
    assert not z[0].any() and not z[1].any()


def test_pair_list():
    assert len(lt_ref.PAIRS) == 32 and lt_ref.PAIRS[:9] == [(0, k) for k in range(1, 9)] + [(1, 2)] and lt_ref.PAIRS[31] == (5, 7)
    d = np.zeros(72); d[8 * 5 + 2] = 0.3                              # band 5 wins entry 2 against the bands 6 and 7: bit 7 - 2 of the bytes 30, 31
    want = np.zeros(32, np.uint8); want[30] = want[31] = 1 << 5
    assert np.array_equal(lt_ref.bits(d), want) and np.array_equal(lt_ref.bits_loops(d), want)
    d[:] = 0.2                                                        # ties give 0
    assert not lt_ref.bits(d).any()


def test_gauss_tables():
    import mpmath as mp
    mp.mp.dps = 60
    G, Lc = uvs.api.LineTracker.gauss_tables()
    rG, rLc = lt_ref.gauss_tables()
    assert np.array_equal(bits(G), bits(rG)) and np.array_equal(bits(Lc), bits(rLc))
    assert G[31] == 1.0 and Lc[10] == 1.0 and np.array_equal(G, G[::-1]) and np.array_equal(Lc, Lc[::-1])
    for tab, centre, den in ((G, 31, 1922), (Lc, 10, 98)):
        for i, v in enumerate(tab):
            assert v == math.exp(-float((i - centre) ** 2) / float(den))
            exact = mp.exp(-mp.mpf((i - centre) ** 2) / den)
            assert abs(mp.mpf(float(v)) - exact) <= mp.mpf(float(np.spacing(v))), (centre, i)


# ================================================================ CPU: the match rule
def test_match_rule_on_crafted_descriptors():
    c = lc.crafted_match()
    for fn in (lt_ref.match, lt_ref.match_loops):
        mop, dist, poc = fn(c["prev_desc"], c["prev_ends"], c["cur_desc"], c["cur_ends"], c["prev_status"], c["cur_status"])
        assert mop.tolist() == c["match_of_prev"].tolist()            # q 0, 7: the tie goes to t = 0; q 3: both gates at exactly 900 pass;
        assert dist.tolist() == c["distance"].tolist()                # q 4, 5: a gate at 901 / 961 fails; q 6: a SHORT line is no query
        assert poc.tolist() == c["prev_of_cur"].tolist()              # t 0: q 7 over q 0; t 2: q 2 over q 1; t 5 (SHORT) is nobody's match
    # without OK current lines there is no distance either
    mop, dist, poc = lt_ref.match(c["prev_desc"], c["prev_ends"], c["cur_desc"][5:], c["cur_ends"][5:], c["prev_status"], c["cur_status"][5:])
    assert (mop == -1).all() and (dist == -1).all() and poc.tolist() == [-1]


def test_match_forms_agree_on_random_descriptors():
    r = lc.random_match(96, 80, seed=5)
    ps = (np.arange(96) % 11 == 3).astype(np.int32); cs = (np.arange(80) % 7 == 2).astype(np.int32) * 2
    a = lt_ref.match(r["prev_desc"], r["prev_ends"], r["cur_desc"], r["cur_ends"], ps, cs)
    b = lt_ref.match_loops(r["prev_desc"], r["prev_ends"], r["cur_desc"], r["cur_ends"], ps, cs)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert (a[0] >= 0).sum() > 10 and ((a[0] < 0) & (a[1] >= 0)).sum() > 10      # accepted ones and gated ones


@pytest.mark.parametrize("name", sorted(lc.SCENES))
def test_every_line_of_a_shifted_scene_matches_itself(name):
    n = lc.SCENES[name][2]
    a = lc.ref_frame(name, "A"); b = lc.ref_frame(name, "B")
    assert (a["status"] == 0).all() and (b["status"] == 0).all()
    mop, dist, poc = lc.ref_pair(name)
    assert np.array_equal(mop, np.arange(n)) and np.array_equal(poc, np.arange(n))
    D = lt_ref.hamming(a["desc"], b["desc"])
    own = D[np.arange(n), np.arange(n)]; other = (D + 1000 * np.eye(n, dtype=np.int64)).min()
    print(f"{name}: own distance <= {own.max()}, nearest other line {other}")
    assert np.array_equal(dist, own) and own.max() < other


@pytest.mark.parametrize("name", sorted(lc.SCENES))
def test_a_scene_shifted_by_31_matches_nothing(name):
    mop, dist, poc = lc.ref_pair(name, (31, 0))
    assert (mop == -1).all() and (poc == -1).all() and (dist >= 0).all()


@pytest.mark.parametrize("variant", lt_ref.VARIANTS)
def test_each_planted_defect_changes_a_descriptor(variant):
    changed = 0
    for name in lc.SMALL:
        sc = lc.scene(name)
        grad = lt_ref.gradient(sc["A"])
        segs = list(sc["segs_a"]) + [np.array(s) for s in lc.extras(name).values()]
        for i, seg in enumerate(segs):
            good = lt_ref.describe_line(grad, seg, lc.MAX_LENGTH); bad = lt_ref.describe_line(grad, seg, lc.MAX_LENGTH, variant)
            changed += int(not np.array_equal(good["desc"], bad["desc"]) or not np.array_equal(bits(good["desc_float"]), bits(bad["desc_float"])))
    assert changed > 0, variant
    if variant == "truncate":          # only a support region that leaves the image can tell: the corner extras do
        sc = lc.scene("96x80"); grad = lt_ref.gradient(sc["A"]); seg = lc.extras("96x80")["corner"]
        assert not np.array_equal(lt_ref.describe_line(grad, seg, lc.MAX_LENGTH)["row_sums"], lt_ref.describe_line(grad, seg, lc.MAX_LENGTH, variant)["row_sums"])


# ================================================================ CPU: layout, symbols, the host mirror's bookkeeping
def test_lt_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "uvs_solver.h")).read()
    for s in LT_SYMBOLS:
        assert s + "(" in hdr, s
        assert s in uvs.api.EXPORTS, s
    assert "#define UVS_ABI_VERSION 7" in hdr
    L = uvs.api.lib()
    for s in LT_SYMBOLS:
        assert hasattr(L, s), s
    assert L.uvs_abi_version() == 7
    Hst = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
    for s in HOST_SYMBOLS:
        assert hasattr(Hst, s), s


def test_lt_struct_layout_matches_header():
    code = r'''
#include <stdio.h>
#include <stddef.h>
#include "uvs_solver.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(uvs_lt_item), offsetof(uvs_lt_item, image), offsetof(uvs_lt_item, stream), offsetof(uvs_lt_item, width),
         offsetof(uvs_lt_item, height), offsetof(uvs_lt_item, n_lines), offsetof(uvs_lt_item, segments));
  printf("%zu %zu %zu %zu\n", sizeof(uvs_lt_result), offsetof(uvs_lt_result, n_described), offsetof(uvs_lt_result, n_matched), offsetof(uvs_lt_result, status));
  printf("%d %d %d %d %d %d %d %d %d %d %d\n", UVS_LT_MAX_STREAMS, UVS_LT_MAX_LINES, UVS_LT_MAX_LENGTH, UVS_LT_MIN_SIZE, UVS_LT_ROWS, UVS_LT_DESC_FLOATS,
         UVS_LT_DESC_BYTES, UVS_LT_GATE2, UVS_LT_OK, UVS_LT_SHORT, UVS_LT_LONG);
  printf("%d\n", UVS_VP_MAX_LINES);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c"); exe = os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    I, R = abi.LtItem, abi.LtResult
    assert out[:7] == [C.sizeof(I), I.image.offset, I.stream.offset, I.width.offset, I.height.offset, I.n_lines.offset, I.segments.offset]
    assert out[7:11] == [C.sizeof(R), R.n_described.offset, R.n_matched.offset, R.status.offset]
    assert out[11:22] == [abi.LT_MAX_STREAMS, abi.LT_MAX_LINES, abi.LT_MAX_LENGTH, abi.LT_MIN_SIZE, abi.LT_ROWS, abi.LT_DESC_FLOATS, abi.LT_DESC_BYTES,
                          abi.LT_GATE2, abi.LT_OK, abi.LT_SHORT, abi.LT_LONG]
    assert out[22] == abi.LT_MAX_LINES == lt_ref.MAX_LINES and abi.LT_MAX_LENGTH == lt_ref.MAX_LENGTH and abi.LT_GATE2 == lt_ref.GATE2
    assert (lt_ref.OK, lt_ref.SHORT, lt_ref.LONG) == (abi.LT_OK, abi.LT_SHORT, abi.LT_LONG) and lt_ref.MAX_COORD == abi.KF_MAX_COORD
    arr, keep = abi.lt_items([dict(image=np.zeros((30, 40), np.uint8), segs=np.zeros((3, 4)), stream=2)])
    assert (arr[0].width, arr[0].height, arr[0].n_lines, arr[0].stream) == (40, 30, 3, 2)


def test_lt_create_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    assert uvs.api.lib().uvs_lt_create(0, 1, 96, 80, 16, 80, C.byref(h)) == abi.UVS_ERR_NO_DEVICE
    with pytest.raises(RuntimeError):
        uvs.api.LineTracker()
    G, Lc = uvs.api.LineTracker.gauss_tables()            # ... and the tables need none
    assert G.shape == (63,) and Lc.shape == (21,)


class HostLines:
    """ctypes face of uvs::LineFeatureTracker behind line_feature_tracker_capi.cpp; device < 0: the bookkeeping alone (no GPU)."""

    def __init__(self, device, cam=lc.CAM, max_width=376, max_height=240, max_lines=64, max_length=lc.MAX_LENGTH, margins=(0, 0), th_angle=None):
        L = self.L = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
        L.uvs_host_lt_book_create.restype = C.c_void_p; L.uvs_host_lt_book_create.argtypes = [abi.c_double_p, C.c_int, C.c_int]
        L.uvs_host_lt_create.restype = C.c_void_p; L.uvs_host_lt_create.argtypes = [C.c_int, abi.c_double_p] + [C.c_int] * 7 + [C.c_double]
        L.uvs_host_lt_destroy.argtypes = [C.c_void_p]; L.uvs_host_lt_destroy.restype = None
        L.uvs_host_lt_apply_matches.argtypes = [C.c_void_p, C.c_double, C.c_int, abi.c_double_p, abi.c_i32_p]
        L.uvs_host_lt_read_image.argtypes = [C.c_void_p, abi.c_u8_p, C.c_int, C.c_int, C.c_double, C.c_int, abi.c_double_p]
        L.uvs_host_lt_update_ids.argtypes = [C.c_void_p]; L.uvs_host_lt_reset.argtypes = [C.c_void_p]
        L.uvs_host_lt_get.argtypes = [C.c_void_p, C.c_int, abi.c_i32_p, abi.c_i32_p] + [abi.c_double_p] * 4
        L.uvs_host_lt_last.argtypes = [C.c_void_p, C.c_int, abi.c_u8_p, abi.c_i32_p, abi.c_i32_p, abi.c_i32_p]
        c = np.array(cam, np.float64)
        if device < 0:
            self.h = L.uvs_host_lt_book_create(abi._dp(c), *margins)
        else:
            self.h = L.uvs_host_lt_create(device, abi._dp(c), max_width, max_height, max_lines, max_length, margins[0], margins[1],
                                          int(th_angle is not None), float(th_angle or 0.0))
        assert self.h, "uvs_host_lt_create"

    def close(self):
        if self.h:
            self.L.uvs_host_lt_destroy(self.h); self.h = None

    def apply_matches(self, time, segs, prev_index):
        segs = np.ascontiguousarray(segs, np.float64).reshape(-1, 4); pi = np.ascontiguousarray(prev_index, np.int32)
        return self.L.uvs_host_lt_apply_matches(self.h, time, len(segs), abi._dp(segs) if len(segs) else None, pi.ctypes.data_as(abi.c_i32_p) if len(pi) else None)

    def read_image(self, img, time, segs):
        img = np.ascontiguousarray(img, np.uint8); segs = np.ascontiguousarray(segs, np.float64).reshape(-1, 4)
        return self.L.uvs_host_lt_read_image(self.h, img.ctypes.data_as(abi.c_u8_p), img.shape[1], img.shape[0], time, len(segs), abi._dp(segs) if len(segs) else None)

    def update_ids(self):
        return self.L.uvs_host_lt_update_ids(self.h)

    def reset(self):
        return self.L.uvs_host_lt_reset(self.h)

    def get(self):
        n = self.L.uvs_host_lt_get(self.h, 0, None, None, None, None, None, None)
        m = max(n, 1)
        o = dict(ids=np.zeros(m, np.int32), track_cnt=np.zeros(m, np.int32), pts=np.zeros((m, 4)), un_pts=np.zeros((m, 4)), velocity=np.ones((m, 4)),
                 vps=np.zeros((m, 3)))
        assert self.L.uvs_host_lt_get(self.h, m, o["ids"].ctypes.data_as(abi.c_i32_p), o["track_cnt"].ctypes.data_as(abi.c_i32_p), abi._dp(o["pts"]),
                                      abi._dp(o["un_pts"]), abi._dp(o["velocity"]), abi._dp(o["vps"])) == n
        return {k: v[:n] for k, v in o.items()}

    def last(self, n):
        desc = np.zeros((max(n, 1), 32), np.uint8); st = np.zeros(max(n, 1), np.int32); dist = np.zeros(max(n, 1), np.int32); res = np.zeros(2, np.int32)
        assert self.L.uvs_host_lt_last(self.h, n, desc.ctypes.data_as(abi.c_u8_p), st.ctypes.data_as(abi.c_i32_p), dist.ctypes.data_as(abi.c_i32_p),
                                       res.ctypes.data_as(abi.c_i32_p)) == 0
        return desc[:n], st[:n], dist[:n], res


def lift_ref(pts, cam, margins=(0, 0)):
    """liftProjective4line of [n, 4] pixel end points, operation by operation."""
    fx, fy, cx, cy = cam
    cx = cx - margins[0]; cy = cy - margins[1]
    k11, k13, k22, k23 = 1.0 / fx, -cx / fx, 1.0 / fy, -cy / fy
    out = np.zeros_like(pts)
    out[:, 0::2] = (k11 * pts[:, 0::2] + k13) / 1.0
    out[:, 1::2] = (k22 * pts[:, 1::2] + k23) / 1.0
    return out


def test_host_mirror_bookkeeping_with_a_stubbed_match():
    """readImage4Line's ids and counts (reference :351-433, :449-488, updateID) with the matches given by hand."""
    h = HostLines(-1, margins=(8, 4))
    segA = np.array([[10.5, 20.25, 50.0, 22.0], [70.9, 30.0, 30.1, 60.7], [5.0, 5.0, 5.0, 40.0], [-3.5, 7.5, 12.0, -2.5]])
    assert h.apply_matches(0.1, segA, np.full(4, -1, np.int32)) == 0
    g = h.get()
    assert g["ids"].tolist() == [-1] * 4 and g["track_cnt"].tolist() == [1] * 4 and not g["velocity"].any()
    # the gate points: ordered by x, truncated towards zero
    assert g["pts"].tolist() == [[10, 20, 50, 22], [30, 60, 70, 30], [5, 5, 5, 40], [-3, 7, 12, -2]]
    assert np.array_equal(bits(g["un_pts"]), bits(lift_ref(g["pts"], lc.CAM, (8, 4))))
    assert h.update_ids() == 4 and h.get()["ids"].tolist() == [0, 1, 2, 3]
    # frame 2: five lines; 0 continues previous 2, 1 is new, 2 continues 0, 3 continues 3, 4 points outside the previous lines (counts as new)
    segB = np.vstack([segA[[2, 1, 0, 3]] + 2.0, [[100.0, 100.0, 140.0, 100.0]]])
    assert h.apply_matches(0.2, segB, np.array([2, -1, 0, 3, 9], np.int32)) == 0
    g = h.get()
    assert g["ids"].tolist() == [2, -1, 0, 3, -1] and g["track_cnt"].tolist() == [2, 1, 2, 2, 1]
    assert h.update_ids() == 5 and h.get()["ids"].tolist() == [2, 4, 0, 3, 5]
    # frame 3: two lines continue, track_cnt counts 3; an empty frame leaves nothing; after it everything is new
    assert h.apply_matches(0.3, segB[[0, 1]], np.array([0, 1], np.int32)) == 0
    g = h.get()
    assert g["ids"].tolist() == [2, 4] and g["track_cnt"].tolist() == [3, 2]
    assert h.apply_matches(0.4, np.zeros((0, 4)), np.zeros(0, np.int32)) == 0 and len(h.get()["ids"]) == 0 and h.update_ids() == 0
    assert h.apply_matches(0.5, segA[:2], np.array([0, 1], np.int32)) == 0
    assert h.get()["ids"].tolist() == [-1, -1] and h.update_ids() == 2 and h.get()["ids"].tolist() == [6, 7]
    assert h.reset() == 0 and len(h.get()["ids"]) == 0
    h.close()


# ================================================================ GPU
@pytest.fixture(scope="module")
def tracker():
    """Two slots of the small scenes' size; max_length 80 makes the 90 px extra LONG."""
    t = uvs.api.LineTracker(device=0, max_streams=2, max_width=131, max_height=97, max_lines=32, max_length=lc.MAX_LENGTH)
    yield t
    t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", lc.SMALL)
def test_gpu_debug_line_equals_the_restatement(tracker, name):
    grads = {}
    for label, img, seg in all_lines(name):
        g = grads.setdefault(id(img), lt_ref.gradient(img))
        want = lt_ref.describe_line(g, seg, lc.MAX_LENGTH)
        got = tracker.debug_line(img, seg)
        assert got["geom"].tolist() == want["geom"].tolist(), label
        assert got["row_sums"].dtype == np.int64 and np.array_equal(got["row_sums"], want["row_sums"]), label
        assert np.array_equal(bits(got["desc_float"]), bits(want["desc_float"])), label
        assert np.array_equal(got["desc"], want["desc"]), label


def _same_item(got, want, what):
    for k in ("desc", "status", "prev_index", "distance"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert (got["n_described"], got["n_matched"]) == (want["n_described"], want["n_matched"]), what


@pytest.mark.gpu
def test_gpu_track_in_a_batch_equals_each_item_alone_and_the_restatement(tracker):
    names = lc.SMALL
    sc = [lc.scene(n) for n in names]
    ex = [np.array(list(lc.extras(n).values())) for n in names]            # the extras ride along: SHORT and LONG lines among the OK ones
    fa = [dict(stream=s, image=sc[s]["A"], segs=np.vstack([sc[s]["segs_a"], ex[s]])) for s in range(2)]
    fb = [dict(stream=s, image=sc[s]["B"], segs=np.vstack([sc[s]["segs_b"], ex[s] + np.tile(lc.SHIFT, 2)])) for s in range(2)]
    for s in range(2):
        tracker.reset(s)
    batch_a = tracker.track(fa); batch_b = tracker.track(fb[::-1])[::-1]      # the second call lists the slots the other way round
    for s in range(2):
        slot = lt_ref.Slot(lc.MAX_LENGTH)
        want_a = slot.track(fa[s]["image"], fa[s]["segs"]); want_b = slot.track(fb[s]["image"], fb[s]["segs"])
        _same_item(batch_a[s], want_a, (names[s], "A")); _same_item(batch_b[s], want_b, (names[s], "B"))
        n = len(sc[s]["segs_a"])
        assert (batch_a[s]["prev_index"] == -1).all() and batch_a[s]["n_matched"] == 0
        assert np.array_equal(batch_b[s]["prev_index"][:n], np.arange(n))       # the identity on the shifted scenes
        assert sorted(set(batch_b[s]["status"].tolist())) == [0, 1, 2]
        tracker.reset(s)
        alone_a = tracker.track([fa[s]])[0]; alone_b = tracker.track([fb[s]])[0]
        _same_item(alone_a, batch_a[s], (names[s], "A alone")); _same_item(alone_b, batch_b[s], (names[s], "B alone"))
    assert tracker.last_device_ms > 0.0 and tracker.last_ms >= tracker.last_device_ms


@pytest.mark.gpu
def test_gpu_track_376x240():
    name = "376x240"
    sc = lc.scene(name); n = lc.SCENES[name][2]
    t = uvs.api.LineTracker(device=0, max_streams=1, max_width=376, max_height=240, max_lines=64, max_length=lc.MAX_LENGTH)
    a = t.track([dict(stream=0, image=sc["A"], segs=sc["segs_a"])])[0]; b = t.track([dict(stream=0, image=sc["B"], segs=sc["segs_b"])])[0]
    t.close()
    ra = lc.ref_frame(name, "A"); rb = lc.ref_frame(name, "B"); mop, dist, poc = lc.ref_pair(name)
    assert np.array_equal(a["desc"], ra["desc"]) and np.array_equal(b["desc"], rb["desc"])
    assert np.array_equal(b["prev_index"], poc) and np.array_equal(poc, np.arange(n)) and np.array_equal(b["distance"], dist)
    assert (b["n_described"], b["n_matched"]) == (n, n)


@pytest.mark.gpu
def test_gpu_reset_and_an_empty_frame_empty_the_previous_set(tracker):
    sc = lc.scene("96x80")
    fa = dict(stream=0, image=sc["A"], segs=sc["segs_a"]); fb = dict(stream=0, image=sc["B"], segs=sc["segs_b"])
    n = len(sc["segs_a"])
    tracker.reset(0)
    tracker.track([fa])
    assert tracker.track([fb])[0]["n_matched"] == n
    tracker.track([fa]); tracker.reset(0)
    r = tracker.track([fb])[0]
    assert r["n_matched"] == 0 and (r["prev_index"] == -1).all() and (r["distance"] == -1).all() and r["n_described"] == n
    # a frame without lines: nothing comes back, and the next frame has no previous lines to continue
    tracker.track([fa])
    e = tracker.track([dict(stream=0, image=sc["B"])])[0]
    assert len(e["desc"]) == 0 and (e["n_described"], e["n_matched"]) == (0, 0)
    r = tracker.track([fa])[0]
    assert r["n_matched"] == 0 and (r["prev_index"] == -1).all()
    assert tracker.track([fb])[0]["n_matched"] == n
    # the other slot saw none of this
    tracker.reset(1)
    assert tracker.track([dict(stream=1, image=sc["B"], segs=sc["segs_b"])])[0]["n_matched"] == 0


@pytest.mark.gpu
def test_gpu_match_on_crafted_and_random_descriptors():
    t = uvs.api.LineTracker(device=0, max_streams=1, max_width=32, max_height=32, max_lines=1024, max_length=64)
    c = lc.crafted_match()
    ok_p = c["prev_status"] == 0; ok_c = c["cur_status"] == 0              # uvs_lt_match takes every line as OK: the SHORT ones are left out
    want = lt_ref.match(c["prev_desc"][ok_p], c["prev_ends"][ok_p], c["cur_desc"][ok_c], c["cur_ends"][ok_c])
    got = t.match(c["prev_desc"][ok_p], c["prev_ends"][ok_p], c["cur_desc"][ok_c], c["cur_ends"][ok_c])
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert got[0].tolist() == [0, 2, 2, 3, -1, -1, 0] and got[2].tolist() == [6, -1, 2, 3, -1]
    r = lc.random_match()
    want = lt_ref.match(r["prev_desc"], r["prev_ends"], r["cur_desc"], r["cur_ends"])
    got = t.match(r["prev_desc"], r["prev_ends"], r["cur_desc"], r["cur_ends"])
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert (want[0] >= 0).sum() > 100 and ((want[0] < 0) & (want[1] >= 0)).sum() > 100
    # an empty side
    mop, dist, poc = t.match(r["prev_desc"][:5], r["prev_ends"][:5], np.zeros((0, 32), np.uint8), np.zeros((0, 4), np.int32))
    assert mop.tolist() == [-1] * 5 and dist.tolist() == [-1] * 5 and len(poc) == 0
    mop, dist, poc = t.match(np.zeros((0, 32), np.uint8), np.zeros((0, 4), np.int32), r["cur_desc"][:5], r["cur_ends"][:5])
    assert len(mop) == 0 and poc.tolist() == [-1] * 5
    # the checks of uvs_lt_match
    assert t.match_raw(r["prev_desc"], r["prev_ends"], r["cur_desc"], r["cur_ends"], n_prev=1025)[0] == abi.UVS_ERR_CAPACITY
    assert t.match_raw(r["prev_desc"], r["prev_ends"], r["cur_desc"], r["cur_ends"], n_cur=-1)[0] == abi.UVS_ERR_INVALID_ARG
    assert t.match_raw(np.zeros((0, 32), np.uint8), np.zeros((0, 4), np.int32), r["cur_desc"], r["cur_ends"], n_prev=3)[0] == abi.UVS_ERR_INVALID_ARG
    assert "uvs_lt_match" in t.last_error()
    got = t.match(r["prev_desc"], r["prev_ends"], r["cur_desc"], r["cur_ends"])
    assert np.array_equal(got[0], want[0])
    t.close()


@pytest.mark.gpu
def test_gpu_argument_checks_leave_the_handle_usable(tracker):
    L = uvs.api.lib()
    h = C.c_void_p()
    for args, rc in (((0, 0, 96, 80, 8, 80), abi.UVS_ERR_INVALID_ARG), ((0, 1, 7, 80, 8, 80), abi.UVS_ERR_INVALID_ARG), ((0, 1, 96, 80, 0, 80), abi.UVS_ERR_INVALID_ARG),
                     ((0, 1, 96, 80, 8, 1), abi.UVS_ERR_INVALID_ARG), ((0, 65, 96, 80, 8, 80), abi.UVS_ERR_CAPACITY), ((0, 1, 4097, 80, 8, 80), abi.UVS_ERR_CAPACITY),
                     ((0, 1, 96, 80, 1025, 80), abi.UVS_ERR_CAPACITY), ((0, 1, 96, 80, 8, 2049), abi.UVS_ERR_CAPACITY), ((99, 1, 96, 80, 8, 80), abi.UVS_ERR_NO_DEVICE)):
        assert L.uvs_lt_create(*args, C.byref(h)) == rc and not h, args
    assert L.uvs_lt_create(0, 1, 96, 80, 8, 80, None) == abi.UVS_ERR_INVALID_ARG
    sc = lc.scene("96x80"); n = len(sc["segs_a"])
    fa = dict(stream=0, image=sc["A"], segs=sc["segs_a"]); fb = dict(stream=0, image=sc["B"], segs=sc["segs_b"])
    tracker.reset(0)
    tracker.track([fa])
    bad = lambda **kw: dict(fb, **kw)
    nan = sc["segs_b"].copy(); nan[3, 2] = np.nan
    far = sc["segs_b"].copy(); far[0, 0] = 1.5e6
    cases = [([fb], dict(n_items=0), abi.UVS_ERR_INVALID_ARG), ([fb], dict(n_items=3), abi.UVS_ERR_CAPACITY),
             ([bad(stream=2)], {}, abi.UVS_ERR_INVALID_ARG), ([bad(stream=-1)], {}, abi.UVS_ERR_INVALID_ARG),
             ([fb, bad(image=sc["A"])], {}, abi.UVS_ERR_INVALID_ARG),                                   # the stream twice
             ([bad(n_lines=-1)], {}, abi.UVS_ERR_INVALID_ARG), ([bad(n_lines=33)], {}, abi.UVS_ERR_CAPACITY),
             ([bad(segs=np.zeros((0, 4)), n_lines=2)], {}, abi.UVS_ERR_INVALID_ARG),                     # a null array behind a positive count
             ([bad(image=np.zeros((7, 96), np.uint8))], {}, abi.UVS_ERR_INVALID_ARG), ([bad(image=np.zeros((98, 96), np.uint8))], {}, abi.UVS_ERR_CAPACITY),
             ([bad(image=np.zeros((80, 132), np.uint8))], {}, abi.UVS_ERR_CAPACITY),
             ([bad(segs=nan)], {}, abi.UVS_ERR_INVALID_ARG), ([bad(segs=far)], {}, abi.UVS_ERR_INVALID_ARG)]
    cases += [([fb], dict(null=(k,)), abi.UVS_ERR_INVALID_ARG) for k in ("items", "desc", "line_status", "prev_index", "distance", "results")]
    for items, kw, rc in cases:
        assert tracker.track_raw(items, **kw)[0] == rc, (kw, rc)
        assert "uvs_lt_track" in tracker.last_error()
    for k in ("image", "segment", "geom", "row_sums", "desc_float", "desc"):
        assert tracker.debug_line_raw(sc["A"], sc["segs_a"][0], null=(k,))[0] == abi.UVS_ERR_INVALID_ARG
    assert tracker.debug_line_raw(np.zeros((98, 96), np.uint8), sc["segs_a"][0])[0] == abi.UVS_ERR_CAPACITY
    assert tracker.debug_line_raw(sc["A"], [0.0, np.inf, 1.0, 1.0])[0] == abi.UVS_ERR_INVALID_ARG
    assert L.uvs_lt_reset(tracker._h, 2) == abi.UVS_ERR_INVALID_ARG and L.uvs_lt_reset(None, 0) == abi.UVS_ERR_INVALID_ARG
    assert L.uvs_lt_last_error(None) == b"null line tracker" and L.uvs_lt_last_device_ms(None) == 0.0
    # none of the rejected calls, and no debug call, changed the slot: frame B still continues every line of frame A
    r = tracker.track([fb])[0]
    assert r["n_matched"] == n and np.array_equal(r["prev_index"], np.arange(n)) and tracker.last_error() == ""


@pytest.mark.gpu
def test_gpu_host_mirror_read_image_over_three_frames():
    """uvs::LineFeatureTracker::readImage4Line: ids persist, track_cnt counts 1, 2, 3, new lines get -1 and then fresh ids."""
    sc = lc.scene("131x97"); n = len(sc["segs_a"])
    h = HostLines(0, max_width=131, max_height=97, max_lines=32, th_angle=math.pi / 180.0)
    # frame 1: A without its last two lines;  frame 2: B, whole (two new lines);  frame 3: A again, in reverse order
    assert h.read_image(sc["A"], 0.1, sc["segs_a"][:n - 2]) == 0
    g = h.get()
    assert g["ids"].tolist() == [-1] * (n - 2) and g["track_cnt"].tolist() == [1] * (n - 2)
    assert h.update_ids() == n - 2 and h.get()["ids"].tolist() == list(range(n - 2))
    assert h.read_image(sc["B"], 0.2, sc["segs_b"]) == 0
    g = h.get()
    assert g["ids"].tolist() == list(range(n - 2)) + [-1, -1] and g["track_cnt"].tolist() == [2] * (n - 2) + [1, 1]
    desc, st, dist, res = h.last(n)
    want = lc.ref_frame("131x97", "B")
    assert np.array_equal(desc, want["desc"]) and (st == 0).all() and res.tolist() == [n, n - 2]
    assert np.array_equal(g["pts"], want["ends"].astype(np.float64)) and np.array_equal(bits(g["un_pts"]), bits(lift_ref(g["pts"], lc.CAM)))
    assert not g["velocity"].any() and g["vps"].shape == (n, 3) and set(np.unique(g["vps"][:, 2])) <= {0.0, 1.0}
    assert h.update_ids() == n and h.get()["ids"].tolist() == list(range(n))
    assert h.read_image(sc["A"], 0.3, sc["segs_a"][::-1]) == 0
    g = h.get()
    assert g["ids"].tolist() == list(range(n))[::-1] and g["track_cnt"].tolist() == ([3] * (n - 2) + [2, 2])[::-1]
    assert h.reset() == 0 and h.read_image(sc["B"], 0.4, sc["segs_b"]) == 0 and h.get()["ids"].tolist() == [-1] * n
    h.close()
