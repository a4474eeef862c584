"""Segment detection of the line front end (uvs_lt_detect, uvs_lt_detect_track, uvs_lt_debug_detect; csrc/uvs_line_detect.hip): Burns-style
line-support regions, the project's own rule (include/uvs_solver.h), pinned to tests/ld_ref.py bit for bit.  Neither ELSED nor OpenCV could be
compared; what pins the rule is the header's statement, the two forms of it in ld_ref (vectorized against plain loops), an independent
labelling, the exact sector inequalities, conditions on what the reference finds in the scenes of ld_cases, and planted misreadings.

CPU: the restatement against itself, the sector rule, the region names, the crafted images, the three conditions on the scenes, the
misreadings, the header against abi.py, the host mirror's overload with an injected detection.  GPU: uvs_lt_debug_detect stage by stage,
uvs_lt_detect alone and in a batch, OVERFLOW, the crafted images, uvs_lt_detect_track against detect + track and the references' replay, the
argument checks, and uvs::LineFeatureTracker::readImage4Line(image) over three frames."""
import ctypes as C
import math
import os
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import ld_cases as lc
import ld_ref
import lt_cases
import lt_ref
from helpers import abi, uvs
from test_line_track import HostLines, lift_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lc.PARAMS
T, MIN_PIXELS, MIN_LENGTH = P["grad_threshold"], P["min_pixels"], P["min_length"]
LD_SYMBOLS = ["uvs_lt_detect", "uvs_lt_detect_track", "uvs_lt_last_detect_device_ms", "uvs_lt_debug_detect"]
HOST_SYMBOLS = ["uvs_host_lt_stub_create", "uvs_host_lt_stub_inject", "uvs_host_lt_stub_finished", "uvs_host_lt_set_detect",
                "uvs_host_lt_read_image_detect", "uvs_host_lt_last_detect"]
STAGES = (("blur", "blur"), ("grad", "grad"), ("sector_a", "secA"), ("sector_b", "secB"), ("name_a", "nameA"), ("name_b", "nameB"), ("vote", "vote"))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_detection(got, want, what):
    """A device result (api dict) or a reference result against a reference result, every returned value."""
    for k in ("n_found", "n_returned", "n_support"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert list(got["n_regions"]) == list(want["n_regions"]), what
    assert got.get("det_status", got.get("status")) == want["status"], what
    assert np.array_equal(got["info"], want["info"]), what
    assert np.array_equal(bits(got["seg"]), bits(want["seg"])) and np.array_equal(bits(got["width2"]), bits(want["width2"])), what


# ================================================================ CPU: the restatement
@pytest.mark.parametrize("name", lc.SMALL + lc.CRAFTED_SMALL)
def test_vectorized_form_equals_loop_form(name):
    img = lc.scene(name)["A"] if name in lc.SCENES else lc.crafted(name)
    v = lc.ref_stages(name); l = ld_ref.stages(img, T, MIN_PIXELS, MIN_LENGTH, loops=True)
    for k in ("blur", "grad", "secA", "secB", "nameA", "nameB", "vote"):
        assert np.array_equal(v[k], l[k]), (name, k)
    assert v["n_support"] == l["n_support"] and v["n_regions"] == l["n_regions"]
    key = lambda k: (k["info"][0], k["info"][1])
    kv = sorted(v["kept"], key=key); kl = sorted(l["kept"], key=key)
    assert [k["info"] for k in kv] == [k["info"] for k in kl], name
    for a, b in zip(kv, kl):
        assert np.array_equal(bits(a["seg"]), bits(b["seg"])) and np.array_equal(bits([a["width2"], a["length"]]), bits([b["width2"], b["length"]])), (name, a["info"])
    d = ld_ref.detect(img, T, MIN_PIXELS, MIN_LENGTH, lc.MAX_LINES, loops=True)
    same_detection(d, lc.ref(name), name)


def test_blur_by_hand():
    assert np.array_equal(ld_ref.blur(np.full((9, 11), 77, np.uint8)), np.full((9, 11), 77))      # the taps sum to 16 x 16 = 256
    img = np.zeros((9, 9), np.uint8); img[4, 4] = 255
    k = np.array([1, 4, 6, 4, 1])
    want = (255 * np.outer(k, k) + 128) >> 8
    assert np.array_equal(ld_ref.blur(img)[2:7, 2:7], want)
    img = np.zeros((8, 8), np.uint8); img[0, 0] = 255                                             # reflect-101 never repeats the border pixel itself
    assert ld_ref.blur(img)[0, 0] == (255 * 6 * 6 + 128) >> 8 and ld_ref.blur(img)[1, 1] == (255 * 4 * 4 + 128) >> 8
    img = np.zeros((8, 8), np.uint8); img[1, 1] = 255                                             # ... but pixel 1 is seen twice from pixel 0: at x = 1 and at x = -1
    assert ld_ref.blur(img)[0, 0] == (255 * (4 + 4) * (4 + 4) + 128) >> 8


def _exact_sector(gx, gy):
    """The header's inequalities in exact rationals, by the angle's tangent: the sector boundaries of B are at tan = 408 / 985 and 985 / 408."""
    if gx > 0 and gy >= 0:
        q, px, py = 0, gx, gy
    elif gx <= 0 and gy > 0:
        q, px, py = 1, gy, -gx
    elif gx < 0 and gy <= 0:
        q, px, py = 2, -gx, -gy
    else:
        q, px, py = 3, -gy, gx
    assert px > 0 and py >= 0
    t = Fraction(py, px)
    return 2 * q + (t >= 1), (2 * q + (t >= Fraction(408, 985)) + (t >= Fraction(985, 408))) % 8


def test_sector_rule_on_a_grid_and_on_every_boundary():
    pts = {(gx, gy) for gx in range(-1020, 1021, 51) for gy in range(-1020, 1021, 51)}
    for k in range(1, 3):                                       # the multiples of the boundary vectors inside |g| <= 1020, in all four quadrants
        for a, b in ((408 * k, 985 * k), (985 * k, 408 * k)):
            pts |= {(sx * (a + da), sy * (b + db)) for sx in (-1, 1) for sy in (-1, 1) for da in (-1, 0, 1) for db in (-1, 0, 1)}
    for k in (1, 2, 7, 510, 1020):
        pts |= {(k, k), (-k, k), (k, -k), (-k, -k), (k, 0), (-k, 0), (0, k), (0, -k), (k, k - 1), (k - 1, k), (-k, k - 1), (1 - k, -k)}
    pts.discard((0, 0))
    pts = sorted(pts)
    gx = np.array([p[0] for p in pts], np.int64); gy = np.array([p[1] for p in pts], np.int64)
    A, B = ld_ref.sectors(gx, gy, np.abs(gx) + np.abs(gy), 1)
    for (x, y), a, b in zip(pts, A, B):
        assert (int(a), int(b)) == ld_ref.sector_of(x, y) == _exact_sector(x, y), (x, y)
        # a turn by 90 degrees moves both sectors on by 2
        assert ld_ref.sector_of(-y, x) == ((int(a) + 2) % 8, (int(b) + 2) % 8), (x, y)
        # away from a boundary the sectors are those of the angle
        ang = math.degrees(math.atan2(y, x)) % 360.0
        if min(ang % 45.0, 45.0 - ang % 45.0) > 0.01:
            assert int(a) == int(ang // 45.0), (x, y)
        if min((ang + 22.5) % 45.0, 45.0 - (ang + 22.5) % 45.0) > 0.01:
            assert int(b) == int((ang + 22.5) // 45.0) % 8, (x, y)
    # on the boundaries themselves: the larger sector (>=)
    assert ld_ref.sector_of(5, 5) == (1, 1) and ld_ref.sector_of(985, 408) == (0, 1) and ld_ref.sector_of(408, 985) == (1, 2)
    assert ld_ref.sector_of(985, 407) == (0, 0) and ld_ref.sector_of(5, 0) == (0, 0) and ld_ref.sector_of(0, 5) == (2, 2) and ld_ref.sector_of(5, -1) == (7, 0)
    assert abs(math.degrees(math.atan2(408, 985)) - 22.5) < 1e-4


@pytest.mark.parametrize("name", lc.SMALL + ("376x240",) + lc.CRAFTED)
def test_region_names_against_an_independent_labelling(name):
    from scipy import ndimage
    st = lc.ref_stages(name)
    for sec, nm in ((st["secA"], st["nameA"]), (st["secB"], st["nameB"])):
        assert np.array_equal(nm >= 0, sec != ld_ref.NONE)
        idx = np.arange(sec.size).reshape(sec.shape)
        n_regions = 0
        for s in np.unique(sec[sec != ld_ref.NONE]):
            lab, n = ndimage.label(sec == s, structure=np.ones((3, 3), int))
            n_regions += n
            m = lab > 0
            first = ndimage.minimum(idx, lab, np.arange(1, n + 1))          # the smallest linear index of every component
            assert np.array_equal(nm[m], first[lab[m] - 1].astype(np.int64)), (name, int(s))
        assert n_regions == len(np.unique(nm[nm >= 0]))


def test_crafted_images():
    c = lc.ref("constant")
    assert (c["n_found"], c["n_support"], c["n_regions"]) == (0, 0, [0, 0]) and c["seg"].shape == (0, 4)
    # the ramp: gx = 8 x 6 > T and gy = 0 everywhere but in a few columns at the left and right border, where reflect-101 flattens the blurred
    # ramp (gx == 0 in the border column itself): ONE region of every support pixel in both partitions, sector 0; the tie n_A == n_B votes A,
    # so A's region is returned with full support and B's has none
    r = lc.ref("ramp"); st = lc.ref_stages("ramp"); H, W = lc.crafted("ramp").shape
    cols = np.flatnonzero(st["secA"][0] != ld_ref.NONE)
    c0 = int(cols[0])
    assert 1 <= c0 <= 3 and cols.tolist() == list(range(c0, W - c0)) and (st["secA"] == st["secA"][0]).all() and (st["gy"] == 0).all()
    assert (st["gx"][:, 4:-4] == 48).all() and (st["gx"][:, [0, -1]] == 0).all()
    n = (W - 2 * c0) * H
    assert r["n_support"] == n and r["n_regions"] == [1, 1] and r["n_found"] == 1 and r["info"].tolist() == [[c0, 0, n, n]]
    assert set(np.unique(st["vote"])) == {0, ld_ref.NONE} and set(np.unique(st["secA"])) == set(np.unique(st["secB"])) == {0, ld_ref.NONE}
    # ... the weights are mirrored left to right and the same in every row: the segment runs along the middle row from the first to the last
    # support column (the region is wider than tall), and no pixel is off the axis by more than the rows allow
    assert np.allclose(r["seg"][0], [c0, (H - 1) / 2, W - 1 - c0, (H - 1) / 2], atol=1e-9) and W - 2 * c0 > H
    # the exact edges sit on the sector boundaries: gy == 0 -> (0, 0); gx == 0 -> (2, 2); gx == gy -> (1, 1); gx == -gy, gx > 0 -> (7, 7)
    for name, sectors in (("step_vertical", (0, 0)), ("step_horizontal", (2, 2)), ("step_diagonal", (1, 1)), ("step_antidiagonal", (7, 7))):
        st = lc.ref_stages(name)
        inner = (slice(8, -8), slice(8, -8))
        a = st["secA"][inner]; b = st["secB"][inner]
        assert set(np.unique(a[a != ld_ref.NONE])) == {sectors[0]} and set(np.unique(b[b != ld_ref.NONE])) == {sectors[1]}, name
        gx, gy = st["gx"][inner][a != ld_ref.NONE], st["gy"][inner][a != ld_ref.NONE]
        assert {"step_vertical": (gy == 0).all(), "step_horizontal": (gx == 0).all(), "step_diagonal": (gx == gy).all(),
                "step_antidiagonal": (gx == -gy).all()}[name]
        assert lc.ref(name)["n_found"] >= 1 and lc.ref(name)["length"][0] > 30
    # one edge from corner to corner: one long segment along the diagonal of the 376 x 240 image
    d = lc.ref("corner_to_corner")
    assert d["length"][0] > 0.95 * math.hypot(376, 240) and d["info"][0, 2] > 1000
    s = d["seg"][0]
    assert abs((s[3] - s[1]) / (s[2] - s[0]) - 240 / 376) < 0.01
    # the 2 px checkerboard: hundreds of regions of at most 3 pixels, none kept;  at the higher contrast they chain along the diagonals (by
    # their corners: 8-connectivity), and many are kept
    k = lc.ref("checkerboard"); st = lc.ref_stages("checkerboard")
    assert k["n_found"] == 0 and min(k["n_regions"]) > 250 and np.bincount(st["nameA"][st["nameA"] >= 0]).max() <= 3
    k = lc.ref("checkerboard_strong")
    assert 100 < k["n_found"] <= lc.MAX_LINES and min(k["n_regions"]) > 250
    # the bent edges: a region with exactly 2 s == n is no candidate; a candidate with s < n is fitted over all its pixels
    st = lc.ref_stages("bent_half"); A = st["nameA"]; name = 78
    assert int((A == name).sum()) == 270 and int(((A == name) & (st["vote"] == 0)).sum()) == 135
    assert name not in lc.ref("bent_half")["info"][:, 0].tolist() and lc.ref("bent_half")["n_found"] == 1
    v = lc.ref("bent_voters")
    assert v["info"].tolist() == [[1309, 1, 193, 193], [78, 0, 186, 94]]
    # OVERFLOW: the first max_lines of the ranking are the same segments
    full = lc.ref("131x97"); four = lc.ref("131x97", max_lines=4)
    assert full["n_found"] > 4 and four["status"] == ld_ref.OVERFLOW and four["n_returned"] == 4 and four["n_found"] == full["n_found"]
    assert np.array_equal(bits(four["seg"]), bits(full["seg"][:4])) and full["status"] == ld_ref.OK
    assert (np.diff(full["length"]) <= 0).all()


# ================================================================ CPU: what the reference finds in the scenes
@pytest.mark.parametrize("name", sorted(lc.SCENES))
def test_both_long_edges_of_every_bar_are_found(name):
    sc = lc.scene(name)
    for which in "AB":
        r = lc.ref(name, which)
        edges = sc["edges_" + which.lower()]
        worst_off, worst_cover = 0.0, 1.0
        for e in edges:
            fits = [lc.edge_report(s, e) for s in r["seg"]]
            fits = [f for f in fits if f[0] <= 1.0]
            assert fits, (name, which, e.tolist())
            off, cover = max(fits, key=lambda f: f[1])
            worst_off = max(worst_off, off); worst_cover = min(worst_cover, cover)
        print(f"{name} {which}: {len(edges)} edges, worst cover {worst_cover:.3f}, worst offset {worst_off:.3f} px")
        assert worst_cover >= 0.9 and worst_off <= 1.0
        assert int((r["length"] >= lc.LONG).sum()) == len(edges)          # exactly two long segments per bar
        assert r["status"] == ld_ref.OK


@pytest.mark.parametrize("name", sorted(lc.SCENES))
def test_every_long_line_of_b_continues_its_line_of_a(name):
    sc = lc.scene(name)
    ra = lc.ref(name, "A"); rb = lc.ref(name, "B")
    slot = lt_ref.Slot(lt_cases.MAX_LENGTH)
    slot.track(sc["A"], ra["seg"]); w = slot.track(sc["B"], rb["seg"])
    mid_a = 0.5 * (ra["seg"][:, :2] + ra["seg"][:, 2:]) + np.array(lc.SHIFT, np.float64)
    long_b = np.flatnonzero(rb["length"] >= lc.LONG)
    assert len(long_b) == len(sc["edges_b"])
    for j in long_b:
        d = np.linalg.norm(mid_a - 0.5 * (rb["seg"][j, :2] + rb["seg"][j, 2:]), axis=1)
        i = int(np.argmin(d))
        assert d[i] <= 1.5 and w["prev_index"][j] == i, (name, int(j), float(d[i]))


@pytest.mark.parametrize("variant", ld_ref.VARIANTS)
def test_each_planted_misreading_changes_a_returned_value(variant):
    changed = []
    for name in lc.SMALL + lc.CRAFTED_SMALL:
        good = lc.ref(name); bad = lc.ref(name, variant=variant)
        same = (good["n_found"] == bad["n_found"] and np.array_equal(good["info"], bad["info"]) and np.array_equal(bits(good["seg"]), bits(bad["seg"]))
                and np.array_equal(bits(good["width2"]), bits(bad["width2"])))
        if not same:
            changed.append(name)
    print(variant, "changes", changed)
    assert changed, variant


# ================================================================ CPU: layout, symbols, the host mirror
def test_ld_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "uvs_solver.h")).read()
    L = uvs.api.lib()
    for s in LD_SYMBOLS:
        assert s + "(" in hdr and s in uvs.api.EXPORTS and hasattr(L, s), s
    assert "#define UVS_ABI_VERSION 7" in hdr and L.uvs_abi_version() == 7
    Hst = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
    for s in HOST_SYMBOLS:
        assert hasattr(Hst, s), s
    assert L.uvs_lt_last_detect_device_ms(None) == 0.0


def test_ld_struct_layout_matches_header():
    code = r'''
#include <stdio.h>
#include <stddef.h>
#include "uvs_solver.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(uvs_lt_det_item), offsetof(uvs_lt_det_item, image), offsetof(uvs_lt_det_item, stream),
         offsetof(uvs_lt_det_item, width), offsetof(uvs_lt_det_item, height), offsetof(uvs_lt_det_item, reserved));
  printf("%zu %zu %zu %zu\n", sizeof(uvs_lt_det_params), offsetof(uvs_lt_det_params, grad_threshold), offsetof(uvs_lt_det_params, min_pixels),
         offsetof(uvs_lt_det_params, min_length));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(uvs_lt_det_result), offsetof(uvs_lt_det_result, status), offsetof(uvs_lt_det_result, n_found),
         offsetof(uvs_lt_det_result, n_returned), offsetof(uvs_lt_det_result, n_support), offsetof(uvs_lt_det_result, n_regions));
  printf("%d %d %d\n", UVS_LT_DET_MAX_THRESHOLD, UVS_LT_DET_OK, UVS_LT_DET_OVERFLOW);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c"); exe = os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    I, Pm, R = abi.LtDetItem, abi.LtDetParams, abi.LtDetResult
    assert out[:6] == [C.sizeof(I), I.image.offset, I.stream.offset, I.width.offset, I.height.offset, I.reserved.offset]
    assert out[6:10] == [C.sizeof(Pm), Pm.grad_threshold.offset, Pm.min_pixels.offset, Pm.min_length.offset]
    assert out[10:16] == [C.sizeof(R), R.status.offset, R.n_found.offset, R.n_returned.offset, R.n_support.offset, R.n_regions.offset]
    assert out[16:] == [abi.LT_DET_MAX_THRESHOLD, abi.LT_DET_OK, abi.LT_DET_OVERFLOW] and (ld_ref.OK, ld_ref.OVERFLOW) == (abi.LT_DET_OK, abi.LT_DET_OVERFLOW)
    arr, keep = abi.lt_det_items([dict(image=np.zeros((30, 40), np.uint8), stream=2)])
    assert (arr[0].width, arr[0].height, arr[0].stream, arr[0].reserved) == (40, 30, 2, 0)


class HostDetect(HostLines):
    """HostLines with the hooks of the overload of readImage4Line without segments; device == -2: the stub whose detection is injected."""

    def __init__(self, device, **kw):
        if device == -2:
            L = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
            L.uvs_host_lt_stub_create.restype = C.c_void_p; L.uvs_host_lt_stub_create.argtypes = [abi.c_double_p, C.c_int, C.c_int]
            HostLines.__init__(self, -1, **kw)
            self.close()
            m = kw.get("margins", (0, 0))
            self.h = L.uvs_host_lt_stub_create(abi._dp(np.array(kw.get("cam", lt_cases.CAM), np.float64)), m[0], m[1])
            assert self.h
        else:
            HostLines.__init__(self, device, **kw)
        L = self.L
        L.uvs_host_lt_stub_inject.argtypes = [C.c_void_p, C.c_int, C.c_int, abi.c_double_p, abi.c_i32_p]
        L.uvs_host_lt_stub_finished.argtypes = [C.c_void_p]
        L.uvs_host_lt_set_detect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double]
        L.uvs_host_lt_read_image_detect.argtypes = [C.c_void_p, abi.c_u8_p, C.c_int, C.c_int, C.c_double]
        L.uvs_host_lt_last_detect.argtypes = [C.c_void_p, C.c_int, abi.c_double_p, abi.c_double_p, abi.c_i32_p, abi.c_i32_p, abi.c_i32_p]

    def inject(self, segs, prev_index, rc=0):
        segs = np.ascontiguousarray(segs, np.float64).reshape(-1, 4); pi = np.ascontiguousarray(prev_index, np.int32)
        return self.L.uvs_host_lt_stub_inject(self.h, rc, len(segs), abi._dp(segs) if len(segs) else None, pi.ctypes.data_as(abi.c_i32_p) if len(pi) else None)

    def read_image_detect(self, img, time):
        img = np.ascontiguousarray(img, np.uint8)
        return self.L.uvs_host_lt_read_image_detect(self.h, img.ctypes.data_as(abi.c_u8_p), img.shape[1], img.shape[0], time)

    def last_detect(self):
        res = np.zeros(6, np.int32)
        n = self.L.uvs_host_lt_last_detect(self.h, 0, None, None, None, None, res.ctypes.data_as(abi.c_i32_p))
        m = max(n, 1)
        seg = np.zeros((m, 4)); w2 = np.zeros(m); info = np.zeros((m, 4), np.int32); prev = np.zeros(m, np.int32)
        assert self.L.uvs_host_lt_last_detect(self.h, m, abi._dp(seg), abi._dp(w2), abi._ip(info), abi._ip(prev), res.ctypes.data_as(abi.c_i32_p)) == n
        return dict(seg=seg[:n], width2=w2[:n], info=info[:n], prev_index=prev[:n], status=int(res[0]), n_found=int(res[1]), n_returned=int(res[2]),
                    n_support=int(res[3]), n_regions=[int(res[4]), int(res[5])])


def test_host_mirror_overload_with_an_injected_detection():
    """readImage4Line(img, width, height, time): ids, counts, gate points and normalized points from a detection given by hand."""
    h = HostDetect(-2, margins=(8, 4))
    img = np.zeros((40, 60), np.uint8)
    segA = np.array([[10.5, 20.25, 50.0, 22.0], [70.9, 30.0, 30.1, 60.7], [5.0, 5.0, 5.0, 40.0]])
    assert h.inject(segA, np.full(3, -1, np.int32)) == 0 and h.read_image_detect(img, 0.1) == 0
    g = h.get()
    assert g["ids"].tolist() == [-1] * 3 and g["track_cnt"].tolist() == [1] * 3
    assert g["pts"].tolist() == [[10, 20, 50, 22], [30, 60, 70, 30], [5, 5, 5, 40]]
    assert np.array_equal(bits(g["un_pts"]), bits(lift_ref(g["pts"], lt_cases.CAM, (8, 4))))
    assert h.update_ids() == 3 and h.get()["ids"].tolist() == [0, 1, 2]
    d = h.last_detect()
    assert d["n_returned"] == 3 and np.array_equal(d["seg"], segA) and d["prev_index"].tolist() == [-1] * 3
    # frame 2: line 0 continues previous 2, line 1 is new, line 2 continues 0, line 3 points outside the previous lines
    segB = np.vstack([segA[[2, 1, 0]] + 2.0, [[100.0, 100.0, 140.0, 100.0]]])
    assert h.inject(segB, np.array([2, -1, 0, 7], np.int32)) == 0 and h.read_image_detect(img, 0.2) == 0
    g = h.get()
    assert g["ids"].tolist() == [2, -1, 0, -1] and g["track_cnt"].tolist() == [2, 1, 2, 1]
    assert h.update_ids() == 4 and h.get()["ids"].tolist() == [2, 3, 0, 4]
    # a failed detection changes nothing and does not reach the vanishing points' step
    assert h.inject(segA, np.array([0, 1, 2], np.int32), rc=abi.UVS_ERR_CAPACITY) == 0 and h.read_image_detect(img, 0.3) == abi.UVS_ERR_CAPACITY
    assert h.get()["ids"].tolist() == [2, 3, 0, 4] and h.L.uvs_host_lt_stub_finished(h.h) == 2
    # a frame in which nothing is detected leaves nothing, and the next frame's lines are new
    assert h.inject(np.zeros((0, 4)), np.zeros(0, np.int32)) == 0 and h.read_image_detect(img, 0.4) == 0 and len(h.get()["ids"]) == 0
    assert h.inject(segA[:2], np.array([0, 1], np.int32)) == 0 and h.read_image_detect(img, 0.5) == 0
    assert h.get()["ids"].tolist() == [-1, -1] and h.update_ids() == 2 and h.get()["ids"].tolist() == [5, 6]
    h.close()
    # the plain bookkeeping has no detector: the overload reports that and changes nothing
    b = HostDetect(-1)
    assert b.read_image_detect(img, 0.1) == abi.UVS_ERR_NO_DEVICE and len(b.get()["ids"]) == 0
    b.close()


# ================================================================ GPU
@pytest.fixture(scope="module")
def tracker():
    """Two slots of the small scenes' size."""
    t = uvs.api.LineTracker(device=0, max_streams=2, max_width=131, max_height=97, max_lines=lc.MAX_LINES, max_length=lt_cases.MAX_LENGTH)
    yield t
    t.close()


@pytest.fixture(scope="module")
def big():
    """One slot of the 376 x 240 images."""
    t = uvs.api.LineTracker(device=0, max_streams=1, max_width=376, max_height=240, max_lines=lc.MAX_LINES, max_length=lt_cases.MAX_LENGTH)
    yield t
    t.close()


def _same_stages(got, want, what):
    for g, w in STAGES:
        assert got[g].dtype == want[w].dtype and np.array_equal(got[g], want[w]), (what, g)


@pytest.mark.gpu
@pytest.mark.parametrize("name", lc.SMALL + lc.CRAFTED_SMALL)
def test_gpu_debug_detect_stage_by_stage(tracker, name):
    img = lc.scene(name)["A"] if name in lc.SCENES else lc.crafted(name)
    _same_stages(tracker.debug_detect(img, **P), lc.ref_stages(name), name)
    if name in lc.SCENES:
        _same_stages(tracker.debug_detect(lc.scene(name)["B"], **P), lc.ref_stages(name, "B"), name + " B")


@pytest.mark.gpu
def test_gpu_debug_detect_corner_to_corner(big):
    _same_stages(big.debug_detect(lc.crafted("corner_to_corner"), **P), lc.ref_stages("corner_to_corner"), "corner_to_corner")


@pytest.mark.gpu
def test_gpu_detect_each_small_scene_alone_and_in_a_batch(tracker):
    sc = [lc.scene(n) for n in lc.SMALL]
    for which in "AB":
        alone = [tracker.detect([dict(image=s[which])], **P)[0] for s in sc]
        for n, a in zip(lc.SMALL, alone):
            same_detection(a, lc.ref(n, which), (n, which))
            assert a["tail_is_zero"]
        # two items of different sizes in one batch, in either order: each equals itself alone
        for order in ((0, 1), (1, 0)):
            batch = tracker.detect([dict(image=sc[i][which]) for i in order], **P)
            for k, i in enumerate(order):
                same_detection(batch[k], lc.ref(lc.SMALL[i], which), (lc.SMALL[i], which, "batch", order))
                for key in ("seg", "width2"):
                    assert np.array_equal(bits(batch[k][key]), bits(alone[i][key]))
    assert tracker.last_detect_device_ms > 0.0 and tracker.last_ms >= tracker.last_detect_device_ms


@pytest.mark.gpu
def test_gpu_detect_overflow_returns_the_head_of_the_ranking():
    t = uvs.api.LineTracker(device=0, max_streams=1, max_width=131, max_height=97, max_lines=4, max_length=lt_cases.MAX_LENGTH)
    got = t.detect([dict(image=lc.scene("131x97")["A"])], **P)[0]
    # with other parameters very many short segments are kept: the search for the last returned key runs over a long list
    many = t.detect([dict(image=lc.scene("131x97")["A"])], grad_threshold=4, min_pixels=2, min_length=0.5)[0]
    t.close()
    same_detection(got, lc.ref("131x97", max_lines=4), "overflow")
    assert got["det_status"] == abi.LT_DET_OVERFLOW and got["n_returned"] == 4 < got["n_found"]
    want = ld_ref.detect(lc.scene("131x97")["A"], 4, 2, 0.5, 4)
    assert want["n_found"] > 100
    same_detection(many, want, "overflow, many kept")


@pytest.mark.gpu
def test_gpu_detect_crafted_images(tracker):
    for name in lc.CRAFTED_SMALL:
        got = tracker.detect([dict(image=lc.crafted(name))], **P)[0]
        same_detection(got, lc.ref(name), name)
    const = tracker.detect([dict(image=lc.crafted("constant"))], **P)[0]
    assert (const["n_found"], const["n_support"], const["n_regions"]) == (0, 0, [0, 0]) and const["tail_is_zero"]
    H, W = lc.crafted("ramp").shape
    ramp = tracker.detect([dict(image=lc.crafted("ramp"))], **P)[0]
    assert ramp["n_regions"] == [1, 1] and ramp["n_found"] == 1 and ramp["info"][0, 1] == 0 and ramp["info"][0, 2] == ramp["info"][0, 3] == ramp["n_support"] > (W - 8) * H
    # ties in the ranking: a mirrored pair of edges has two segments of exactly one length; the name decides
    img = np.full((48, 80), 60, np.uint8); img[:, 20:60] = 190
    got = tracker.detect([dict(image=img)], **P)[0]
    want = ld_ref.detect(img, T, MIN_PIXELS, MIN_LENGTH, lc.MAX_LINES)
    same_detection(got, want, "mirrored edges")
    assert want["n_found"] == 2 and want["length"][0] == want["length"][1] and want["info"][0, 0] < want["info"][1, 0]


@pytest.mark.gpu
def test_gpu_detect_corner_to_corner_and_the_large_scene(big):
    got = big.detect([dict(image=lc.crafted("corner_to_corner"))], **P)[0]
    same_detection(got, lc.ref("corner_to_corner"), "corner_to_corner")
    got = big.detect([dict(image=lc.scene("376x240")["A"])], **P)[0]
    same_detection(got, lc.ref("376x240"), "376x240")
    assert int((np.hypot(got["seg"][:, 2] - got["seg"][:, 0], got["seg"][:, 3] - got["seg"][:, 1]) >= lc.LONG).sum()) == len(lc.scene("376x240")["edges_a"])


def _same_track(got, want, what):
    for k in ("desc", "status", "prev_index", "distance"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert (got["n_described"], got["n_matched"]) == (want["n_described"], want["n_matched"]), what


@pytest.mark.gpu
def test_gpu_detect_track_equals_detect_then_track_and_the_replay(tracker):
    sc = [lc.scene(n) for n in lc.SMALL]
    for s in range(2):
        tracker.reset(s)
    # one call per frame, both slots in it (the second frame lists the slots the other way round)
    fa = tracker.detect_track([dict(stream=s, image=sc[s]["A"]) for s in (0, 1)], **P)
    fb = tracker.detect_track([dict(stream=s, image=sc[s]["B"]) for s in (1, 0)], **P)[::-1]
    # ... then a third frame through uvs_lt_track: the slots hold what detect_track left
    third = tracker.track([dict(stream=s, image=sc[s]["A"], segs=fa[s]["seg"]) for s in (0, 1)])
    # the same by uvs_lt_detect followed by uvs_lt_track
    for s in range(2):
        tracker.reset(s)
    da = tracker.detect([dict(image=sc[s]["A"]) for s in (0, 1)], **P)
    ta = tracker.track([dict(stream=s, image=sc[s]["A"], segs=da[s]["seg"]) for s in (0, 1)])
    db = tracker.detect([dict(image=sc[s]["B"]) for s in (0, 1)], **P)
    tb = tracker.track([dict(stream=s, image=sc[s]["B"], segs=db[s]["seg"]) for s in (0, 1)])
    third2 = tracker.track([dict(stream=s, image=sc[s]["A"], segs=da[s]["seg"]) for s in (0, 1)])
    for s, name in enumerate(lc.SMALL):
        same_detection(fa[s], lc.ref(name, "A"), (name, "A")); same_detection(fb[s], lc.ref(name, "B"), (name, "B"))
        _same_track(fa[s], ta[s], (name, "A")); _same_track(fb[s], tb[s], (name, "B")); _same_track(third[s], third2[s], (name, "third"))
        # the references' replay
        slot = lt_ref.Slot(lt_cases.MAX_LENGTH)
        wa = slot.track(sc[s]["A"], lc.ref(name, "A")["seg"]); wb = slot.track(sc[s]["B"], lc.ref(name, "B")["seg"])
        _same_track(fa[s], wa, (name, "A, replay")); _same_track(fb[s], wb, (name, "B, replay"))
        # every long line of B continues its own line of A
        mid_a = 0.5 * (fa[s]["seg"][:, :2] + fa[s]["seg"][:, 2:]) + np.array(lc.SHIFT, np.float64)
        for j in np.flatnonzero(np.hypot(*(fb[s]["seg"][:, 2:] - fb[s]["seg"][:, :2]).T) >= lc.LONG):
            d = np.linalg.norm(mid_a - 0.5 * (fb[s]["seg"][j, :2] + fb[s]["seg"][j, 2:]), axis=1)
            assert d.min() <= 1.5 and fb[s]["prev_index"][j] == int(np.argmin(d))
    assert tracker.last_detect_device_ms > 0.0


@pytest.mark.gpu
def test_gpu_argument_checks_leave_the_handle_usable(tracker):
    sc = lc.scene("96x80")
    a = dict(stream=0, image=sc["A"]); b = dict(stream=0, image=sc["B"])
    tracker.reset(0)
    fa = tracker.detect_track([a], **P)[0]
    small = np.zeros((7, 96), np.uint8); tall = np.zeros((98, 96), np.uint8); wide = np.zeros((80, 132), np.uint8)
    INV, CAP = abi.UVS_ERR_INVALID_ARG, abi.UVS_ERR_CAPACITY
    cases = [([b], dict(n_items=0), INV), ([b], dict(n_items=3), CAP), ([dict(b, image=small)], {}, INV), ([dict(b, image=tall)], {}, CAP),
             ([dict(b, image=wide)], {}, CAP), ([b], dict(grad_threshold=0), INV), ([b], dict(grad_threshold=2041), INV), ([b], dict(min_pixels=1), INV),
             ([b], dict(min_length=0.0), INV), ([b], dict(min_length=-1.0), INV), ([b], dict(min_length=float("nan")), INV), ([b], dict(min_length=float("inf")), INV)]
    both = cases + [([b], dict(null=(k,)), INV) for k in ("items", "params", "seg", "width2", "info", "det_results")]
    for items, kw, rc in both:
        assert tracker.detect_raw(items, **dict(P, **kw))[0] == rc, (kw, rc)
        assert "uvs_lt_detect" in tracker.last_error()
    track_only = [([dict(b, stream=2)], {}, INV), ([dict(b, stream=-1)], {}, INV), ([b, dict(b, image=sc["A"])], {}, INV)]
    track_only += [([b], dict(null=(k,)), INV) for k in ("desc", "line_status", "prev_index", "distance", "results")]
    for items, kw, rc in both + track_only:
        assert tracker.detect_track_raw(items, **dict(P, **kw))[0] == rc, (kw, rc)
        assert "uvs_lt_detect_track" in tracker.last_error()
    # uvs_lt_detect ignores the stream
    assert tracker.detect_raw([dict(b, stream=5)], **P)[0] == abi.UVS_OK
    for k in ("image", "params", "blur", "grad", "sector_a", "sector_b", "name_a", "name_b", "vote"):
        assert tracker.debug_detect_raw(sc["A"], null=(k,), **P)[0] == INV
    assert tracker.debug_detect_raw(tall, **P)[0] == CAP and tracker.debug_detect_raw(small, **P)[0] == INV
    assert tracker.debug_detect_raw(sc["A"], **dict(P, min_pixels=0))[0] == INV
    L = uvs.api.lib()
    assert L.uvs_lt_detect(None, 1, None, None, None, None, None, None) == INV
    # none of the rejected calls, and no stateless call, changed the slot: frame B still continues frame A's lines, as the replay says
    fb = tracker.detect_track([b], **P)[0]
    slot = lt_ref.Slot(lt_cases.MAX_LENGTH)
    slot.track(sc["A"], lc.ref("96x80", "A")["seg"]); wb = slot.track(sc["B"], lc.ref("96x80", "B")["seg"])
    same_detection(fb, lc.ref("96x80", "B"), "B after the rejected calls"); _same_track(fb, wb, "B after the rejected calls")
    assert fb["n_matched"] >= len(sc["edges_b"]) and tracker.last_error() == "" and fa["n_matched"] == 0


@pytest.mark.gpu
def test_gpu_host_mirror_read_image_without_segments_over_three_frames():
    """uvs::LineFeatureTracker::readImage4Line(image): the segments are uvs_lt_detect's, ids persist, track_cnt counts, vps are attached."""
    name = "131x97"
    sc = lc.scene(name)
    ra = lc.ref(name, "A"); rb = lc.ref(name, "B")
    h = HostDetect(0, max_width=131, max_height=97, max_lines=lc.MAX_LINES, th_angle=math.pi / 180.0)
    assert h.L.uvs_host_lt_set_detect(h.h, T, MIN_PIXELS, MIN_LENGTH) == 0
    slot = lt_ref.Slot(lt_cases.MAX_LENGTH)
    ids, cnt, next_id = np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    for f, (which, r) in enumerate((("A", ra), ("B", rb), ("A", ra))):
        assert h.read_image_detect(sc[which], 0.1 * (f + 1)) == 0
        w = slot.track(sc[which], r["seg"])
        d = h.last_detect()
        same_detection(d, r, (f, which))
        assert np.array_equal(d["prev_index"], w["prev_index"])
        n = r["n_returned"]
        desc, st, dist, res = h.last(n)
        assert np.array_equal(desc, w["desc"]) and np.array_equal(st, w["status"]) and np.array_equal(dist, w["distance"])
        assert res.tolist() == [w["n_described"], w["n_matched"]]
        # the bookkeeping of the reference on these matches
        cont = w["prev_index"] >= 0
        new_ids = np.where(cont, ids[np.maximum(w["prev_index"], 0)] if len(ids) else -1, -1)
        new_cnt = np.where(cont, (cnt[np.maximum(w["prev_index"], 0)] if len(cnt) else 0) + 1, 1)
        g = h.get()
        assert g["ids"].tolist() == new_ids.tolist() and g["track_cnt"].tolist() == new_cnt.tolist()
        assert np.array_equal(g["pts"], w["ends"].astype(np.float64)) and np.array_equal(bits(g["un_pts"]), bits(lift_ref(g["pts"], lt_cases.CAM)))
        assert g["vps"].shape == (n, 3) and set(np.unique(g["vps"][:, 2])) <= {0.0, 1.0}
        assert h.update_ids() == n
        for i in range(n):
            if new_ids[i] < 0:
                new_ids[i] = next_id; next_id += 1
        assert h.get()["ids"].tolist() == new_ids.tolist()
        ids, cnt = new_ids, new_cnt
        if f:
            assert int(cont.sum()) >= len(sc["edges_a"]) and cnt.max() == f + 1
    assert h.reset() == 0 and h.read_image_detect(sc["B"], 0.4) == 0 and h.get()["ids"].tolist() == [-1] * rb["n_returned"]
    h.close()
