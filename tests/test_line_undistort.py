"""Undistortion of the line front end's images (uvs_lt_set_undistort, uvs_lt_set_remap, uvs_lt_get_remap, uvs_lt_undistort and the mapped
slots of uvs_lt_detect_track; csrc/uvs_line_undistort.hip): a Q5 fixed-point map and a bilinear remap with a zero border, the project's own
rule (include/uvs_solver.h), pinned to tests/ud_ref.py word for word and byte for byte.  cv::undistort could not be compared; what pins the
rule is the header's statement, the two forms of it in ud_ref, known answers (no distortion, whole-pixel shifts, a half-pixel mean), planted
misreadings, and its accuracy on an analytic image rendered through kf_ref's inverse camera model.

CPU: the restatement against itself, the known answers, the misreadings, the accuracy, the straight edges of the reference's detection, the
header against abi.py.  GPU: the map, the image alone, in a batch and with a shared slot, uvs_lt_set_remap, uvs_lt_detect_track on raw frames
against undistort + detect_track, a mixed batch, the unmapped tracker against ld_cases, the straight edges, the argument checks, and
uvs::LineFeatureTracker::setUndistortion over three raw frames."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ld_cases as lc
import ld_ref
import lt_cases
import ud_cases as uc
import ud_ref
from helpers import abi, uvs
from test_line_detect import HostDetect, _same_track, bits, same_detection
from test_line_track import lift_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lc.PARAMS
UD_SYMBOLS = ["uvs_lt_set_undistort", "uvs_lt_set_remap", "uvs_lt_get_remap", "uvs_lt_undistort", "uvs_lt_last_undistort_device_ms"]
HOST_SYMBOLS = ["uvs_host_lt_set_undistortion"]
# the case on which each planted misreading must show
MISREADING_CASE = {"truncate": "40x32_m0_barrel", "round_511": "40x32_m0_barrel", "border_per_pixel": "96x80_m5_pincushion",
                   "p1_p2_swapped": "96x80_m0_barrel", "margin_after_map": "40x32_m5_barrel"}


# ================================================================ CPU: the restatement and its known answers
@pytest.mark.parametrize("name", uc.SMALL)
def test_vectorized_form_equals_loop_form(name):
    c = uc.CASES[name]
    m = ud_ref.build_map_loops(c["cam"], c["W"], c["H"], c["cm"], c["rm"])
    assert m.dtype == np.int32 and np.array_equal(m, uc.ref_map(name))
    assert np.array_equal(ud_ref.remap_loops(uc.raw(name), m), uc.ref_image(name))
    assert uc.ref_image(name).shape == (c["H"] - 2 * c["rm"], c["W"] - 2 * c["cm"])


def test_the_cases_cover_the_border_and_the_tail():
    outside = {}
    for name in uc.CASES:
        c = uc.CASES[name]; m = uc.ref_map(name)
        xi, yi = m[..., 0] >> 5, m[..., 1] >> 5
        outside[name] = int(((xi < 0) | (xi + 1 >= c["W"]) | (yi < 0) | (yi + 1 >= c["H"])).sum())
    assert all(outside[n] == 0 for n in uc.CASES if "barrel" in n)                  # a barrel map stays inside the source
    assert outside["131x97_m0_pincushion"] > 1000 and outside["96x80_m5_pincushion"] > 100
    # taps that straddle the border: some outputs there are neither zero nor a full interpolation
    m = uc.ref_map("131x97_m0_pincushion")
    assert int((uc.ref_image("131x97_m0_pincushion") == 0).sum()) > 500
    assert {(uc.ref_map(n).shape[0] * uc.ref_map(n).shape[1]) % 4 for n in uc.CASES} == {0, 3}      # 1 and 2: the hand-made maps of the GPU test


@pytest.mark.parametrize("margins", uc.MARGINS)
def test_zero_coefficients_give_the_cropped_input(margins):
    cm, rm = margins
    for name in ("40x32_m0_barrel", "131x97_m0_barrel"):
        c = uc.CASES[name]; img = uc.raw(name)
        cam = c["cam"][:4] + (0.0, 0.0, 0.0, 0.0)
        m = ud_ref.build_map(cam, c["W"], c["H"], cm, rm)
        vo, uo = np.mgrid[0:c["H"] - 2 * rm, 0:c["W"] - 2 * cm]
        assert np.array_equal(m[..., 0], 32 * (uo + cm)) and np.array_equal(m[..., 1], 32 * (vo + rm))
        assert np.array_equal(ud_ref.remap(img, m), img[rm:c["H"] - rm, cm:c["W"] - cm])


def test_whole_pixel_shifts_and_the_zero_border():
    img = uc.raw("40x32_m0_barrel"); H, W = img.shape
    vo, uo = np.mgrid[0:H, 0:W]
    for dx, dy in ((3, 0), (0, -2), (-5, 4), (W, 0), (-1, -1)):
        m = np.stack([32 * (uo + dx), 32 * (vo + dy)], -1).astype(np.int32)
        want = np.zeros_like(img)
        ys, xs = vo + dy, uo + dx
        ok = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
        want[ok] = img[ys[ok], xs[ok]]
        assert np.array_equal(ud_ref.remap(img, m), want), (dx, dy)
    # a map may be of any size and point anywhere: far outside is zero, and the clamp of uvs_lt_set_remap keeps it far outside
    far = np.full((9, 10, 2), 2 ** 31 - 1, np.int32); far[..., 1] = -2 ** 31
    assert np.array_equal(ud_ref.clamp_map(far)[0, 0], [2 ** 24, -2 ** 24]) and not ud_ref.remap(img, ud_ref.clamp_map(far)).any()


def test_half_pixel_mean_on_a_two_column_step():
    src = np.zeros((8, 8), np.uint8); src[:, 0] = 10; src[:, 1] = 21
    m = np.zeros((8, 8, 2), np.int32); m[..., 0] = 16; m[..., 1] = 32 * np.arange(8)[:, None]      # x = 0.5 (ax = 16), y whole (ay = 0)
    # (16 * 32 * 10 + 16 * 32 * 21 + 512) >> 10 = (15872 + 512) >> 10 = 16: the mean 15.5 rounds up
    assert (ud_ref.remap(src, m) == 16).all() and (ud_ref.remap_loops(src, m) == 16).all()
    assert (ud_ref.remap(src, m, "round_511") == 15).all()
    # the same half pixel across the left border: one tap is outside and counts as zero, the other is 10 -> 5
    m[..., 0] = -16
    assert (ud_ref.remap(src, m) == 5).all() and not ud_ref.remap(src, m, "border_per_pixel").any()
    # the weights sum to 1024: a constant image stays constant, 255 does not saturate
    full = np.full((8, 8), 255, np.uint8)
    m[..., 0] = 32 * 3 + 13; m[..., 1] = 32 * 3 + 29
    assert (ud_ref.remap(full, m) == 255).all()


@pytest.mark.parametrize("variant", ud_ref.VARIANTS)
def test_each_planted_misreading_changes_a_returned_value(variant):
    changed = [n for n in uc.SMALL
               if not (np.array_equal(uc.ref_map(n), uc.ref_map(n, variant)) and np.array_equal(uc.ref_image(n), uc.ref_image(n, variant)))]
    print(variant, "changes", changed)
    assert MISREADING_CASE[variant] in changed, variant
    if variant == "margin_after_map":            # without margins there is nothing to misplace
        assert all("_m5_" in n for n in changed)


def _accuracy_terms(cam, W, H):
    """The constants of test_accuracy_on_an_analytic_image's bound for the camera, over the ideal pixels of the image grown by 4 px."""
    fx, fy, cx, cy, k1, k2, p1, p2 = cam
    assert fx == fy
    xs = np.array([-4.0, W + 3.0]); ys = np.array([-4.0, H + 3.0])
    s_max = max(((x - cx) / fx) ** 2 + ((y - cy) / fy) ** 2 for x in xs for y in ys)
    s = np.linspace(0.0, s_max, 20001); r = np.sqrt(s)
    kr = 1 + k1 * s + k2 * s * s; dkr = k1 + 2 * k2 * s
    pt = abs(p1) + abs(p2)
    sigma = float(np.minimum(np.abs(kr), np.abs(kr + 2 * s * dkr)).min()) - 12 * pt * math.sqrt(s_max)
    M2 = float((6 * np.abs(dkr) * r + 8 * abs(k2) * r ** 3).max()) + 12 * pt
    assert sigma > 0.3
    L = 1.0 / sigma
    return L, L ** 3 * M2 / fx


def test_accuracy_on_an_analytic_image():
    """A smooth image I (three sinusoids, in pixels of the distortion-free camera) is rendered into the raw frame through kf_ref's inverse model
    (ud_cases.ideal_of_raw: liftProjective, iterated on; g~), rounded to 8 bits, undistorted by ud_ref and compared with I at the output pixels.

    The bound, with d the forward model (ideal pixel -> raw pixel), g = d^-1, R = I o g the exact raw image, G_I = sum A |k| >= |grad I|,
    C_I = sum A |k|^2 >= |Hess I|, L = 1 / sigma_min(Dd) >= |Dg| and H = L^3 |D^2 d| >= |D^2 g| (from D^2 g = -Dg D^2 d [Dg ., Dg .]):
      0.5                        the remap's rounding ((s + 512) >> 10)
      0.5                        the raw frame's rounding to 8 bits, under weights that sum to one
      G_I L sqrt(2) rho          the inverse model's residual rho (raw px, measured on kf_ref alone): |g~ - g| <= L sqrt(2) rho
      (C_I L^2 + G_I H) / 4      the bilinear remainder (1/8)(|R_xx| + |R_yy|) on a unit cell, |Hess R| <= |Hess I| |Dg|^2 + |grad I| |D^2 g|
      G_I L sqrt(2) / 64         the map's quantisation, at most 1/64 px per axis, times |grad R| <= G_I L
    sigma_min and |D^2 d| come from the radial model's closed forms (the Jacobian's eigenvalues kr and kr + 2 s kr' at s = r^2; the second
    derivative at most 6 |kr'| r + 8 |k2| r^3, divided by fx for pixels) on a fine grid of s over the image grown by 4 px, with 12 (|p1| + |p2|)
    (times r for the Jacobian) allowed for the tangential terms.  For this case the bound is 2.37 grey levels and the measured maximum 1.00 (also in DESIGN.md 3.17)."""
    name = "131x97_m0_barrel"
    c = uc.CASES[name]; W, H, cam = c["W"], c["H"], c["cam"]
    A = np.array([40.0, 30.0, 20.0]); lam = np.array([90.0, 70.0, 60.0]); th = np.array([0.3, 1.9, 2.8]); ph = np.array([0.5, 2.0, 4.0])
    k = 2 * np.pi / lam
    I = lambda x, y: 128.0 + sum(A[i] * np.sin(k[i] * (np.cos(th[i]) * x + np.sin(th[i]) * y) + ph[i]) for i in range(3))
    G_I = float((A * k).sum()); C_I = float((A * k * k).sum())
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    ideal, rho = uc.ideal_of_raw(cam, np.stack([u.ravel(), v.ravel()], 1))
    raw = I(ideal[:, 0], ideal[:, 1]).reshape(H, W)
    assert raw.min() >= 0.0 and raw.max() <= 255.0 and rho < 1e-9
    out = ud_ref.undistort(np.rint(raw).astype(np.uint8), cam)
    m = uc.ref_map(name); xi, yi = m[..., 0] >> 5, m[..., 1] >> 5
    inside = (xi >= 0) & (xi + 1 < W) & (yi >= 0) & (yi + 1 < H)
    assert inside.all()                          # the barrel map never reaches the zero border
    L, Hg = _accuracy_terms(cam, W, H)
    bound = 0.5 + 0.5 + G_I * L * math.sqrt(2) * rho + (C_I * L * L + G_I * Hg) / 4 + G_I * L * math.sqrt(2) / 64
    err = float(np.abs(out.astype(np.float64) - I(u, v))[inside].max())
    print(f"accuracy: G_I {G_I:.3f}, C_I {C_I:.4f}, L {L:.3f}, H {Hg:.4f}, rho {rho:.2e}: bound {bound:.3f}, measured maximum {err:.3f} grey levels")
    assert 2.0 < bound < 2.6 and err <= bound
    # the comparison sees a map that is off by a pixel
    off = ud_ref.remap(np.rint(raw).astype(np.uint8), m + np.array([32, 0], np.int32))
    assert float(np.abs(off.astype(np.float64) - I(u, v))[inside & (xi + 2 < W)].max()) > bound


def test_straight_edges_in_the_reference_detection():
    """The bars of ld_cases through the barrel camera: ld_ref finds both long edges of every bar in ud_ref's undistorted image under
    test_line_detect's thresholds (cover >= 0.9, offset <= 1.0 px: they did not have to move for the interpolation's blur), and loses some of
    them in the raw frame, where they are bent."""
    sc = uc.bar_scene()
    fits = uc.edge_fits(uc.bar_ref("undistorted")["seg"], sc["edges"])
    assert all(f is not None and f[1] >= 0.9 and f[0] <= 1.0 for f in fits), fits
    bent = uc.edge_fits(uc.bar_ref("raw")["seg"], sc["edges"])
    assert sum(f is None or f[1] < 0.9 or f[0] > 1.0 for f in bent) >= 1, bent
    assert not (sc["undistorted"] == 0).any() and len(sc["edges"]) >= 4


# ================================================================ CPU: symbols
def test_ud_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "uvs_solver.h")).read()
    L = uvs.api.lib()
    for s in UD_SYMBOLS:
        assert s + "(" in hdr and s in uvs.api.EXPORTS and hasattr(L, s), s
    assert "#define UVS_ABI_VERSION 7" in hdr and L.uvs_abi_version() == 7
    Hst = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
    for s in HOST_SYMBOLS:
        assert hasattr(Hst, s), s
    assert L.uvs_lt_last_undistort_device_ms(None) == 0.0
    INV = abi.UVS_ERR_INVALID_ARG
    assert L.uvs_lt_set_undistort(None, 0, None, 8, 8, 0, 0) == INV and L.uvs_lt_set_remap(None, 0, 8, 8, 8, 8, None) == INV
    assert L.uvs_lt_get_remap(None, 0, None, None, None) == INV and L.uvs_lt_undistort(None, 1, None, None) == INV


# ================================================================ GPU
@pytest.fixture(scope="module")
def tracker():
    """Four slots of the small cases' size."""
    t = uvs.api.LineTracker(device=0, max_streams=4, max_width=uc.MAX_W, max_height=uc.MAX_H, max_lines=lc.MAX_LINES, max_length=lt_cases.MAX_LENGTH)
    yield t
    t.close()


def _set(t, stream, name):
    c = uc.CASES[name]
    t.set_undistort(stream, c["cam"], c["W"], c["H"], c["cm"], c["rm"])


@pytest.mark.gpu
def test_gpu_map_and_image_of_every_small_case(tracker):
    for name in uc.SMALL:
        _set(tracker, 0, name)
        m = tracker.get_remap(0)
        assert m.dtype == np.int32 and m.shape == uc.ref_map(name).shape and np.array_equal(m, uc.ref_map(name)), name
        assert tracker.get_remap_raw(0, sizes_only=True) == (abi.UVS_OK, m.shape[1::-1])
        got = tracker.undistort([dict(stream=0, image=uc.raw(name))])[0]
        assert got.dtype == np.uint8 and np.array_equal(got, uc.ref_image(name)), name
    assert tracker.last_undistort_device_ms > 0.0 and tracker.last_ms >= tracker.last_undistort_device_ms
    tracker.set_undistort(0, None, 0, 0)


@pytest.mark.gpu
def test_gpu_batches_and_a_shared_slot(tracker):
    # four cases of three sizes in one batch, in two orders; then all twelve, four at a time
    for names in (uc.SMALL[0:4], uc.SMALL[2:6][::-1], uc.SMALL[4:8], uc.SMALL[8:12]):
        for s, n in enumerate(names):
            _set(tracker, s, n)
        got = tracker.undistort([dict(stream=s, image=uc.raw(n)) for s, n in enumerate(names)])
        for g, n in zip(got, names):
            assert np.array_equal(g, uc.ref_image(n)), (names, n)
    # two images through one slot, and a third through another, in one call
    a, b = "131x97_m5_pincushion", "131x97_m0_barrel"
    _set(tracker, 2, a); _set(tracker, 0, b)
    other = np.ascontiguousarray(uc.raw(a)[::-1, ::-1])
    got = tracker.undistort([dict(stream=2, image=uc.raw(a)), dict(stream=0, image=uc.raw(b)), dict(stream=2, image=other)])
    assert np.array_equal(got[0], uc.ref_image(a)) and np.array_equal(got[1], uc.ref_image(b))
    assert np.array_equal(got[2], ud_ref.remap(other, uc.ref_map(a)))
    for s in range(4):
        tracker.set_undistort(s, None, 0, 0)


@pytest.mark.gpu
def test_gpu_the_large_case():
    c = uc.CASES[uc.LARGE]
    t = uvs.api.LineTracker(device=0, max_streams=1, max_width=c["W"], max_height=c["H"], max_lines=lc.MAX_LINES, max_length=lt_cases.MAX_LENGTH)
    _set(t, 0, uc.LARGE)
    m = t.get_remap(0); got = t.undistort([dict(stream=0, image=uc.raw(uc.LARGE))])[0]
    t.close()
    assert np.array_equal(m, uc.ref_map(uc.LARGE)) and np.array_equal(got, uc.ref_image(uc.LARGE))


@pytest.mark.gpu
def test_gpu_set_remap_round_trips_and_drives_the_same_kernel(tracker):
    name = "96x80_m5_pincushion"
    c = uc.CASES[name]
    tracker.set_remap(1, c["W"], c["H"], uc.ref_map(name))
    assert np.array_equal(tracker.get_remap(1), uc.ref_map(name))
    assert np.array_equal(tracker.undistort([dict(stream=1, image=uc.raw(name))])[0], uc.ref_image(name))
    # hand-made maps of any size: pixel counts that leave one and two pixels to the last lane, positions on and far beyond every border
    img = uc.raw(name)
    rng = np.random.default_rng(7)
    for ho, wo in ((9, 9), (9, 10), (8, 8), (97, 131)):
        m = rng.integers(-3 * 32, (max(c["W"], c["H"]) + 3) * 32, (ho, wo, 2)).astype(np.int32)
        m[0, :4] = [[2 ** 31 - 1, 5], [-2 ** 31, 64], [40, 2 ** 31 - 1], [-1, -1]]
        m[1, :4] = [[-32, 0], [32 * c["W"] - 32, 32 * c["H"] - 32], [32 * c["W"] - 31, 32 * c["H"] - 31], [32 * c["W"], 0]]
        tracker.set_remap(1, c["W"], c["H"], m)
        assert np.array_equal(tracker.get_remap(1), ud_ref.clamp_map(m)), (ho, wo)
        got = tracker.undistort([dict(stream=1, image=img)])[0]
        assert got.shape == (ho, wo) and np.array_equal(got, ud_ref.remap(img, ud_ref.clamp_map(m))), (ho, wo)
    tracker.set_undistort(1, None, 0, 0)


def _frames():
    """Three raw frames of the bar scene, two pixels apart: the lines of one continue those of the last."""
    r = uc.bar_scene()["raw"]
    return [r, np.ascontiguousarray(np.roll(r, (2, 2), (0, 1))), np.ascontiguousarray(np.roll(r, (4, 3), (0, 1)))]


def _same_frame(got, want, what):
    same_detection(got, dict(want, status=want["det_status"]), what)
    _same_track(got, want, what)


@pytest.mark.gpu
def test_gpu_detect_track_on_raw_frames_equals_undistort_then_detect_track(tracker):
    sc = uc.bar_scene()
    plain = uvs.api.LineTracker(device=0, max_streams=1, max_width=uc.MAX_W, max_height=uc.MAX_H, max_lines=lc.MAX_LINES, max_length=lt_cases.MAX_LENGTH)
    tracker.reset(0)
    tracker.set_undistort(0, sc["cam"], sc["W"], sc["H"], 5, 3)
    last = None
    for f, raw in enumerate(_frames()):
        und = tracker.undistort([dict(stream=0, image=raw)])[0]
        assert und.shape == (sc["H"] - 6, sc["W"] - 10) and np.array_equal(und, ud_ref.undistort(raw, sc["cam"], 5, 3))
        got = tracker.detect_track([dict(stream=0, image=raw)], **P)[0]
        want = plain.detect_track([dict(stream=0, image=und)], **P)[0]
        _same_frame(got, want, f)
        assert got["n_returned"] >= 6 and (f == 0 or got["n_matched"] >= 4)
        last = (und, got["seg"])
    # the slots afterwards: one more frame through uvs_lt_track, which takes the image as it is
    a = tracker.track([dict(stream=0, image=last[0], segs=last[1])])[0]
    b = plain.track([dict(stream=0, image=last[0], segs=last[1])])[0]
    _same_track(a, b, "the slots afterwards")
    assert a["n_matched"] >= 6
    # the first frame of all is also the reference detection of ud_ref's image
    tracker.reset(0)
    tracker.set_undistort(0, sc["cam"], sc["W"], sc["H"])
    got = tracker.detect_track([dict(stream=0, image=sc["raw"])], **P)[0]
    same_detection(got, uc.bar_ref("undistorted"), "margins 0 against ld_ref")
    plain.close()
    tracker.set_undistort(0, None, 0, 0)


@pytest.mark.gpu
def test_gpu_mixed_batch_gives_each_item_its_solitary_bits(tracker):
    sc = uc.bar_scene(); frames = _frames()
    small = lc.scene("96x80")
    tracker.set_undistort(0, sc["cam"], sc["W"], sc["H"], 5, 3)

    def run(batched):
        for s in (0, 1):
            tracker.reset(s)                      # the map stays
        out = []
        for f in range(2):
            items = [dict(stream=0, image=frames[f]), dict(stream=1, image=small["AB"[f]])]
            if f:
                items = items[::-1]
            res = tracker.detect_track(items, **P) if batched else [tracker.detect_track([it], **P)[0] for it in items]
            out.append(res[::-1] if f else res)
        return out

    alone = run(False); batch = run(True)
    for f in range(2):
        for s in (0, 1):
            _same_frame(batch[f][s], alone[f][s], (f, s))
        same_detection(batch[f][1], lc.ref("96x80", "AB"[f]), ("the plain slot", f))
    assert batch[1][0]["n_matched"] >= 4 and batch[1][1]["n_matched"] >= 4
    tracker.set_undistort(0, None, 0, 0)


@pytest.mark.gpu
def test_gpu_a_tracker_without_a_map_returns_what_ld_cases_expects(tracker):
    for s in range(2):
        tracker.reset(s)
    sc = [lc.scene(n) for n in lc.SMALL]
    fa = tracker.detect_track([dict(stream=s, image=sc[s]["A"]) for s in (0, 1)], **P)
    # a map that was set and switched off again leaves nothing behind
    _set(tracker, 1, "131x97_m5_barrel")
    tracker.set_undistort(1, None, 0, 0)
    fb = tracker.detect_track([dict(stream=s, image=sc[s]["B"]) for s in (0, 1)], **P)
    for s, name in enumerate(lc.SMALL):
        same_detection(fa[s], lc.ref(name, "A"), (name, "A")); same_detection(fb[s], lc.ref(name, "B"), (name, "B"))
        assert fb[s]["n_matched"] >= len(sc[s]["edges_b"])
    assert tracker.get_remap_raw(1)[0] == abi.UVS_ERR_INVALID_ARG


@pytest.mark.gpu
def test_gpu_straight_edges_after_the_undistortion(tracker):
    sc = uc.bar_scene()
    tracker.reset(0)
    tracker.set_undistort(0, sc["cam"], sc["W"], sc["H"])
    got = tracker.detect_track([dict(stream=0, image=sc["raw"])], **P)[0]
    tracker.set_undistort(0, None, 0, 0)
    tracker.reset(0)
    bent = tracker.detect_track([dict(stream=0, image=sc["raw"])], **P)[0]
    fits = uc.edge_fits(got["seg"], sc["edges"])
    print("undistorted:", fits)
    assert all(f is not None and f[1] >= 0.9 and f[0] <= 1.0 for f in fits), fits
    worse = uc.edge_fits(bent["seg"], sc["edges"])
    print("raw:", worse)
    assert sum(f is None or f[1] < 0.9 or f[0] > 1.0 for f in worse) >= 1, worse


@pytest.mark.gpu
def test_gpu_argument_checks_leave_the_handle_usable(tracker):
    sc = uc.bar_scene(); cam = sc["cam"]; img = sc["raw"]; W, H = sc["W"], sc["H"]
    INV, CAP = abi.UVS_ERR_INVALID_ARG, abi.UVS_ERR_CAPACITY
    tracker.reset(0)
    tracker.set_undistort(0, cam, W, H, 5, 3)
    first = tracker.detect_track([dict(stream=0, image=img)], **P)[0]
    nan = float("nan")
    for args, rc in (((4, cam, W, H, 5, 3), INV), ((-1, cam, W, H, 5, 3), INV), ((0, (nan,) + cam[1:], W, H, 5, 3), INV),
                     ((0, cam[:4] + (float("inf"), 0, 0, 0), W, H, 5, 3), INV), ((0, (0.0,) + cam[1:], W, H, 5, 3), INV),
                     ((0, cam[:1] + (-3.0,) + cam[2:], W, H, 5, 3), INV), ((0, cam, W, H, -1, 3), INV), ((0, cam, W, H, 5, -1), INV),
                     ((0, cam, W, H, 62, 3), INV), ((0, cam, W, H, 5, 45), INV), ((0, cam, W, H, 2000000000, 3), INV), ((0, cam, 7, H, 0, 0), INV),
                     ((0, cam, W + 1, H, 5, 3), CAP), ((0, cam, W, H + 1, 5, 3), CAP)):
        assert tracker.set_undistort_raw(*args) == rc, args
        assert "uvs_lt_set_undistort" in tracker.last_error()
    m = ud_ref.build_map(cam, W, H, 5, 3)
    for kw, rc in ((dict(stream=4), INV), (dict(null=True), INV), (dict(out_width=7), INV), (dict(out_height=0), INV), (dict(src_width=3), INV),
                   (dict(out_width=W + 1), CAP), (dict(out_height=H + 1), CAP), (dict(src_width=W + 1), CAP), (dict(src_height=H + 1), CAP)):
        a = dict(stream=0, src_width=W, src_height=H, map_xy=m); a.update(kw)
        assert tracker.set_remap_raw(**a) == rc, kw
        assert "uvs_lt_set_remap" in tracker.last_error()
    assert tracker.get_remap_raw(4)[0] == INV and tracker.get_remap_raw(1)[0] == INV and tracker.get_remap_raw(0, null=("out_width",))[0] == INV
    raw = dict(stream=0, image=img)
    for items, kw, rc in (([raw], dict(n_images=0), INV), ([raw], dict(n_images=5), CAP), ([raw], dict(null=("images",)), INV), ([raw], dict(null=("out",)), INV),
                          ([dict(raw, stream=4)], {}, INV), ([dict(raw, stream=1)], {}, INV), ([dict(raw, image=img[:, :W - 1])], {}, INV),
                          ([dict(raw, image=img[:H - 1])], {}, INV), ([raw, dict(raw, stream=2)], {}, INV)):
        assert tracker.undistort_raw(items, **kw)[0] == rc, kw
        assert "uvs_lt_undistort" in tracker.last_error()
    # detect_track on a mapped slot wants the map's source size
    assert tracker.detect_track_raw([dict(stream=0, image=img[:, :90])], **P)[0] == INV and "source size" in tracker.last_error()
    # none of the rejected calls changed the map or the slot; uvs_lt_reset keeps the map and empties the lines
    assert np.array_equal(tracker.get_remap(0), m)
    second = tracker.detect_track([dict(stream=0, image=img)], **P)[0]
    same_detection(second, dict(first, status=first["det_status"]), "after the rejected calls")
    assert second["n_matched"] >= 6 and first["n_returned"] >= 6 and first["n_matched"] == 0
    tracker.reset(0)
    assert np.array_equal(tracker.get_remap(0), m) and np.array_equal(tracker.undistort([raw])[0], ud_ref.remap(img, m))
    third = tracker.detect_track([dict(stream=0, image=img)], **P)[0]
    assert third["n_matched"] == 0 and tracker.last_error() == ""
    same_detection(third, dict(first, status=first["det_status"]), "after reset")
    # uvs_lt_detect is stateless and ignores the stream: the raw frame is detected as it is
    plain = tracker.detect([dict(stream=0, image=img)], **P)[0]
    same_detection(plain, uc.bar_ref("raw"), "uvs_lt_detect")
    tracker.set_undistort(0, None, 0, 0)
    assert tracker.undistort_raw([raw])[0] == INV


class HostUndistort(HostDetect):
    def __init__(self, device, **kw):
        HostDetect.__init__(self, device, **kw)
        self.L.uvs_host_lt_set_undistortion.argtypes = [C.c_void_p] + [C.c_double] * 4

    def set_undistortion(self, k1, k2, p1, p2):
        return self.L.uvs_host_lt_set_undistortion(self.h, k1, k2, p1, p2)


@pytest.mark.gpu
def test_gpu_host_mirror_set_undistortion_then_three_raw_frames():
    """uvs::LineFeatureTracker::setUndistortion: the camera rounded through float as the reference's CV_32F matrices hold it, the constructor's
    margins; readImage4Line(raw frame) then equals the Python path, and the lifted end points use the shifted principal point."""
    sc = uc.bar_scene(); W, H = sc["W"], sc["H"]; margins = (5, 3)
    cam = sc["cam"]
    cam32 = tuple(float(np.float32(v)) for v in cam)
    assert cam32 != cam
    h = HostUndistort(0, cam=cam[:4], max_width=W, max_height=H, max_lines=lc.MAX_LINES, margins=margins)
    assert h.L.uvs_host_lt_set_detect(h.h, P["grad_threshold"], P["min_pixels"], P["min_length"]) == 0
    assert h.set_undistortion(*cam[4:]) == 0
    t = uvs.api.LineTracker(device=0, max_streams=1, max_width=W, max_height=H, max_lines=lc.MAX_LINES, max_length=lt_cases.MAX_LENGTH)
    t.set_undistort(0, cam32, W, H, *margins)
    assert np.array_equal(t.get_remap(0), ud_ref.build_map(cam32, W, H, *margins))
    for f, raw in enumerate(_frames()):
        assert h.read_image_detect(raw, 0.1 * (f + 1)) == 0
        want = t.detect_track([dict(stream=0, image=raw)], **P)[0]
        d = h.last_detect()
        same_detection(d, dict(want, status=want["det_status"]), f)
        assert np.array_equal(d["prev_index"], want["prev_index"])
        desc, st, dist, res = h.last(want["n_returned"])
        assert np.array_equal(desc, want["desc"]) and np.array_equal(st, want["status"]) and np.array_equal(dist, want["distance"])
        assert res.tolist() == [want["n_described"], want["n_matched"]]
        g = h.get()
        assert len(g["ids"]) == want["n_returned"] >= 6 and np.array_equal(bits(g["un_pts"]), bits(lift_ref(g["pts"], cam[:4], margins)))
        assert h.update_ids() == want["n_returned"]
        if f:
            assert want["n_matched"] >= 4 and g["track_cnt"].max() == f + 1
    # a rejected setUndistortion reports the error and leaves the map
    assert h.set_undistortion(float("nan"), 0.0, 0.0, 0.0) == abi.UVS_ERR_INVALID_ARG
    assert h.read_image_detect(_frames()[0], 0.4) == 0 and h.last_detect()["n_returned"] >= 6
    t.close(); h.close()
