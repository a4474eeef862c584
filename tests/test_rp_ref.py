"""The references of the relative pose (tests/rp_ref.py) against each other, the conditions on the cases (tests/rp_cases.py) that make counts,
masks and the choice exact quantities, the planted defects that the comparison of tests/test_relative_pose.py must catch, and what of the
host mirror and the C ABI needs no device.  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest

import rp_cases
import rp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVED = [n for n in rp_cases.NAMES if n not in rp_cases.GATED]


def compare(got, name):
    """The comparison the GPU test makes for steps 4 to 6 -> the names of what fails (empty: the result passes)."""
    h = rp_cases.hp(name)
    return rp_ref.exact_mismatches(got, h) + rp_ref.within(rp_ref.errors(got, h), rp_cases.e_ref(name))


@pytest.mark.parametrize("name", SOLVED)
def test_case_conditions(name):
    """The 60-digit evaluation alone: no comparison within 1e-9 of its threshold, the best count at least 2 ahead, F's second singular value at
    least 1e-3 of its first; and the two conditions that keep the singular vectors themselves away from a flip."""
    h = rp_cases.hp(name)
    g = sorted(int(v) for v in h["good"])
    print(f"{name}: margin {h['margin']:.2e} gap {h['gap']:.2e} sign margin {h['sign_margin']:.2e} sv {h['sv']} good {h['good']}")
    assert h["margin"] >= rp_cases.MIN_MARGIN
    assert g[3] - g[2] >= rp_cases.MIN_LEAD
    assert h["sv"][1] >= rp_cases.MIN_SV_RATIO * h["sv"][0]
    assert h["sign_margin"] >= rp_cases.MIN_SIGN_MARGIN and h["gap"] >= rp_cases.MIN_GAP


def test_cases_are_what_they_say():
    st = {n: rp_cases.ref(n)["status"] for n in rp_cases.NAMES}
    assert st["low_parallax_64"] == rp_ref.LOW_PARALLAX and st["few_corres_20"] == rp_ref.FEW_CORRES
    assert len(rp_cases.case("few_corres_20")["left"]) == 20
    assert st["inliers_le12_21"] == rp_ref.FEW_INLIERS and 0 < rp_cases.hp("inliers_le12_21")["inlier_cnt"] <= 12
    assert st["inliers_gt12_21"] == rp_ref.OK and rp_cases.hp("inliers_gt12_21")["inlier_cnt"] > 12
    assert all(st[n] == rp_ref.OK for n in SOLVED if n != "inliers_le12_21")
    assert sorted({len(rp_cases.case(n)["left"]) for n in SOLVED}) == [21, 64, 65, 150]
    c = rp_cases.case("outliers30_150"); r = rp_cases.ref("outliers30_150")
    assert c["outlier"].sum() == 45 and r["keep"][c["outlier"]].sum() <= 2 and rp_cases.hp("outliers30_150")["mask"][c["outlier"]].sum() == 0
    b = rp_cases.hp("beyond_65")
    assert b["mask"][-13:].sum() == 0 and rp_cases.ref("beyond_65")["keep"][-13:].sum() >= 10      # beyond max_depth: RANSAC inliers that recoverPose drops
    for g in rp_cases.GATED:      # a gated item: nothing but the gate's fields
        r = rp_cases.ref(g)
        assert r["ok"] == 0 and r["chosen"] == -1 and r["ransac_status"] == 1 and not r["mask"].any() and not r["F"].any()


@pytest.mark.parametrize("name", SOLVED)
def test_restatement_meets_60_digits(name):
    r, h = rp_cases.ref(name), rp_cases.hp(name)
    err, e_ref = rp_ref.errors(r, h), rp_cases.e_ref(name)
    print(f"{name}: " + ", ".join(f"{k} {err[k]:.2e}" for k in rp_ref.METRICS))
    assert rp_ref.exact_mismatches(r, h) == []
    assert rp_ref.within(err, e_ref) == []
    for M in (h["R"], h["Rotation"]):      # what is compared is a rotation, and the two statements of the pose agree
        assert abs(np.linalg.det(M) - 1) < 1e-12 and np.abs(M @ M.T - np.eye(3)).max() < 1e-12
    assert np.abs(h["Rotation"] @ h["t"] + h["Translation"]).max() < 1e-12 and abs(np.linalg.norm(h["t"]) - 1) < 1e-12


def test_recovered_pose_is_the_scene():
    """Rotation / Translation of solveRelativeRT: the pose of the second camera in the first one's frame, up to scale."""
    n, gen, seed, kw = rp_cases.SPEC["rot20_150"]
    h = rp_cases.hp("rot20_150")
    R, t = np.asarray(kw["R"]), np.asarray(kw["t"], float)
    assert np.abs(h["R"] - R).max() < 5e-3 and np.abs(h["t"] - t / np.linalg.norm(t)).max() < 5e-2


def _with_defect(name, defect):
    c = rp_cases.case(name); r = rp_cases.ref(name)
    return rp_ref.recover(r["F"], r["keep"], rp_ref.round32(c["left"]), rp_ref.round32(c["right"]), defect=defect)


@pytest.mark.parametrize("defect", [d for d in rp_ref.DEFECTS if d != "strict_choice"])
def test_planted_defect_is_caught(defect):
    caught = {n: compare(_with_defect(n, defect), n) for n in SOLVED}
    print(defect, {n: c for n, c in caught.items() if c})
    assert compare(_with_defect(SOLVED[0], None), SOLVED[0]) == []      # the comparison passes the restatement itself
    if defect == "no_x_depth":
        assert "good" in caught["beyond_65"] and "mask" in caught["beyond_65"]
    elif defect == "translation_rt":
        assert all("Translation" in caught[n] and "R" not in caught[n] for n in ("rot20_65", "rot20_150"))
    else:
        assert sum(bool(c) for c in caught.values()) >= 2


def test_planted_strict_choice_is_caught_on_a_tie():
    """The chain of >= on a planted tie: an all-zero RANSAC mask makes every count 0, and the reference's chain takes candidate 0."""
    name = "sideways_64"
    c = rp_cases.case(name); r = rp_cases.ref(name)
    l32, r32 = rp_ref.round32(c["left"]), rp_ref.round32(c["right"])
    zero = np.zeros(len(l32), np.uint8)
    want = rp_ref.recover_hp(r["F"], zero, l32, r32)
    good = rp_ref.recover(r["F"], zero, l32, r32)
    bad = rp_ref.recover(r["F"], zero, l32, r32, defect="strict_choice")
    assert list(want["good"]) == [0, 0, 0, 0] and want["chosen"] == 0
    assert rp_ref.exact_mismatches(good, want) == []
    assert "chosen" in rp_ref.exact_mismatches(bad, want) and bad["chosen"] == 3
    assert rp_ref.choose([5, 5, 1, 0]) == 0 and rp_ref.choose([5, 5, 1, 0], strict=True) == 3 and rp_ref.choose([1, 5, 5, 0]) == 1


def test_gate_order_and_rounding():
    rng = np.random.default_rng(3)
    l = rng.uniform(-0.5, 0.5, (30, 2)); r = l + 0.2
    assert rp_ref.gate(l[:20], r[:20])[0] == rp_ref.FEW_CORRES and rp_ref.gate(l[:21], r[:21])[0] == rp_ref.OK
    assert rp_ref.gate(l, l + 1e-4)[0] == rp_ref.LOW_PARALLAX
    assert rp_ref.gate(l[:12], r[:12], dict(rp_ref.PARAMS, min_corres=10))[0] == rp_ref.FEW_POINTS
    s = 0.0
    for a, b in zip(l, r):
        s = s + float(np.sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1])))
    assert rp_ref.gate(l, r)[1] == s / 30
    x = np.array([[0.1, 1 / 3]])
    assert np.array_equal(rp_ref.round32(x), np.array([[float(np.float32(0.1)), float(np.float32(1 / 3))]])) and rp_ref.round32(x)[0, 0] != 0.1


# ---------------------------------------------------------------- the host mirror and the C ABI, without a device
def _host():
    H = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
    H.uvs_host_get_corresponding.restype = C.c_int
    return H


def pack_tracks(tracks):
    start = np.array([s for s, _ in tracks], np.int32); nv = np.array([len(p) for _, p in tracks], np.int32)
    pts = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for _, p in tracks]))
    return start, nv, pts


def test_get_corresponding_on_hand_made_tracks(uvs):
    # five tracks: which of them span (l, 10), and in which order they come
    mk = lambda start, n, tag: (start, np.array([[tag + 0.01 * f, -tag + 0.02 * f, 1.0] for f in range(start, start + n)]))
    tracks = [mk(0, 11, 1.0), mk(3, 8, 2.0), mk(0, 10, 3.0), mk(5, 6, 4.0), mk(2, 9, 5.0)]
    start, nv, pts = pack_tracks(tracks)
    H = _host()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)); dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for l, want in ((0, [0]), (2, [0, 4]), (3, [0, 1, 4]), (5, [0, 1, 3, 4]), (9, [0, 1, 3, 4])):
        left = np.zeros((8, 3)); right = np.zeros((8, 3))
        n = H.uvs_host_get_corresponding(len(tracks), ip(start), ip(nv), dp(pts), l, 10, dp(left), dp(right), 8)
        assert n == len(want)
        for k, t in enumerate(want):
            s, p = tracks[t]
            assert np.array_equal(left[k], p[l - s]) and np.array_equal(right[k], p[10 - s])
        al, ar = uvs.api.RelativePose.corresponding(tracks, l)
        assert np.array_equal(al, left[:n, :2]) and np.array_equal(ar, right[:n, :2])
    # the ten items of a window, in the order and with the counts of getCorresponding
    items = uvs.api.RelativePose.window_items([tracks])
    assert [it["frame_l"] for it in items] == list(range(10)) and [len(it["left"]) for it in items] == [1, 1, 2, 3, 3, 4, 4, 4, 4, 4]


def test_window_level_l():
    assert rp_ref.window_l(range(10), [0, 0, 0, 0, 1, 1, 1, 1, 1, 1]) == 4
    assert rp_ref.window_l([2, 5, 7], [0, 0, 1]) == 7 and rp_ref.window_l(range(10), [0] * 10) == -1 and rp_ref.window_l([], []) == -1


def test_abi_structs_and_refusals_without_a_device(uvs):
    abi, L = uvs.abi, uvs.api.lib()
    assert C.sizeof(abi.RpItem) == 40 and C.sizeof(abi.RpParams) == 56 and C.sizeof(abi.RpItemResult) == 336 and C.sizeof(abi.RpWindowResult) == 104
    assert L.uvs_abi_version() == 7
    with open(os.path.join(ROOT, "include", "uvs_solver.h")) as f:
        hdr = f.read()
    for s in ("uvs_rp_create", "uvs_rp_destroy", "uvs_rp_last_error", "uvs_rp_default_params", "uvs_rp_relative_pose", "uvs_rp_last_device_ms"):
        assert s + "(" in hdr and s in uvs.api.EXPORTS and hasattr(L, s), s
    p = abi.RpParams()
    L.uvs_rp_default_params(C.byref(p))
    for k, v in abi.RP_PARAM_DEFAULTS.items():
        assert getattr(p, k) == v == rp_ref.PARAMS[k], k
    # a null handle is refused before anything else is looked at, and reads as such
    assert L.uvs_rp_relative_pose(None, 1, None, None, None, None, 1, None) == abi.UVS_ERR_INVALID_ARG
    assert L.uvs_rp_last_error(None) == b"null relative-pose handle" and L.uvs_rp_last_device_ms(None, 0) == 0.0
    h = C.c_void_p()
    assert L.uvs_rp_create(0, 0, 64, C.byref(h)) == abi.UVS_ERR_INVALID_ARG and L.uvs_rp_create(0, 8, 0, C.byref(h)) == abi.UVS_ERR_INVALID_ARG
    assert L.uvs_rp_create(0, 8, 64, None) == abi.UVS_ERR_INVALID_ARG
    assert L.uvs_rp_create(0, abi.RP_MAX_ITEMS + 1, 64, C.byref(h)) == abi.UVS_ERR_CAPACITY and L.uvs_rp_create(0, 8, 8193, C.byref(h)) == abi.UVS_ERR_CAPACITY
    assert not h
    L.uvs_rp_destroy(None)
