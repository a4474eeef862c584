"""uvs_rp_relative_pose on the device against its two references (tests/rp_ref.py): the gates, the rounding and the RANSAC bit for bit against
the numpy restatement (tests/fr_ref.py for the RANSAC); the counts, masks, the choice and the window's l exactly, and R, t, Rotation, Translation
within 8 max(E_ref, 2^-53), against the 60-digit evaluation, E_ref being the numpy restatement's own error on the case (tests/rp_cases.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import rp_cases
import rp_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rp(gpu_api):
    h = gpu_api.RelativePose(device=0, max_items=16, max_points=256)
    yield h
    h.close()


@pytest.fixture(scope="module")
def batch(rp):
    """All cases as one batch of 11 items, a window each; run twice."""
    items = [rp_cases.item(n, window=k) for k, n in enumerate(rp_cases.NAMES)]
    return rp.solve(items), rp.solve(items)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check(name, res, mask):
    """One item's result against the references."""
    want = rp_cases.expected(name)
    assert res["status"] == want["status"] and res["n"] == want["n"]
    assert np.array_equal(u64(res["average_parallax"]), u64(want["average_parallax"]))
    for k in ("ransac_status", "n_inliers", "hypothesis", "root"):
        assert res[k] == want[k], k
    if want.get("half_margin", 0.0) > 1e-6:      # `iterations` hangs on the library's log where num / denom lies within rounding of a half-integer
        assert res["iterations"] == want["iterations"]
    assert np.array_equal(u64(res["F"]), u64(want["F"]))
    assert np.array_equal(res["good"], want["good"]) and res["chosen"] == want["chosen"] and res["inlier_cnt"] == want["inlier_cnt"] and res["ok"] == want["ok"]
    assert np.array_equal(mask, want["mask"])
    if name in rp_cases.GATED:
        for k in rp_ref.METRICS:
            assert not np.asarray(res[k]).any()
        return
    err, e_ref = rp_ref.errors(res, want), rp_cases.e_ref(name)
    print(f"{name}: " + ", ".join(f"{k} {err[k]:.2e} (E_ref {e_ref[k]:.2e})" for k in rp_ref.METRICS))
    assert rp_ref.within(err, e_ref) == []


@pytest.mark.parametrize("name", rp_cases.NAMES)
def test_single_against_references(rp, name):
    res, masks, win = rp.solve([rp_cases.item(name)])
    check(name, res[0], masks[0])
    want = rp_cases.expected(name)
    assert win["l"][0] == (0 if want["ok"] else -1)
    if want["ok"]:
        assert np.array_equal(u64(win["Rotation"][0]), u64(res["Rotation"][0])) and np.array_equal(u64(win["Translation"][0]), u64(res["Translation"][0]))
    else:
        assert not win["Rotation"][0].any() and not win["Translation"][0].any()


def test_batch_against_references(batch):
    (res, masks, win), _ = batch
    assert len(res) >= 11
    for k, name in enumerate(rp_cases.NAMES):
        check(name, res[k], masks[k])
        assert win["l"][k] == (0 if rp_cases.expected(name)["ok"] else -1)


def test_ransac_mask_is_fr_ref(rp, gpu_api):
    """The RANSAC mask stays on the device; what reaches the caller of it is the final mask = it AND the cheirality tests.  uvs_ft_reject through
    a tracker handle on the same rounded items gives the new call's RANSAC fields -- moving the kernel changed nothing -- and its mask is
    tests/fr_ref.py's."""
    names = [n for n in rp_cases.NAMES if n not in rp_cases.GATED]
    res, masks, _ = rp.solve([rp_cases.item(n, window=k) for k, n in enumerate(names)])
    ft = gpu_api.FeatureTracker(device=0, max_streams=len(names), max_width=96, max_height=80, levels=1, max_points=256)
    got = ft.reject([dict(prev=rp_ref.round32(rp_cases.case(n)["left"]), next=rp_ref.round32(rp_cases.case(n)["right"]), seed=rp_cases.case(n)["seed"]) for n in names],
                    rp_ref.PARAMS["f_threshold"], rp_ref.PARAMS["confidence"])
    ft.close()
    for k, n in enumerate(names):
        want = rp_cases.ref(n)
        assert (got[k]["status"], got[k]["n_inliers"], got[k]["hypothesis"], got[k]["root"], got[k]["iterations"]) == \
               (res[k]["ransac_status"], res[k]["n_inliers"], res[k]["hypothesis"], res[k]["root"], res[k]["iterations"])
        assert np.array_equal(u64(got[k]["F"]), u64(res[k]["F"]))
        assert np.array_equal(got[k]["keep"], want["keep"])
        assert not (masks[k] & ~got[k]["keep"].astype(bool)).any()      # the final mask lies within the RANSAC mask


def test_batch_independence(rp, batch):
    (res, masks, win), (res2, masks2, win2) = batch
    assert res.tobytes() == res2.tobytes() and win.tobytes() == win2.tobytes() and all(np.array_equal(a, b) for a, b in zip(masks, masks2))
    for k, name in enumerate(rp_cases.NAMES):
        one, m1, _ = rp.solve([rp_cases.item(name)])
        assert one[0].tobytes() == res[k].tobytes(), name
        assert np.array_equal(m1[0], masks[k])


def window_items(gpu_api):
    return gpu_api.RelativePose.window_items([rp_cases.window_tracks()])


def test_window_of_ten_items(rp, gpu_api):
    items = window_items(gpu_api)
    res, masks, win = rp.solve(items)
    assert list(res["status"][:4]) == [rp_ref.LOW_PARALLAX] * 4 and not res["ok"][:4].any()
    assert res["ok"][4:].all()
    assert win["l"][0] == 4
    assert np.array_equal(u64(win["Rotation"][0]), u64(res["Rotation"][4])) and np.array_equal(u64(win["Translation"][0]), u64(res["Translation"][4]))
    for k, it in enumerate(items):      # every item is the restatement's
        want = rp_ref.relative_pose(it["left"], it["right"], it["seed"])
        assert res["status"][k] == want["status"] and np.array_equal(u64(res["average_parallax"][k]), u64(want["average_parallax"]))
        assert np.array_equal(u64(res["F"][k]), u64(want["F"])) and res["n_inliers"][k] == want["n_inliers"]
    l, Rot, T, _, _ = rp.relative_pose_windows([rp_cases.window_tracks()])
    assert l[0] == 4 and np.array_equal(u64(Rot[0]), u64(win["Rotation"][0])) and np.array_equal(u64(T[0]), u64(win["Translation"][0]))
    # the second camera stands to the right of frame 4's: Translation points along +x
    assert T[0][0] > 0.99


def test_refusals_leave_the_handle_usable(rp, gpu_api):
    abi = gpu_api.abi
    good = [rp_cases.item("sideways_64", window=0, frame_l=0), rp_cases.item("inliers_gt12_21", window=0, frame_l=3)]
    ok_res, ok_masks, ok_win = rp.solve(good)

    def refused(items, **kw):
        rc, res, masks, win = rp.solve_raw(items, **kw)
        assert rc == abi.UVS_ERR_INVALID_ARG and rp.last_error().startswith("uvs_rp_relative_pose")
        fill = bytes([rp.FILL])
        assert res.tobytes() == fill * res.nbytes and win.tobytes() == fill * win.nbytes and all((m == rp.FILL).all() for m in masks)      # nothing written
        again = rp.solve(good)
        assert again[0].tobytes() == ok_res.tobytes() and again[2].tobytes() == ok_win.tobytes()

    nan = dict(good[0]); nan["left"] = good[0]["left"].copy(); nan["left"][5, 1] = np.nan
    refused([nan, good[1]])
    inf = dict(good[1]); inf["right"] = good[1]["right"].copy(); inf["right"][0, 0] = np.inf
    refused([good[0], inf])
    refused([dict(good[0], window=1), dict(good[1], window=0)])                      # a decreasing window
    refused([good[0], dict(good[1], frame_l=0)])                                     # a repeated frame_l
    refused([good[0], dict(good[1], frame_l=10)])
    refused([dict(good[0], window=2), dict(good[1], window=2)], n_windows=2)         # a window outside 0 .. n_windows - 1
    refused([dict(good[0], n=257)])                                                  # n above the capacity
    refused([dict(good[0], n=-1)])
    refused(good * 9)                                                                # 18 items above the capacity of 16 (and repeated frames)
    for name in ("items", "params", "mask", "item_results", "window_results", "left", "right"):
        refused(good, null=(name,))
    refused(good, n_items=0)
    refused(good, n_windows=0)
    for bad in (dict(confidence=1.0), dict(f_threshold=0.0), dict(max_depth=np.nan), dict(focal_length=-1.0), dict(min_ransac_points=7)):
        refused(good, params=abi.rp_params(**bad))


def test_estimator_relative_pose(rp, gpu_api):
    """Estimator::relativePose through the capi hook on a short synthetic segment: the l, Rotation and Translation of api.RelativePose."""
    from test_rp_ref import pack_tracks
    tracks = rp_cases.window_tracks()
    start, nv, pts = pack_tracks(tracks)
    H = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
    H.uvs_host_relative_pose.restype = C.c_int
    H.uvs_host_relative_pose.argtypes = [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_uint64, C.POINTER(C.c_double),
                                         C.POINTER(C.c_double), C.POINTER(C.c_int)]
    R = np.zeros((3, 3)); T = np.zeros(3); l = C.c_int(-1)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)); dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert H.uvs_host_relative_pose(len(tracks), ip(start), ip(nv), dp(pts), 0, dp(R), dp(T), C.byref(l)) == 1
    wl, wR, wT, _, _ = rp.relative_pose_windows([tracks])
    assert l.value == wl[0] == 4 and np.array_equal(u64(R), u64(wR[0])) and np.array_equal(u64(T), u64(wT[0]))
    # a window at rest: no pair passes, the hook says so
    still = [(s, np.repeat(p[:1], len(p), axis=0)) for s, p in tracks]
    start, nv, pts = pack_tracks(still)
    assert H.uvs_host_relative_pose(len(still), ip(start), ip(nv), dp(pts), 0, dp(R), dp(T), C.byref(l)) == 0
    assert rp.relative_pose_windows([still])[0][0] == -1
