"""Triangulation of landmarks on the GPU (uvs_tri_*, csrc/uvs_triangulate.hip) against the 60-digit values of tests/tri_ref.py.

The bound is never a literal: for every baseline class the test computes E_ref, the largest error of the numpy restatement (numpy.linalg.svd of
svd_A, the reference's definition) against the 60-digit values on the same cases, and holds the device to BOUND = 8 times that -- two correct
SVD algorithms differ by a small factor, the normal-equation shortcut by 18 (0.02 m) and 113 (0.002 m) times E_ref
(tests/test_tri_ref.py).  Each test prints what it measured before it asserts."""
import ctypes as C
import os

import numpy as np
import pytest

import tri_cases as tc
import tri_ref
from helpers import abi, uvs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 8.0
CLASSES = tuple(tc.BASELINES)


@pytest.fixture(scope="module")
def tri():
    t = uvs.api.Triangulator(device=0, max_windows=3, max_points=200, max_lines=200, init_depth=tc.INIT_DEPTH)
    yield t
    t.close()


@pytest.fixture(scope="module")
def device(tri):
    """name -> (depth, pt_flag, orth, ln_flag) of ONE call over the 3 windows of each class, and of the edge window."""
    return {name: tri.triangulate(tc.edge() if name == "edge" else tc.scene(name)) for name in CLASSES + ("edge",)}


@pytest.mark.parametrize("cls", CLASSES)
def test_depths_against_sixty_digits(device, cls):
    depth, flag, _, _ = device[cls]
    _, hp = tc.refs(cls)
    e_ref, keep = tc.e_ref_points(cls)
    err = tri_ref.depth_errors(depth[keep], hp["depth"][keep]).max()
    print(f"class {cls}: device {err:.2e}, E_ref {e_ref:.2e}, ratio {err / e_ref:.2f}; {int((~keep).sum())} of {len(keep)} left out; flags {np.bincount(flag, minlength=3)}")
    assert (~keep).sum() <= 0.02 * len(keep)
    assert np.array_equal(flag[keep], hp["pt_flag"][keep])
    assert err <= BOUND * e_ref


@pytest.mark.parametrize("cls", CLASSES)
def test_lines_against_sixty_digits(device, cls):
    _, _, orth, flag = device[cls]
    _, hp = tc.refs(cls)
    e_ref, ok = tc.e_ref_lines(cls)
    err = tri_ref.line_errors(orth[ok], hp["U"][ok], hp["phi"][ok]).max()
    print(f"class {cls}: device {err:.2e}, E_ref {e_ref:.2e}, ratio {err / e_ref:.2f}")
    assert np.array_equal(flag, hp["ln_flag"])
    assert np.all((orth[ok, 0] >= 0.0) & (orth[ok, 0] <= np.pi))
    assert err <= BOUND * e_ref


def test_edge_cases(device):
    depth, pf, orth, lf = device["edge"]
    b = tc.edge()
    _, hp = tc.refs("edge")
    print("edge:", depth, pf, orth, lf)
    assert np.array_equal(pf, hp["pt_flag"]) and np.array_equal(pf, b["expect_pt_flag"]) and pf[2] in (1, 2)
    assert depth[1] == tc.INIT_DEPTH and depth[2] == tc.INIT_DEPTH          # behind the start camera; identical camera centres
    e_pt, e_ln = tc.e_ref_points("0.2")[0], tc.e_ref_lines("0.2")[0]          # the ordinary landmarks of this window are of that class (0.25 m per frame)
    assert abs(depth[0] - hp["depth"][0]) <= BOUND * e_pt * hp["depth"][0]
    assert np.array_equal(lf, hp["ln_flag"]) and lf[1] == 2 and np.all(orth[1] == 0.0)          # coinciding planes: four zeros
    assert tri_ref.line_errors(orth[:1], hp["U"][:1], hp["phi"][:1])[0] <= BOUND * e_ln


def test_check_lines(tri):
    c = tc.check_scene()
    _, hp, z = tc.check_refs()
    flag = tri.check_lines(c["pose"], c["ex_pose"], c["ln_window"], c["ln_start"], c["ln_sp0"], c["ln_ep0"], c["orth_old"])
    decided = np.abs(z).min(axis=1) > 1e-9
    print(f"check_lines: {np.bincount(flag, minlength=3)} flags, {int((~decided).sum())} undecided")
    assert decided.all() and np.array_equal(flag, hp)


def test_shift_depth(tri):
    s = tc.shift_scene()
    (out64, _, _), z, (out_hp, flag_hp) = tc.shift_refs()
    e_ref = (np.abs(out64 - out_hp) / np.abs(out_hp)).max()
    out, flag = tri.shift_depth(s["uv0"], s["depth"], s["marg_R"], s["marg_P"], s["new_R"], s["new_P"])
    err = (np.abs(out - out_hp) / np.abs(out_hp)).max()
    print(f"shift_depth: device {err:.2e}, E_ref {e_ref:.2e}")
    assert np.all(np.abs(z) > 1e-9) and np.array_equal(flag, flag_hp) and np.all(out[flag == 1] == tc.INIT_DEPTH)
    assert err <= BOUND * e_ref
    tri.set_init_depth(7.5)          # the fallback is the handle's
    out2, flag2 = tri.shift_depth(s["uv0"][:1], -np.abs(s["depth"][:1]), s["marg_R"], s["marg_P"], s["new_R"], s["new_P"])
    tri.set_init_depth(tc.INIT_DEPTH)
    assert out2[0] == 7.5 and flag2[0] == 1


def test_batches_and_repeats_give_the_same_bits(tri, device):
    for cls in CLASSES:
        b = tc.scene(cls)
        again = tri.triangulate(b)
        for a, g in zip(device[cls], again):
            assert np.array_equal(a.view(np.uint8), g.view(np.uint8))
        for w in range(3):
            one, p, l = tc.window_of(b, w)
            depth, pf, orth, lf = tri.triangulate(one)
            assert np.array_equal(depth.view(np.uint64), device[cls][0][p].view(np.uint64)) and np.array_equal(pf, device[cls][1][p])
            assert np.array_equal(orth.view(np.uint64), device[cls][2][l].view(np.uint64)) and np.array_equal(lf, device[cls][3][l])


def test_empty_batches_and_refused_inputs(tri):
    b = tc.scene("0.2")
    INV = abi.UVS_ERR_INVALID_ARG
    before = tri.triangulate(b)[0]
    empty = dict(pose=b["pose"], ex_pose=b["ex_pose"])
    assert tri.triangulate_raw(empty)[0] == abi.UVS_OK
    assert tri.triangulate_raw(empty, null=("pose", "ex_pose"), n_windows=0)[0] == abi.UVS_OK          # nothing to do: nothing is looked at
    points_only = {k: v for k, v in b.items() if not k.startswith("ln_")}; lines_only = {k: v for k, v in b.items() if not k.startswith("pt_")}
    rc, depth, pf, orth, lf = tri.triangulate_raw(points_only)
    assert rc == abi.UVS_OK and len(orth) == 0 and np.array_equal(depth.view(np.uint64), tri.triangulate(b)[0].view(np.uint64))
    rc, depth, pf, orth, lf = tri.triangulate_raw(lines_only)
    assert rc == abi.UVS_OK and len(depth) == 0 and np.array_equal(orth.view(np.uint64), tri.triangulate(b)[2].view(np.uint64))
    assert tri.check_lines_raw(b["pose"], b["ex_pose"], [], [], np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 4)))[0] == abi.UVS_OK
    assert tri.shift_depth_raw(np.zeros((0, 3)), [], np.eye(3), np.zeros(3), np.eye(3), np.zeros(3))[0] == abi.UVS_OK

    def refused(**change):
        bad = dict(b)
        for k, v in change.items():
            a = np.array(b[k]); a[v[0]] = v[1]; bad[k] = a
        rc, depth, pf, orth, lf = tri.triangulate_raw(bad)
        assert np.all(pf == -1) and np.all(lf == -1)          # nothing was written: no launch, no download
        return rc

    one_view = dict(b); one_view["pt_obs_begin"] = np.r_[0, b["pt_obs_begin"][1:] - (b["pt_obs_begin"][1] - 1)].astype(np.int32)
    assert tri.triangulate_raw(one_view)[0] == INV                             # the first track with one view
    twelve = tc.window_of(b, 0)[0]; twelve["pt_start"] = np.array([0], np.int32); twelve["pt_obs_begin"] = np.array([0, 12], np.int32); twelve["pt_obs"] = np.ones((12, 3))
    assert tri.triangulate_raw(twelve)[0] == INV                               # more than 11 views
    assert refused(pt_start=(1, 10)) == INV                                    # start + views > 11
    assert refused(pt_start=(1, -1)) == INV
    assert refused(ln_fj=(0, int(b["ln_fi"][0]))) == INV                       # ln_fj <= ln_fi
    assert refused(ln_fj=(0, 11)) == INV
    assert refused(ln_fi=(0, -1)) == INV
    assert refused(pt_window=(129, 3)) == INV and refused(pt_window=(0, -1)) == INV and refused(ln_window=(129, 3)) == INV
    assert refused(pt_window=(5, 0)) == INV and refused(ln_window=(5, 0)) == INV          # decreasing
    assert tri.triangulate_raw(b, n_windows=0)[0] == INV and tri.triangulate_raw(b, n_windows=4)[0] == INV          # above max_windows
    assert tri.triangulate_raw(b, null=("pose",))[0] == INV and tri.triangulate_raw(b, null=("pt_obs",))[0] == INV and tri.triangulate_raw(b, null=("ln_flag",))[0] == INV
    assert tri.triangulate_raw(b, null=("batch",))[0] == INV
    assert tri.triangulate_raw(b, init_depth=0.0)[0] == INV and tri.triangulate_raw(b, init_depth=float("nan"))[0] == INV
    assert tri.set_init_depth_raw(-1.0) == INV
    small = uvs.api.Triangulator(device=0, max_windows=3, max_points=129, max_point_obs=2000, max_lines=129)
    try:
        assert small.triangulate_raw(points_only)[0] == INV and small.triangulate_raw(lines_only)[0] == INV          # 130 landmarks, 129 fit
        assert "capacity" in small.last_error()
        tight = uvs.api.Triangulator(device=0, max_windows=3, max_points=130, max_point_obs=int(b["pt_obs_begin"][-1]) - 1, max_lines=130)
        assert tight.triangulate_raw(points_only)[0] == INV and tight.triangulate_raw(lines_only)[0] == abi.UVS_OK
        tight.close()
        c = tc.check_scene()
        assert small.check_lines_raw(c["pose"], c["ex_pose"], c["ln_window"], c["ln_start"], c["ln_sp0"], c["ln_ep0"], c["orth_old"])[0] == INV
        s = tc.shift_scene()
        assert small.shift_depth_raw(s["uv0"], s["depth"], s["marg_R"], s["marg_P"], s["new_R"], s["new_P"])[0] == INV
    finally:
        small.close()
    c = tc.check_scene()
    bad_start = c["ln_start"].copy(); bad_start[5] = 11
    assert tri.check_lines_raw(c["pose"], c["ex_pose"], c["ln_window"], bad_start, c["ln_sp0"], c["ln_ep0"], c["orth_old"])[0] == INV
    # the handle is still good
    assert np.array_equal(tri.triangulate(b)[0].view(np.uint64), before.view(np.uint64))
    h = C.c_void_p()
    assert uvs.api.lib().uvs_tri_create(0, 0, 10, 20, 10, C.byref(h)) == INV and uvs.api.lib().uvs_tri_create(0, abi.TRI_MAX_WINDOWS + 1, 10, 20, 10, C.byref(h)) == abi.UVS_ERR_CAPACITY


def test_triangulate_windows_on_synth_windows(tri):
    ws = [uvs.synth.make_window(31, n_points=30, n_lines=8, n_tagged=4), uvs.synth.make_window(32, n_points=17, n_lines=5, n_tagged=2, pt_track=4)]
    inv_depth, line_orth, pf, lf = tri.triangulate_windows(ws)
    b = tc.tracks_of_windows(ws)
    depth64, pf64, orth64, lf64 = tri_ref.triangulate(b, tc.INIT_DEPTH)
    hp = tri_ref.triangulate_hp(b, tc.INIT_DEPTH)
    assert [len(v) for v in inv_depth] == [30, 17] and [v.shape for v in line_orth] == [(8, 4), (5, 4)]
    depth = 1.0 / np.concatenate(inv_depth); orth = np.concatenate(line_orth)
    assert np.array_equal(np.concatenate(pf), hp["pt_flag"]) and np.array_equal(pf64, hp["pt_flag"]) and np.all(hp["ln_flag"] == 0) and np.all(np.concatenate(lf) == 0)
    e_pt = tri_ref.depth_errors(depth64, hp["depth"]).max(); e_ln = tri_ref.line_errors(orth64, hp["U"], hp["phi"]).max()
    err_pt = tri_ref.depth_errors(depth, hp["depth"]).max(); err_ln = tri_ref.line_errors(orth, hp["U"], hp["phi"]).max()
    print(f"synth windows: points device {err_pt:.2e} E_ref {e_pt:.2e}; lines device {err_ln:.2e} E_ref {e_ln:.2e}")
    # 1 / (1 / depth) adds two roundings to the device's value
    assert err_pt <= BOUND * e_pt + 4 * np.finfo(float).eps and err_ln <= BOUND * e_ln
    for w, d, o in zip(ws, inv_depth, line_orth):         # ... and the arrays fit the windows they are for
        assert d.shape == w.inv_depth.shape and o.shape == w.line_orth.shape


def test_host_mirror_device_route_agrees_with_the_host_route():
    """uvs_host_triangulate_device against the unchanged uvs_host_triangulate on the 0.2 m class, where the SVD of svd_A and the eigenvectors of
    svd_A^T svd_A agree; at low parallax the host route loses digits the device keeps, which is documented, not asserted."""
    lib = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
    b, _, _ = tc.window_of(tc.scene("0.2"), 2)
    n_pt, n_ln = len(b["pt_window"]), len(b["ln_window"])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)); ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    pose = np.ascontiguousarray(b["pose"][0]); ex = np.ascontiguousarray(b["ex_pose"][0])
    nobs = np.diff(b["pt_obs_begin"]).astype(np.int32); start = np.ascontiguousarray(b["pt_start"]); obs = np.ascontiguousarray(b["pt_obs"])
    ln_start = np.ascontiguousarray(b["ln_fi"]); ln_nobs = np.full(n_ln, 2, np.int32)
    results = {}
    for name in ("uvs_host_triangulate", "uvs_host_triangulate_device"):
        depth = np.full(n_pt, -1.0); orth = np.zeros((n_ln, 4))
        assert getattr(lib, name)(dp(pose), dp(ex), n_pt, ip(start), ip(nobs), dp(obs), 0, ip(ln_start), ip(ln_nobs), dp(obs), dp(obs), dp(depth), dp(orth)) == 0
        results[name] = depth
    used = b["pt_start"] < 8          # the reference's selection rule stays host bookkeeping: the others keep their -1 on both routes
    host, dev = results["uvs_host_triangulate"], results["uvs_host_triangulate_device"]
    print(f"host mirror: {int(used.sum())} of {n_pt} points used, device route against host route {np.abs(dev[used] / host[used] - 1).max():.2e}")
    assert used.sum() >= 40 and np.all(host[~used] == -1.0) and np.all(dev[~used] == -1.0)
    assert np.abs(dev[used] / host[used] - 1).max() <= 1e-9
    # lines: consecutive views of the host hook's track layout, so the pairs one frame apart
    sc = tc.scene("0.2")
    adj = np.flatnonzero((sc["ln_window"] == 2) & (sc["ln_fj"] == sc["ln_fi"] + 1))
    assert len(adj) >= 3
    ln_start = np.ascontiguousarray(sc["ln_fi"][adj]); ln_nobs = np.full(len(adj), 2, np.int32)
    sp = np.ascontiguousarray(np.stack([sc["ln_sp_i"][adj], sc["ln_sp_j"][adj]], axis=1).reshape(-1, 3)); ep = np.ascontiguousarray(np.stack([sc["ln_ep_i"][adj], sc["ln_ep_j"][adj]], axis=1).reshape(-1, 3))
    orths = {}
    for name in ("uvs_host_triangulate", "uvs_host_triangulate_device"):
        depth = np.zeros(1); orth = np.zeros((len(adj), 4))
        assert getattr(lib, name)(dp(pose), dp(ex), 0, ip(start), ip(nobs), dp(obs), len(adj), ip(ln_start), ip(ln_nobs), dp(sp), dp(ep), dp(depth), dp(orth)) == 0
        orths[name] = orth
    for h, d in zip(orths["uvs_host_triangulate"], orths["uvs_host_triangulate_device"]):
        assert np.abs(tri_ref.U_of_psi(h[:3]) - tri_ref.U_of_psi(d[:3])).max() <= 1e-9 and abs(h[3] - d[3]) <= 1e-9 * max(abs(h[3]), 1e-300)


def test_host_mirror_check_and_shift_through_the_device():
    """FeatureManager::setLineOrtho and removeBackShiftDepth by the host loops and through a uvs_tri handle: the same flags, the same parameters kept
    or replaced, and depths within the bound of the 60-digit values on both routes."""
    lib = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
    c = tc.check_scene(); _, flag_hp, _ = tc.check_refs()
    s = tc.shift_scene(); (out64, _, _), _, (out_hp, _) = tc.shift_refs()
    e_ref = (np.abs(out64 - out_hp) / np.abs(out_hp)).max()
    sel = np.flatnonzero(c["ln_window"] == 2)
    f64 = lambda a: np.ascontiguousarray(a, np.float64)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)); ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    pose, ex = f64(c["pose"][2]), f64(c["ex_pose"][2])
    start, sp, ep, old = np.ascontiguousarray(c["ln_start"][sel]), f64(c["ln_sp0"][sel]), f64(c["ln_ep0"][sel]), f64(c["orth_old"][sel])
    new = f64(old + 0.125)
    uv0, uv1, mR, mP, nR, nP = f64(s["uv0"]), f64(s["uv0"] * [0.5, 0.5, 1.0]), f64(s["marg_R"]), f64(s["marg_P"]), f64(s["new_R"]), f64(s["new_P"])
    got = {}
    for use_device in (0, 1):
        flag = np.zeros(len(sel), np.int32); orth = np.zeros((len(sel), 4)); depth = f64(s["depth"]).copy()
        assert lib.uvs_host_check_and_shift(use_device, dp(pose), dp(ex), len(sel), ip(start), dp(sp), dp(ep), dp(old), dp(new), ip(flag), dp(orth),
                                            len(depth), dp(uv0), dp(uv1), dp(depth), dp(mR), dp(mP), dp(nR), dp(nP)) == 0
        got[use_device] = (flag, orth, depth)
        assert np.array_equal(flag, flag_hp[sel]) and (flag == 1).sum() >= 20 and (flag == 2).sum() >= 40
        assert np.array_equal(orth[flag == 1], new[flag == 1]) and np.array_equal(orth[flag == 2], old[flag == 2])
        err = (np.abs(depth - out_hp) / np.abs(out_hp)).max()
        print(f"removeBackShiftDepth, {'device' if use_device else 'host'} route: {err:.2e}, E_ref {e_ref:.2e}")
        assert err <= BOUND * e_ref
    assert lib.uvs_host_device_triangulation_switch() == 7          # Estimator: off by default, a handle while on, none after
