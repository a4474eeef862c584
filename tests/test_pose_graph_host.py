"""The host mirror of PoseGraph (host/pose_graph.{h,cpp}, libuvs_host.so): a keyframe stream through addKeyFrame / optimize4DoF gives the poses
of a direct uvs_pg_optimize call, keyframes after the optimized one carry the reference's drift (pose_graph.cpp:570-591), and the corrected
path written as a result file scores through trajectory.ate."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import pg_cases as pc
import pg_ref
from helpers import abi, uvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def test_host_pose_graph_entry_exported():
    host = C.CDLL(HOST)
    assert hasattr(host, "uvs_host_pose_graph_run")


@pytest.mark.gpu
def test_gpu_host_pose_graph_matches_direct_call_and_carries_drift():
    stamps, p, R = pc.mh05_keyframes(2.0)
    pv, Rv = pc.drift(p, R, 3)
    loops = pc.revisit_loops(stamps, p, R, 103)
    n = len(p)
    loop_index = -np.ones(n, np.int32); info = np.zeros((n, 8))
    for k, j, rt, ry in loops:
        rq = pg_ref.R_to_quat(R[j].T @ R[k])
        loop_index[k] = j; info[k] = [rt[0], rt[1], rt[2], rq[3], rq[0], rq[1], rq[2], ry]
    cur = max(k for k, _, _, _ in loops if k < n - 20)   # the solve runs at this loop; later keyframes (and loops) come after it
    n_before = cur + 3                                  # two keyframes already in the list behind cur, the rest added after the solve
    assert n_before < n
    before = [lp for lp in loops if lp[0] <= cur]
    q = pg_ref.R_to_quat(Rv)
    out_pose = np.zeros((n, 7)); drift = np.zeros(4); rep = abi.PgReport()
    host = C.CDLL(HOST)
    host.uvs_host_pose_graph_run.restype = C.c_int
    with tempfile.TemporaryDirectory() as d:
        tum = os.path.join(d, "pose_graph.txt"); tum_vio = os.path.join(d, "vio.txt")
        rc = host.uvs_host_pose_graph_run(0, n, _dp(np.ascontiguousarray(stamps)), _dp(np.ascontiguousarray(pv)), _dp(q), _ip(np.ones(n, np.int32)),
                                          _ip(loop_index), _dp(info), n_before, cur, tum.encode(), _dp(out_pose), _dp(drift), C.byref(rep))
        assert rc == abi.UVS_OK
        # 1. the optimized keyframes equal a direct uvs_pg_optimize call on the same window
        w = pc.window(pv, Rv, before)
        yaw_t, rep_d = uvs.api.PoseGraphSolver(max_keyframes=256, max_loops=64).optimize(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
        assert list(rep.accepted[:rep.num_iterations + 1]) == list(rep_d.accepted[:rep_d.num_iterations + 1])
        assert abs(rep.final_cost - rep_d.final_cost) <= 1e-9 * rep_d.final_cost
        assert np.abs(out_pose[w["first"]:cur + 1, :3] - yaw_t[:, 1:]).max() < 1e-7
        yaw_host = pg_ref.R2ypr(pg_ref.quat_to_R(out_pose[w["first"]:cur + 1, 3:]))[:, 0]
        assert np.abs(pg_ref.normalize_angle(yaw_host - yaw_t[:, 0])).max() < 1e-6
        # 2. every keyframe after cur: P = r_drift P_vio + t_drift, R = r_drift R_vio
        r_drift = pg_ref.ypr2R(drift[0], 0.0, 0.0)
        for k in range(cur + 1, n):
            assert np.abs(out_pose[k, :3] - (r_drift @ pv[k] + drift[1:])).max() < 1e-9
            assert np.abs(pg_ref.quat_to_R(out_pose[k, 3:]) - r_drift @ Rv[k]).max() < 1e-9
        # 3. the corrected path scores through trajectory.ate, well below the drifted one
        uvs.trajectory.write_tum(tum_vio, stamps, pv, q)
        gt = os.path.join(ROOT, "tests", "golden", "mh05_groundtruth.npz")
        a_corr, a_vio = uvs.trajectory.ate(tum, gt), uvs.trajectory.ate(tum_vio, gt)
        assert a_corr["n_matched"] == n
        assert a_corr["rmse_m"] < 0.8 * a_vio["rmse_m"], (a_corr, a_vio)
