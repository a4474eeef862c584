"""The host mirror of loop detection's verification step (host/pose_graph.{h,cpp}: KeyFrame::findConnection through uvs_lc_verify,
PoseGraph::addKeyFrameWithCandidate): the MH_05 keyframe stream with its loop candidates gives the loops and the corrected poses of the
Python path (api.LoopVerifier, then api.PoseGraphSolver on the same window)."""
import ctypes as C
import os

import numpy as np
import pytest

import lc_cases as lc
import pg_cases
import pg_ref
from helpers import abi, uvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so")


def test_host_loop_verify_entry_exported():
    host = C.CDLL(HOST)
    assert hasattr(host, "uvs_host_pose_graph_verify_run")


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


@pytest.mark.gpu
def test_gpu_host_find_connection_matches_the_python_path():
    W = lc.mh05_world()
    true, _ = lc.mh05_candidates(W)
    n = len(W["p"])
    cand = -np.ones(n, np.int32)
    for k, j in true:
        cand[k] = j
    kf = W["kf"]
    nq = np.array([len(f["p3d"]) for f in kf], np.int32); nk = np.array([len(f["uv"]) for f in kf], np.int32)
    p3d = np.ascontiguousarray(np.concatenate([f["p3d"] for f in kf])); qd = np.ascontiguousarray(np.concatenate([f["qdesc"] for f in kf]))
    uv = np.ascontiguousarray(np.concatenate([f["uv"] for f in kf])); od = np.ascontiguousarray(np.concatenate([f["odesc"] for f in kf]))
    q = pg_ref.R_to_quat(W["Rv"]); tic, qic = np.ascontiguousarray(W["tic"]), np.ascontiguousarray(W["qic"])
    acc = np.zeros(n, np.int32); info = np.zeros((n, 8)); pose = np.zeros((n, 7))
    host = C.CDLL(HOST)
    host.uvs_host_pose_graph_verify_run.restype = C.c_int
    d = C.c_double; i32 = C.c_int32; u64 = C.c_uint64
    rc = host.uvs_host_pose_graph_verify_run(0, n, _p(np.ascontiguousarray(W["stamps"]), d), _p(np.ascontiguousarray(W["pv"]), d), _p(q, d),
                                             _p(np.ones(n, np.int32), i32), _p(tic, d), _p(qic, d), _p(nq, i32), _p(p3d, d), _p(qd, u64),
                                             _p(nk, i32), _p(uv, d), _p(od, u64), _p(cand, i32), _p(acc, i32), _p(info, d), _p(pose, d))
    assert rc == abi.UVS_OK
    # the Python path: the same pairs (same seeds) through api.LoopVerifier
    v = uvs.api.LoopVerifier(max_pairs=64)
    res = []
    pairs = [W["pair_of"](k, j) for k, j in true]
    for s in range(0, len(pairs), 64):
        res += v.verify(pairs[s:s + 64], W["tic"], W["qic"])[0]
    v.close()
    py_acc = {k: r for (k, _), r in zip(true, res) if r["accepted"]}
    assert sorted(py_acc) == sorted(np.flatnonzero(acc).tolist())
    assert len(py_acc) >= 20
    for k, r in py_acc.items():
        assert np.abs(info[k] - r["loop_info"]).max() < 1e-6, k
    loops = [(k, j, np.array(py_acc[k]["loop_info"][:3]), float(py_acc[k]["loop_info"][7])) for k, j in true if k in py_acc]
    w = pg_cases.window(W["pv"], W["Rv"], loops)
    yaw_t, _ = uvs.api.PoseGraphSolver(max_keyframes=512, max_loops=64).optimize(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
    sl = slice(w["first"], w["last"] + 1)
    assert np.abs(pose[sl, :3] - yaw_t[:, 1:]).max() < 1e-5
    yaw_host = pg_ref.R2ypr(pg_ref.quat_to_R(pose[sl, 3:]))[:, 0]
    assert np.abs(pg_ref.normalize_angle(yaw_host - yaw_t[:, 0])).max() < 1e-4
    p_true = W["p"][sl]
    assert pg_cases.positions_ate(pose[sl, :3], p_true) <= 0.6 * pg_cases.positions_ate(W["pv"][sl], p_true)
