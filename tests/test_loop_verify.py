"""Loop verification (uvs_lc_*, csrc/uvs_loop_verify.hip): BRIEF matching and PnP-RANSAC of KeyFrame::findConnection on the GPU against the
numpy restatement tests/lc_ref.py.

CPU tests pin lc_ref itself (matching against a brute-force loop, the LM Jacobian, the selection rule, the generator, noiseless PnP) and the
ctypes layouts.  GPU tests compare the device with lc_ref: every match index, every hypothesis's inlier count, the selection, the inlier mask,
the refined pose and loop_info, the gates, determinism and batching, and an MH_05 run whose verified loops correct the drifted trajectory."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import lc_cases as lc
import lc_ref
import pg_cases
import pg_ref
from helpers import abi, uvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = lc_ref.REASON


# ================================================================ CPU: the restatement
def test_match_equals_brute_force_loop():
    for case in [lc.matching_pair(12), lc.planted_pair(2, n_in=70, n_out=30)[0]]:
        q, o = case["qdesc"], case["odesc"]
        ref = lc_ref.match(q, o)
        for i in range(len(q)):
            best, idx = 128, -1
            for j in range(len(o)):
                d = sum(bin(int(q[i, w]) ^ int(o[j, w])).count("1") for w in range(4))
                if d < best:
                    best, idx = d, j
            assert ref[i] == (idx if idx != -1 and best < 80 else -1), i


def test_matching_edges_are_what_the_reference_decides():
    case = lc.matching_pair(12)
    m = lc_ref.match(case["qdesc"], case["odesc"])
    assert m[0] == 0          # distance 79: kept
    assert m[1] == -1         # 80: dropped (bestDist < 80)
    assert m[2] == -1 and m[3] == -1     # 127, 128
    assert m[4] == 4 and m[5] == 5 and m[6] == 6
    assert m[7] == 7          # two equal minima: the first index
    assert m[8] == 9          # equal distance, different bits: the first index
    assert m[9] == 12         # the later keypoint is strictly closer
    assert m[10] == 13 and m[11] == -1


def test_lm_jacobian_matches_central_differences():
    rng = np.random.default_rng(1)
    Rm = lc_ref.exp_so3(rng.normal(0, 0.5, 3))[None]; t = rng.normal(0, 0.3, (1, 3))
    X = rng.normal(0, 1, (1, 7, 3)) + [0, 0, 6]; uv = rng.normal(0, 0.2, (1, 7, 2))
    r, J, _ = lc_ref.residual_jacobian(Rm, t, X, uv)
    h = 1e-6
    for c in range(6):
        d = np.zeros(6); d[c] = h
        rp, _, _ = lc_ref.residual_jacobian(lc_ref.exp_so3(d[:3])[None] @ Rm, t + d[3:], X, uv)
        rm, _, _ = lc_ref.residual_jacobian(lc_ref.exp_so3(-d[:3])[None] @ Rm, t - d[3:], X, uv)
        assert np.abs((rp - rm) / (2 * h) - J[..., c]).max() < 1e-7, c


def test_update_num_iters_and_selection_rule():
    # RANSACUpdateNumIters by hand: log(0.01) / log(1 - (1 - ep)^5)
    assert lc_ref.update_num_iters(0.99, 0.0, 5, 100) == 0
    assert lc_ref.update_num_iters(0.99, 0.5, 5, 100) == 100     # log(0.01) / log(1 - 0.5^5) = 145: capped
    assert lc_ref.update_num_iters(0.99, 0.2, 5, 100) == int(np.rint(np.log(0.01) / np.log(1 - 0.8 ** 5)))     # 12
    assert lc_ref.update_num_iters(0.99, 0.2, 5, 100) == 12
    n = 50
    counts = -np.ones(100, np.int32)
    counts[0] = 4                     # <= 4 never becomes the best
    counts[1] = 20                    # best; ep = 0.6 -> niters stays 100
    counts[2] = 20                    # equal: not better
    counts[3] = 40                    # ep = 0.2 -> niters = 12
    counts[11] = 41                   # examined (11 < 12): ep = 0.18 -> niters = 10 <= 11: the loop ends here
    counts[12] = 50
    best, iters = lc_ref.select(counts, n)
    assert (best, iters) == (11, 12)
    counts[11] = 39
    assert lc_ref.select(counts, n) == (3, 12)
    assert lc_ref.select(-np.ones(100, np.int32), n) == (-1, 100)
    c = np.full(100, 4, np.int32); c[99] = 5
    assert lc_ref.select(c, n) == (99, 100)
    c[0] = n                          # all inliers: niters = 0 after the first hypothesis
    assert lc_ref.select(c, n) == (0, 1)


def test_generator_draws_distinct_in_range_indices():
    seen = set()
    for seed in (0, 1, 2 ** 63 + 5, 2 ** 64 - 1):
        for n in (5, 6, 26, 1000):
            for h in range(100):
                s = lc_ref.draw(seed, h, n)
                assert s is not None and len(set(s)) == 5 and all(0 <= v < n for v in s)
                seen.add(tuple(s))
    assert len(seen) > 1000
    assert lc_ref.draw(7, 0, 4) is None           # 5 distinct out of 4: invalid
    assert lc_ref.mix64(0) == 0 and lc_ref.mix64(1) == 0x5692161D100B05E5


def test_noiseless_pnp_recovers_the_pose():
    pair, info = lc.planted_pair(40, n_in=80, px_noise=0.0, yaw_gap=12.0, offset=(0.5, 0.2, -0.1))
    tic, qic = lc.extrinsic()
    r = lc_ref.verify(pair, tic, qic)
    assert r["accepted"] and r["n_inliers"] == 80
    assert np.abs(r["PnP_T_old"] - info["old_t"]).max() < 1e-9
    assert np.abs(lc_ref.quat_to_R(r["PnP_q_old"]) - info["old_R"]).max() < 1e-9
    assert abs(r["loop_info"][7] - (-12.0)) < 1e-9


# ================================================================ CPU: the ABI
LC_SYMBOLS = ["uvs_lc_create", "uvs_lc_destroy", "uvs_lc_last_error", "uvs_lc_verify", "uvs_lc_debug_pair"]


def test_lc_symbols_exported():
    L = uvs.api.lib()
    for s in LC_SYMBOLS:
        assert hasattr(L, s), s


def test_lc_struct_layout_matches_header():
    code = r'''
#include <stdio.h>
#include <stddef.h>
#include "uvs_solver.h"
int main(void) {
  printf("%zu %zu\n", sizeof(uvs_lc_pair), sizeof(uvs_lc_result));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(uvs_lc_pair, p3d), offsetof(uvs_lc_pair, desc), offsetof(uvs_lc_pair, vio_t),
         offsetof(uvs_lc_pair, vio_q), offsetof(uvs_lc_pair, old_uv_norm), offsetof(uvs_lc_pair, old_desc), offsetof(uvs_lc_pair, seed),
         offsetof(uvs_lc_pair, n_old));
  printf("%zu %zu %zu %zu %zu %zu\n", offsetof(uvs_lc_result, ransac_iters), offsetof(uvs_lc_result, loop_info), offsetof(uvs_lc_result, PnP_T_old),
         offsetof(uvs_lc_result, PnP_q_old), offsetof(uvs_lc_result, hyp_inliers), (size_t)UVS_LC_N_HYPOTHESES);
  printf("%d %d %d %d\n", UVS_LC_MAX_PAIRS, UVS_LC_MAX_QUERY, UVS_LC_MAX_OLD, UVS_LC_T_GATE);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c"); exe = os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    P, Rs = abi.LcPair, abi.LcResult
    assert out[:2] == [C.sizeof(P), C.sizeof(Rs)]
    assert out[2:10] == [P.p3d.offset, P.desc.offset, P.vio_t.offset, P.vio_q.offset, P.old_uv_norm.offset, P.old_desc.offset, P.seed.offset, P.n_old.offset]
    assert out[10:16] == [Rs.ransac_iters.offset, Rs.loop_info.offset, Rs.PnP_T_old.offset, Rs.PnP_q_old.offset, Rs.hyp_inliers.offset, abi.LC_N_HYPOTHESES]
    assert out[16:] == [abi.LC_MAX_PAIRS, abi.LC_MAX_QUERY, abi.LC_MAX_OLD, len(abi.LC_REASONS) - 1]
    assert abi.LC_REASONS.index("T_GATE") == R["T_GATE"] and abi.LC_REASONS.index("FEW_INLIERS") == R["FEW_INLIERS"]


def test_loop_verifier_create_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    assert uvs.api.lib().uvs_lc_create(0, 1, 16, 16, C.byref(h)) == abi.UVS_ERR_NO_DEVICE
    with pytest.raises(RuntimeError):
        uvs.api.LoopVerifier()


# ================================================================ the MH_05 end-to-end case (shared by the CPU calibration and the GPU test)
ACCEPT_RATE = 0.8          # of the true revisit candidates that share >= 40 landmarks
MIN_SHARED = 40
LOOP_T_ERR, LOOP_YAW_ERR = 0.03, 0.3
ATE_RATIO = 0.6


def _mh05_run(verify_many):
    """verify_many(list of pairs) -> list of result dicts.  -> dict of the end-to-end numbers and the verified loops."""
    W = lc.mh05_world()
    true, decoys = lc.mh05_candidates(W)
    res_t = verify_many([W["pair_of"](k, j) for k, j in true])
    res_d = verify_many([W["pair_of"](k, j) for k, j in decoys])
    eligible = [i for i, (k, j) in enumerate(true) if lc.shared(W, k, j) >= MIN_SHARED]
    loops, t_err, y_err = [], [], []
    for (k, j), r in zip(true, res_t):
        if r["accepted"]:
            rt, ry = lc.true_loop_info(W, k, j)
            t_err.append(np.linalg.norm(r["loop_info"][:3] - rt)); y_err.append(abs(float(pg_ref.normalize_angle(r["loop_info"][7] - ry))))
            loops.append((k, j, np.array(r["loop_info"][:3]), float(r["loop_info"][7])))
    w = pg_cases.window(W["pv"], W["Rv"], loops)
    w["p_true"] = W["p"][w["first"]:w["last"] + 1]
    return dict(W=W, true=true, decoys=decoys, res_t=res_t, res_d=res_d, eligible=eligible, loops=loops, window=w,
                accept_rate=np.mean([res_t[i]["accepted"] for i in eligible]), decoys_accepted=int(sum(r["accepted"] for r in res_d)),
                t_err=max(t_err), yaw_err=max(y_err))


def _check_mh05(run, corrected_t):
    w = run["window"]
    a_before = pg_cases.positions_ate(w["t"], w["p_true"]); a_after = pg_cases.positions_ate(corrected_t, w["p_true"])
    assert len(run["eligible"]) >= 20
    assert run["accept_rate"] >= ACCEPT_RATE, run["accept_rate"]
    assert run["decoys_accepted"] == 0
    assert run["t_err"] < LOOP_T_ERR and run["yaw_err"] < LOOP_YAW_ERR, (run["t_err"], run["yaw_err"])
    assert a_after <= ATE_RATIO * a_before, (a_after, a_before)
    return a_before, a_after


def test_mh05_end_to_end_numbers_with_the_numpy_reference():
    """The calibration of the GPU end-to-end test: the same case through lc_ref + pg_ref."""
    run = _mh05_run(lambda pairs: [lc_ref.verify(p, *lc.extrinsic()) for p in pairs])
    w = run["window"]
    x, _ = pg_ref.optimize(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
    _check_mh05(run, x[:, 1:])


# ================================================================ GPU
def _gpu_verifier(**kw):
    return uvs.api.LoopVerifier(**kw)


# The LM stops on a step below FLT_EPSILON relative (as CvLevMarq), so a refined pose is pinned to its convergence tolerance, not to the last
# bit: lc_ref itself moves yaw_35's loop_info by 4e-9 when the 3-D points are perturbed by 1e-15 relative.  Integers compare exactly.
POSE_TOL = 1e-7


def _compare(name, pair, r, mo, inl, tol=POSE_TOL):
    tic, qic = lc.extrinsic()
    ref = lc_ref.verify(pair, tic, qic)
    assert np.array_equal(mo, ref["match_old"]), name
    assert ref["margin"] > 1e-9, (name, ref["margin"])          # no match borderline under lc_ref: a count mismatch is never a rounding flip
    for k in ("accepted", "reason", "n_matches", "n_inliers", "best_hypothesis", "ransac_iters"):
        assert r[k] == ref[k], (name, k, r[k], ref[k])
    assert np.array_equal(r["hyp_inliers"], ref["hyp_inliers"]), (name, np.flatnonzero(r["hyp_inliers"] != ref["hyp_inliers"]))
    assert np.array_equal(inl, ref["inlier"]), name
    for k in ("loop_info", "PnP_T_old", "PnP_q_old"):
        a, b = np.asarray(r[k]), np.asarray(ref[k])
        assert np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))), (name, k, a, b)
    return ref


@pytest.mark.gpu
def test_gpu_matching_and_ransac_match_the_reference_on_every_unit_case():
    v = _gpu_verifier(max_pairs=4)
    tic, qic = lc.extrinsic()
    for name, pair in lc.unit_pairs().items():
        res, mo, inl = v.verify([pair], tic, qic)
        _compare(name, pair, res[0], mo[0], inl[0])
    v.close()


@pytest.mark.gpu
def test_gpu_gates_reject_with_the_right_reason():
    v = _gpu_verifier(max_pairs=16)
    tic, qic = lc.extrinsic()
    cases = lc.unit_pairs()
    want = {"matches_25": R["FEW_MATCHES"], "matches_26": R["ACCEPTED"], "shuffled_3d": R["RANSAC_FAILED"], "yaw_35": R["YAW_GATE"],
            "offset_25m": R["T_GATE"], "inliers_25": R["FEW_INLIERS"], "inliers_26": R["ACCEPTED"], "clean": R["ACCEPTED"]}
    names = list(want)
    res, _, _ = v.verify([cases[n] for n in names], tic, qic)
    for n, r in zip(names, res):
        assert r["reason"] == want[n], (n, r["reason"])
        assert r["accepted"] == (want[n] == R["ACCEPTED"]), n
    by = dict(zip(names, res))
    assert by["inliers_25"]["n_inliers"] == 25 and by["inliers_26"]["n_inliers"] == 26
    assert by["matches_25"]["n_matches"] == 25 and by["matches_26"]["n_matches"] == 26
    assert abs(by["yaw_35"]["loop_info"][7] + 35.0) < 0.5
    assert np.linalg.norm(by["offset_25m"]["loop_info"][:3]) > 20.0
    v.close()


def _bits(res, mo, inl):
    out = []
    for r, m, i in zip(res, mo, inl):
        out.append((tuple((k, np.asarray(v).tobytes()) for k, v in sorted(r.items())), m.tobytes(), i.tobytes()))
    return out


@pytest.mark.gpu
def test_gpu_determinism_and_batch_equals_one_at_a_time():
    v = _gpu_verifier(max_pairs=32)
    tic, qic = lc.extrinsic()
    cases = list(lc.unit_pairs().values())
    empty_q = dict(cases[0]); empty_q["p3d"] = np.zeros((0, 3)); empty_q["qdesc"] = np.zeros((0, 4), np.uint64)
    empty_o = dict(cases[1]); empty_o["uv"] = np.zeros((0, 2)); empty_o["odesc"] = np.zeros((0, 4), np.uint64)
    batch = [cases[0], empty_q, cases[1], cases[11], empty_o] + cases[2:] + [cases[0]]
    a = _bits(*v.verify(batch, tic, qic))
    b = _bits(*v.verify(batch, tic, qic))
    assert a == b
    one = [_bits(*v.verify([p], tic, qic))[0] for p in batch]
    assert a == one
    res, mo, _ = v.verify([empty_q, empty_o], tic, qic)
    assert [r["reason"] for r in res] == [R["NO_MATCHES"], R["NO_MATCHES"]]
    assert len(mo[0]) == 0 and np.all(mo[1] == -1)
    v.close()


@pytest.mark.gpu
def test_gpu_mh05_end_to_end_loops_correct_the_drift():
    v = _gpu_verifier(max_pairs=64)
    tic, qic = lc.extrinsic()

    def verify_many(pairs):
        out = []
        for s in range(0, len(pairs), 64):
            out += v.verify(pairs[s:s + 64], tic, qic)[0]
        return out

    run = _mh05_run(verify_many)
    ref = [lc_ref.verify(p, tic, qic) for p in [run["W"]["pair_of"](k, j) for k, j in run["true"]]]
    assert [r["accepted"] for r in run["res_t"]] == [r["accepted"] for r in ref]
    w = run["window"]
    yaw_t, rep = uvs.api.PoseGraphSolver(max_keyframes=512, max_loops=64).optimize(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
    a_before, a_after = _check_mh05(run, yaw_t[:, 1:])
    print(f"MH_05: {len(run['eligible'])} eligible candidates, accepted {run['accept_rate']:.2f}; decoys accepted {run['decoys_accepted']} of "
          f"{len(run['decoys'])}; loop_info error <= {run['t_err'] * 100:.2f} cm / {run['yaw_err']:.3f} deg; ATE {a_before:.3f} -> {a_after:.3f} m")
    v.close()


def _non_finite_cases():
    """`clean` with one matched input made non-finite -> name -> (pair, the match index m that is bad, or None for vio_t)."""
    base = lc.unit_pairs()["clean"]
    mo = lc_ref.match(base["qdesc"], base["odesc"])
    mi = np.flatnonzero(mo >= 0)
    m = 7; q = int(mi[m])
    out = {}
    for name, val in (("p3d_nan", np.nan), ("p3d_inf", np.inf)):
        p = dict(base); p["p3d"] = np.array(base["p3d"], np.float64); p["p3d"][q, 1] = val
        out[name] = (p, m)
    p = dict(base); p["uv"] = np.array(base["uv"], np.float64); p["uv"][mo[q], 0] = np.nan
    out["uv_nan"] = (p, m)
    p = dict(base); p["vio_t"] = np.array(base["vio_t"], np.float64); p["vio_t"][2] = np.nan
    out["vio_t_nan"] = (p, None)
    return out


@pytest.mark.gpu
def test_gpu_non_finite_inputs_follow_the_kernels_rules():
    """uvs_lc_verify forwards non-finite coordinates to the kernel, whose rules then apply: a hypothesis whose initial cost is not finite is
    invalid (-1), and a match whose error is NaN is never an inlier.  The call succeeds and every double it returns is finite."""
    v = _gpu_verifier(max_pairs=1)
    tic, qic = lc.extrinsic()
    for name, (pair, m) in _non_finite_cases().items():
        rc, res, mo, inl = v.verify_raw([pair], tic, qic)
        assert rc == abi.UVS_OK, name
        r, mo, inl = res[0], mo[0], inl[0]
        ref = lc_ref.verify(pair, tic, qic)
        n = ref["n_matches"]
        assert np.array_equal(mo, ref["match_old"]) and r["n_matches"] == n == 60, name
        for k in ("loop_info", "PnP_T_old", "PnP_q_old"):
            assert np.all(np.isfinite(r[k])), (name, k, r[k])
        if m is None:
            assert r["reason"] == R["RANSAC_FAILED"] and r["accepted"] == 0 and r["best_hypothesis"] == -1 and r["ransac_iters"] == 100, name
            assert np.all(r["hyp_inliers"] == -1) and not inl.any() and r["n_inliers"] == 0, name
            assert not r["loop_info"].any() and not r["PnP_T_old"].any() and np.array_equal(r["PnP_q_old"], [0.0, 0.0, 0.0, 1.0]), name
            assert ref["reason"] == R["RANSAC_FAILED"] and np.all(ref["hyp_inliers"] == -1), name
            continue
        seed = int(pair["seed"]) & lc_ref.M64
        drew = np.array([m in lc_ref.draw(seed, h, n) for h in range(lc_ref.N_HYP)])
        assert 0 < drew.sum() < lc_ref.N_HYP, name
        assert np.all(r["hyp_inliers"][drew] == -1) and np.all(r["hyp_inliers"][~drew] >= 0), (name, r["hyp_inliers"])
        assert ref["margin"] > 1e-9, (name, ref["margin"])
        assert np.array_equal(r["hyp_inliers"], ref["hyp_inliers"]), (name, np.flatnonzero(r["hyp_inliers"] != ref["hyp_inliers"]))
        for k in ("accepted", "reason", "n_inliers", "best_hypothesis", "ransac_iters"):
            assert r[k] == ref[k], (name, k, r[k], ref[k])
        assert np.array_equal(inl, ref["inlier"]), name
        q = int(np.flatnonzero(mo >= 0)[m])
        assert inl[q] == 0 and r["n_inliers"] == 59 and r["accepted"] == 1, name
        for k in ("loop_info", "PnP_T_old", "PnP_q_old"):
            a, b = np.asarray(r[k]), np.asarray(ref[k])
            assert np.all(np.abs(a - b) <= POSE_TOL * np.maximum(1.0, np.abs(b))), (name, k, a, b)
    v.close()


@pytest.mark.gpu
def test_gpu_argument_checks():
    v = _gpu_verifier(max_pairs=2, max_query=64, max_old=128)
    tic, qic = lc.extrinsic()
    ok = lc.planted_pair(1)[0]
    assert v.verify_raw([ok], tic, qic)[0] == abi.UVS_OK
    for k in ("pairs", "tic", "qic", "match_old", "inlier", "results"):
        assert v.verify_raw([ok], tic, qic, null=(k,))[0] == abi.UVS_ERR_INVALID_ARG, k
    assert v.verify_raw([ok], tic, qic, n_pairs=0)[0] == abi.UVS_ERR_INVALID_ARG
    assert v.verify_raw([ok, ok, ok], tic, qic)[0] == abi.UVS_ERR_CAPACITY
    big_q = lc.planted_pair(2, n_in=65)[0]
    assert v.verify_raw([big_q], tic, qic)[0] == abi.UVS_ERR_CAPACITY
    big_o = lc.planted_pair(3, n_in=30, n_distract=99)[0]
    assert v.verify_raw([big_o], tic, qic)[0] == abi.UVS_ERR_CAPACITY
    assert v.verify_raw([ok], tic, np.asarray(qic) * 1.01)[0] == abi.UVS_ERR_INVALID_ARG
    bad = dict(ok); bad["vio_q"] = np.array([0.0, 0.0, 0.0, 2.0])
    assert v.verify_raw([bad], tic, qic)[0] == abi.UVS_ERR_INVALID_ARG
    assert "unit quaternion" in uvs.api.lib().uvs_lc_last_error(v._h).decode()
    arr, keep = abi.lc_pairs([ok])
    arr[0].p3d = None
    out = (abi.LcResult * 1)(); mo = np.zeros(64, np.int32); inl = np.zeros(64, np.uint8)
    t_ = np.ascontiguousarray(tic); q_ = np.ascontiguousarray(qic)
    rc = uvs.api.lib().uvs_lc_verify(v._h, 1, C.cast(arr, C.POINTER(abi.LcPair)), abi._dp(t_), abi._dp(q_), mo.ctypes.data_as(C.POINTER(C.c_int32)),
                                     inl.ctypes.data_as(C.POINTER(C.c_uint8)), C.cast(out, C.POINTER(abi.LcResult)))
    assert rc == abi.UVS_ERR_INVALID_ARG
    arr[0].n_query = -1
    rc = uvs.api.lib().uvs_lc_verify(v._h, 1, C.cast(arr, C.POINTER(abi.LcPair)), abi._dp(t_), abi._dp(q_), mo.ctypes.data_as(C.POINTER(C.c_int32)),
                                     inl.ctypes.data_as(C.POINTER(C.c_uint8)), C.cast(out, C.POINTER(abi.LcResult)))
    assert rc == abi.UVS_ERR_INVALID_ARG
    assert v.verify_raw([ok], tic, qic)[0] == abi.UVS_OK           # the handle still works after every rejected call
    v.close()
    h = C.c_void_p()
    L = uvs.api.lib()
    assert L.uvs_lc_create(0, 1, abi.LC_MAX_QUERY + 1, 16, C.byref(h)) == abi.UVS_ERR_CAPACITY
    assert L.uvs_lc_create(0, 0, 16, 16, C.byref(h)) == abi.UVS_ERR_INVALID_ARG
    assert L.uvs_lc_create(0, 1, 16, 16, None) == abi.UVS_ERR_INVALID_ARG
