"""Loop verification's PnP (k_lc_verify, csrc/uvs_loop_verify.hip) pinned to the 60-digit reference of tests/lc_hp.py, stage by stage, from the
trace uvs_lc_debug_pair records.

CPU tests prove the checker without a GPU: lc_ref's own FP64 trace stays within half of every bound (which leaves a factor two for a device
whose operation order differs but whose rounding count is what was counted), planted errors fail at their stage, the 60-digit mathematics
agrees with analytic facts, and the trace layout is the header's.  GPU tests run the same checker on the device's trace and hold every stage to
its bound, with nothing excused.  The figures go to the file UVS_LC_LOG names."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import lc_cases as lc
import lc_hp
import lc_ref
from helpers import abi, uvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = lc_hp.F

# name -> how much of stages 2, 4 and 6 is checked: every iteration, or (max_query: 1024 matches) iteration 0 and the last one of every record
CASES = {"matches_26": "all", "clean": "all", "outliers_60pct": "all", "behind_camera": "all", "over_256": "all", "shuffled_3d": "all", "max_query": "ends"}


def pair_of(name):
    if name == "over_256":          # 300 matches: the strided j += 256 loops of the mask and the refinement take a second trip
        return lc.planted_pair(15, n_in=280, n_out=20)[0]
    return lc.unit_pairs()[name]


@pytest.fixture(scope="module", autouse=True)
def lc_log():
    lc_hp.pool()                     # the reference's workers exist before anything touches the GPU
    yield
    lc_hp.write_log()
    lc_hp.shutdown()


_ref = {}


def ref_trace(name):
    """lc_ref's result and trace of a case, computed once."""
    if name not in _ref:
        _ref[name] = lc_ref.verify(pair_of(name), *lc.extrinsic(), trace=True)
    return _ref[name]


def as_trace(out, raw):
    return dict(raw=raw, result=out, match_old=out["match_old"], inlier=out["inlier"])


def show(name, rep):
    print(f"{name}: excused {rep.excused}; " + "; ".join(f"{s} {rep.ratio[s]:.3g}" for s in lc_hp.STAGES))
    print("   " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(rep.figures.items())))


# ================================================================ CPU: the checker and its bounds
@pytest.mark.parametrize("name", list(CASES))
def test_lc_ref_trace_is_within_half_of_every_bound(name):
    """Measured (worst error / bound over the cases): prior 0.25, normal equations 0.16, step 0.20, candidate 0.25, orthonormality 0.16,
    finish 0.32; lc_ref's stage-4 figure is at most 1.950 u scale and its yaw figure at most 1.894 u |yaw| (the constants of lc_hp)."""
    out, raw = ref_trace(name)
    pair = pair_of(name)
    rep = lc_hp.check_trace(as_trace(out, raw), pair, lc.extrinsic(), iters_mode=CASES[name], ref=(out, raw), name="lc_ref " + name)
    show(name, rep)
    assert rep.failures == []
    assert rep.excused == 0
    for s in lc_hp.STAGES:
        assert rep.ratio[s] <= 0.5, (s, rep.ratio[s], rep.where[s])
    # the measured library constants hold lc_ref itself
    assert rep.figures.get("stage4_raw", 0.0) <= lc_hp.K4_LC_REF
    yaws = [lc_hp.yaw_error_in_u(lc_ref.quat_to_R(pair["vio_q"]))]
    if out["best_hypothesis"] >= 0:
        yaws.append(lc_hp.yaw_error_in_u(lc_ref.quat_to_R(out["PnP_q_old"])))
    print(f"   lc_ref's yaw error / (u |yaw|): {max(yaws):.3f}")
    lc_hp.log(f"{'lc_ref ' + name:28s} yaw error / (u |yaw|) {max(yaws):.3f}")
    assert max(yaws) <= lc_hp.K_ATAN2_LC_REF
    if name == "shuffled_3d":
        assert out["reason"] == lc_ref.REASON["RANSAC_FAILED"]
    else:
        assert out["best_hypothesis"] >= 0 and "distance" in rep.figures


PLANT_CASE, PLANT_HYP, PLANT_IT = "matches_26", 3, 1


def _planted(kind):
    out, raw = ref_trace(PLANT_CASE)
    out = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in out.items()}; raw = raw.copy()
    rec = raw[:lc_ref.TRACE_STAGE].reshape(lc_ref.N_HYP + 1, lc_ref.TRACE_REC)
    r = rec[PLANT_HYP, lc_ref.TRACE_HEAD:].reshape(lc_ref.LM_ITERS, lc_ref.TRACE_ITER)[PLANT_IT]
    assert rec[PLANT_HYP, 6] > PLANT_IT + 1 and r[41] == 1.0
    if kind == "acc":                 # a diagonal J^T J entry: every term is positive, so its scale S is the entry itself up to the |.| inside J
        r[13] *= 1 + 1e-12
    elif kind == "d":                 # the component that carries the largest share of its own row
        A = np.array(lc_hp.unpack_upper(list(r[13:34])), float)
        i = int(np.argmax(np.abs(np.diag(A) * r[42:48])))
        r[42 + i] *= 1 + 1e-10
    elif kind == "cand":
        r[48 + 4] += 1e-13
    elif kind == "accepted":
        r[62] = 1.0 - r[62]
    elif kind == "count":
        out["hyp_inliers"][PLANT_HYP] += 1
    elif kind == "loop_info":
        out["loop_info"][1] *= 1 + 1e-12
    return out, raw


@pytest.mark.parametrize("kind,stage", [("none", None), ("acc", "2 normal eq"), ("d", "3 step"), ("cand", "4 candidate"), ("accepted", "5 decisions"),
                                        ("count", "7 counts"), ("loop_info", "9 finish")])
def test_checker_catches_planted_errors(kind, stage):
    out, raw = _planted(kind)
    rep = lc_hp.check_trace(as_trace(out, raw), pair_of(PLANT_CASE), lc.extrinsic(), hyps=[PLANT_HYP], ref=ref_trace(PLANT_CASE))
    if stage is None:
        assert rep.failures == [] and all(rep.ratio[s] <= 0.5 for s in lc_hp.STAGES)
        return
    assert rep.stage_failed(stage), (kind, rep.ratio, rep.failures)
    # the stages before it that do not read the planted value stay clean
    for s in lc_hp.STAGES[:lc_hp.STAGES.index(stage)]:
        if kind == "count" and s == "8 selection":
            continue
        assert not rep.stage_failed(s), (kind, s, rep.ratio[s], rep.where[s])


def test_hp_jacobian_matches_central_differences():
    rng = np.random.default_rng(3)
    R = lc_hp.exp_so3(lc_hp.V(rng.normal(0, 0.5, 3))); t = lc_hp.V(rng.normal(0, 0.3, 3))
    h = F(10) ** -20
    for _ in range(4):
        X = lc_hp.V(rng.normal(0, 1, 3) + [0, 0, 6]); uv = lc_hp.V(rng.normal(0, 0.2, 2))
        _, J, _, Jb, _ = lc_hp.residual_jacobian(R, t, X, uv)
        for c in range(6):
            d = [F(0)] * 6; d[c] = h
            rp = lc_hp.residual_jacobian(lc_hp.matmul(lc_hp.exp_so3(d[:3]), R), [t[i] + d[3 + i] for i in range(3)], X, uv)[0]
            rm = lc_hp.residual_jacobian(lc_hp.matmul(lc_hp.exp_so3([-v for v in d[:3]]), R), [t[i] - d[3 + i] for i in range(3)], X, uv)[0]
            for k in range(2):
                assert abs((rp[k] - rm[k]) / (2 * h) - J[k][c]) < F(10) ** -30 * (1 + abs(J[k][c])), (c, k)       # the quotient's own error is h^2 f''' / 6, h^2 = 1e-40
                assert Jb[k][c] >= abs(J[k][c])


def test_hp_gradient_of_a_noiseless_pair_vanishes_at_the_true_pose():
    rng = np.random.default_rng(4)
    R = lc_hp.exp_so3(lc_hp.V(rng.normal(0, 0.7, 3))); t = lc_hp.V(rng.normal(0, 0.5, 3))
    Xs, us = [], []
    for _ in range(12):
        Xc = lc_hp.V(np.r_[rng.uniform(-1, 1, 2), rng.uniform(2, 8)])
        Xs.append(lc_hp.matvec(lc_hp.transpose(R), [Xc[i] - t[i] for i in range(3)])); us.append([Xc[0] / Xc[2], Xc[1] / Xc[2]])
    acc, _ = lc_hp.normal_equations(R, t, Xs, us)
    assert max(abs(v) for v in acc[21:28]) < F(10) ** -50
    # and from a displaced pose the 60-digit Gauss-Newton comes back to it
    Rm, tm, _, _ = lc_hp.minimiser(lc_hp.matmul(lc_hp.exp_so3(lc_hp.V([1e-3, -2e-3, 1e-3])), R), [t[0] + F("0.001"), t[1], t[2] - F("0.002")], Xs, us)
    assert lc_hp.pose_distance(R, t, Rm, tm) < F(10) ** -45


def test_hp_exp_is_orthonormal_to_50_digits():
    rng = np.random.default_rng(5)
    for w in [rng.normal(0, 1, 3), rng.normal(0, 1e-9, 3), rng.normal(0, 1e-25, 3), rng.normal(0, 40, 3), np.zeros(3)]:
        E = lc_hp.exp_so3(lc_hp.V(w))
        assert lc_hp.orthonormality(E) < F(10) ** -50
        assert all(lc_hp.exp_so3_scale(lc_hp.V(w))[i][j] >= abs(E[i][j]) for i in range(3) for j in range(3))
    # against the FP64 restatement, to FP64 accuracy
    w = rng.normal(0, 0.3, 3)
    assert np.abs(np.array(lc_hp.exp_so3(lc_hp.V(w)), float) - lc_ref.exp_so3(w)).max() < 1e-15


def test_no_case_has_a_borderline_adaptive_iteration_count():
    """RANSACUpdateNumIters rounds num / denom to an integer: no committed case may have it within 1e-9 of a half-integer, so the selection
    (stage 8) is compared exactly and nothing is excused."""
    for name in CASES:
        out, _ = ref_trace(name)
        n = out["n_matches"]; best_count = 0; niters = lc_ref.N_HYP; h = 0
        while h < niters:
            c = int(out["hyp_inliers"][h])
            if c > max(best_count, lc_ref.MODEL_POINTS - 1):
                best_count = c
                denom = 1.0 - (1.0 - (n - c) / n) ** lc_ref.MODEL_POINTS
                if denom >= np.finfo(np.float64).tiny and np.log(denom) < 0:
                    q = np.log(1.0 - lc_ref.CONFIDENCE) / np.log(denom)
                    assert abs((q % 1.0) - 0.5) > 1e-9, (name, h, q)
                niters = lc_ref.update_num_iters(lc_ref.CONFIDENCE, (n - c) / n, lc_ref.MODEL_POINTS, niters)
            h += 1
        assert (out["best_hypothesis"], out["ransac_iters"]) == lc_ref.select(out["hyp_inliers"], n)


# ================================================================ CPU: the ABI of the debug call
def test_lc_debug_symbol_and_trace_layout_match_the_header():
    L = uvs.api.lib()
    assert hasattr(L, "uvs_lc_debug_pair") and "uvs_lc_debug_pair" in uvs.api.EXPORTS
    code = r'''
#include <stdio.h>
#include "uvs_solver.h"
int main(void) {
  printf("%d %d %d %d %d %d\n", UVS_LC_TRACE_HEAD_LEN, UVS_LC_TRACE_ITER_LEN, UVS_LC_TRACE_REC_LEN, UVS_LC_TRACE_STAGE_OFF, UVS_LC_TRACE_LEN, UVS_LC_MAX_QUERY);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c"); exe = os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert out == [abi.LC_TRACE_HEAD_LEN, abi.LC_TRACE_ITER_LEN, abi.LC_TRACE_REC_LEN, abi.LC_TRACE_STAGE_OFF, abi.LC_TRACE_LEN, abi.LC_MAX_QUERY]
    assert out == [lc_ref.TRACE_HEAD, lc_ref.TRACE_ITER, lc_ref.TRACE_REC, lc_ref.TRACE_STAGE, lc_ref.TRACE_LEN, lc_ref.MAX_QUERY]
    assert abi.LC_LM_ITERS == lc_ref.LM_ITERS
    # the views of abi.lc_trace address what lc_ref writes
    out_, raw = ref_trace("matches_26")
    t = abi.lc_trace(raw)
    assert t["n"] == 26 and t["X"].shape == (26, 3) and np.array_equal(t["mq"], np.flatnonzero(out_["match_old"] >= 0))
    assert np.array_equal(t["start"], t["pose"][out_["best_hypothesis"]]) and t["valid"][:100].all() and t["iters"][100] >= 1
    assert np.array_equal(t["it"][100, 0, 0:12], t["start"]) and t["it"][0, 0, 12] == lc_ref.LAMBDA0


def test_lc_debug_pair_rejects_a_null_handle_and_create_fails_loudly_without_a_gpu():
    L = uvs.api.lib()
    assert L.uvs_lc_debug_pair(None, None, None, None, None, None, None, None) == abi.UVS_ERR_INVALID_ARG
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            uvs.api.LoopVerifier()


# ================================================================ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_trace_is_within_every_bound(name):
    """The device's trace through the same checker: every stage within its bound, nothing excused.  Measured on an MI355X (worst error / bound
    over the cases): prior 0.26, normal equations 0.080, step 0.22, candidate 0.30 (2.344 u scale against the allowance of 7.84), orthonormality
    0.16, finish 0.30, distance to the minimiser 0.021 of its bound; nothing excused."""
    pair = pair_of(name)
    ref = ref_trace(name)
    tic, qic = lc.extrinsic()
    v = uvs.api.LoopVerifier(max_pairs=1)
    try:
        res, mo, inl, t = v.debug_pair(pair, tic, qic)
    finally:
        v.close()
    rep = lc_hp.check_trace(dict(raw=t["raw"], result=res, match_old=mo, inlier=inl), pair, (tic, qic), iters_mode=CASES[name], ref=ref, name="device " + name)
    show(name, rep)
    assert rep.failures == []
    assert rep.excused == 0
    for s in lc_hp.STAGES:
        assert rep.ratio[s] <= 1.0, (s, rep.ratio[s], rep.where[s])
    if name == "shuffled_3d":        # the trace ends after the selection: nothing of the refinement or the finish is written
        assert res["reason"] == lc_ref.REASON["RANSAC_FAILED"] and res["best_hypothesis"] == -1
        assert not t["raw"][abi.LC_N_HYPOTHESES * abi.LC_TRACE_REC_LEN:abi.LC_TRACE_STAGE_OFF].any()
        assert not inl.any() and not res["loop_info"].any()
    else:
        assert res["best_hypothesis"] >= 0 and "distance" in rep.figures
    if name == "over_256":
        assert t["n"] == 300 and res["n_inliers"] > 256
    if name == "outliers_60pct":     # the paths the case is there for: rejected steps and hypotheses that run all 20 iterations
        assert (t["iters"][:100] == 20).any() and any(t["it"][h, :t["iters"][h], 62].min() == 0 for h in range(100))


def _bits(res, mo, inl):
    return (tuple((k, np.asarray(v).tobytes()) for k, v in sorted(res.items())), mo.tobytes(), inl.tobytes())


@pytest.mark.gpu
def test_gpu_debug_call_equals_the_public_call_bit_for_bit_and_is_deterministic():
    v = uvs.api.LoopVerifier(max_pairs=1)
    tic, qic = lc.extrinsic()
    cases = dict(lc.unit_pairs()); cases["over_256"] = pair_of("over_256")
    for name, pair in cases.items():
        res, mo, inl = v.verify([pair], tic, qic)
        dres, dmo, dinl, t = v.debug_pair(pair, tic, qic)
        assert _bits(dres, dmo, dinl) == _bits(res[0], mo[0], inl[0]), name
        dres2, dmo2, dinl2, t2 = v.debug_pair(pair, tic, qic)
        assert _bits(dres2, dmo2, dinl2) == _bits(dres, dmo, dinl) and t2["raw"].tobytes() == t["raw"].tobytes(), name
        assert t["n"] == res[0]["n_matches"], name
        if res[0]["n_matches"] <= lc_ref.MIN_LOOP_NUM:
            assert not t["raw"][:abi.LC_TRACE_STAGE_OFF].any(), name
    v.close()
