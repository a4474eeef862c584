"""The damped LM step of the persistent kernel (uvs_debug_step, form 0 = k_solve) against the extended-precision reference of
tests/lm_step_ref.py, per block group, per radius, on both instantiations of the kernel.

Bounds:
  forward  ||d_G - d*_G|| / ||d*_G|| <= max(10 x FP64 level of the group, 1e-12)   (FP64 level: worst of dense LU in three orders and a plain FP64
                                                                                    Schur path on the same system, lm_step_ref.fp64_level)
  backward ||M y - b|| / (||M|| ||y|| + ||b||) <= max(1e-13, 10 x the FP64 Schur path's), in longdouble at the device's y = d / s.
  model_cost_change and step_norm^2 against longdouble values formed from the device's step: 1e-10 relative; for model_cost_change
  max(1e-10, 10 x lm_step_ref.fp64_mcc_level), the error a careful FP64 solve of the same system leaves in that sum.  The level is 1e-16 .. 1e-14
  everywhere except on prior_td at radius 1e12 (scaled step 2e8 long, cond(M) 3.8e12): 3.5e-11 there, the kernels measured 1.005e-10.
The floors are the pose graph's starting points (test_pose_graph.py: _check_step); the levels measured on an MI355X are in DESIGN.md.
The system is built from the product's own evaluation dump (checked against the oracle's first), which isolates the linear algebra.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import abi
import lm_step_cases as cases
import lm_step_check as chk
import lm_step_ref as ref
from lm_step_check import RADII, REDAMP, _Env, _case, _check_run

SUBSET_256 = ["prior", "full_rows", "small", "td", "extrinsic", "no_jacobi"]      # every option and both Cholesky variants


@pytest.fixture(scope="module")
def step_log():
    yield chk._log
    chk.write_log()


def _run_case(gpu_api, oracle, name, nt, step_log):
    w, opts, sysm, cache = _case(gpu_api, oracle, name)
    with _Env({"UVS_KSOLVE_NT": str(nt)}):
        s = gpu_api.Solver(opts=opts, max_batch=2, **cases.capacity(name))
    try:
        with _Env(cases.environment(name)):
            for radii in (RADII, REDAMP):
                steps, scal = s.debug_step(w, radii, form=0)
                _check_run(w, opts, sysm, cache, radii, steps, scal, f"{name}/k_solve{nt}")
            # the debug instantiation and the product kernel compute the same first step, bit for bit
            first = s.debug_first_iteration(w)["step"]
            one, _ = s.debug_step(w, [opts.initial_trust_region_radius], form=0)
        L = ref.layout(w, opts)
        pad = [16 * f + a for f in range(abi.NUM_FRAMES) for a in range(15)]
        pad += [16 * a + 15 for a in range(6)] if L["ex"] is not None else []
        pad += [175] if L["td"] is not None else []
        if L["relo"] is not None and L["ex"] is None: pad += [16 * a + 15 for a in range(6)]      # relo_Pose beside a fixed extrinsic: the spare rows of the reduced system
        nfr = len(pad)      # (relo_Pose beside a free extrinsic is eliminated on a second level: not among the 176 of debug_first_iteration)
        assert np.array_equal(one[0][:nfr], first[pad]), (name, nt, np.abs(one[0][:nfr] - first[pad]).max())
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.NAMES + cases.RELO_NAMES + ["many_chunks_mid"] + cases.EXTRA_NAMES)
def test_k_solve_step_matches_the_reference(gpu_api, oracle, name, step_log):
    _run_case(gpu_api, oracle, name, 512, step_log)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SUBSET_256 + ["relo", "relo_extrinsic_td"] + cases.EXTRA_NAMES)
def test_k_solve256_step_matches_the_reference(gpu_api, oracle, name, step_log):
    _run_case(gpu_api, oracle, name, 256, step_log)


@pytest.mark.gpu
def test_debug_step_rejects_bad_arguments(gpu_api):
    w, opts = cases.build("small")
    s = gpu_api.Solver(opts=opts, max_batch=2)
    try:
        for radii, form in (([0.0], 0), ([-1.0], 0), ([np.inf], 0), ([np.nan], 0), ([1e4], 7), ([0.0], 1), ([np.nan], 1), ([1e4, -1.0], 1), ([1e4], 2), ([1e4], -1)):
            with pytest.raises(RuntimeError, match="uvs error 1"):
                s.debug_step(w, radii, form=form)
        wc, keep = w.to_c()
        n = 165 + 7 + 12
        st = np.zeros(n + 1); sc = np.zeros(40); r = np.array([1e4])
        assert gpu_api.lib().uvs_debug_step(s._h, C.byref(wc), 0, 1, abi._dp(r), n + 1, abi._dp(st), abi._dp(sc)) == abi.UVS_ERR_INVALID_ARG
        assert gpu_api.lib().uvs_debug_step(s._h, C.byref(wc), 1, 1, abi._dp(r), n + 1, abi._dp(st), abi._dp(sc)) == abi.UVS_ERR_INVALID_ARG
    finally:
        s.close()
