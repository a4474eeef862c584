"""The back substitution of the reduced system (uvs_solve_kernel.h: chol_solve) is unrolled over its eleven block steps, so every step is its
own code: register slot, 16-lane row, block offsets and trip count are constants of the step.  A slip in one of them can hide in a norm over all
176 unknowns, so the residual of the device's step is bounded PER FRAME BLOCK here.

One debug step (uvs_debug_step) per case and radius on k_solve with 512 threads, on k_solve with 256 threads and through the landmark-sharded
kernels (k_large_solve calls the same function).  With y = step / s in longdouble and (M, b) the Jacobi-scaled damped system built from the
product's own evaluation dump (lm_step_check._case, as in tests/test_gpu_lm_step.py):

    || (M y - b)_k ||  <=  tol ( || M_k. || || y || + || b_k || )      for each of the 11 blocks k of 15 frame rows, infinity norms,
    tol = max(1e-13, 10 x the backward error of the FP64 Schur path on the same system)      (the rule of tests/test_gpu_lm_step.py)

and the three forms agree per frame block to the bound tests/test_gpu_instantiations.py puts on two instantiations: 1e-9 max(1, |.|).

Cases: `prior` (the half-row path: far blocks through rows {0..5, 15}), `full_rows` (all 16 rows of the far blocks), `small` (chunks far smaller
than a wave) of tests/lm_step_cases.py, and the window of tests/golden/points_only.npz (no line chunk).  Radii: the first three of
lm_step_check.RADII -- the fresh linearization and two re-dampings up to the default radius 1e4, the radius the product starts with."""
import importlib.util
import os

import numpy as np
import pytest

from helpers import abi
import lm_step_cases as cases
import lm_step_check as chk
import lm_step_ref as ref
from lm_step_check import _Env

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["prior", "full_rows", "small", "points_only_golden"]
RADII = chk.RADII[:3]
FORMS = {"k_solve512": (0, {"UVS_KSOLVE_NT": "512"}), "k_solve256": (0, {"UVS_KSOLVE_NT": "256"}), "k_large": (1, {})}
NB, BS = abi.NUM_FRAMES, 15
INSTANTIATION_BOUND = 1e-9      # tests/test_gpu_instantiations.py: |a - b| <= 1e-9 max(1, |b|)

_golden = {}
_runs = {}


def _golden_case(gpu_api, oracle):
    """The window of tests/golden/points_only.npz as a case of lm_step_check._case: (window, options, system, reference cache)."""
    if not _golden:
        spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
        mg = importlib.util.module_from_spec(spec); spec.loader.exec_module(mg)
        w = mg.dict_to_window(dict(np.load(os.path.join(HERE, "golden", "points_only.npz"))))
        opts = abi.default_options()
        assert len(w.inv_depth) > 0 and len(w.line_orth) == 0 and len(w.ln_lm) == 0 and (w.prior is None or w.prior.n == 0)
        with _Env({"UVS_KSOLVE_NT": "512"}):
            s = gpu_api.Solver(opts=opts, max_batch=2)
        try:
            ev = s.evaluate(w, robust=True)
        finally:
            s.close()
        eo = oracle.evaluate(w, robust=True, opts=opts)
        for nm in ("pt_r", "pt_J", "imu_r", "imu_J"):
            assert chk._blockwise_relerr(getattr(ev, nm), getattr(eo, nm)) < 1e-9, nm
        _golden["case"] = (w, opts, ref.System(w, ev, opts), {})
    return _golden["case"]


def _case(gpu_api, oracle, name):
    return _golden_case(gpu_api, oracle) if name == "points_only_golden" else chk._case(gpu_api, oracle, name)


def _steps(gpu_api, oracle, name):
    """{form: step [len(RADII), n]} of the case, one run per form."""
    if name not in _runs:
        w, opts, sysm, cache = _case(gpu_api, oracle, name)
        out = {}
        for form, (f, env) in FORMS.items():
            with _Env(env):
                s = gpu_api.Solver(opts=opts, max_batch=2, **cases.capacity(name))
            try:
                with _Env(cases.environment(name) if name in cases.NAMES else {}):
                    out[form], _ = s.debug_step(w, RADII, form=f)
            finally:
                s.close()
        _runs[name] = out
    return _runs[name]


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", NAMES)
def test_residual_of_the_step_per_frame_block(gpu_api, oracle, name, form):
    w, opts, sysm, cache = _case(gpu_api, oracle, name)
    steps = _steps(gpu_api, oracle, name)[form]
    grps = ref.groups(w, opts)
    bad = []
    for i, r in enumerate(RADII):
        _, _, bwd64, _, _ = chk._reference(cache, sysm, r, grps)
        tol = max(chk.BWD_FLOOR, 10 * bwd64)
        assert np.all(np.isfinite(steps[i])), (name, form, r)
        M = sysm.M(r)
        y = np.asarray(steps[i], LD) / sysm.s
        res = M @ y - sysm.b
        ynorm = np.abs(y).max()
        ratios = []
        for k in range(NB):
            rows = slice(BS * k, BS * k + BS)
            bound = tol * (np.abs(M[rows]).sum(axis=1).max() * ynorm + np.abs(sysm.b[rows]).max())
            ratios.append(float(np.abs(res[rows]).max() / bound))
        print(f"{name}/{form} r={r:g}: tol {tol:.2e}, ||r_k|| / bound per block: " + " ".join(f"{v:.3f}" for v in ratios))
        bad += [(r, k, v) for k, v in enumerate(ratios) if not v <= 1.0]
    assert not bad, (name, form, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_the_three_forms_agree_per_frame_block(gpu_api, oracle, name):
    runs = _steps(gpu_api, oracle, name)
    base = runs["k_solve512"]
    bad = []
    for form in ("k_solve256", "k_large"):
        for i, r in enumerate(RADII):
            worst = []
            for k in range(NB):
                a, b = runs[form][i, BS * k:BS * k + BS], base[i, BS * k:BS * k + BS]
                worst.append(float(np.abs(a - b).max() / (INSTANTIATION_BOUND * max(1.0, np.abs(b).max()))))
            print(f"{name}: {form} against k_solve512, r={r:g}: |difference| / bound per block: " + " ".join(f"{v:.2e}" for v in worst))
            bad += [(form, r, k, v) for k, v in enumerate(worst) if not v <= 1.0]
    assert not bad, (name, bad)
