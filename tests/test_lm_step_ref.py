"""CPU pins of the extended-precision step reference (tests/lm_step_ref.py) that the GPU step tests compare the kernels with."""
import numpy as np
import pytest

from helpers import abi, dense_normal_equations
import lm_step_cases as cases
import lm_step_ref as ref


def test_reference_residual_is_extended_precision(oracle):
    """The longdouble solve satisfies its own system to <= 1e-17 (relative backward error), at small and at large radius."""
    w, opts = cases.build("prior_free")
    ev = oracle.evaluate(w, robust=True, opts=opts)
    sysm = ref.System(w, ev, opts)
    for r in (1e-2, 1e4, 1e10):
        _, y = ref.damped_step(sysm, r)
        assert ref.backward_error(sysm.M(r), sysm.b, y) <= 1e-17, r


def test_reference_matches_the_dense_fp64_step(oracle):
    """On a well-conditioned system (small radius) the reference equals pyref_lm's dense FP64 step (Jacobi scaling, clamped diagonal)."""
    w, opts = cases.build("prior_free")
    ev = oracle.evaluate(w, robust=True, opts=opts)
    H, g = dense_normal_equations(w, ev)
    s = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    Hs, gs = H * np.outer(s, s), g * s
    sysm = ref.System(w, ev, opts)
    for r in (1e-2, 1.0):
        y = np.linalg.solve(Hs + np.diag(np.clip(np.diag(Hs), 1e-6, 1e32) / r), -gs)
        delta, _ = ref.damped_step(sysm, r)
        e = ref.group_errors(s * y, delta, ref.groups(w, opts))
        assert max(e.values()) <= 1e-13, (r, max(e, key=e.get), max(e.values()))


@pytest.mark.parametrize("name", ["prior_free", "no_jacobi", "td", "extrinsic", "prior", "prior_extrinsic", "skipped_imu"])
def test_reference_model_cost_change_matches_the_oracle(oracle, name):
    """model_cost_change of the reference step equals the oracle's first iteration (max_num_iterations = 1, initial radius r): the scaling,
    damping, extra columns (td, extrinsic) and the prior's column map (pose, speed/bias and EX_POSE blocks) follow the same conventions."""
    w, opts = cases.build(name, marginalize_fn=oracle.marginalize)
    ev = oracle.evaluate(w, robust=True, opts=opts)
    sysm = ref.System(w, ev, opts)
    for r in (1e-2, 1e2, 1e4, 1e8):
        _, y = ref.damped_step(sysm, r)
        mcc = float(y @ sysm.b - 0.5 * y @ sysm.Hs @ y)
        o = cases.options(name); o.max_num_iterations = 1; o.initial_trust_region_radius = r
        _, rep = oracle.solve(w, opts=o)
        assert abs(rep.model_cost_change[1] - mcc) <= 1e-10 * abs(mcc), (r, rep.model_cost_change[1], mcc)


@pytest.mark.parametrize("name", cases.NAMES)
def test_step_case_structure(oracle, name):
    """Each case has the structure its name promises."""
    w, opts = cases.build(name, marginalize_fn=oracle.marginalize)
    cases.check_structure(name, w, opts)
