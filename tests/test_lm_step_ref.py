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


@pytest.mark.parametrize("name", ["prior_free", "no_jacobi", "td", "extrinsic", "prior", "prior_extrinsic", "skipped_imu", "prior_td", "weak"])
def test_reference_model_cost_change_matches_the_oracle(oracle, name):
    """model_cost_change of the reference step equals the oracle's first iteration (max_num_iterations = 1, initial radius r): the scaling,
    damping, extra columns (td, extrinsic) and the prior's column map (pose, speed/bias and EX_POSE blocks) follow the same conventions."""
    w, opts = cases.build(name, marginalize_fn=cases.oracle_marginalize(oracle, name))
    ev = oracle.evaluate(w, robust=True, opts=opts)
    sysm = ref.System(w, ev, opts)
    for r in (1e-2, 1e2, 1e4, 1e8):
        _, y = ref.damped_step(sysm, r)
        mcc = float(y @ sysm.b - 0.5 * y @ sysm.Hs @ y)
        o = cases.options(name); o.max_num_iterations = 1; o.initial_trust_region_radius = r
        _, rep = oracle.solve(w, opts=o)
        assert abs(rep.model_cost_change[1] - mcc) <= 1e-10 * abs(mcc), (r, rep.model_cost_change[1], mcc)


@pytest.mark.parametrize("name", cases.NAMES + cases.RELO_NAMES + cases.BIG_NAMES + ["many_chunks_plain"] + cases.EXTRA_NAMES)
def test_step_case_structure(oracle, name):
    """Each case has the structure its name promises."""
    w, opts = cases.build(name, marginalize_fn=cases.oracle_marginalize(oracle, name))
    cases.check_structure(name, w, opts)


def test_projection_block_matches_the_autograd_factor():
    """The longdouble projection factor of the relocalization rows (residual and analytic tangent Jacobians, no loss) against pyref's independent
    FP64 point residual with autograd Jacobians: 1e-9 relative to the largest entry of each (FP64 autograd carries the error)."""
    import torch
    import pyref
    w, opts = cases.build("relo_extrinsic")
    first = {}
    for k in range(len(w.pt_lm)): first.setdefault(int(w.pt_lm[k]), int(w.pt_fi[k]))
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    for k in range(0, len(w.relo_lm), max(1, len(w.relo_lm) // 6)):
        lm = int(w.relo_lm[k]); fi = first[lm]
        r, J = ref.projection_block(w.pose[fi], w.relo_pose, w.ex_pose, w.inv_depth[lm], w.relo_pi[k], w.relo_pj[k], opts.point_sqrt_info, 0.0)
        args = (t(w.pose[fi]), t(w.relo_pose), t(w.ex_pose), t(w.inv_depth[lm]), t(w.relo_pi[k]), t(w.relo_pj[k]), opts.point_sqrt_info)
        r0 = pyref.point_residual(*args).numpy(); J0 = pyref.point_jacobian(*args).numpy()
        assert np.abs(np.asarray(r, np.float64) - r0).max() <= 1e-9 * max(np.abs(r0).max(), 1.0), k
        assert np.abs(np.asarray(J, np.float64) - J0).max() <= 1e-9 * np.abs(J0).max(), (k, np.abs(np.asarray(J, np.float64) - J0).max(), np.abs(J0).max())


@pytest.mark.parametrize("name", cases.RELO_NAMES)
def test_reference_model_cost_change_with_relocalization_blocks_matches_the_oracle(oracle, name):
    """As test_reference_model_cost_change_matches_the_oracle on windows with relocalization blocks, whose rows the reference restates itself in
    longdouble (lm_step_ref.relo_rows): fixed extrinsic, free extrinsic, free extrinsic with td, with and without the n = 75 prior."""
    w, opts = cases.build(name, marginalize_fn=oracle.marginalize)
    ev = oracle.evaluate(w, robust=True, opts=opts)
    sysm = ref.System(w, ev, opts)
    assert sysm.L["relo"] is not None and sysm.L["n"] == sysm.L["frames"] + len(w.inv_depth) + 4 * len(w.line_orth)
    for r in (1e-2, 1e2, 1e4, 1e8):
        _, y = ref.damped_step(sysm, r)
        mcc = float(y @ sysm.b - 0.5 * y @ sysm.Hs @ y)
        o = cases.options(name); o.max_num_iterations = 1; o.initial_trust_region_radius = r
        _, rep = oracle.solve(w, opts=o)
        print(f"{name} r={r:g} oracle {rep.model_cost_change[1]:.17g} reference {mcc:.17g} rel {abs(rep.model_cost_change[1] - mcc) / abs(mcc):.2e}")
        assert abs(rep.model_cost_change[1] - mcc) <= 1e-10 * abs(mcc), (r, rep.model_cost_change[1], mcc)


def test_weak_case_is_weak_in_numbers(oracle):
    """`weak`: landmark pivots seven orders (points) and four orders (lines) under the largest, cond(M) < 1e13 at the default radius (cases.check_weak)."""
    w, opts = cases.build("weak")
    sysm = ref.System(w, oracle.evaluate(w, robust=True, opts=opts), opts)
    pt, ln, cond = cases.check_weak(sysm)
    print(f"weak: smallest / largest point pivot {pt:.2e}, smallest line-block eigenvalue / largest {ln:.2e}, cond(M) at 1e4 {cond:.2e}")


def test_fp64_level_of_model_cost_change(oracle):
    """lm_step_ref.fp64_mcc_level, the term of the GPU tests' model_cost_change bound max(1e-10, 10 x level): 1e-14 or less on the windows whose scaled step is
    1e5 long (the bound stays 1e-10 there), 1e-11 .. 1e-10 on prior_td at radius 1e12, where the prior's TD block stretches the step to 2e8 and the residual of
    a careful FP64 solve against that step is what no FP64 form of the sum gets under (measured on the CPU: 4.4e-11 for 0.5 (y.Dy + y.b), 7.4e-11 for
    y.b - y^T Hs y / 2 in FP64; the kernels gave 1.0e-10 on an MI355X)."""
    for name in ("prior", "td", "tracks2", "relo_extrinsic_td", "weak"):
        w, opts = cases.build(name, marginalize_fn=cases.oracle_marginalize(oracle, name))
        sysm = ref.System(w, oracle.evaluate(w, robust=True, opts=opts), opts)
        for r in (1e4, 1e12):
            assert ref.fp64_mcc_level(sysm, r) <= 1e-14, (name, r)
    w, opts = cases.build("prior_td", marginalize_fn=cases.oracle_marginalize(oracle, "prior_td"))
    sysm = ref.System(w, oracle.evaluate(w, robust=True, opts=opts), opts)
    assert ref.fp64_mcc_level(sysm, 1e8) <= 1e-13
    lvl = ref.fp64_mcc_level(sysm, 1e12)
    _, y = ref.damped_step(sysm, 1e12)
    assert 1e-11 <= lvl <= 1e-10 and float(np.sqrt(np.sum(y * y))) > 1e8, lvl
