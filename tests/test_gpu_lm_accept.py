"""The acceptance half of an LM iteration -- everything after chol_solve -- of every single-window solver against the 60-digit reference of
tests/lm_accept_ref.py, per case of tests/lm_accept_cases.py and per form:

  k_solve at UVS_KSOLVE_NT = 512 and 256 (the decision in k_solve_body), uvs_large_solve (the host's uvs_large_decide), uvs_large_solve_fused (the fused
  device decision) at UVS_LARGE_CHUNKS_NT / UVS_LARGE_SOLVE_NT = 512; the 256-thread instantiations of the landmark-sharded forms on small, prior_td,
  relo_extrinsic_td and rejected_once; rejected_thrice and converged on k_solve 512 and large_solve_fused 512 only.

Per case K is the first accepted iteration under the reference (1, 2 or 4), delta_k = uvs_debug_step(w, [r0, r0/2, r0/8, ...][:K], form) the device's own
full tangent steps, and the product is solved with max_num_iterations = K and K + 1 (lm_accept_ref.check_one_iteration):

  rejected iterations k < K   accepted[k] == 0; cost[k] == initial_cost bit for bit; radius[k] the halving sequence exactly (the divisors are powers of two);
                              candidate_cost[k] within B of the reference cost at round(x0 (+) delta_k).
  iteration K                 accepted == 1; in the returned state positions, speed / bias, td, inverse depths and line parameters == x0 + delta_K bit for bit
                              (one FP64 addition each), blocks that are not free bit-identical to the input, every quaternion within
                              8 x 2^-53 (1 + |dtheta| / 2) absolute per component of the 60-digit plus and of norm within 4 x 2^-53 of 1.
                              The count behind the 8, from pose_plus (csrc/uvs_factors.h:476) with |q| = 1 and t = |dtheta| / 2, in units of 2^-53: dq = d / 2 is
                              exact; a component of q (x) (dtheta / 2, 1) is a sum of four products, the one with dq.w = 1 exact and three scaled by t (3 t), and
                              three additions of partial sums no larger than 1 + t (3 + 3 t); the squared norm carries 4 of its own (four squares, three
                              additions, relative) of which the reciprocal square root halves the effect (2), rsqrt itself 1, the final product 1:
                              7 + 6 t <= 8 (1 + t).  The count is per component and leaves out the first-order effect of the OTHER components' roundings through
                              the norm (at most |q_i| times their 2-norm, reached only when all four err along q); the measured ratio is logged.
  costs                       the reference is evaluated at the device's own returned FP64 state, so plus and the cost path are judged separately:
                              candidate_cost[K] and final_cost of the K run and cost[K] of the K + 1 run (the linearization's own re-sum at the accepted
                              point) within B = factor_ref.cost_bound(ref, 10) [+ the relocalization blocks' share] + C_q 2^-53 A of the reference.
  scalars, both runs          relative_decrease[k] == (cost[k-1] - candidate_cost[k]) / model_cost_change[k] formed in FP64 from the report's numbers, bit for
                              bit; |rho - rho*| <= (B_cost + B_cand) / |mcc| + 1e-10 |rho*|; model_cost_change[k] within 1e-10 of the debug step's (logged:
                              whether bit-equal); step_norm[k] within 1 ulp of sqrt(step_norm^2) of the debug step; radius[K] within 4 ulp of the longdouble
                              update formed from the device's rho.
  full default solves         the same recurrences at every iteration; accepted[k] what rho > min_relative_decrease and mcc > 0 give; cost[k] == cost[k-1]
                              after a rejection; the divisor of the radius back at 2 after a success; num_successful; FUNCTION_TOL exactly when
                              |cost - candidate| <= ftol cost at the last iteration; final_cost within B of the reference at the returned state (what pins
                              prior_quad at a converged dx).
  batch                       small, prior and rejected_once in one uvs_batch_upload / uvs_batch_solve / uvs_batch_download: states and reports bit-identical to
                              each window solved alone.
After a rejection the fused loop re-damps its landmark partials in place where uvs_debug_step form 1 re-linearizes (lm_accept_ref.Runner): on that form, at
iterations k >= 2, the checks that hang on the step itself hold to 1e-10 of the step instead of bit for bit (its steps differ by 1e-13 from form 1's).
Every ratio to its bound goes to the file UVS_STEP_LOG names; the worst per form are in DESIGN.md section 4.
"""
import numpy as np
import pytest

import factor_ref as fr
import lm_accept_cases as cases
import lm_accept_ref as ar
from lm_step_check import _Env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def accept_log():
    list(fr.pool().map(abs, range(64)))      # the reference's workers exist before anything touches the GPU
    yield
    ar.write_log()
    fr.shutdown()


def _nt_env(nt):
    return {"UVS_LARGE_CHUNKS_NT": str(nt), "UVS_LARGE_SOLVE_NT": str(nt), "UVS_KSOLVE_NT": str(nt)}


class Device(ar.Runner):
    """One form of the product: a fresh handle per option set (the options are read at uvs_create)."""

    def __init__(self, gpu_api, form, nt):
        self.api, self.form, self.nt, self.name = gpu_api, form, nt, f"{form}{nt}"
        self.steps_after_rejection_exact = form != "large_solve_fused"      # the fused loop re-damps in place after a rejection; form 1 of uvs_debug_step re-linearizes

    def _solver(self, opts):
        with _Env(_nt_env(self.nt)):
            return self.api.Solver(opts=opts, max_batch=4)

    def solve(self, w, opts):
        s = self._solver(opts)
        try:
            if self.form == "k_solve": return s.solve(w)
            if self.form == "large_solve": return s.large_solve(w)
            st, rep, _ = s.large_solve_fused(w)
            return st, rep
        finally:
            s.close()

    def steps(self, w, opts, radii):
        s = self._solver(opts)
        try:
            return s.debug_step(w, radii, form=0 if self.form == "k_solve" else 1)
        finally:
            s.close()


_built = {}


def _case(gpu_api, oracle, name):
    """(window, options, reference costs per state), once per case: the prior cases carry the product's own marginalization."""
    if name not in _built:
        o = cases.options(name)
        with _Env({"UVS_KSOLVE_NT": "512"}):
            s = gpu_api.Solver(opts=o, max_batch=2)
        try:
            w, o = cases.build(name, oracle, marginalize_fn=lambda win, flag: s.marginalize(win, flag))
        finally:
            s.close()
        cases.check_structure(name, w, o, oracle)
        _built[name] = (w, o, ar.Costs(name))
    return _built[name]


def _run(gpu_api, oracle, name, form, nt):
    w, o, costs = _case(gpu_api, oracle, name)
    dev = Device(gpu_api, form, nt)
    F = ar.check_one_iteration(name, w, o, cases.K[name], dev, costs, ar._log)
    F += ar.check_full_solve(name, w, o, dev, costs, ar._log)
    assert not F, (name, dev.name, len(F), F[:6])


@pytest.mark.parametrize("name", cases.NAMES)
def test_k_solve_acceptance_half(gpu_api, oracle, name):
    _run(gpu_api, oracle, name, "k_solve", 512)


@pytest.mark.parametrize("name", [n for n in cases.NAMES if n not in cases.FEW_FORMS])
def test_k_solve256_acceptance_half(gpu_api, oracle, name):
    _run(gpu_api, oracle, name, "k_solve", 256)


@pytest.mark.parametrize("name", [n for n in cases.NAMES if n not in cases.FEW_FORMS])
def test_large_solve_acceptance_half(gpu_api, oracle, name):
    _run(gpu_api, oracle, name, "large_solve", 512)


@pytest.mark.parametrize("name", cases.NAMES)
def test_large_solve_fused_acceptance_half(gpu_api, oracle, name):
    _run(gpu_api, oracle, name, "large_solve_fused", 512)


@pytest.mark.parametrize("form", ["large_solve", "large_solve_fused"])
@pytest.mark.parametrize("name", cases.SUBSET_256)
def test_large256_acceptance_half(gpu_api, oracle, name, form):
    _run(gpu_api, oracle, name, form, 256)


def _same(a, b):
    sa, ra = a; sb, rb = b
    ok = all(np.array_equal(getattr(sa, nm), getattr(sb, nm)) for nm in ("pose", "speedbias", "ex_pose", "relo_pose", "inv_depth", "line_orth")) and sa.td == sb.td
    return ok and bytes(ra) == bytes(rb)


def test_batch_is_bit_identical_to_each_window_alone(gpu_api, oracle):
    """small, prior and rejected_once in one upload / solve / download, under rejected_once's options (its restart radius 9e4: the batch then holds a window
    that rejects a step beside two that do not) against each window through uvs_solve_window on the same handle."""
    ws = [_case(gpu_api, oracle, nm)[0] for nm in ("small", "prior", "rejected_once")]
    o = _case(gpu_api, oracle, "rejected_once")[1]
    s = gpu_api.Solver(opts=o, max_batch=4)
    try:
        alone = [s.solve(w) for w in ws]
        s.upload(ws); s.solve_resident()
        states, reps = s.download()
    finally:
        s.close()
    assert alone[2][1].accepted[1] == 0 and alone[2][1].accepted[2] == 1
    for k, nm in enumerate(("small", "prior", "rejected_once")):
        assert _same(alone[k], (states[k], reps[k])), nm
