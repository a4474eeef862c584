"""Windows for the tests of the LM iteration's acceptance half (tests/test_lm_accept_ref.py, tests/test_gpu_lm_accept.py): name -> (window, options, K),
K the first accepted iteration of a solve of the window under the reference formulation, each with a structure check against the CPU oracle that the
case is what its name promises.  These are the smallest windows at which each path exists:

  small, prior (n = 75), prior_td (n = 76), prior_extrinsic, points_only, lines_only, skipped_imu, relo (relo_Pose in the spare rows),
  relo_extrinsic_td (second-level elimination)      the windows of tests/lm_step_cases.py; the first step at the default radius is accepted: K = 1.
  rejected_once      the stressed window of tests/gpu_soak_rejections.py (generator seed 77) with index 14 (no prior), restarted from the oracle's state
                     after 2 iterations at the oracle's radius[2] = 9e4: reject (rho = -0.247), accept at 4.5e4 (rho = 0.168).  K = 2.
  rejected_thrice    index 7 (with a prior), restarted after 3 iterations at 2.7e5: three rejections (rho = -0.498, -0.360, -0.137), accepted at 4 218.75
                     (rho = 0.263): the divisors 2, 4, 8 of consecutive rejections.  K = 4.
  converged          `prior` restarted from the oracle's own 10-iteration solution at the default radius: the step is small, cost - candidate is
                     cancellation, and the prior's dx is as large as it gets (3e-2).  K = 1.
Radius 1e16 (invalid steps, accepted = -1) is left out on purpose: whether the device's Cholesky flag agrees there is a cond > 1e13 matter that
lm_step_check already excuses.
"""
import numpy as np

from helpers import abi, synth
import lm_step_cases as step_cases
import lm_accept_ref as ar

FROM_STEP_CASES = ["small", "prior", "prior_td", "prior_extrinsic", "points_only", "lines_only", "skipped_imu", "relo", "relo_extrinsic_td"]
NAMES = FROM_STEP_CASES + ["rejected_once", "rejected_thrice", "converged"]
FEW_FORMS = ("rejected_thrice", "converged")                              # run on k_solve 512 and large_solve_fused 512 only
SUBSET_256 = ["small", "prior_td", "relo_extrinsic_td", "rejected_once"]      # the 256-thread instantiations of the landmark-sharded forms
# (index of the stressed window, iterations before the restart, radius of the restart, rho of the restarted solve's first iterations)
REJECTED = {"rejected_once": (14, 2, 9e4, [-0.247, 0.168]), "rejected_thrice": (7, 3, 2.7e5, [-0.498, -0.360, -0.137, 0.263])}
K = {nm: 1 for nm in NAMES}
K.update(rejected_once=2, rejected_thrice=4)
STRESS_SEED = 77


def options(name):
    return step_cases.options("prior" if name == "converged" else name) if name not in REJECTED else abi.default_options()


class _Marg:
    def __init__(self, fn): self.marginalize = fn


def stressed(index, marginalize_fn):
    """Window `index` of the sequence tests/gpu_soak_rejections.py draws (the generator is shared by the windows, so 0 .. index are all drawn)."""
    from gpu_soak_rejections import stressed_window
    rng = np.random.default_rng(STRESS_SEED)
    for i in range(index + 1):
        w, amp = stressed_window(i, _Marg(marginalize_fn), rng)
    return w


def build(name, oracle, marginalize_fn=None):
    """-> (window, options).  The prior comes from `marginalize_fn(window, flag)` (the product's on the GPU; default: the oracle's); the states a case is
    restarted from are the ORACLE's, so that a case is the same window wherever it is built from the same prior."""
    mf = marginalize_fn or step_cases.oracle_marginalize(oracle, name)
    if name in REJECTED:
        index, nit, radius, _ = REJECTED[name]
        w = stressed(index, mf); o = abi.default_options()
        st, rep = oracle.solve(w, ar.options_like(o, max_num_iterations=nit))
        assert rep.num_iterations == nit and rep.radius[nit] == radius, (name, rep.num_iterations, rep.radius[nit])
        return ar.restart(w, o, st, radius)
    if name == "converged":
        w, o = step_cases.build("prior", marginalize_fn=mf)
        st, rep = oracle.solve(w, o)
        assert rep.num_iterations == 10, rep.num_iterations
        return ar.restart(w, o, st, o.initial_trust_region_radius)
    return step_cases.build(name, marginalize_fn=mf)


def check_structure(name, w, o, oracle):
    """The case is what its name promises, under the oracle: the window's structure, the accept / reject pattern of its first K + 1 iterations, the rho the
    module docstring states, and the halving sequence of the radius."""
    k = K[name]
    st, rep = oracle.solve(w, ar.options_like(o, max_num_iterations=k + 1))
    acc = list(rep.accepted[1:k + 1])
    assert acc == [0] * (k - 1) + [1], (name, acc)
    if name in REJECTED:
        index, nit, radius, rho = REJECTED[name]
        assert (w.prior is not None and w.prior.n > 0) == bool(index % 2), name
        assert o.initial_trust_region_radius == radius
        got = [rep.relative_decrease[i] for i in range(1, k + 1)]
        assert np.allclose(got, rho, atol=2e-3, rtol=0), (name, got)
        assert [rep.radius[i] for i in range(1, k)] == ar.halving(radius, k - 1), name
        assert len(w.inv_depth) >= 100 and len(w.line_orth) >= 30 and len(w.relo_lm) == 0
    elif name == "converged":
        step_cases.check_structure("prior", w, o)
        assert rep.cost[0] < 1e-6 * 7e9, rep.cost[0]                      # (the start of `prior` costs 7e9)
        assert rep.step_norm[1] < 0.1 and abs(rep.cost[0] - rep.candidate_cost[1]) < 1e-3 * rep.cost[0], (rep.step_norm[1], rep.cost[0], rep.candidate_cost[1])
    else:
        step_cases.check_structure(name, w, o)
    return st, rep
