"""60-digit reference of the ACCEPTANCE half of a Levenberg-Marquardt iteration of the sliding-window solve: everything after the damped step.

TEST INFRASTRUCTURE ONLY; mpmath + numpy.  The half forms the candidate x (+) delta, evaluates its cost, forms relative_decrease, decides, updates
the radius, sums the cost again at the accepted point and reports gradient_max_norm.  What is restated here:

  plus(w, opts, delta)   x (+) delta at 60 digits over the layout of lm_step_ref.layout: poses (the frames, Ex_Pose when it is free, relo_Pose when the
                         window has relocalization blocks) p + dp, normalize(q (x) (dtheta / 2, 1)); speed / bias, td, inverse depths and the four line
                         parameters by addition.  -> (the mpf values, the window rounded to FP64 once).
  restart(w, state, r)   a copy of `w` whose state is `state`, and the options to solve it with: initial_trust_region_radius = r.
  cost(key, w, opts)     the cost of every residual block at the state of `w` (tests/factor_ref.py in its residual-only mode, the relocalization blocks
                         included), summed in mpf and rounded once; with the bound B of DESIGN.md section 4:
                             B = factor_ref.cost_bound(ref, C) + [relocalization blocks: sum |r| B_r + 1e-13 cost_relo] + C_q 2^-53 A
                         C = 10 as in tests/test_gpu_factors.py.  The last term is the FORMULATION model of the prior inside the solve: there the prior's cost is
                         the quadratic form c0 + g0 . dx + dx . (H0 dx) / 2 with H0 = J0^T J0, g0 = J0^T r0, c0 = r0 . r0 / 2 rounded once per solve, not
                         |r0 + J0 dx|^2 / 2; away from dx = 0 its three terms cancel.  A = 1/2 sum_k (|r0_k| + sum_j |J0_kj| |dx_j|)^2 bounds the absolute
                         terms of all three together, C_q = quad_constant(n) = 3 n + 16 counts the roundings on the longest path (derivation: DESIGN.md
                         section 4).  Neither the oracle nor the device enters a number.
  scalars                relative_decrease, the radius update min(rmax, r / max(1/3, 1 - (2 rho - 1)^3)), the halving sequence r/2, r/8, r/64, ...,
                         step_norm and gradient_max_norm = || x - Plus(x, -g) ||_inf in np.longdouble.

Measured on the canonical prior window (synth.make_window(11, with_prior=True): 750 point and 280 line / VP blocks, 10 IMU blocks, the n = 75 prior): the
residual-only reference without levels 1.5 s serially and 0.7 s on 8 workers, with its +-1 ulp levels (four draws per block, what cost() needs for B) 2.5 s on 8
workers; the full mode with its central differences 2.1 s serially for a TENTH of the blocks.

The checker (check_one_iteration, check_full_solve) holds one thing under test -- the oracle, a numpy restatement, a form of the device -- to every bound of
tests/test_gpu_lm_accept.py's docstring; tests/test_lm_accept_ref.py runs it on the CPU.
"""
import numpy as np
import mpmath as mp
from mpmath import mpf

from helpers import abi
import factor_ref as fr
import lm_step_ref

LD = np.longdouble
C = 10
EPS = 2.0 ** -53
NF = abi.NUM_FRAMES


def quad_constant(n):
    """Roundings on the longest path of one absolute term of c0 + sum_i dx_i (g0_i + y_i / 2), y = H0 dx, into the window's cost:
    n for the entry of H0 = J0^T J0, n for the dot product y_i = H0_i . dx, 1 for g0_i + y_i / 2 (the halving is exact), 1 for the product with dx_i, n for
    the sum over i if it were sequential, 14 for the cost sum of the workgroup however it is ordered (a tree over at most 2^10 shares, the partial sums of
    the split rows): 3 n + 16.  The terms of g0 . dx (n + n + 2 + 14) and of c0 (n + 1 + 14) pass fewer."""
    return 3 * n + 16


# ---------------------------------------------------------------- plus
def _mpv(a):
    return [mpf(float(x)) for x in np.asarray(a, np.float64).ravel()]


def _pose_plus(x, d):
    x = _mpv(x)
    q = fr._qmul(x[3:7], [d[3] / 2, d[4] / 2, d[5] / 2, mpf(1)])
    n = mp.sqrt(sum(c * c for c in q))
    return [x[0] + d[0], x[1] + d[1], x[2] + d[2]] + [c / n for c in q]


def plus(w, opts, delta):
    """x (+) delta at 60 digits.  -> (dict of mpf lists: pose [11][7], speedbias [11][9], ex_pose [7], td, relo_pose [7], inv_depth, line_orth [n][4];
    a copy of `w` at the FP64 rounding of those).  Blocks that are not free are returned as they are."""
    mp.mp.dps = fr.DPS
    L = lm_step_ref.layout(w, opts)
    d = [mpf(float(v)) for v in np.asarray(delta, np.float64).ravel()]
    assert len(d) == L["n"], (len(d), L["n"])
    X = dict(pose=[_pose_plus(w.pose[f], d[15 * f:15 * f + 6]) for f in range(NF)],
             speedbias=[[a + b for a, b in zip(_mpv(w.speedbias[f]), d[15 * f + 6:15 * f + 15])] for f in range(NF)],
             ex_pose=_pose_plus(w.ex_pose, d[L["ex"]:L["ex"] + 6]) if L["ex"] is not None else _mpv(w.ex_pose),
             td=mpf(float(w.td)) + d[L["td"]] if L["td"] is not None else mpf(float(w.td)),
             relo_pose=_pose_plus(w.relo_pose, d[L["relo"]:L["relo"] + 6]) if L["relo"] is not None else _mpv(w.relo_pose),
             inv_depth=[a + b for a, b in zip(_mpv(w.inv_depth), d[L["pt"]:L["ln"]])],
             line_orth=[[a + b for a, b in zip(_mpv(w.line_orth[k]), d[L["ln"] + 4 * k:L["ln"] + 4 * k + 4])] for k in range(len(w.line_orth))])
    f64 = lambda v: np.array([float(c) for c in v])
    o = w.copy()
    o.pose = np.array([f64(p) for p in X["pose"]]); o.speedbias = np.array([f64(p) for p in X["speedbias"]])
    o.ex_pose = f64(X["ex_pose"]) if L["ex"] is not None else w.ex_pose.copy()
    o.td = float(X["td"])
    o.relo_pose = f64(X["relo_pose"]) if L["relo"] is not None else w.relo_pose.copy()
    o.inv_depth = f64(X["inv_depth"]).reshape(len(w.inv_depth)); o.line_orth = np.array([f64(p) for p in X["line_orth"]]).reshape(len(w.line_orth), 4)
    return X, o


def with_state(w, st):
    """A copy of `w` at the state `st` (abi.State), relo_Pose included when the window has relocalization blocks."""
    o = w.with_state(st)
    if len(w.relo_lm): o.relo_pose = np.array(st.relo_pose, np.float64).copy()
    return o


def options_like(opts, **kw):
    o = abi.Options(); copy_fields = [f[0] for f in abi.Options._fields_]
    for nm in copy_fields: setattr(o, nm, getattr(opts, nm))
    for k, v in kw.items(): setattr(o, k, v)
    return o


def restart(w, opts, state, radius):
    """-> (a copy of `w` whose state is `state`, the options of `opts` with initial_trust_region_radius = radius)."""
    return with_state(w, state), options_like(opts, initial_trust_region_radius=float(radius))


# ---------------------------------------------------------------- the cost and its bound
class Cost:
    """cost (the 60-digit sum rounded once), cost_mp, B and its parts: blocks (factor_ref.cost_bound), relo, quad; A and n of the prior; dx_max."""


def cost(key, w, opts, level_stride=1, draws=4):
    mp.mp.dps = fr.DPS
    R = fr.evaluate_cached(key, w, opts, jacobians=False, relo=True, level_stride=level_stride, draws=draws)[True]
    out = Cost()
    out.ref = R
    out.cost_mp = R.cost_mp; out.cost = float(R.cost_mp)
    out.blocks = fr.cost_bound(R, C)
    out.relo = 0.0
    if len(w.relo_lm):
        rr = R.relo_r; lv = fr._fill(R.level["relo_r"], R.have["relo"])
        Br = np.maximum(C * lv.max(axis=1), fr.FLOOR * np.abs(rr).max(axis=1))
        out.relo = float((np.abs(rr).sum(axis=1) * Br).sum()) + fr.FLOOR * float(R.cost_terms["relo"].sum())
    out.n = w.prior.n if (w.prior is not None and w.prior.n > 0) else 0
    out.A = R.aux["prior"][0]["quad_A"] if out.n else 0.0
    out.dx_max = float(np.abs(R.aux["prior"][0]["dx"]).max()) if out.n else 0.0
    out.quad = quad_constant(out.n) * EPS * out.A if out.n else 0.0
    out.B = out.blocks + out.relo + out.quad
    return out


# ---------------------------------------------------------------- scalars, np.longdouble
def relative_decrease(cost0, cand, mcc):
    return (LD(cost0) - LD(cand)) / LD(mcc)


def radius_update(radius, rho, rmax):
    t = LD(2) * LD(rho) - LD(1)
    return min(LD(rmax), LD(radius) / max(LD(1) / LD(3), LD(1) - t * t * t))


def halving(r0, n):
    """The radii after 1 .. n consecutive rejections from r0: r0/2, r0/8, r0/64, r0/1024 (divisors 2, 4, 8, 16: powers of two, every one exact)."""
    out, r, d = [], LD(r0), LD(2)
    for _ in range(n):
        r = r / d; d = d * LD(2); out.append(float(r))
    return out


def step_norm(w, opts, delta):
    """|| x (+) delta - x || over the ambient parameters, from the 60-digit plus."""
    X, _ = plus(w, opts, delta)
    t = mpf(0)
    for nm in ("pose", "speedbias"):
        for a, b in zip(X[nm], getattr(w, nm)): t += sum((u - mpf(float(v))) ** 2 for u, v in zip(a, b))
    for nm in ("ex_pose", "relo_pose"): t += sum((u - mpf(float(v))) ** 2 for u, v in zip(X[nm], getattr(w, nm)))
    t += (X["td"] - mpf(float(w.td))) ** 2
    t += sum((u - mpf(float(v))) ** 2 for u, v in zip(X["inv_depth"], w.inv_depth))
    for a, b in zip(X["line_orth"], w.line_orth): t += sum((u - mpf(float(v))) ** 2 for u, v in zip(a, b))
    return float(mp.sqrt(t))


def gradient_max_norm(w, opts, g):
    """|| x - Plus(x, -g) ||_inf: Euclidean blocks |g|, pose blocks through the 60-digit plus.  g over the layout of lm_step_ref.layout (any float type)."""
    g = np.asarray(g, LD)
    X, _ = plus(w, opts, np.asarray(-g, np.float64))      # (the quaternion part alone needs plus; it is taken at the FP64 rounding of g, whose 1e-16 is far below the bounds that use this)
    L = lm_step_ref.layout(w, opts)
    eu = np.ones(len(g), bool)
    worst = 0.0
    blocks = [(15 * f, w.pose[f], X["pose"][f]) for f in range(NF)]
    if L["ex"] is not None: blocks.append((L["ex"], w.ex_pose, X["ex_pose"]))
    if L["relo"] is not None: blocks.append((L["relo"], w.relo_pose, X["relo_pose"]))
    for off, x, xp in blocks:
        eu[off + 3:off + 6] = False
        worst = max(worst, max(abs(float(xp[k] - mpf(float(x[k])))) for k in range(3, 7)))
    return max(worst, float(np.abs(g[eu]).max()))


# ---------------------------------------------------------------- the checker: one thing under test (the oracle, a restatement, a device form) against all of the above
class Runner:
    """What the checker needs of the thing under test.  solve(w, opts) -> (abi.State, abi.Report).  steps(w, opts, radii) -> (delta [n, layout], scal [n, >= 5]:
    the thing's own full tangent step per radius and cost, gmax, ok, model_cost_change, step_norm^2), or None when it cannot show its steps; then
    candidate(w, opts, radius) -> the FP64 candidate state of the first iteration at `radius`, as a window.
    steps_after_rejection_exact: whether steps() shows, bit for bit, the steps the solve takes AFTER a rejection.  uvs_debug_step does for k_solve (form 0 re-damps
    the stored linearization as the product kernel does) and for uvs_large_solve (form 1 re-linearizes at the same state as uvs_large_decide makes the host loop do);
    the fused loop re-damps its landmark partials in place (redamp_chunk) and has no storing instantiation of that path, so its steps after a rejection differ from
    form 1's in the last digits (measured 1e-13 of the step).  Where they are not exact, the checks that hang on the step itself (returned state = x0 + delta,
    quaternions against plus(x0, delta), step_norm) hold to STEP_TOL of the step at iterations k >= 2 instead of bit for bit; iteration 1 is exact in every form."""
    name = "?"
    steps_after_rejection_exact = True

    def solve(self, w, opts): raise NotImplementedError

    def steps(self, w, opts, radii): return None

    def candidate(self, w, opts, radius): raise NotImplementedError


class SolveRunner(Runner):
    """A runner that has a solve and nothing else (the oracle): the candidate of a rejected iteration is what a one-iteration solve returns that accepts any
    step with a positive model_cost_change (min_relative_decrease = -1e300)."""

    def __init__(self, name, solve): self.name, self._solve = name, solve

    def solve(self, w, opts): return self._solve(w, opts)

    def candidate(self, w, opts, radius):
        st, rep = self._solve(w, options_like(opts, initial_trust_region_radius=float(radius), max_num_iterations=1, min_relative_decrease=-1e300))
        assert rep.num_iterations == 1 and rep.accepted[1] == 1, (rep.num_iterations, rep.accepted[1], rep.termination)
        return with_state(w, st)


class Failures(list):
    def need(self, ok, *what):
        if not ok: self.append(what)
        return ok


def _ulps(a, b):
    return abs(float(a) - float(b)) / np.spacing(abs(float(b))) if np.isfinite(a) and np.isfinite(b) else np.inf


def _state_key(w):
    import hashlib
    h = hashlib.sha1()
    for a in (w.pose, w.speedbias, w.ex_pose, [w.td], w.relo_pose, w.inv_depth, w.line_orth): h.update(np.ascontiguousarray(a, np.float64).tobytes())
    return h.hexdigest()[:12]


class Costs:
    """cost() per state of one case, computed once per distinct FP64 state."""

    def __init__(self, name, level_stride=1): self.name, self.stride, self.memo = name, level_stride, {}

    def __call__(self, w, opts):
        k = _state_key(w)
        if k not in self.memo: self.memo[k] = cost(f"accept-{self.name}", w, opts, level_stride=self.stride)
        return self.memo[k]


STEP_TOL = 1e-10        # lm_step_check's tolerance between two FP64 formations of one step's scalars
MARGIN = 100            # every decision of the reference lies MARGIN x (B_cost + B_cand) / |mcc| away from min_relative_decrease
SHARP = 1e-11           # the bound at a case's own state is at most SHARP of the cost it bounds ...
SHARP_ANY = 1e-10       # ... and at every other state a test evaluates the reference at (the candidates, the returned states) at most SHARP_ANY: see check_cost


def _decision(F, log, tag, k, rho_ref, cb, rep, opts, accepted):
    """The condition on a case (reference-only figures) and the thing's decision at iteration k."""
    slack = cb / abs(rep.model_cost_change[k])
    margin = abs(rho_ref - opts.min_relative_decrease)
    F.need(margin > MARGIN * slack, tag, k, "the case's decision is too close to min_relative_decrease", rho_ref, slack)
    F.need(int(accepted) == int(rho_ref > opts.min_relative_decrease), tag, k, "decision", int(accepted), rho_ref)
    log.append(f"{tag:44s} k={k} decision margin / (B_cost + B_cand)/|mcc| = {margin / slack:.3g} (must exceed {MARGIN})")


def check_recurrences(F, log, tag, rep, opts, r0):
    """What holds at every iteration of any solve on the report's own numbers: relative_decrease formed in FP64 from cost, candidate_cost and
    model_cost_change, bit for bit; the decision; the radius after it (accepted: within 4 ulp of the longdouble update; rejected: the division by 2, 4, 8, ...
    exactly, the divisor back at 2 after a success); cost unchanged after a rejection; num_successful; the termination by function tolerance."""
    n = int(rep.num_iterations); decr = 2.0; radius = float(r0); nsucc = 0
    stopped = rep.termination in (abi.TERM_NAMES.index("PARAMETER_TOL"), abi.TERM_NAMES.index("FUNCTION_TOL"))
    worst_r = 0.0
    for k in range(1, n + 1):
        c0, cand, mcc, rd = rep.cost[k - 1], rep.candidate_cost[k], rep.model_cost_change[k], rep.relative_decrease[k]
        if rep.accepted[k] == -1: F.need(False, tag, k, "an invalid step: out of scope, the case must not take one"); break
        F.need(rd == (c0 - cand) / mcc, tag, k, "relative_decrease is not (cost - candidate) / model_cost_change of the report", rd, (c0 - cand) / mcc)
        last = k == n and stopped and not opts.function_tol_keeps_candidate
        good = rd > opts.min_relative_decrease and mcc > 0
        if not last: F.need(int(rep.accepted[k]) == int(good), tag, k, "accepted", int(rep.accepted[k]), rd)
        if rep.accepted[k] == 1:
            nsucc += 1
            want = float(radius_update(radius, rd, opts.max_trust_region_radius))
            u = _ulps(rep.radius[k], want); worst_r = max(worst_r, u)
            F.need(u <= 4, tag, k, "radius after an accepted step", rep.radius[k], want, u)
            radius = rep.radius[k]; decr = 2.0
        else:
            F.need(rep.cost[k] == c0, tag, k, "cost changed by a rejected step", rep.cost[k], c0)
            if not last:
                F.need(rep.radius[k] == radius / decr, tag, k, "radius after a rejected step", rep.radius[k], radius / decr, decr)
                radius = rep.radius[k]; decr *= 2.0
    F.need(rep.num_successful == nsucc, tag, "num_successful", rep.num_successful, nsucc)
    if n >= 1:
        ftol = abs(rep.cost[n - 1] - rep.candidate_cost[n]) <= opts.function_tolerance * rep.cost[n - 1]
        is_f, is_p = rep.termination == abi.TERM_NAMES.index("FUNCTION_TOL"), rep.termination == abi.TERM_NAMES.index("PARAMETER_TOL")
        F.need(is_f == (ftol and not is_p), tag, "FUNCTION_TOL exactly when |cost - candidate| <= ftol cost at the last iteration", int(rep.termination), ftol)
    log.append(f"{tag:44s} recurrences over {n} iterations ({nsucc} accepted): worst radius update {worst_r:.2f} ulp of the longdouble value (bound 4)")


def check_cost(F, log, tag, what, got, c, sharp=SHARP_ANY):
    """|got - reference| <= B, and the bound itself sharp enough to supersede the 1e-9 / 1e-10 trace parities: B <= 1e-11 cost at the state that defines the
    case.  At the state after ONE step from a synthetic start the same B is 1.5e-11 .. 7.3e-11 of the cost on every window (cost 3e2 .. 2e3 there, of which the
    IMU rows' share of B, C x their +-1 ulp level x |r|, is 1e-8 whatever the window), and 2.5e-11 at the end of prior_td (the quadratic form's A at |dx| = 1.7):
    no seed changes either, so those states are held to 1e-10, still under the parities, and their figures are logged."""
    ratio = abs(got - c.cost) / c.B
    F.need(c.B <= sharp * c.cost, tag, what, "the bound is not sharp", c.B, c.cost, sharp)
    F.need(ratio <= 1.0, tag, what, "cost outside the bound", got, c.cost, abs(got - c.cost), c.B)
    log.append(f"{tag:44s} {what:24s} {got:.17g} reference {c.cost:.17g} |diff| {abs(got - c.cost):.2e} B {c.B:.2e} (blocks {c.blocks:.1e} relo {c.relo:.1e} quad {c.quad:.1e}; B/cost {c.B / c.cost:.1e}) ratio {ratio:.3f}"
               + (f"  prior: |dx| {c.dx_max:.1e}, |diff| = {abs(got - c.cost) / (EPS * c.A):.1f} x 2^-53 A (C_q = {quad_constant(c.n)}; all of |diff| laid at the quadratic form's door)" if c.n else ""))


def _delta_of(nm, d, L):
    fr_ = d[:15 * NF].reshape(NF, 15)
    return {"positions": fr_[:, :3], "speed / bias": fr_[:, 6:], "inverse depths": d[L["pt"]:L["ln"]], "line parameters": d[L["ln"]:]}[nm]


def check_state(F, log, tag, w, opts, st, delta, exact=True):
    """The returned state of the run that stops after the accepted iteration: blocks that are not free bit-identical to the input; every quaternion's norm
    within 4 x 2^-53 of 1; and, when the step `delta` is known, Euclidean parts = x0 + delta bit for bit (one FP64 addition each) and every quaternion within
    8 x 2^-53 (1 + |dtheta| / 2) per component of the 60-digit plus.  exact=False (Runner.steps_after_rejection_exact): those two to STEP_TOL of the step."""
    L = lm_step_ref.layout(w, opts)
    if L["ex"] is None: F.need(np.array_equal(st.ex_pose, w.ex_pose), tag, "the fixed extrinsic moved")
    if L["td"] is None: F.need(float(st.td) == float(w.td), tag, "the fixed td moved", st.td, w.td)
    quats = [(f"pose[{f}]", st.pose[f], 15 * f, w.pose[f]) for f in range(NF)]
    if L["ex"] is not None: quats.append(("ex_pose", st.ex_pose, L["ex"], w.ex_pose))
    if L["relo"] is not None: quats.append(("relo_pose", st.relo_pose, L["relo"], w.relo_pose))
    worst_n = max(abs(float(np.sqrt(np.sum(np.asarray(q[3:7], LD) ** 2)) - 1)) for _, q, _, _ in quats)
    F.need(worst_n <= 4 * EPS, tag, "a quaternion is not unit", worst_n / EPS)
    msg = f"{tag:44s} state: worst | |q| - 1 | {worst_n / EPS:.2f} x 2^-53 (bound 4)"
    if delta is not None:
        X, ref = plus(w, opts, delta)
        d = np.asarray(delta, np.float64)
        for nm, got, want in (("positions", st.pose[:, :3], w.pose[:, :3] + d[:15 * NF].reshape(NF, 15)[:, :3]), ("speed / bias", st.speedbias, w.speedbias + d[:15 * NF].reshape(NF, 15)[:, 6:]),
                              ("inverse depths", st.inv_depth, w.inv_depth + d[L["pt"]:L["ln"]]), ("line parameters", st.line_orth.reshape(-1), w.line_orth.reshape(-1) + d[L["ln"]:])):
            err = float(np.abs(np.asarray(got) - want).max()) if np.size(want) else 0.0
            F.need(np.array_equal(got, want) if exact else err <= STEP_TOL * float(np.abs(_delta_of(nm, d, L)).max()), tag, nm + " are not x0 + delta", err)
        same = (lambda a, b, dd: np.array_equal(a, b)) if exact else (lambda a, b, dd: float(np.abs(np.asarray(a) - b).max()) <= STEP_TOL * float(np.abs(dd).max()))
        if L["td"] is not None: F.need(same(float(st.td), float(w.td) + d[L["td"]], d[L["td"]]), tag, "td is not x0 + delta")
        if L["ex"] is not None: F.need(same(st.ex_pose[:3], w.ex_pose[:3] + d[L["ex"]:L["ex"] + 3], d[L["ex"]:L["ex"] + 3]), tag, "extrinsic position is not x0 + delta")
        if L["relo"] is not None: F.need(same(st.relo_pose[:3], w.relo_pose[:3] + d[L["relo"]:L["relo"] + 3], d[L["relo"]:L["relo"] + 3]), tag, "relo position is not x0 + delta")
        worst_q = 0.0
        for (nm, q, off, q0), xq in zip(quats, X["pose"] + ([X["ex_pose"]] if L["ex"] is not None else []) + ([X["relo_pose"]] if L["relo"] is not None else [])):
            dth = float(np.sqrt(np.sum(d[off + 3:off + 6] ** 2)))
            bound = 8 * EPS * (1 + dth / 2) + (0.0 if exact else STEP_TOL * dth / 2)
            e = max(abs(float(mpf(float(q[3 + i])) - xq[3 + i])) for i in range(4))
            worst_q = max(worst_q, e / bound)
            F.need(e <= bound, tag, nm + " quaternion against the 60-digit plus", e, bound)
        msg += f", worst quaternion error / bound {worst_q:.3f}"
    log.append(msg)


def check_one_iteration(name, w, opts, K, runner, costs, log):
    """The runner's acceptance half on case `name`, whose first accepted iteration is K: the product solved with max_num_iterations = K and K + 1, every
    bound of tests/test_gpu_lm_accept.py's docstring.  -> Failures (empty: all met)."""
    F = Failures(); tag = f"{name}/{runner.name}"
    r0 = float(opts.initial_trust_region_radius)
    radii = [r0] + halving(r0, K - 1)
    sk = runner.steps(w, opts, radii)
    delta, scal = sk if sk is not None else (None, None)
    stK, repK = runner.solve(w, options_like(opts, max_num_iterations=K))
    stK1, repK1 = runner.solve(w, options_like(opts, max_num_iterations=K + 1))
    c0 = costs(w, opts)
    check_cost(F, log, tag, "initial_cost", repK.initial_cost, c0, SHARP)
    if not F.need(repK.num_iterations == K and repK1.num_iterations >= K, tag, "iterations", repK.num_iterations, repK1.num_iterations): return F
    cands = {}
    # ---- rejected iterations k < K
    for k in range(1, K):
        F.need(repK.accepted[k] == 0, tag, k, "accepted", repK.accepted[k])
        F.need(repK.cost[k] == repK.initial_cost, tag, k, "cost after a rejection is not the initial cost", repK.cost[k], repK.initial_cost)
        F.need(repK.radius[k] == radii[k], tag, k, "radius is not the halving sequence", repK.radius[k], radii[k])
        cw = plus(w, opts, delta[k - 1])[1] if delta is not None else runner.candidate(w, opts, radii[k - 1])
        cands[k] = costs(cw, opts)
        check_cost(F, log, tag, f"candidate_cost[{k}] (rejected)", repK.candidate_cost[k], cands[k])
    # ---- iteration K
    F.need(repK.accepted[K] == 1, tag, K, "accepted", repK.accepted[K])
    exact = K == 1 or runner.steps_after_rejection_exact
    check_state(F, log, tag, w, opts, stK, delta[K - 1] if delta is not None else None, exact)
    wK = with_state(w, stK)
    cands[K] = cK = costs(wK, opts)      # the reference at the returned FP64 state: plus and the cost path are judged separately
    check_cost(F, log, tag, f"candidate_cost[{K}]", repK.candidate_cost[K], cK)
    check_cost(F, log, tag, "final_cost", repK.final_cost, cK)
    # the K + 1 run: the same K iterations (the reference at the K run's state serves it), then the linearization's own sum at the accepted point
    same = all(repK1.candidate_cost[k] == repK.candidate_cost[k] and repK1.model_cost_change[k] == repK.model_cost_change[k] and repK1.accepted[k] == repK.accepted[k] for k in range(1, K + 1))
    F.need(same, tag, "the first K iterations of the K + 1 run are not those of the K run")
    check_cost(F, log, tag, f"cost[{K}] of the K + 1 run", repK1.cost[K], cK)
    if repK1.num_iterations == K + 1 and repK1.accepted[K + 1] == 1:
        cands[K + 1] = costs(with_state(w, stK1), opts)
        check_cost(F, log, tag, f"candidate_cost[{K + 1}]", repK1.candidate_cost[K + 1], cands[K + 1])
    # ---- scalars, every iteration of both runs
    for run, rep in (("K", repK), ("K + 1", repK1)):
        check_recurrences(F, log, f"{tag} {run} run", rep, opts, r0)
        for k in range(1, int(rep.num_iterations) + 1):
            if k not in cands: continue
            prev = c0 if k <= K else cK
            rho_ref = float(relative_decrease(prev.cost, cands[k].cost, rep.model_cost_change[k]))
            cb = prev.B + cands[k].B
            bound = cb / abs(rep.model_cost_change[k]) + 1e-10 * abs(rho_ref)
            e = abs(rep.relative_decrease[k] - rho_ref)
            F.need(e <= bound, tag, run, k, "relative_decrease against the reference", rep.relative_decrease[k], rho_ref, e, bound)
            log.append(f"{tag:44s} {run} run k={k} relative_decrease {rep.relative_decrease[k]:.12g} reference {rho_ref:.12g} |diff| {e:.2e} bound {bound:.2e} ratio {e / bound:.3f}")
            if run == "K": _decision(F, log, tag, k, rho_ref, cb, rep, opts, rep.accepted[k])
            elif k == K + 1: _decision(F, log, tag, k, rho_ref, cb, rep, opts, rep.accepted[k])
        if scal is not None:
            for k in range(1, K + 1):
                m, s2 = scal[k - 1, 3], scal[k - 1, 4]
                F.need(abs(rep.model_cost_change[k] - m) <= 1e-10 * abs(m), tag, run, k, "model_cost_change against the debug step's", rep.model_cost_change[k], m)
                u = _ulps(rep.step_norm[k], np.sqrt(s2))
                F.need(u <= 1 if (k == 1 or runner.steps_after_rejection_exact) else abs(rep.step_norm[k] - np.sqrt(s2)) <= STEP_TOL * np.sqrt(s2), tag, run, k, "step_norm against sqrt(step_norm^2) of the debug step", rep.step_norm[k], np.sqrt(s2), u)
                if run == "K": log.append(f"{tag:44s} k={k} model_cost_change {'bit-equal to' if rep.model_cost_change[k] == m else 'differs from'} the debug step's ({abs(rep.model_cost_change[k] - m) / abs(m):.1e}), step_norm {u:.1f} ulp")
    u = _ulps(repK.radius[K], float(radius_update(radii[K - 1], repK.relative_decrease[K], opts.max_trust_region_radius)))
    F.need(u <= 4, tag, "radius[K] against the longdouble update from the thing's own rho", u)
    return F


def check_full_solve(name, w, opts, runner, costs, log):
    """A full solve under the case's options: the recurrences at every iteration, and final_cost within B of the reference at the returned state."""
    F = Failures(); tag = f"{name}/{runner.name} full"
    st, rep = runner.solve(w, opts)
    check_recurrences(F, log, tag, rep, opts, opts.initial_trust_region_radius)
    check_cost(F, log, tag, "final_cost", rep.final_cost, costs(with_state(w, st), opts))
    return F


from lm_step_check import _log, write_log      # one log for the whole LM iteration: the damped step's figures and the acceptance half's -> the file UVS_STEP_LOG names
