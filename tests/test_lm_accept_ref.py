"""The reference of the LM iteration's acceptance half (tests/lm_accept_ref.py, the residual-only mode of tests/factor_ref.py) and its cases
(tests/lm_accept_cases.py), on the CPU:

  * plus against pyref_lm.plus to a few ulp, its quaternions unit to 1e-55; the residual-only mode against the full mode, exactly;
  * every case is what its name promises (structure check against the oracle), every decision of the reference lies 100 x (B_cost + B_cand) / |mcc| away
    from min_relative_decrease and every bound is at most 1e-11 of its cost (both asserted inside the checker, from reference figures alone);
  * the ORACLE is held to every bound tests/test_gpu_lm_accept.py holds the device to, through the same checker (lm_accept_ref.check_one_iteration,
    check_full_solve), so a bound that the formulation in careful FP64 cannot meet is found here and not on the GPU;
  * teeth: a plain numpy FP64 restatement of the half (pyref_lm's plus generalised to the layout, the oracle's evaluation for the blocks' cost, the
    quadratic prior) passes on all cases, and each of six planted defects makes the checker fail on at least one.
"""

import numpy as np
import pytest

from helpers import abi
import factor_ref as fr
import lm_accept_cases as cases
import lm_accept_ref as ar
import lm_step_ref
import pyref_lm

LD = np.longdouble


@pytest.fixture(scope="module", autouse=True)
def pool():
    list(fr.pool().map(abs, range(64)))
    yield
    ar.write_log()
    fr.shutdown()


_built = {}


def _case(oracle, name):
    if name not in _built:
        w, o = cases.build(name, oracle)
        _built[name] = (w, o, ar.Costs(name))
    return _built[name]


# ---------------------------------------------------------------- the reference itself
def test_plus_matches_the_fp64_plus_and_its_quaternions_are_unit():
    import mpmath as mp
    w, o = cases.step_cases.build("small")
    rng = np.random.default_rng(3)
    L = lm_step_ref.layout(w, o)
    for scale in (1e-6, 1e-2, 0.5):
        d = scale * rng.standard_normal(L["n"])
        X, x = ar.plus(w, o, d)
        ref = pyref_lm.plus(w, d)
        for f in range(abi.NUM_FRAMES):
            assert abs(mp.sqrt(sum(c * c for c in X["pose"][f][3:])) - 1) < mp.mpf("1e-55")
        assert np.array_equal(x.pose[:, :3], ref.pose[:, :3]) and np.array_equal(x.speedbias, ref.speedbias)
        assert np.array_equal(x.inv_depth, ref.inv_depth) and np.array_equal(x.line_orth, ref.line_orth)
        assert np.abs(x.pose[:, 3:] - ref.pose[:, 3:]).max() <= 4 * 2.0 ** -53
        assert np.array_equal(x.ex_pose, w.ex_pose) and x.td == w.td and np.array_equal(x.relo_pose, w.relo_pose)
    # a free extrinsic, a free td and relo_Pose: their slots of the layout
    w, o = cases.step_cases.build("relo_extrinsic_td")
    L = lm_step_ref.layout(w, o)
    d = 1e-3 * rng.standard_normal(L["n"])
    X, x = ar.plus(w, o, d)
    for nm, off, x0 in (("ex_pose", L["ex"], w.ex_pose), ("relo_pose", L["relo"], w.relo_pose)):
        want = pyref_lm.pose_plus(x0, d[off:off + 6])
        assert np.abs(getattr(x, nm) - want).max() <= 4 * 2.0 ** -53 and np.array_equal(getattr(x, nm)[:3], want[:3])
        assert abs(mp.sqrt(sum(c * c for c in X[nm][3:])) - 1) < mp.mpf("1e-55")
    assert x.td == w.td + d[L["td"]]
    assert ar.halving(1e4, 4) == [5e3, 1.25e3, 156.25, 9.765625]


def test_residual_only_mode_is_the_full_mode_without_its_jacobians(oracle):
    w, o = cases.step_cases.build("relo_extrinsic_td")
    w2, o2, _ = _case(oracle, "prior")
    for win, op, sub in ((w, o, dict(pt=list(range(0, 40, 3)), ln=list(range(0, 30, 4)), imu=[0, 5], prior=False)), (w2, o2, dict(pt=[1, 2], ln=[3], imu=[], prior=True))):
        full = fr.evaluate(win, op, subset=sub, draws=2)
        ronly = fr.evaluate(win, op, subset=sub, draws=2, jacobians=False)
        for robust in (False, True):
            a, b = full[robust], ronly[robust]
            for nm in ("pt_r", "ln_r", "vp_r", "imu_r", "prior_r"):
                assert np.array_equal(getattr(a, nm), getattr(b, nm)), nm
                assert np.array_equal(a.level[nm], b.level[nm], equal_nan=True), nm
                assert np.array_equal(a.model[nm], b.model[nm]), nm
            assert a.cost == b.cost
            for fam in ("pt", "ln", "vp", "imu"): assert np.array_equal(a.cost_terms[fam], b.cost_terms[fam])
            assert a.cost_terms["prior"] == b.cost_terms["prior"]
            assert abs(float(b.cost_mp) - b.cost) <= 1e-15 * b.cost and not np.any(b.pt_J) and not np.any(b.imu_J)


def test_relocalization_blocks_of_the_reference_match_the_longdouble_restatement():
    w, o = cases.step_cases.build("relo")
    R = fr.evaluate(w, o, subset=dict(pt=[], ln=[], imu=[], prior=False, relo=list(range(len(w.relo_lm)))), draws=0, jacobians=False, relo=True)[True]
    rows = lm_step_ref.relo_rows(w, o)
    assert len(rows) == len(w.relo_lm) >= 3
    for k, (_, _, r) in enumerate(rows):
        assert np.abs(R.relo_r[k] - np.asarray(r, np.float64)).max() <= 1e-12 * max(1.0, np.abs(R.relo_r[k]).max()), k
    assert float(R.cost_mp) > 0 and R.cost == 0.0


def test_gradient_max_norm_matches_the_oracle(oracle):
    for name in ("small", "relo_extrinsic_td"):
        w, o = cases.step_cases.build(name)
        _, g = lm_step_ref.normal_equations(w, oracle.evaluate(w, True, o), o)
        got = ar.gradient_max_norm(w, o, g)
        want = oracle.solve(w, ar.options_like(o, max_num_iterations=1))[1].gradient_max_norm[0]
        assert abs(got - want) <= 1e-12 * want, (name, got, want)
    # a pose block alone: a rotation gradient of any size moves the quaternion by at most 2
    w, o = cases.step_cases.build("small")
    g = np.zeros(lm_step_ref.layout(w, o)["n"]); g[3:6] = [3e9, -1e9, 2e9]; g[21] = 1.5
    assert ar.gradient_max_norm(w, o, g) == 1.5


# ---------------------------------------------------------------- the cases and the oracle
@pytest.mark.parametrize("name", cases.NAMES)
def test_case_structure_and_the_oracle_within_every_bound(oracle, name):
    w, o, costs = _case(oracle, name)
    cases.check_structure(name, w, o, oracle)
    run = ar.SolveRunner("oracle", oracle.solve)
    F = ar.check_one_iteration(name, w, o, cases.K[name], run, costs, ar._log)
    F += ar.check_full_solve(name, w, o, run, costs, ar._log)
    assert not F, (name, len(F), F[:6])


# ---------------------------------------------------------------- teeth
class Restated(ar.Runner):
    """The acceptance half in plain numpy FP64, after a step that comes from lm_step_ref (longdouble, rounded): plus, the cost (the oracle's evaluation of the
    blocks, the relocalization blocks from lm_step_ref.projection_block, the prior in its quadratic form), rho, the decision, the radius."""

    def __init__(self, oracle, defect=None):
        self.oracle, self.defect, self.name = oracle, defect, "restated" + ("" if defect is None else "/" + defect)

    def _prior_setup(self, w):
        p = w.prior; J0, r0 = p.J0(), p.r0()
        return J0.T @ J0, J0.T @ r0, 0.5 * (r0 @ r0)

    def _prior_dx(self, w, x):
        p = w.prior; dx = np.zeros(p.n); x0 = np.array(p.x0[:])
        for b in range(p.n_blocks):
            kind, fr_, size, idx, off = p.block_kind[b], p.block_frame[b], p.block_size[b], p.block_idx[b], p.x0_off[b]
            v = np.asarray(x.pose[fr_] if kind == 0 else x.speedbias[fr_] if kind == 1 else x.ex_pose if kind == 2 else [x.td], np.float64)
            if size != 7: dx[idx:idx + size] = v[:size] - x0[off:off + size]
            else:
                dx[idx:idx + 3] = v[:3] - x0[off:off + 3]
                q0 = x0[off + 3:off + 7]; qi = np.array([-q0[0], -q0[1], -q0[2], q0[3]]) / (q0 @ q0)
                e = pyref_lm.quat_mul(qi, v[3:7])
                dx[idx + 3:idx + 6] = (2.0 if e[3] >= 0 else -2.0) * e[:3]
        return dx

    def cost(self, w, opts, x, quad):
        ev = self.oracle.evaluate(x, True, opts)
        c = ev.cost
        if quad is not None:
            n = w.prior.n; H0, g0, c0 = quad
            c -= 0.5 * float(ev.prior_r[:n] @ ev.prior_r[:n])
            dx = self._prior_dx(w, x)
            y = (H0.astype(np.float32) @ dx.astype(np.float32)).astype(np.float64) if self.defect == "float32_y" else H0 @ dx
            c += c0 + dx @ (g0 + 0.5 * y)
        first = {}
        for k in range(len(w.pt_lm)): first.setdefault(int(w.pt_lm[k]), int(w.pt_fi[k]))
        for k in range(len(w.relo_lm)):
            lm = int(w.relo_lm[k])
            r, _ = lm_step_ref.projection_block(x.pose[first[lm]], x.relo_pose, x.ex_pose, x.inv_depth[lm], w.relo_pi[k], w.relo_pj[k], opts.point_sqrt_info, 0.0)
            s = float(np.sum(r * r)); b = opts.loss_point ** 2
            c += 0.5 * b * np.log1p(s / b)
        return float(c), ev

    def _plus(self, w, opts, d):
        L = lm_step_ref.layout(w, opts); x = w.copy()

        def pp(p, dd):
            q = pyref_lm.quat_mul(p[3:], np.array([0.5 * dd[3], 0.5 * dd[4], 0.5 * dd[5], 1.0]))
            return np.concatenate([p[:3] + dd[:3], q if self.defect == "unnormalised" else q / np.linalg.norm(q)])
        for f in range(abi.NUM_FRAMES):
            x.pose[f] = pp(w.pose[f], d[15 * f:15 * f + 6]); x.speedbias[f] = w.speedbias[f] + d[15 * f + 6:15 * f + 15]
        if L["ex"] is not None: x.ex_pose = pp(w.ex_pose, d[L["ex"]:L["ex"] + 6])
        if L["td"] is not None: x.td = float(w.td) + d[L["td"]]
        if L["relo"] is not None: x.relo_pose = pp(w.relo_pose, d[L["relo"]:L["relo"] + 6])
        x.inv_depth = w.inv_depth + d[L["pt"]:L["ln"]]; x.line_orth = w.line_orth + d[L["ln"]:].reshape(-1, 4)
        return x

    def _step(self, sysm, radius):
        d, y = lm_step_ref.damped_step(sysm, radius)
        mcc = float(y @ sysm.b - LD(0.5) * (y @ sysm.Hs @ y))
        return np.asarray(d, np.float64), mcc

    def steps(self, w, opts, radii):
        sysm = lm_step_ref.System(w, self.oracle.evaluate(w, True, opts), opts)
        out = np.zeros((len(radii), sysm.L["n"])); scal = np.zeros((len(radii), 40))
        for k, r in enumerate(radii):
            out[k], scal[k, 3] = self._step(sysm, r)
            xc = self._plus(w, opts, out[k])
            scal[k, 4] = self._step_norm(w, xc) ** 2
        return out, scal

    @staticmethod
    def _ambient(x):
        return np.concatenate([x.pose.ravel(), x.speedbias.ravel(), x.ex_pose, [x.td], x.relo_pose, x.inv_depth, x.line_orth.ravel()])

    def _step_norm(self, a, b):
        return float(np.sqrt(float(np.sum((np.asarray(self._ambient(b), LD) - np.asarray(self._ambient(a), LD)) ** 2))))

    def solve(self, w, opts):
        quad = self._prior_setup(w) if (w.prior is not None and w.prior.n > 0) else None
        rep = abi.Report(); x = w.copy()
        cost, ev = self.cost(w, opts, x, quad)
        sysm = lm_step_ref.System(x, ev, opts)
        radius, decr, it, nsucc = float(opts.initial_trust_region_radius), 2.0, 0, 0
        rep.initial_cost = cost; rep.cost[0] = cost; rep.radius[0] = radius; rep.accepted[0] = 1
        rejected_cand = None; rejected_cost = None; term = 0
        while it < opts.max_num_iterations:
            it += 1
            d, mcc = self._step(sysm, radius)
            xc = self._plus(x, opts, d)
            xe = xc      # the state the candidate's cost is evaluated at
            if self.defect == "stale_trig" and len(w.line_orth):
                xe = xc.copy(); xe.line_orth[len(w.line_orth) // 2, 1] = x.line_orth[len(w.line_orth) // 2, 1]
            if self.defect == "wrong_buffer" and rejected_cand is not None and len(w.inv_depth):
                xc = xc.copy(); xc.inv_depth[len(w.inv_depth) // 3] = rejected_cand.inv_depth[len(w.inv_depth) // 3]; xe = xc
            cand, evc = self.cost(w, opts, xe, quad)
            if self.defect == "cost_1e-11": cand *= 1 + 1e-11
            rel = ((rejected_cost if (self.defect == "rho_from_rejected" and rejected_cost is not None) else cost) - cand) / mcc
            rep.model_cost_change[it] = mcc; rep.candidate_cost[it] = cand; rep.relative_decrease[it] = rel; rep.step_norm[it] = self._step_norm(x, xc)
            if abs(cost - cand) <= opts.function_tolerance * cost:
                rep.cost[it] = cost; rep.radius[it] = radius; term = 3; break
            if rel > opts.min_relative_decrease and mcc > 0:
                x = xc; nsucc += 1; rep.accepted[it] = 1
                radius = min(opts.max_trust_region_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3)); decr = 2.0
                cost = cand
                if it < opts.max_num_iterations:      # the linearization's own sum at the accepted point
                    cost, ev = self.cost(w, opts, x, quad); sysm = lm_step_ref.System(x, ev, opts)
                rejected_cand = rejected_cost = None
            else:
                rep.accepted[it] = 0; radius = radius / decr; decr *= 2.0; rejected_cand, rejected_cost = xc, cand
            rep.cost[it] = cost; rep.radius[it] = radius
        rep.termination = term; rep.num_iterations = it; rep.num_successful = nsucc; rep.final_cost = cost
        st = abi.State(len(w.inv_depth), len(w.line_orth))
        st.pose, st.speedbias, st.ex_pose, st.td, st.relo_pose = x.pose.copy(), x.speedbias.copy(), x.ex_pose.copy(), float(x.td), x.relo_pose.copy()
        st.inv_depth, st.line_orth = x.inv_depth.copy(), x.line_orth.copy()
        return st, rep


@pytest.mark.parametrize("name", cases.NAMES)
def test_clean_restatement_passes(oracle, name):
    w, o, costs = _case(oracle, name)
    F = ar.check_one_iteration(name, w, o, cases.K[name], Restated(oracle), costs, ar._log)
    assert not F, (name, len(F), F[:6])


# defect -> the case it is planted on (the smallest that has the path) and a word of the failure it must cause
DEFECTS = {"unnormalised": ("small", "not unit"), "stale_trig": ("small", "cost outside the bound"), "wrong_buffer": ("rejected_once", "inverse depths"),
           "float32_y": ("prior", "cost outside the bound"), "rho_from_rejected": ("rejected_once", "relative_decrease is not"), "cost_1e-11": ("converged", "cost outside the bound")}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_planted_defect_is_caught(oracle, defect):
    name, word = DEFECTS[defect]
    w, o, costs = _case(oracle, name)
    F = ar.check_one_iteration(name, w, o, cases.K[name], Restated(oracle, defect), costs, [])
    assert any(word in str(f) for f in F), (defect, name, F[:6])
