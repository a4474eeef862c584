"""The factor kernels (csrc/uvs_factors.h, the whitening and prior_dx of csrc/uvs_solve_kernel.h) against the 60-digit reference of tests/factor_ref.py.

  * uvs_evaluate (point_eval<true, true>, line_geom<true>, imu_raw<30, 0, true, 15>): every residual block of every case of tests/factor_cases.py, per row
    group x parameter group, within B = max(C level_in, C model, 1e-13 scale) -- the bound and the C = 10 that tests/test_factor_ref.py holds the CPU oracle
    to; both come from the reference alone.  Inside the VP guard: Jacobian exactly zero, residual within the model term.
  * the solvers' own instantiations (point_eval<true, false> / <false, false>, cached line_trig, imu_raw<48, 1, false, PARTS> over four waves, lin_imu_tiles):
    cost, and g and diag H per block group, of uvs_debug_first_iteration (512- and 256-thread k_solve) against lm_step_ref.System built from the REFERENCE's
    evaluation, with B propagated to first order; initial_cost of solve, large_solve and large_solve_fused within sum |r| B_r.
The figures go to the file UVS_FACTOR_LOG names.
"""
import numpy as np
import pytest

from helpers import abi
import factor_cases as cases
import factor_ref as fr
import lm_accept_ref
import lm_step_ref
from lm_step_check import _Env

pytestmark = pytest.mark.gpu
C = 10
LD = np.longdouble


@pytest.fixture(scope="module", autouse=True)
def factor_log():
    list(fr.pool().map(abs, range(64)))      # the reference's workers exist before anything touches the GPU
    yield
    fr.write_log()
    fr.shutdown()


_refs = {}


def _case(gpu_api, name):
    """(window, options, reference): the prior cases carry the product's own marginalization of the previous window."""
    if name not in _refs:
        o = cases.options(name)
        if name in ("prior", "prior_moved"):
            s = gpu_api.Solver(opts=o, max_batch=2)
            try: w, o = cases.build(name, marginalize_fn=lambda win, flag: s.marginalize(win, flag))
            finally: s.close()
        else:
            w, o = cases.build(name)
        cases.check_structure(name, w, o)
        _refs[name] = (w, o, fr.evaluate_cached(name, w, o, level_stride=cases.level_stride(name)))
    return _refs[name]


@pytest.mark.parametrize("name", cases.NAMES)
def test_evaluate_is_within_the_bound(gpu_api, name):
    w, o, R = _case(gpu_api, name)
    s = gpu_api.Solver(opts=o, max_batch=2)
    try:
        evs = {robust: s.evaluate(w, robust=robust) for robust in (False, True)}
    finally:
        s.close()
    failures = []
    for robust in (False, True):
        ref, ev = R[robust], evs[robust]
        recs = fr.check(ev, ref, C)
        fr.log_records(f"device {name} robust={int(robust)}", recs)
        cb = fr.cost_bound(ref, C)
        fr.log(f"device {name} robust={int(robust)}: cost {ev.cost:.17g} reference {ref.cost:.17g} |diff| {abs(ev.cost - ref.cost):.2e} bound {cb:.2e}")
        failures += [(robust,) + r for r in recs if not r[8] <= 1.0]
        if not abs(ev.cost - ref.cost) <= cb: failures.append((robust, "cost", ev.cost, ref.cost, cb))
    for lab, (fam, k) in sorted(getattr(w, "edge", {}).items()):
        rs = [r for r in fr.check(evs[True], R[True], C, families=("vp",) if lab.startswith("vp") else (fam,)) if r[1] == k]
        worst = max(rs, key=lambda r: r[8])
        fr.log(f"device {name} edge {lab:28s} {fam} block {k}: worst err {worst[4]:.2e} ({worst[2]} x {worst[3]}) level_in {worst[5]:.2e} model {worst[6]:.2e} err/B {worst[8]:.3f}")
        if lab.startswith("vp") and R[True].aux["ln"][k]["guarded"]:
            assert np.all(evs[True].vp_J[k] == 0.0) and np.all(evs[False].vp_J[k] == 0.0), lab      # the documented deviation D8
    assert not failures, (name, len(failures), sorted(failures, key=lambda r: -r[9] if len(r) > 9 else 0)[:6])


# ---------------------------------------------------------------- the solver kernels' own instantiations
def _abs_eval(w, ref, B, with_bounds):
    """An Eval-shaped object of |values| (+ the entry bounds): (|J| + B_J)^T (|J| + B_J) - |J|^T |J| bounds the error of J^T J entry by entry."""
    e = abi.Eval(w)
    for nm in ("pt_r", "pt_J", "pt_Jtd", "ln_r", "ln_J", "vp_r", "vp_J", "imu_r", "imu_J"):
        setattr(e, nm, np.abs(getattr(ref, nm)) + (B[nm] if with_bounds else 0.0))
    e.prior_r = np.zeros_like(ref.prior_r)
    return e


def _prior_columns(w, L):
    p = w.prior; cols, src = [], []
    for b in range(p.n_blocks):
        kind, frm, size, idx = p.block_kind[b], p.block_frame[b], p.block_size[b], p.block_idx[b]
        loc = 6 if size == 7 else size
        base = 15 * frm if kind == abi.BLOCK_POSE else 15 * frm + 6 if kind == abi.BLOCK_SPEEDBIAS else L["ex"] if kind == abi.BLOCK_EX_POSE else L["td"]
        if base is None: continue
        cols += [base + k for k in range(loc)]; src += [idx + k for k in range(loc)]
    return cols, src


def _normal_equations_reference(w, o, ref):
    """(H, g, their entrywise first-order bounds dH, dg, layout) over the whole parameter vector, from the reference's evaluation."""
    L = lm_step_ref.layout(w, o)
    H, g = lm_step_ref.normal_equations(w, ref, o)
    B = fr.entry_bounds(ref, C)
    Ha, ga = lm_step_ref.normal_equations(w, _abs_eval(w, ref, B, False), o)
    Hb, gb = lm_step_ref.normal_equations(w, _abs_eval(w, ref, B, True), o)
    dH = np.asarray(Hb - Ha, np.float64); dg = np.asarray(gb - ga, np.float64)
    if w.prior is not None and w.prior.n > 0:
        cols, src = _prior_columns(w, L)
        dg[cols] += np.abs(w.prior.J0()[:, src]).T @ B["prior_r"][:w.prior.n]
    return H, g, dH, dg, L


def _first_iteration_reference(w, o, ref):
    """(g_reduced, diag H, their entrywise first-order bounds) over the frame columns of lm_step_ref.layout, from the reference's evaluation.
    g_reduced = g_f - H_fl H_ll^-1 g_l of the damped system in unscaled coordinates (helpers.lm_reduced_system), in longdouble; the bound carries
    dg_f + |H_fl H_ll^-1| dg_l + dH_fl |H_ll^-1 g_l| + |H_fl H_ll^-1| dH_ll |H_ll^-1 g_l|, the damping's share of dH_ll included."""
    H, g, dH, dg, L = _normal_equations_reference(w, o, ref); F, P = L["frames"], L["n"]
    hd = np.diag(H).copy(); dhd = np.diag(dH).copy()
    s = LD(1) / (LD(1) + np.sqrt(hd)) if o.jacobi_scaling else np.ones(P, LD)
    radius = LD(o.initial_trust_region_radius)
    dd = np.clip(s * s * hd, LD(o.min_lm_diagonal), LD(o.max_lm_diagonal)) / (radius * s * s)
    ddd = dhd / float(radius) * (1.0 + o.min_lm_diagonal * (1.0 + 1.0 / np.sqrt(np.maximum(np.asarray(hd, np.float64), 1e-300))))
    Hd = H + np.diag(dd)
    npt, nln = len(w.inv_depth), len(w.line_orth)
    X = np.zeros((P - F, F), LD); y = np.zeros(P - F, LD)      # H_ll^-1 H_lf, H_ll^-1 g_l: 1 x 1 point blocks, 4 x 4 line blocks
    if npt:
        d = np.diag(Hd)[F:F + npt]
        X[:npt] = Hd[F:F + npt, :F] / d[:, None]; y[:npt] = g[F:F + npt] / d
    if nln:
        idx = F + npt + 4 * np.arange(nln)[:, None] + np.arange(4)[None, :]
        Cb = Hd[idx[:, :, None], idx[:, None, :]]
        rhs = np.concatenate([Hd[idx][:, :, :F], g[idx][:, :, None]], axis=2)
        sol = lm_step_ref._chol_solve_batch(lm_step_ref._chol_batch(Cb), rhs)
        X[npt:] = sol[:, :, :F].reshape(4 * nln, F); y[npt:] = sol[:, :, F].reshape(4 * nln)
    gr = g[:F] - Hd[:F, F:] @ y
    Xa, ya = np.abs(np.asarray(X, np.float64)), np.abs(np.asarray(y, np.float64))
    dHll = dH[F:, F:] + np.diag(ddd[F:])
    dgr = dg[:F] + Xa.T @ dg[F:] + dH[:F, F:] @ ya + Xa.T @ (dHll @ ya)
    return gr, dgr, hd[:F], dhd[:F], L


def _frame_pad(L):
    pad = [16 * f + a for f in range(abi.NUM_FRAMES) for a in range(15)]
    pad += [16 * a + 15 for a in range(6)] if L["ex"] is not None else []
    pad += [175] if L["td"] is not None else []
    return pad


@pytest.mark.parametrize("nt", [512, 256])
@pytest.mark.parametrize("name", cases.SOLVE_NAMES)
def test_first_iteration_matches_the_reference(gpu_api, name, nt):
    """cost, g and diag H of uvs_debug_first_iteration per block group; the bound per group is B propagated to first order, floor 1e-13 of the group's norm."""
    w, o, R = _case(gpu_api, name)
    ref = R[True]
    gr, dgr, hd, dhd, L = _first_iteration_reference(w, o, ref)
    with _Env({"UVS_KSOLVE_NT": str(nt)}):
        s = gpu_api.Solver(opts=o, max_batch=2)
    try:
        d = s.debug_first_iteration(w)
    finally:
        s.close()
    pad = _frame_pad(L)
    failures = []
    cb = fr.cost_bound(ref, C)
    fr.log(f"k_solve{nt} {name}: cost {d['cost']:.17g} reference {ref.cost:.17g} |diff| {abs(d['cost'] - ref.cost):.2e} bound {cb:.2e}")
    if not abs(d["cost"] - ref.cost) <= cb: failures.append(("cost", d["cost"], ref.cost, cb))
    for what, dev, val, dv in (("g", d["g"][pad], gr, dgr), ("hd", d["hd"][pad], hd, dhd)):
        worst = (0.0, None)
        for nm, ix in lm_step_ref.groups(w, o):
            if ix[0] >= L["frames"]: continue
            err = float(np.sqrt(np.sum((np.asarray(dev[ix], LD) - val[ix]) ** 2)))
            nrm = float(np.sqrt(np.sum(val[ix] ** 2)))
            bound = max(float(np.sqrt(np.sum(dv[ix] ** 2))), 1e-13 * nrm)
            ratio = err / bound if bound > 0 else (0.0 if err == 0 else np.inf)
            worst = max(worst, (ratio, (nm, err, nrm, bound)))
            if not ratio <= 1.0: failures.append((what, nm, err, nrm, bound))
        fr.log(f"k_solve{nt} {name}: {what} worst group {worst[1][0]}: err {worst[1][1]:.2e} of norm {worst[1][2]:.2e}, bound {worst[1][3]:.2e}, err / bound {worst[0]:.3f}")
    assert not failures, (name, nt, failures[:6])


@pytest.mark.parametrize("name", cases.SOLVE_NAMES)
def test_initial_cost_of_every_solver_matches_the_reference(gpu_api, name):
    """initial_cost of solve (both k_solve instantiations), large_solve and large_solve_fused against the reference's cost, bound sum |r| B_r; and their
    gradient_max_norm[0] against || x - Plus(x, -g*) ||_inf of the reference's gradient (lm_accept_ref.gradient_max_norm), bound: the largest entry bound
    propagated for g, plus 1e-13 of the value."""
    w, o, R = _case(gpu_api, name)
    ref = R[True]; cb = fr.cost_bound(ref, C)
    _, g, _, dg, _ = _normal_equations_reference(w, o, ref)
    gmax = lm_accept_ref.gradient_max_norm(w, o, g); gb = float(dg.max()) + 1e-13 * gmax
    got = {}; grad = {}
    for nt in (512, 256):
        with _Env({"UVS_KSOLVE_NT": str(nt)}):
            s = gpu_api.Solver(opts=o, max_batch=2)
        try:
            reps = {f"solve{nt}": s.solve(w)[1]}
            if nt == 512: reps.update(large_solve=s.large_solve(w)[1], large_solve_fused=s.large_solve_fused(w)[1])
            for nm, r in reps.items(): got[nm], grad[nm] = r.initial_cost, r.gradient_max_norm[0]
        finally:
            s.close()
    bad = []
    for nm, c0 in got.items():
        fr.log(f"{nm} {name}: initial_cost {c0:.17g} reference {ref.cost:.17g} |diff| {abs(c0 - ref.cost):.2e} bound {cb:.2e}")
        if not abs(c0 - ref.cost) <= cb: bad.append((nm, c0, ref.cost, cb))
        fr.log(f"{nm} {name}: gradient_max_norm[0] {grad[nm]:.17g} reference {gmax:.17g} |diff| {abs(grad[nm] - gmax):.2e} bound {gb:.2e}")
        if not abs(grad[nm] - gmax) <= gb: bad.append((nm, "gradient_max_norm", grad[nm], gmax, gb))
    assert not bad, (name, bad)
