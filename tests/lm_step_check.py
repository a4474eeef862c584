"""What the damped-step GPU tests share (tests/test_gpu_lm_step.py: k_solve, tests/test_gpu_lm_step_large.py: the landmark-sharded kernels): the
radii, the bounds of DESIGN.md section 4, the checks of one run against tests/lm_step_ref.py and the per-case cache of window, system and reference."""
import os

import numpy as np

from helpers import abi
import lm_step_cases as cases
import lm_step_ref as ref
import pyref_lm

RADII = [1e-2, 1.0, 1e4, 1e6, 1e8, 1e10, 1e12]      # radii[0] fresh, each later one a re-damping of the stored linearization
REDAMP = [1e4, 5e3, 1.25e3, 156.25]                 # the radii after consecutive rejections from the default 1e4
FWD_FLOOR, BWD_FLOOR = 1e-12, 1e-13
LD = np.longdouble


def _blockwise_relerr(a, b):
    """Worst over residual blocks (first axis) of max |a - b| / max |b| within the block."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if b.size == 0: return 0.0
    a = a.reshape(len(a), -1); b = b.reshape(len(b), -1)
    den = np.maximum(np.abs(b).max(axis=1), 1e-300)
    return float((np.abs(a - b).max(axis=1) / den).max())


def _pose_plus_ld(x, d):
    q = pyref_lm.quat_mul(np.asarray(x[3:], LD), np.array([LD(0.5) * d[3], LD(0.5) * d[4], LD(0.5) * d[5], LD(1)]))
    return np.concatenate([np.asarray(x[:3], LD) + d[:3], q / np.sqrt(np.sum(q * q))])


def _step_norm2(w, opts, delta):
    """||x (+) delta - x||^2 over the ambient parameters (what the kernel sums), in longdouble from the device's own step."""
    L = ref.layout(w, opts); d = np.asarray(delta, LD); t = LD(0)
    for f in range(abi.NUM_FRAMES):
        e = _pose_plus_ld(w.pose[f], d[15 * f:15 * f + 6]) - np.asarray(w.pose[f], LD)
        t += np.sum(e * e) + np.sum(d[15 * f + 6:15 * f + 15] ** 2)
    if L["ex"] is not None:
        e = _pose_plus_ld(w.ex_pose, d[L["ex"]:L["ex"] + 6]) - np.asarray(w.ex_pose, LD); t += np.sum(e * e)
    if L["td"] is not None: t += d[L["td"]] ** 2
    if L["relo"] is not None:
        e = _pose_plus_ld(w.relo_pose, d[L["relo"]:L["relo"] + 6]) - np.asarray(w.relo_pose, LD); t += np.sum(e * e)
    t += np.sum(d[L["pt"]:] ** 2)
    return float(t)


_log = []


def _reference(cache, sysm, r, grps):
    """(delta*, FP64 level per group, FP64 Schur backward error, cond(M), FP64 level of model_cost_change) at radius r, once per case and radius."""
    if r not in cache:
        delta, _ = ref.damped_step(sysm, r)
        lvl, bwd64 = ref.fp64_level(sysm, r, delta, grps)
        cache[r] = (delta, lvl, bwd64, np.linalg.cond(np.asarray(sysm.M(r), np.float64)), ref.fp64_mcc_level(sysm, r))
    return cache[r]


def _check_run(w, opts, sysm, cache, radii, steps, scal, tag):
    grps = ref.groups(w, opts)
    for k, r in enumerate(radii):
        delta, lvl, bwd64, cond, mcc64 = _reference(cache, sysm, r, grps)
        dev = steps[k]
        assert np.all(np.isfinite(dev)), (tag, r)
        M = sysm.M(r)
        assert scal[k, 2] == 1.0 or cond > 1e13, (tag, r, cond)
        err = ref.group_errors(dev, delta.astype(np.float64), grps)
        worst = max(err[g] / max(10 * lvl[g], FWD_FLOOR) for g, _ in grps)
        bad = [(g, err[g], lvl[g]) for g, _ in grps if err[g] > max(10 * lvl[g], FWD_FLOOR)]
        assert not bad, (tag, r, bad[:4])
        y = np.asarray(dev, LD) / sysm.s
        bwd = ref.backward_error(M, sysm.b, y)
        assert bwd <= max(BWD_FLOOR, 10 * bwd64), (tag, r, bwd, bwd64)
        mcc = float(y @ sysm.b - LD(0.5) * (y @ sysm.Hs @ y))
        # 1e-10, or ten times what careful FP64 reaches on this system (lm_step_ref.fp64_mcc_level): that is 1e-16 .. 1e-14 and changes nothing except on
        # prior_td at radius 1e12, whose scaled step is 2e8 long: level 7.4e-11 there on the CPU and 3.5e-11 on the product's evaluation, the kernels measured 1.005e-10 on an MI355X
        assert abs(scal[k, 3] - mcc) <= max(1e-10, 10 * mcc64) * abs(mcc), (tag, r, scal[k, 3], mcc, mcc64)
        s2 = _step_norm2(w, opts, dev)
        assert abs(scal[k, 4] - s2) <= 1e-10 * s2, (tag, r, scal[k, 4], s2)
        _log.append(f"{tag:28s} r={r:8.3g}  fwd max {max(err.values()):.2e} (fp64 {max(lvl.values()):.2e}, worst ratio to bound {worst:.2f})  bwd {bwd:.2e} (fp64 schur {bwd64:.2e})  cond {cond:.1e}  mcc {abs(scal[k, 3] - mcc) / abs(mcc):.1e} (fp64 {mcc64:.1e})" + ("" if scal[k, 2] == 1.0 else "  CHOLESKY FLAG 0 (excused: cond > 1e13)"))


class _Env:
    """Sets environment variables for the duration of a block (UVS_KSOLVE_NT is read at uvs_create, UVS_CHOL_FULL_ROWS at every upload)."""

    def __init__(self, env): self.env, self.old = env, {}

    def __enter__(self):
        for k, v in self.env.items(): self.old[k] = os.environ.get(k); os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


_cases = {}


def _case(gpu_api, oracle, name):
    """(window, options, system from the product's evaluation dump, per-radius reference cache), built once per case: the prior cases
    carry the product's own marginalization of the previous window, and the dump is checked against the oracle's before it is used."""
    if name not in _cases:
        opts = cases.options(name)
        with _Env({"UVS_KSOLVE_NT": "512"}):
            s = gpu_api.Solver(opts=opts, max_batch=2, **cases.capacity(name))
        try:
            w, opts = cases.build(name, marginalize_fn=lambda win, flag: s.marginalize(win, flag))
            cases.check_structure(name, w, opts)
            ev = s.evaluate(w, robust=True)
        finally:
            s.close()
        eo = oracle.evaluate(w, robust=True, opts=opts)
        for nm in ("pt_r", "pt_J", "ln_r", "ln_J", "vp_r", "vp_J", "imu_r", "imu_J"):
            assert _blockwise_relerr(getattr(ev, nm), getattr(eo, nm)) < 1e-9, (name, nm)
        if w.prior is not None and w.prior.n:
            assert _blockwise_relerr(ev.prior_r[None, :w.prior.n], eo.prior_r[None, :w.prior.n]) < 1e-9, name
        if opts.estimate_td: assert _blockwise_relerr(ev.pt_Jtd, eo.pt_Jtd) < 1e-9, name
        _cases[name] = (w, opts, ref.System(w, ev, opts), {})
        if name == "weak": cases.check_weak(_cases[name][2])
    return _cases[name]


def write_log():
    """The measured figures of every run so far -> the file UVS_STEP_LOG names (each test module's fixture calls this at its end)."""
    path = os.environ.get("UVS_STEP_LOG")
    if path:
        with open(path, "w") as f: f.write("\n".join(_log) + "\n")
