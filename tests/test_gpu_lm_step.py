"""The damped LM step of the persistent kernel (uvs_debug_step, form 0 = k_solve) against the extended-precision reference of
tests/lm_step_ref.py, per block group, per radius, on both instantiations of the kernel.

Bounds:
  forward  ||d_G - d*_G|| / ||d*_G|| <= max(10 x FP64 level of the group, 1e-12)   (FP64 level: worst of dense LU in three orders and a plain FP64
                                                                                    Schur path on the same system, lm_step_ref.fp64_level)
  backward ||M y - b|| / (||M|| ||y|| + ||b||) <= max(1e-13, 10 x the FP64 Schur path's), in longdouble at the device's y = d / s.
The floors are the pose graph's starting points (test_pose_graph.py: _check_step); the levels measured on an MI355X are in DESIGN.md.
The system is built from the product's own evaluation dump (checked against the oracle's first), which isolates the linear algebra.
"""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import abi
import lm_step_cases as cases
import lm_step_ref as ref
import pyref_lm

RADII = [1e-2, 1.0, 1e4, 1e6, 1e8, 1e10, 1e12]      # radii[0] fresh, each later one a re-damping of the stored linearization
REDAMP = [1e4, 5e3, 1.25e3, 156.25]                 # the radii after consecutive rejections from the default 1e4
FWD_FLOOR, BWD_FLOOR = 1e-12, 1e-13
LD = np.longdouble
SUBSET_256 = ["prior", "full_rows", "small", "td", "extrinsic", "no_jacobi"]      # every option and both Cholesky variants


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
    t += np.sum(d[L["pt"]:] ** 2)
    return float(t)


_log = []


def _reference(cache, sysm, r, grps):
    """(delta*, FP64 level per group, FP64 Schur backward error, cond(M)) at radius r, once per case and radius."""
    if r not in cache:
        delta, _ = ref.damped_step(sysm, r)
        lvl, bwd64 = ref.fp64_level(sysm, r, delta, grps)
        cache[r] = (delta, lvl, bwd64, np.linalg.cond(np.asarray(sysm.M(r), np.float64)))
    return cache[r]


def _check_run(w, opts, sysm, cache, radii, steps, scal, tag):
    grps = ref.groups(w, opts)
    for k, r in enumerate(radii):
        delta, lvl, bwd64, cond = _reference(cache, sysm, r, grps)
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
        assert abs(scal[k, 3] - mcc) <= 1e-10 * abs(mcc), (tag, r, scal[k, 3], mcc)
        s2 = _step_norm2(w, opts, dev)
        assert abs(scal[k, 4] - s2) <= 1e-10 * s2, (tag, r, scal[k, 4], s2)
        _log.append(f"{tag:28s} r={r:8.3g}  fwd max {max(err.values()):.2e} (fp64 {max(lvl.values()):.2e}, worst ratio to bound {worst:.2f})  bwd {bwd:.2e} (fp64 schur {bwd64:.2e})  cond {cond:.1e}")


@pytest.fixture(scope="module")
def step_log():
    yield _log
    path = os.environ.get("UVS_STEP_LOG")
    if path:
        with open(path, "w") as f: f.write("\n".join(_log) + "\n")


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
            s = gpu_api.Solver(opts=opts, max_batch=2)
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
    return _cases[name]


def _run_case(gpu_api, oracle, name, nt, step_log):
    w, opts, sysm, cache = _case(gpu_api, oracle, name)
    with _Env({"UVS_KSOLVE_NT": str(nt)}):
        s = gpu_api.Solver(opts=opts, max_batch=2)
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
        assert np.array_equal(one[0][:L["frames"]], first[pad]), (name, nt, np.abs(one[0][:L["frames"]] - first[pad]).max())
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.NAMES)
def test_k_solve_step_matches_the_reference(gpu_api, oracle, name, step_log):
    _run_case(gpu_api, oracle, name, 512, step_log)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SUBSET_256)
def test_k_solve256_step_matches_the_reference(gpu_api, oracle, name, step_log):
    _run_case(gpu_api, oracle, name, 256, step_log)


@pytest.mark.gpu
def test_debug_step_rejects_bad_arguments(gpu_api):
    w, opts = cases.build("small")
    s = gpu_api.Solver(opts=opts, max_batch=2)
    try:
        for radii, form in (([0.0], 0), ([-1.0], 0), ([np.inf], 0), ([np.nan], 0), ([1e4], 7)):
            with pytest.raises(RuntimeError, match="uvs error 1"):
                s.debug_step(w, radii, form=form)
        wc, keep = w.to_c()
        n = 165 + 7 + 12
        st = np.zeros(n + 1); sc = np.zeros(40); r = np.array([1e4])
        assert gpu_api.lib().uvs_debug_step(s._h, C.byref(wc), 0, 1, abi._dp(r), n + 1, abi._dp(st), abi._dp(sc)) == abi.UVS_ERR_INVALID_ARG
    finally:
        s.close()
