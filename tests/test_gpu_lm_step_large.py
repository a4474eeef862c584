"""The damped LM step of the landmark-sharded kernels (uvs_debug_step form 1: k_large_chunks -> k_large_reduce -> k_large_solve -> k_large_backsub)
against the extended-precision reference of tests/lm_step_ref.py, per block group, per radius, on both instantiations of k_large_chunks /
k_large_solve, on one rank and as two shards driven from one process.

Same bounds as tests/test_gpu_lm_step.py (lm_step_check.py); in this form every radius after the first is a
RE-LINEARIZATION at the same state, which is how uvs_large_decide handles a rejected step.  The step comes from the buffers k_large_backsub itself
reads and writes (its storing instantiation), the scalars from the code uvs_large_decide uses.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import abi, synth
import lm_step_cases as cases
import lm_step_check as chk
import lm_step_ref as ref
from lm_step_check import RADII, REDAMP, FWD_FLOOR, _Env, _case, _check_run, _reference

SUBSET_256 = ["prior", "full_rows", "small", "td", "extrinsic", "no_jacobi"]      # as for k_solve: every option and both Cholesky variants
SHARDED = ["prior", "ragged", "td", "tracks2", "many_chunks_plain"]      # tracks2: each shard leaves pose blocks untouched that the other one fills


@pytest.fixture(scope="module")
def step_log():
    yield chk._log
    chk.write_log()


def _nt_env(nt):
    return {"UVS_LARGE_CHUNKS_NT": str(nt), "UVS_LARGE_SOLVE_NT": str(nt), "UVS_KSOLVE_NT": str(nt)}


def _cross_form(w, opts, sysm, cache, large, ksolve, tag):
    """Frame step of form 1 against form 0 at the default radius: they factor the same reduced system with different summation orders, so per group
    they differ by no more than the sum of the two forms' own bounds."""
    r = opts.initial_trust_region_radius
    grps = [(g, ix) for g, ix in ref.groups(w, opts) if g not in ("points", "lines")]
    delta, lvl, _, _, _ = _reference(cache, sysm, r, ref.groups(w, opts))
    worst = 0.0
    for g, ix in grps:
        den = float(np.sqrt(np.sum(delta[ix] ** 2)))
        e = float(np.linalg.norm(large[ix] - ksolve[ix])) / den if den > 0 else float(np.linalg.norm(large[ix] - ksolve[ix]))
        bound = 2 * max(10 * lvl[g], FWD_FLOOR)
        worst = max(worst, e / bound)
        assert e <= bound, (tag, g, e, bound)
    chk._log.append(f"{tag:28s} r={r:8.3g}  frame step of form 1 against form 0: worst ratio to the sum of their bounds {worst:.3f}")


def _run_large(gpu_api, oracle, name, nt):
    w, opts, sysm, cache = _case(gpu_api, oracle, name)
    env = dict(_nt_env(nt), **cases.create_environment(name))
    with _Env(env):
        s = gpu_api.Solver(opts=opts, max_batch=2, **cases.capacity(name))
    o1 = cases.options(name); o1.max_num_iterations = 1
    with _Env(env):
        s1 = gpu_api.Solver(opts=o1, max_batch=2, **cases.capacity(name))
    try:
        with _Env(cases.environment(name)):
            for radii in (RADII, REDAMP):
                steps, scal = s.debug_step(w, radii, form=1)
                _check_run(w, opts, sysm, cache, radii, steps, scal, f"{name}/k_large{nt}")
                # the launch geometry the handle really ran: chunks, chunk workgroups of k_large_chunks (= rows of k_large_reduce), of k_large_backsub
                if name == "many_chunks_grid20": assert np.all(scal[:, 5:8] == [60, 20, 40]), scal[0, 5:8]
                elif name == "many_chunks_mid": assert np.all(scal[:, 5] == scal[:, 6]) and np.all(scal[:, 5] >= 128) and np.all(scal[:, 7] == scal[:, 5]), scal[0, 5:8]
                else: assert np.all(scal[:, 5] == scal[:, 6]) and np.all(scal[:, 5] < 128), scal[0, 5:8]      # the canonical windows: one chunk per workgroup
            one, _ = s.debug_step(w, [opts.initial_trust_region_radius], form=1)
            zero, _ = s.debug_step(w, [opts.initial_trust_region_radius], form=0)
            _cross_form(w, opts, sysm, cache, one[0], zero[0], f"{name}/k_large{nt}")
            # the storing instantiation and the product kernels compute the same step, bit for bit: the landmarks of an ordinary one-iteration
            # large_solve are the start values plus the stored steps (backsub_candidate forms the candidate by that one addition)
            st, rep = s1.large_solve(w)
            again, _ = s.debug_step(w, [opts.initial_trust_region_radius], form=1)
        assert np.array_equal(one, again), (name, nt)
        L = ref.layout(w, opts)
        assert rep.accepted[1] == 1, (name, nt, rep.accepted[1])      # (every case's first step at the default radius is an accepted one)
        assert np.array_equal(st.inv_depth, w.inv_depth + one[0][L["pt"]:L["ln"]]), (name, nt)
        assert np.array_equal(st.line_orth.reshape(-1), w.line_orth.reshape(-1) + one[0][L["ln"]:]), (name, nt)
        assert np.array_equal(st.speedbias.reshape(-1), (w.speedbias + one[0][:165].reshape(11, 15)[:, 6:]).reshape(-1)), (name, nt)
    finally:
        s.close(); s1.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.NAMES + cases.RELO_NAMES + cases.BIG_NAMES + cases.EXTRA_NAMES)
def test_k_large_step_matches_the_reference(gpu_api, oracle, name, step_log):
    _run_large(gpu_api, oracle, name, 512)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SUBSET_256 + ["relo", "relo_extrinsic_td", "many_chunks_grid20"] + cases.EXTRA_NAMES)
def test_k_large256_step_matches_the_reference(gpu_api, oracle, name, step_log):
    _run_large(gpu_api, oracle, name, 256)


@pytest.mark.gpu
@pytest.mark.parametrize("name,nt", [(n, 512) for n in SHARDED] + [("td", 256), ("tracks2", 256)])
def test_two_shards_in_one_process_give_the_step_of_the_whole_window(gpu_api, oracle, name, nt, step_log):
    """Two handles on one device, each with the landmarks k mod 2 of the window, the `reduced` vectors and the step scalars summed on the host
    between the calls (no RCCL, no second process): the assembled step against the reference of the UNSHARDED window, same bounds.  The frame
    part is bit-identical on the two ranks (they solve the same all-reduced system); the landmarks come from their owners."""
    w, opts, sysm, cache = _case(gpu_api, oracle, name)
    shards = [synth.shard_landmarks(w, r, 2) for r in range(2)]
    assert all(len(sh[1]) > 0 and len(sh[2]) > 0 for sh in shards)
    L = ref.layout(w, opts)
    for radii in (RADII, REDAMP):
        o = cases.options(name); o.initial_trust_region_radius = radii[0]      # (the step-wise form starts at the radius of the handle's options)
        with _Env(_nt_env(nt)):
            solvers = [gpu_api.Solver(opts=o, max_batch=2, **cases.capacity(name)) for _ in range(2)]
        try:
            with _Env(cases.environment(name)):
                out = gpu_api.Solver.debug_step_sharded(solvers, [sh[0] for sh in shards], radii)
        finally:
            for s in solvers: s.close()
        steps = np.zeros((len(radii), L["n"]))
        for (step, scal), (sw, pk, lk) in zip(out, shards):
            assert np.array_equal(step[:, :L["frames"]], out[0][0][:, :L["frames"]]), name
            assert np.array_equal(scal[:, :5], out[0][1][:, :5]), name
            npt = len(pk)
            steps[:, L["pt"] + pk] = step[:, L["frames"]:L["frames"] + npt]
            cols = (L["ln"] + 4 * lk[:, None] + np.arange(4)[None, :]).reshape(-1)
            steps[:, cols] = step[:, L["frames"] + npt:]
        steps[:, :L["frames"]] = out[0][0][:, :L["frames"]]
        _check_run(w, opts, sysm, cache, radii, steps, out[0][1], f"{name}/k_large{nt} x 2 shards")


@pytest.mark.gpu
def test_two_shards_refuse_relocalization_blocks_in_the_step_form(gpu_api):
    w = synth.add_relocalization(synth.make_window(21), relo_frame=4, seed=21)
    opts = abi.default_options()
    shards = [synth.shard_landmarks(w, r, 2)[0] for r in range(2)]
    assert sum(len(sh.relo_lm) for sh in shards) == len(w.relo_lm) > 0
    solvers = [gpu_api.Solver(opts=opts, max_batch=2) for _ in range(2)]
    try:
        with pytest.raises(RuntimeError, match="uvs error %d" % abi.UVS_ERR_UNSUPPORTED):
            gpu_api.Solver.debug_step_sharded(solvers, shards, [1e4])
        # ... and uvs_debug_step form 1 on a handle that was told of two ranks
        s = solvers[0]
        s._check(gpu_api.lib().uvs_large_set_nranks(s._h, 2))
        with pytest.raises(RuntimeError, match="uvs error %d" % abi.UVS_ERR_UNSUPPORTED):
            s.debug_step(shards[0], [1e4], form=1)
        s._check(gpu_api.lib().uvs_large_set_nranks(s._h, 1))
    finally:
        for s in solvers: s.close()


@pytest.mark.gpu
def test_large_debug_step_rejects_bad_arguments(gpu_api):
    w, opts = cases.build("small")
    s = gpu_api.Solver(opts=opts, max_batch=2)
    L = gpu_api.lib()
    try:
        for radii in ([0.0], [-1.0], [np.inf], [np.nan], [1e4, 0.0]):
            with pytest.raises(RuntimeError, match="uvs error 1"):
                s.debug_step(w, radii, form=1)
        wc, keep = w.to_c()
        n = 165 + 7 + 12
        st = np.zeros(n + 1); sc = np.zeros(40); r = np.array([1e4])
        assert L.uvs_debug_step(s._h, C.byref(wc), 1, 1, abi._dp(r), n + 1, abi._dp(st), abi._dp(sc)) == abi.UVS_ERR_INVALID_ARG
        # the getter of the step-wise form: no solve in progress, flag not set, wrong length, bad next radius
        assert L.uvs_large_debug_step(s._h, 0.0, n, abi._dp(st), abi._dp(sc)) == abi.UVS_ERR_INVALID_ARG
        s.debug_step(w, [1e2], form=1)      # leaves a stored step behind: the next solve, stepped with the flag off, must not hand it out
        s._check(L.uvs_large_begin(s._h, C.byref(wc)))
        s._check(L.uvs_large_linearize(s._h)); s._check(L.uvs_large_step(s._h))
        assert L.uvs_large_debug_step(s._h, 0.0, n, abi._dp(st), abi._dp(sc)) == abi.UVS_ERR_INVALID_ARG
        s._check(L.uvs_large_set_debug_step(s._h, 1))
        assert L.uvs_large_debug_step(s._h, 0.0, n, abi._dp(st), abi._dp(sc)) == abi.UVS_ERR_INVALID_ARG      # flag on, but the last step did not store
        s._check(L.uvs_large_step(s._h))
        assert L.uvs_large_debug_step(s._h, 0.0, n + 1, abi._dp(st), abi._dp(sc)) == abi.UVS_ERR_INVALID_ARG
        for bad in (-1.0, np.inf, np.nan):
            assert L.uvs_large_debug_step(s._h, bad, n, abi._dp(st), abi._dp(sc)) == abi.UVS_ERR_INVALID_ARG
        assert L.uvs_large_debug_step(s._h, 0.0, n, abi._dp(st), abi._dp(sc)) == abi.UVS_OK
        one, _ = s.debug_step(w, [opts.initial_trust_region_radius], form=1)
        assert np.array_equal(one[0], st[:n])
        s._check(L.uvs_large_set_debug_step(s._h, 0))
    finally:
        s.close()
