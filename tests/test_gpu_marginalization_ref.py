"""The marginalization prior of the three product paths, entry by entry against the 60-digit Schur complement of tests/marg_ref.py.

Paths: `device` = uvs_marginalize (k_marg_linearize + the host finish of csrc/uvs_marg.h), `host` = the same call under UVS_MARG_HOST=1, `batch` =
uvs_marginalize_batch (k_marg_linearize_batch + the parallel Jacobi of k_marg_finish), all windows of one option set in one call.
Cases: helpers.MARG_REF_CASES -- default options 70 (no prior), 71, 72, 41, 73, 74; estimate_td 88 and 89 with 88's prior; estimate_extrinsic 80 and 81 with
80's prior; both options 83 with a foreign prior.  Every window with a prior under MARGIN_OLD (0) and MARGIN_SECOND_NEW (1).

Per case the product's evaluation dump is first held against the oracle's blockwise to 1e-9 (as tests/test_gpu_back_substitution.py does), so the reference is
built from inputs another suite pins.  Then, in the metric of marg_ref.compare (errors relative to sqrt(A_ii A_jj) of the reference),
    eH <= max(1e-13, 10 x FP64 level of H)      eb <= max(1e-13, 10 x FP64 level of b)
the level being what two plain numpy FP64 restatements of the same operation reach on the same system (marg_ref.fp64_level).  The ratio e / bound is printed per
pair of frame blocks.  Block tables and linearization points: bit for bit those of the oracle.  A MARGIN_SECOND_NEW whose prior has no pose block of frame
WINDOW_SIZE - 1 must hand the prior back unchanged, bit for bit.

The eps cut that acts: helpers.marg_ref_weak_window has two dropped points with information ~1e-14.  The one-window device path must notice them and hand the call to the host
path, the batched path likewise; the reference is the reference's own rule at 60 digits (marg_ref.reference_with_cut), the level that of the two FP64 forms that cut per block."""
import numpy as np
import pytest

from helpers import abi, prior_information_named, MARG_REF_CASES, marg_ref_options, marg_ref_case, marg_ref_weak_window
import lm_step_check as chk
import marg_ref as mr

PATHS = ["device", "host", "batch"]
ROWS = [(name, flag) for name, (_, _, prior) in MARG_REF_CASES.items() for flag in ((0, 1) if prior is not None else (0,))]

_runs = {}


def _run(gpu_api, oracle, optset):
    """{case: dict(w, ev, opts, priors = {(flag, path): abi.Prior}, oracle = {flag: abi.Prior})} of one option set: one solver, one batched call."""
    if optset not in _runs:
        opts = marg_ref_options(optset)
        names = [n for n, c in MARG_REF_CASES.items() if c[0] == optset]
        s = gpu_api.Solver(opts=opts, max_batch=2)
        try:
            out = {}
            for name in names:
                w = marg_ref_case(name, s.solve, s.marginalize)
                out[name] = dict(w=w, ev=s.evaluate(w, robust=True), opts=opts, priors={}, oracle={})
            jobs = [(n, f) for n, f in ROWS if n in names]
            for n, f in jobs:
                out[n]["priors"][f, "device"] = s.marginalize(out[n]["w"], f)
                with chk._Env({"UVS_MARG_HOST": "1"}):
                    out[n]["priors"][f, "host"] = s.marginalize(out[n]["w"], f)
                out[n]["oracle"][f] = oracle.marginalize(out[n]["w"], f, opts=opts)
            batch, status = s.marginalize_batch([out[n]["w"] for n, f in jobs], [f for n, f in jobs])
            assert status == [0] * len(jobs)
            for (n, f), p in zip(jobs, batch): out[n]["priors"][f, "batch"] = p
        finally:
            s.close()
        _runs[optset] = out
    return _runs[optset]


def _case(gpu_api, oracle, name):
    return _run(gpu_api, oracle, MARG_REF_CASES[name][0])[name]


def _check_dump(name, w, ev, opts, oracle, pt_r_floor=0.0):
    """The product's evaluation dump against the oracle's, blockwise to 1e-9.  The VP blocks, r = vp_factor acos(c) with c next to 1 after a solve, are granted beside it
    what FP64 itself loses there on each side (the error model of tests/factor_ref.py): dr = vp_factor dc / sqrt(1 - c^2), dJ = |J| dc / (1 - c^2), dc = 4 x 2^-53 --
    1e-8 of a residual of 3e-3."""
    eo = oracle.evaluate(w, robust=True, opts=opts)
    for nm in ("pt_J", "ln_r", "ln_J", "imu_r", "imu_J"):
        assert chk._blockwise_relerr(getattr(ev, nm), getattr(eo, nm)) < 1e-9, (name, nm)
    # pt_r_floor: a point residual whose exact value is ZERO (the planted observations of the weak window) has no relative accuracy; r = sqrt_info x a difference of
    # normalized image coordinates of size 1, so FP64 delivers it to a few 2^-53 x sqrt_info ~ 1e-13 absolutely -- such a block is held to 1e-9 x the floor instead
    a, b = np.asarray(ev.pt_r).reshape(len(ev.pt_r), -1), np.asarray(eo.pt_r).reshape(len(eo.pt_r), -1)
    assert np.all(np.abs(a - b).max(axis=1) <= 1e-9 * np.maximum(np.abs(b).max(axis=1), pt_r_floor)), (name, "pt_r")
    if w.prior is not None and w.prior.n:
        assert chk._blockwise_relerr(ev.prior_r[None, :w.prior.n], eo.prior_r[None, :w.prior.n]) < 1e-9, name
    if opts.estimate_td: assert chk._blockwise_relerr(ev.pt_Jtd, eo.pt_Jtd) < 1e-9, name
    on = np.asarray(w.ln_has_vp).ravel() != 0
    nobs = len(on)
    ra, rb = np.asarray(ev.vp_r).reshape(nobs, -1), np.asarray(eo.vp_r).reshape(nobs, -1)
    Ja, Jb = np.asarray(ev.vp_J).reshape(nobs, -1), np.asarray(eo.vp_J).reshape(nobs, -1)
    assert np.array_equal(ra[~on], rb[~on]) and np.array_equal(Ja[~on], Jb[~on]), (name, "rows without a vanishing point")
    if not on.any(): return
    f, dc = float(opts.vp_factor), 4 * 2.0 ** -53
    sin = np.maximum(np.sin(np.abs(rb[on, 0]) / f), 1e-300)
    qr = np.abs(ra[on, 0] - rb[on, 0]) / (1e-9 * np.abs(rb[on, 0]) + 2 * f * dc / sin)
    qJ = np.abs(Ja[on] - Jb[on]).max(axis=1) / ((1e-9 + 2 * dc / sin ** 2) * np.maximum(np.abs(Jb[on]).max(axis=1), 1e-300))
    print("MARGREF %s dump: vp_r, vp_J worst |difference| / allowance %.3g %.3g" % (name, qr.max(), qJ.max()))
    assert qr.max() <= 1.0 and qJ.max() <= 1.0, (name, "vp", qr.max(), qJ.max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MARG_REF_CASES))
def test_evaluation_dump_equals_the_oracles(gpu_api, oracle, name):
    c = _case(gpu_api, oracle, name)
    _check_dump(name, c["w"], c["ev"], c["opts"], oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,flag", ROWS)
def test_prior_against_the_60_digit_reference(gpu_api, oracle, name, flag, path):
    c = _case(gpu_api, oracle, name)
    w, ev, opts, p = c["w"], c["ev"], c["opts"], c["priors"][flag, path]
    ref = mr.reference(w, ev, flag, opts)
    if ref is None:      # nothing to drop: the input prior, bit for bit
        q = w.prior
        assert p.n == q.n and p.n_blocks == q.n_blocks
        for fld in ("block_kind", "block_frame", "block_size", "block_idx", "x0_off"):
            assert list(getattr(p, fld)[:q.n_blocks]) == list(getattr(q, fld)[:q.n_blocks]), (name, path, fld)
        assert np.array_equal(np.asarray(p.x0[:9 * q.n_blocks]), np.asarray(q.x0[:9 * q.n_blocks]))
        assert np.array_equal(p.J0(), q.J0()) and np.array_equal(p.r0(), q.r0()), (name, path)
        print("MARGREF %s flag %d %s: no pose block of frame %d in the prior, returned unchanged" % (name, flag, path, abi.WINDOW_SIZE - 1))
        return
    H, b, cols = prior_information_named(p, flag)
    assert p.n == len(ref[2])
    e = mr.compare(H, b, cols, ref)
    lH, lb, _ = mr.fp64_level(w, ev, flag, opts)
    bH, bb = mr.bound(lH), mr.bound(lb)
    eo = mr.compare(*prior_information_named(c["oracle"][flag], flag), ref)      # printed, not bounded: the reference algorithm's own loss on the same window
    print("MARGREF %s flag %d %s n %d: eH %.2e eb %.2e | FP64 level %.2e %.2e | e / bound %.3g %.3g | oracle %.2e %.2e | per block pair, e / bound: %s"
          % (name, flag, path, p.n, e["eH"], e["eb"], lH, lb, e["eH"] / bH, e["eb"] / bb, eo["eH"], eo["eb"], mr.format_blocks(e, bH)))
    bad = {k: v / bH for k, v in e["blocks"].items() if not v <= bH}
    assert not bad and e["eH"] <= bH, (name, flag, path, e["eH"], bH, bad)
    assert e["eb"] <= bb, (name, flag, path, e["eb"], bb)


@pytest.mark.gpu
@pytest.mark.parametrize("name,flag", ROWS)
def test_block_tables_and_linearization_points_are_the_oracles(gpu_api, oracle, name, flag):
    c = _case(gpu_api, oracle, name)
    po = c["oracle"][flag]
    nb = po.n_blocks
    for path in PATHS:
        p = c["priors"][flag, path]
        assert p.n == po.n and p.n_blocks == nb, (name, flag, path)
        for fld in ("block_kind", "block_frame", "block_size", "block_idx", "x0_off"):
            assert list(getattr(p, fld)[:nb]) == list(getattr(po, fld)[:nb]), (name, flag, path, fld)
        assert np.array_equal(np.asarray(p.x0[:9 * nb]), np.asarray(po.x0[:9 * nb])), (name, flag, path)
    kinds = list(po.block_kind[:nb])
    if flag == 0: assert (abi.UVS_BLOCK_TD in kinds) == bool(c["opts"].estimate_td)


_weak = {}


def _weak_run(gpu_api, oracle):
    if not _weak:
        opts = abi.default_options()
        w = marg_ref_weak_window()
        s = gpu_api.Solver(opts=opts, max_batch=2)
        try:
            ev = s.evaluate(w, robust=True)
            pri = {"device": s.marginalize(w, 0)}
            with chk._Env({"UVS_MARG_HOST": "1"}):
                pri["host"] = s.marginalize(w, 0)
            batch, status = s.marginalize_batch([w, w], [0, 0])
            assert status == [0, 0] and np.array_equal(batch[0].J0(), batch[1].J0())
            pri["batch"] = batch[0]
        finally:
            s.close()
        _weak.update(w=w, ev=ev, opts=opts, priors=pri, oracle=oracle.marginalize(w, 0))
    return _weak


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_a_window_on_which_the_eps_cut_acts(gpu_api, oracle, path):
    c = _weak_run(gpu_api, oracle)
    w, ev, opts, p, po = c["w"], c["ev"], c["opts"], c["priors"][path], c["oracle"]
    _check_dump("weak", w, ev, opts, oracle, pt_r_floor=1e-3)
    H64, _, md, _, _ = mr.assemble(w, ev, 0, opts, mr.F64)
    info = np.sort([H64[k, k] for k in md if k >= mr.F])
    assert info[1] <= 1e-8 and info[2] > 1e-6, info[:4]      # what sends the device path to the host path: a landmark pivot at or under eps
    A, b, cols, lam = mr.reference_with_cut(w, ev, 0, opts)
    assert not np.any((lam >= 1e-10) & (lam <= 1e-6)) and (lam <= 1e-8).sum() == 2, lam[:4]      # the cut is unambiguous in FP64
    e = mr.compare(*prior_information_named(p, 0), (A, b, cols))
    lH, lb, _ = mr.fp64_level(w, ev, 0, opts, cut=True)
    bH, bb = mr.bound(lH), mr.bound(lb)
    eo = mr.compare(*prior_information_named(po, 0), (A, b, cols))
    print("MARGREF weak flag 0 %s n %d: eH %.2e eb %.2e | FP64 level %.2e %.2e | e / bound %.3g %.3g | oracle %.2e %.2e | per block pair, e / bound: %s"
          % (path, p.n, e["eH"], e["eb"], lH, lb, e["eH"] / bH, e["eb"] / bb, eo["eH"], eo["eb"], mr.format_blocks(e, bH)))
    assert e["eH"] <= bH and e["eb"] <= bb, (path, e["eH"], bH, e["eb"], bb)
    nb = po.n_blocks
    assert p.n == po.n and p.n_blocks == nb
    for fld in ("block_kind", "block_frame", "block_size", "block_idx", "x0_off"):
        assert list(getattr(p, fld)[:nb]) == list(getattr(po, fld)[:nb]), (path, fld)
    assert np.array_equal(np.asarray(p.x0[:9 * nb]), np.asarray(po.x0[:9 * nb]))
