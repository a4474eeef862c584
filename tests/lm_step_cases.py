"""Windows for the damped-step tests (tests/test_lm_step_ref.py, tests/test_gpu_lm_step.py): name -> (window, options, environment),
each with a structure check that the case is what its name promises."""
import numpy as np

from helpers import abi, synth

NAMES = ["prior_free", "prior", "prior_extrinsic", "full_rows", "points_only", "lines_only", "small", "tracks2", "tracks10", "ragged",
         "skipped_imu", "td", "extrinsic", "no_jacobi"]
PRIOR_CASES = ("prior", "prior_extrinsic", "full_rows")


def options(name):
    o = abi.default_options()
    if name == "td": o.estimate_td = 1
    if name in ("extrinsic", "prior_extrinsic"): o.estimate_extrinsic = 1
    if name == "no_jacobi": o.jacobi_scaling = 0
    return o


def environment(name):
    """Environment of the solve: full_rows runs the full-row Cholesky (DevWin::chol_half_ok = 0) on an ordinary window."""
    return {"UVS_CHOL_FULL_ROWS": "1"} if name == "full_rows" else {}


def _ragged(w, seed):
    """Keeps a random prefix of every landmark's observations (points >= 1, lines >= 3): tracks of every length in one window."""
    rng = np.random.default_rng(seed)
    o = w.copy()
    keep = np.zeros(len(w.pt_lm), bool)
    for k in range(len(w.inv_depth)):
        ix = np.nonzero(w.pt_lm == k)[0]
        keep[ix[:rng.integers(1, len(ix) + 1)]] = True
    for nm in ("pt_lm", "pt_fi", "pt_fj", "pt_pi", "pt_pj"): setattr(o, nm, getattr(w, nm)[keep])
    keep = np.zeros(len(w.ln_lm), bool)
    for k in range(len(w.line_orth)):
        ix = np.nonzero(w.ln_lm == k)[0]
        keep[ix[:rng.integers(3, len(ix) + 1)]] = True
    for nm in ("ln_lm", "ln_fj", "ln_sp", "ln_ep", "ln_has_vp", "ln_vp"): setattr(o, nm, getattr(w, nm)[keep])
    return o


def build(name, marginalize_fn=None):
    """-> (window, options).  The prior cases need `marginalize_fn(window, flag) -> abi.Prior` (the product's on the GPU, the oracle's on the CPU)."""
    if name == "prior_free":      # the canonical window without a prior: the gauge directions are held by the damping alone
        w = synth.make_window(4)
    elif name in PRIOR_CASES:     # the canonical window with the n = 75 prior of marginalizing the previous window's oldest frame
        w = synth.make_window(11 if name != "prior_extrinsic" else 12, with_prior=True, marginalize_fn=marginalize_fn)
    elif name == "points_only":
        w = synth.make_window(5, n_lines=0, n_tagged=0)
    elif name == "lines_only":
        w = synth.make_window(6, n_points=0, n_tagged=0)
    elif name == "small":         # chunks far smaller than a wave
        w = synth.make_window(7, n_points=7, n_lines=3, n_tagged=2)
    elif name == "tracks2":
        w = synth.make_window(13, pt_track=2, ln_track=2)
    elif name == "tracks10":
        w = synth.make_window(14, pt_track=10, ln_track=10)
    elif name == "ragged":
        w = _ragged(synth.make_window(15, pt_track=9, ln_track=9), 15)
    elif name == "skipped_imu":   # two IMU blocks with sum_dt > 10 s (estimator.cpp:814): frames 3-4 and 7-8 are linked by the landmarks only
        w = synth.make_window(16)
        w.imu = [dict(b) for b in w.imu]
        for b in w.imu:
            if b["frame_i"] in (3, 7): b["skip"] = 1
    elif name == "td":
        w = synth.add_time_offset(synth.make_window(8), seed=8)
    elif name == "extrinsic":
        w = synth.make_window(9)
    elif name == "no_jacobi":
        w = synth.make_window(10)
    else:
        raise KeyError(name)
    return w, options(name)


def _track_lengths(lm, n):
    return np.bincount(lm, minlength=n)


def check_structure(name, w, o):
    np_, nl = len(w.inv_depth), len(w.line_orth)
    assert len(w.relo_lm) == 0
    if name in PRIOR_CASES:
        p = w.prior
        assert p is not None and p.n == 75
        kinds = list(p.block_kind[:p.n_blocks])
        assert kinds.count(abi.BLOCK_POSE) == 10 and kinds.count(abi.BLOCK_SPEEDBIAS) == 1 and kinds.count(abi.BLOCK_EX_POSE) == 1
        assert all(p.block_frame[b] < 2 for b in range(p.n_blocks) if p.block_kind[b] == abi.BLOCK_SPEEDBIAS)      # the half-row Cholesky ...
        assert environment(name).get("UVS_CHOL_FULL_ROWS") == ("1" if name == "full_rows" else None)            # ... unless switched off
    else:
        assert w.prior is None or w.prior.n == 0
    assert bool(o.estimate_td) == (name == "td") and bool(o.estimate_extrinsic) == (name in ("extrinsic", "prior_extrinsic"))
    assert bool(o.jacobi_scaling) == (name != "no_jacobi")
    if name == "points_only": assert np_ > 0 and nl == 0 and len(w.ln_lm) == 0
    elif name == "lines_only": assert np_ == 0 and nl > 0 and len(w.pt_lm) == 0
    elif name == "small": assert (np_, nl) == (7, 3)
    else: assert np_ >= 100 and nl >= 30
    tp = _track_lengths(w.pt_lm, np_) + 1 if np_ else np.zeros(0)      # frames observing a point (anchor + observations)
    tl = _track_lengths(w.ln_lm, nl) if nl else np.zeros(0)
    if name == "tracks2": assert np.all(tp == 2) and np.all(tl == 2)
    if name == "tracks10": assert np.all(tp == 10) and np.all(tl == 10)
    if name == "ragged": assert tp.min() == 2 and tp.max() == 9 and len(np.unique(tp)) == 8 and tl.min() == 3 and len(np.unique(tl)) >= 5
    if name == "td":
        assert w.pt_vel_i is not None and len(w.pt_vel_i) == len(w.pt_lm) and np.abs(w.pt_vel_j).max() > 0
    if np_: assert set(np.unique(w.pt_lm)) == set(range(np_))
    if nl: assert set(np.unique(w.ln_lm)) == set(range(nl))
    skipped = sorted(b["frame_i"] for b in w.imu if b.get("skip", 0))
    assert len(w.imu) == abi.NUM_FRAMES - 1 and skipped == ([3, 7] if name == "skipped_imu" else [])
