"""Pass B1 of a line chunk (csrc/uvs_solve_kernel.h: line_pass_b) and the line half of a re-damping (redamp_prep) run on eight lanes per line: the 14 sums of
H_ll and g_l dealt over the lanes, a lane per damped diagonal entry, a lane per column of the inverse (ln_lanes_solve).  Every sum walks the line's observations
in the order of the one-lane form with the same per-term expression and every derived value is computed by the same operations, so UVS_LINE_B1=1 (the default)
and UVS_LINE_B1=0 (one lane per line) must agree BITWISE: state, report, per-iteration trace.  The switch is read per launch, so both forms run in one process
on one handle.  Line chunks of the windows (lines / observations), from tools/pack_dump and tools/line_ahead_rule chunks:
    bench_prior 20 / 140 twice | one 1 / 7 | three 3 / 21 | lines33 33 / 99 (one line past a trip of 256 / 8) | lines40_t3 40 / 120 (two trips) | lines40_t2 40 / 80 |
    ln_track10 14 / 140, 13 / 130, 13 / 130 | lines_only (no point chunk) | plain16 16 / 112 (pass A not ahead) | mixed: tracks of 1, 2 and 7 in one chunk"""
import importlib, os, sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
uvs = importlib.import_module("uv-slam_amd")
synth, abi = uvs.synth, uvs.abi
from test_gpu_scalar_header import _bits, _same_state, _same_report
from test_gpu_line_pass_ahead import knob
pytestmark = pytest.mark.gpu


def mixed_tracks(index=46):
    """make_window(index, ln_track=7) with line observations deleted: line l keeps the first 1, 2 or all 7 observations of its track (l mod 3 = 0, 1, 2), so one
    chunk holds tracks of three lengths and the lines' observation ranges are no multiples of one another."""
    w = synth.make_window(index, ln_track=7).copy()
    keep = np.zeros(len(w.ln_lm), bool)
    for l in range(len(w.line_orth)):
        o = np.flatnonzero(w.ln_lm == l)
        assert len(o) == 7
        keep[o[:(1, 2, 7)[l % 3]]] = True
    for k in ("ln_lm", "ln_fj", "ln_sp", "ln_ep", "ln_has_vp", "ln_vp"):
        setattr(w, k, np.ascontiguousarray(getattr(w, k)[keep]))
    return w


@pytest.fixture(scope="module")
def windows():
    from oracle_binding import Oracle          # the n = 75 prior comes from the CPU: the windows do not depend on the code under test
    from gpu_soak_rejections import stressed_window
    orc = Oracle()
    w = {}
    w["bench_prior"] = synth.make_window(8100, with_prior=True, marginalize_fn=lambda win, flag: orc.marginalize(win, flag))
    assert w["bench_prior"].prior is not None and w["bench_prior"].prior.n == 75
    w["one"] = synth.make_window(44, n_lines=1, n_tagged=1)
    w["three"] = synth.make_window(43, n_lines=3, n_tagged=2)
    w["lines33"] = synth.make_window(45, n_points=30, n_lines=33, n_tagged=20, ln_track=3)
    w["lines40_t3"] = synth.make_window(41, ln_track=3)
    w["lines40_t2"] = synth.make_window(42, ln_track=2)
    w["ln_track10"] = synth.make_window(32, ln_track=10)
    w["lines_only"] = synth.make_window(33, n_points=0, n_lines=40, n_tagged=30)
    w["plain16"] = synth.make_window(7, n_points=60, n_lines=16, n_tagged=12)
    w["mixed"] = mixed_tracks()
    for i in (0, 4):      # the oracle's traces of these two: accepted steps, rejected ones, accepted ones again
        w["rejections%d" % i] = stressed_window(i, None, np.random.default_rng(77 + i))[0]
    return w


CASES = ["bench_prior", "one", "three", "lines33", "lines40_t3", "lines40_t2", "ln_track10", "lines_only", "plain16", "mixed", "rejections0", "rejections4"]


def _both(s, run):
    with knob(UVS_LINE_B1=0): one = run(s)
    with knob(UVS_LINE_B1=None): lanes = run(s)
    return one, lanes


def _solver(nt=None, max_batch=1):
    with knob(UVS_KSOLVE_NT=nt):      # read at uvs_create
        return uvs.api.Solver(device=0, max_batch=max_batch)


def _check_single(name, w, s, **env):
    with knob(**env):
        (so, ro), (sl, rl) = _both(s, lambda s: s.solve(w))
    assert ro.status == 0 and rl.status == 0 and ro.num_iterations > 1, (name, ro.status, rl.status, ro.num_iterations)
    if name.startswith("rejections"):
        acc = list(ro.accepted[1:ro.num_iterations + 1])
        assert 0 in acc and 1 in acc[acc.index(0):], (name, acc)      # a re-damping between two linearizations
    assert _same_report(rl, ro), (name, "report / per-iteration trace")
    assert _same_state(sl, so), (name, "state")


@pytest.mark.parametrize("name", CASES)
def test_single_window_bitwise(windows, name):
    s = _solver()
    try: _check_single(name, windows[name], s)
    finally: s.close()


def test_heterogeneous_batch_bitwise(windows):
    """Every window above in ONE launch, against the one-lane form and against the single solves."""
    batch = [windows[n] for n in CASES]
    s = _solver(max_batch=len(batch))

    def run(s):
        s.upload(batch); s.solve_resident()
        return s.download()
    (so, ro), (sl, rl) = _both(s, run)
    single = [s.solve(w) for w in batch]
    s.close()
    for i, n in enumerate(CASES):
        assert ro[i].status == 0 and _same_report(rl[i], ro[i]) and _same_state(sl[i], so[i]), n
        assert _same_report(rl[i], single[i][1]) and _same_state(sl[i], single[i][0]), (n, "single")


@pytest.mark.parametrize("name", ["bench_prior", "lines33", "rejections0"])
def test_256_thread_instantiation_bitwise(windows, name):
    """All four waves evaluate (no roles): 32 lines per trip on the same lanes."""
    s = _solver(nt=256)
    try: _check_single(name, windows[name], s)
    finally: s.close()


def test_plain_order_bitwise(windows):
    """UVS_LINE_AHEAD=0: pass B1 behind pass A and its barrier in the same call."""
    s = _solver()
    try: _check_single("bench_prior", windows["bench_prior"], s, UVS_LINE_AHEAD=0)
    finally: s.close()


@pytest.mark.parametrize("name", ["plain16", "lines40_t3"])
def test_large_solve_fused_bitwise(windows, name):
    """k_large_chunks reaches the pass through chunk_eval and the re-damping through redamp_prep."""
    s = _solver()
    (so, ro, _), (sl, rl, _) = _both(s, lambda s: s.large_solve_fused(windows[name]))
    s.close()
    assert ro.status == 0 and rl.status == 0 and ro.num_iterations > 1, (name, ro.status, rl.status)
    assert _same_report(rl, ro) and _same_state(sl, so), name


def test_first_iteration_bitwise(windows):
    s = _solver()
    do, dl = _both(s, lambda s: s.debug_first_iteration(windows["bench_prior"]))
    s.close()
    for k in ("S", "g", "hd", "dd", "step"):
        assert np.array_equal(_bits(dl[k]), _bits(do[k])), k
