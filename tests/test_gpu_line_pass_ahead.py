"""The 512-thread solve kernel evaluates a line chunk's pass A under the previous chunk's gather walk, its records at the base of
csrc/uvs_layout.h: uvs_line_ahead_base (csrc/uvs_solve_kernel.h: linearize_roles).  Every lane evaluates the same observations in the same order and every sum
keeps its order, so UVS_LINE_AHEAD=1 (the default) and UVS_LINE_AHEAD=0 (the plain order) must agree BITWISE: state, report, per-iteration trace.  The switch is
read per launch, so both paths run in one process on one handle."""
import importlib, os, sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
uvs = importlib.import_module("uv-slam_amd")
synth, abi = uvs.synth, uvs.abi
from test_gpu_scalar_header import _bits, _same_state, _same_report
pytestmark = pytest.mark.gpu


class knob:
    """UVS_LINE_AHEAD (read at every launch) / UVS_KSOLVE_NT (read at uvs_create) for the duration of a block."""
    def __init__(self, **kv): self.kv = kv
    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = str(v)
    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


@pytest.fixture(scope="module")
def windows():
    """name -> (window, option set).  The chunk tables of the shapes are those of tests/test_line_ahead_rule.py."""
    from oracle_binding import Oracle          # the n = 75 prior comes from the CPU: the windows do not depend on the code under test
    from gpu_soak_rejections import stressed_window
    orc = Oracle()
    w = {}
    w["bench_prior"] = (synth.make_window(8100, with_prior=True, marginalize_fn=lambda win, flag: orc.marginalize(win, flag)), "")
    assert w["bench_prior"][0].prior is not None and w["bench_prior"][0].prior.n == 75
    w["bench_noprior"] = (synth.make_window(17), "")
    w["lines80"] = (synth.make_window(31, n_lines=80, n_tagged=40, ln_track=5), "")      # bases 12 550, 0, 12 550
    w["lines80_full"] = (synth.make_window(31, n_lines=80, n_tagged=40), "")             # every line chunk fills the staging area: plain order
    w["ln_track10"] = (synth.make_window(32, n_lines=44, ln_track=10), "")               # the rule refuses: plain order
    w["ln_track10_40"] = (synth.make_window(32, ln_track=10), "")                        # bases 12 904, 0, 11 992
    w["lines_only"] = (synth.make_window(33, n_points=0, n_lines=40, n_tagged=30), "")
    w["points_only"] = (synth.make_window(35, n_lines=0, n_tagged=0), "")
    for i in (0, 4):      # the oracle's traces of these two: accepted steps, rejected ones, accepted ones again
        w["rejections%d" % i] = (stressed_window(i, None, np.random.default_rng(77 + i))[0], "")
    w["td"] = (synth.add_time_offset(synth.make_window(88), td_true=0.005), "td")
    w["ex"] = (synth.make_window(80), "ex")
    w["relo"] = (synth.add_relocalization(synth.make_window(3), seed=3), "")
    return w


def _opts(optset):
    o = abi.default_options(); o.estimate_td = int("td" in optset); o.estimate_extrinsic = int("ex" in optset)
    return o


def _both(s, run):
    with knob(UVS_LINE_AHEAD=0): plain = run(s)
    with knob(UVS_LINE_AHEAD=None): ahead = run(s)
    return plain, ahead


CASES = ["bench_prior", "bench_noprior", "lines80", "lines80_full", "ln_track10", "ln_track10_40", "lines_only", "points_only", "rejections0", "rejections4", "td", "ex", "relo"]


@pytest.mark.parametrize("name", CASES)
def test_single_window_bitwise(windows, name):
    w, optset = windows[name]
    s = uvs.api.Solver(opts=_opts(optset), device=0, max_batch=1)
    (sp, rp), (sa, ra) = _both(s, lambda s: s.solve(w))
    s.close()
    assert rp.status == 0 and ra.status == 0 and rp.num_iterations > 1, (name, rp.status, ra.status)
    if name.startswith("rejections"):
        acc = list(rp.accepted[1:rp.num_iterations + 1])
        assert 0 in acc and 1 in acc[acc.index(0):], (name, acc)      # a re-damping between two linearizations
    assert _same_report(ra, rp), (name, "report / per-iteration trace")
    assert _same_state(sa, sp), (name, "state")


def test_heterogeneous_batch_bitwise(windows):
    """Every default-option window above in ONE launch (a workgroup each: ahead at bases of its own, or not at all), against the plain order and against the single solves."""
    names = [n for n in CASES if windows[n][1] == ""]
    batch = [windows[n][0] for n in names]
    s = uvs.api.Solver(device=0, max_batch=len(batch))

    def run(s):
        s.upload(batch); s.solve_resident()
        return s.download()
    (sp, rp), (sa, ra) = _both(s, run)
    single = [s.solve(w) for w in batch[:3]]
    s.close()
    for i, n in enumerate(names):
        assert rp[i].status == 0 and _same_report(ra[i], rp[i]) and _same_state(sa[i], sp[i]), n
    for i, (st, rep) in enumerate(single):
        assert _same_report(ra[i], rep) and _same_state(sa[i], st), names[i]


def test_debug_counter_shows_the_path(windows):
    """A debug launch counts the line chunks whose pass A ran ahead and the full linearizations of the solve: two per linearization on the benchmark's window
    (bases 12 920 and 0), none with the switch off, none in the 256-thread instantiation (no roles), none where the rule refuses."""
    w = windows["bench_prior"][0]
    s = uvs.api.Solver(device=0, max_batch=1)
    (dp, da) = _both(s, lambda s: s.debug_first_iteration(w))
    _, rep = s.solve(w)
    dn = s.debug_first_iteration(windows["bench_noprior"][0])
    dr = s.debug_first_iteration(windows["ln_track10"][0])
    d3 = s.debug_first_iteration(windows["lines80"][0])
    s.close()
    # full linearizations: the first, and one after every accepted step but a last one that ends the solve
    assert da["linearizations"] in (rep.num_successful, rep.num_successful + 1) and da["linearizations"] >= 2, (da["linearizations"], rep.num_successful)
    assert da["line_ahead"] == 2 * da["linearizations"], (da["line_ahead"], da["linearizations"])
    assert dp["line_ahead"] == 0 and dp["linearizations"] == da["linearizations"]
    assert dn["line_ahead"] == 2 * dn["linearizations"] > 0
    assert dr["line_ahead"] == 0 and dr["linearizations"] >= 2
    assert d3["line_ahead"] == 3 * d3["linearizations"] > 0
    for k in ("S", "g", "hd", "dd", "step"):
        assert np.array_equal(_bits(da[k]), _bits(dp[k])), k
    with knob(UVS_KSOLVE_NT=256):
        s = uvs.api.Solver(device=0, max_batch=1)
    d256 = s.debug_first_iteration(w)
    s.close()
    assert d256["line_ahead"] == 0 and d256["linearizations"] >= 2
