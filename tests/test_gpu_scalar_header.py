"""The kernels read the window header, the chunk table and the IMU block table through the scalar cache (csrc/uvs_solve_kernel.h: DevWinK / IntK;
the rule is stated at DevWin in csrc/uvs_layout.h).  That cache is not coherent with anything but the start of a launch, so the hazard is a STALE header or
descriptor: another window's constants reaching a launch that reuses the same device addresses.  The arithmetic is untouched, so every test here reuses device
buffers with windows whose loop-sizing fields all differ and demands BITWISE equality with a fresh handle that has only ever seen those windows."""
import importlib, os, sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
uvs = importlib.import_module("uv-slam_amd")
synth = uvs.synth
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shape_sets():
    """Set A: two canonical windows with the n = 75 prior.  Set B: no prior, a handful of landmarks -- (5 points, no line) and (3 points, 2 lines): a point chunk
    smaller than a wave, another chunk count, another n_points / n_lines / prior_n / n_cimg in every header word that sizes a loop."""
    from oracle_binding import Oracle          # builds the priors of set A on the CPU: the windows do not depend on the code under test
    orc = Oracle()
    a = [synth.make_window(8100 + i, with_prior=True, marginalize_fn=lambda win, flag: orc.marginalize(win, flag)) for i in range(2)]
    assert all(w.prior is not None and w.prior.n == 75 for w in a)
    b = [synth.make_window(8110, n_points=5, n_lines=0, n_tagged=0), synth.make_window(8111, n_points=3, n_lines=2, n_tagged=0)]
    assert all(w.prior is None for w in b)
    return a, b


def _handle(nt=None):
    old = os.environ.get("UVS_KSOLVE_NT")
    if nt is not None: os.environ["UVS_KSOLVE_NT"] = str(nt)      # read per handle at uvs_create
    try:
        return uvs.api.Solver(device=0, max_batch=2)
    finally:
        if nt is not None:
            if old is None: os.environ.pop("UVS_KSOLVE_NT", None)
            else: os.environ["UVS_KSOLVE_NT"] = old


def _resident(s, windows):
    s.upload(windows); s.solve_resident()
    return s.download()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same_state(x, y):
    return all(np.array_equal(_bits(getattr(x, k)), _bits(getattr(y, k))) for k in ("pose", "speedbias", "ex_pose", "inv_depth", "line_orth")) and _bits([x.td])[0] == _bits([y.td])[0]


def _same_report(p, q):
    if (p.status, p.termination, p.num_iterations, p.num_successful) != (q.status, q.termination, q.num_iterations, q.num_successful): return False
    if _bits([p.initial_cost, p.final_cost]).tolist() != _bits([q.initial_cost, q.final_cost]).tolist(): return False
    tp, tq = p.trace(), q.trace()
    return all(np.array_equal(tp[k], tq[k]) if k == "accepted" else np.array_equal(_bits(tp[k]), _bits(tq[k])) for k in tp)


def _assert_same(got, want, what):
    (gs, gr), (ws_, wr) = got, want
    assert len(gs) == len(ws_) == 2
    for i in range(2):
        assert gr[i].status == 0 and wr[i].status == 0, (what, i, gr[i].status, wr[i].status)
        assert _same_report(gr[i], wr[i]), (what, i, "report / per-iteration trace")
        assert _same_state(gs[i], ws_[i]), (what, i, "state")


@pytest.mark.parametrize("nt", [512, 256])
def test_resident_reupload_with_other_headers(shape_sets, nt):
    """One handle, the same device buffers: set A, then set B, then set A again.  Each result equals, bit for bit, what a fresh handle gives for that set alone
    (and A's second result its first).  Both instantiations of the persistent kernel."""
    a, b = shape_sets
    s = _handle(nt)
    first_a = _resident(s, a)
    then_b = _resident(s, b)
    again_a = _resident(s, a)
    s.close()
    f = _handle(nt); fresh_b = _resident(f, b); f.close()
    f = _handle(nt); fresh_a = _resident(f, a); f.close()
    assert fresh_a[1][0].num_iterations > 1 and fresh_b[1][0].num_iterations > 1
    _assert_same(first_a, fresh_a, "A first")
    _assert_same(then_b, fresh_b, "B after A")
    _assert_same(again_a, first_a, "A after B")


def test_stream_alternating_headers(shape_sets):
    """Seven batches of two windows, A B A B A B A, through uvs_batch_stream: three buffer sets, so every set is reused with the other shape set's header and with
    a freshly patched out_host.  Equal to the resident solves of the same windows."""
    a, b = shape_sets
    f = _handle(); want_a = _resident(f, a); f.close()
    f = _handle(); want_b = _resident(f, b); f.close()
    windows = []
    for k in range(7): windows += a if k % 2 == 0 else b
    s = _handle()
    st, rep, ms = s.stream(windows, 2)
    s.close()
    assert len(st) == 14 and ms > 0.0
    for k in range(7):
        ws_, wr = want_a if k % 2 == 0 else want_b
        for j in range(2):
            i = 2 * k + j
            assert rep[i].status == 0 and _bits([rep[i].final_cost])[0] == _bits([wr[j].final_cost])[0], (k, j, rep[i].final_cost, wr[j].final_cost)
            assert rep[i].num_iterations == wr[j].num_iterations and _same_state(st[i], ws_[j]), (k, j)


def _prior_words(p):
    n = p.n
    return [np.array([p.n, p.n_blocks] + list(p.block_kind) + list(p.block_frame) + list(p.block_size) + list(p.block_idx) + list(p.x0_off), dtype=np.int64),
            _bits(p.J0()), _bits(p.r0()), _bits(np.ctypeslib.as_array(p.x0))]


def _shared_ctx_results(s, w):
    """The other kernels built on the same Ctx, one call each: k_large_* (the fused loop), k_marg_linearize, k_evaluate."""
    out = []
    st, rep, _ = s.large_solve_fused(w)
    assert rep.status == 0
    out += [_bits(st.pose), _bits(st.speedbias), _bits(st.inv_depth), _bits(st.line_orth), _bits([rep.initial_cost, rep.final_cost]), np.array([rep.num_iterations, rep.termination]),
            _bits(rep.trace()["cost"]), _bits(rep.trace()["radius"])]
    out += _prior_words(s.marginalize(w, 0))
    ev = s.evaluate(w)
    out += [_bits(getattr(ev, k)) for k in ("pt_r", "pt_J", "ln_r", "ln_J", "vp_r", "vp_J", "imu_r", "imu_J", "prior_r")] + [_bits([ev.cost])]
    return out


def test_kernels_that_share_the_context(shape_sets):
    """large_solve_fused, marginalize and evaluate of a window of set A, then of a window of set B, on ONE handle (each call packs into the handle's single-window
    buffers, so B's header lands where A's was): equal to a fresh handle's results for B, and A's results equal a fresh handle's as well."""
    a, b = shape_sets
    s = _handle()
    got_a = _shared_ctx_results(s, a[0])
    got_b = [_shared_ctx_results(s, w) for w in b]
    s.close()
    f = _handle(); want_b = [_shared_ctx_results(f, w) for w in b[::-1]][::-1]; f.close()      # (the fresh handle sees them in the other order, too)
    f = _handle(); want_a = _shared_ctx_results(f, a[0]); f.close()
    for name, got, want in (("A", got_a, want_a), ("B0", got_b[0], want_b[0]), ("B1", got_b[1], want_b[1])):
        assert len(got) == len(want)
        for k, (x, y) in enumerate(zip(got, want)):
            assert np.array_equal(x, y), (name, k)
