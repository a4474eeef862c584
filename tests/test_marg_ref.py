"""tests/marg_ref.py pinned on the CPU: the 60-digit marginalization reference against an exact known answer, against the longdouble reference it succeeds
and (MARGIN_SECOND_NEW) against the oracle; the oracle's own loss in the scaled metric, printed per case of tests/test_gpu_marginalization_ref.py; and the
proof that the scaled metric sees what max|H - A| / max|A| <= 5e-7 lets through."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

from helpers import abi, marginalization_reference, prior_information_named, MARG_REF_CASES, marg_ref_options, marg_ref_case, marg_ref_weak_window
import marg_ref as mr

_cases = {}


def _case(oracle, name):
    """(post-solve window, the oracle's evaluation dump, options) of a case of helpers.MARG_REF_CASES, the oracle being the solver."""
    if name not in _cases:
        opts = marg_ref_options(MARG_REF_CASES[name][0])
        w = marg_ref_case(name, lambda x: oracle.solve(x, opts=opts), lambda x, f: oracle.marginalize(x, f, opts=opts))
        _cases[name] = (w, oracle.evaluate(w, robust=True, opts=opts), opts)
    return _cases[name]


def test_layout_constants_are_those_of_the_abi():
    assert mr.NF == abi.NUM_FRAMES and mr.NF - 2 == abi.WINDOW_SIZE - 1
    assert (mr.KIND_POSE, mr.KIND_SPEEDBIAS, mr.KIND_EX, mr.KIND_TD) == (abi.BLOCK_POSE, abi.BLOCK_SPEEDBIAS, abi.BLOCK_EX_POSE, abi.UVS_BLOCK_TD)
    assert mr.EPS == 1e-8 and mr.PIVOT_FLOOR == 1e-6 and mr.FLOOR == 1e-13 and mr.bound(0.0) == 1e-13 and mr.bound(0.5) == 5.0


def _integer_window(rng):
    """A window with integer-valued factors: a prior over Pose[0], SpeedBias[0], Pose[1], Pose[2], IMU block 0 and one point anchored at frame 0 with observations
    in frames 1 and 2.  Dropped: the 15 columns of frame 0 and the landmark.  Kept: frame 1 (15), Pose[2] (6), the extrinsic (6)."""
    ri = lambda *s: rng.integers(-4, 5, size=s).astype(np.float64)
    n = 27
    J0 = ri(n, n)
    prior = SimpleNamespace(n=n, n_blocks=4, block_kind=[0, 1, 0, 0], block_frame=[0, 0, 1, 2], block_size=[7, 9, 7, 7], block_idx=[0, 6, 15, 21], J0=lambda: J0)
    e = np.zeros
    w = SimpleNamespace(inv_depth=e(1), line_orth=e((0, 4)), prior=prior, imu=[dict(frame_i=0)], pt_fi=np.array([0, 0]), pt_fj=np.array([1, 2]), pt_lm=np.array([0, 0]),
                        ln_fj=e(0, int), ln_lm=e(0, int), ln_has_vp=e(0, int))
    ev = SimpleNamespace(prior_r=ri(n), imu_J=ri(1, 15, 30), imu_r=ri(1, 15), pt_J=ri(2, 2, 19), pt_r=ri(2, 2), ln_J=e((0, 2, 10)), ln_r=e((0, 2)), vp_J=e((0, 2, 10)), vp_r=e((0, 2)))
    return w, ev


def _exact_schur(w, ev):
    """The same Schur complement in fractions.Fraction, written out for this one window (column order: frame 0, landmark | frame 1, Pose[2], extrinsic)."""
    order = list(range(15)) + ["lm"] + list(range(15, 30)) + list(range(30, 36)) + ["ex%d" % k for k in range(6)]
    pos = {c: i for i, c in enumerate(order)}
    P = len(order)
    H = [[Fraction(0)] * P for _ in range(P)]; g = [Fraction(0)] * P

    def add(cols, J, r):
        J = [[Fraction(int(x)) for x in row] for row in np.asarray(J)]; r = [Fraction(int(x)) for x in np.asarray(r)]
        for a, ca in enumerate(cols):
            g[pos[ca]] += sum(J[k][a] * r[k] for k in range(len(r)))
            for b, cb in enumerate(cols):
                H[pos[ca]][pos[cb]] += sum(J[k][a] * J[k][b] for k in range(len(r)))

    add(list(range(15)) + list(range(15, 21)) + list(range(30, 36)), w.prior.J0(), ev.prior_r)
    add(list(range(30)), ev.imu_J[0], ev.imu_r[0])
    for k, fj in enumerate((1, 2)):
        add(list(range(6)) + list(range(15 * fj, 15 * fj + 6)) + ["ex%d" % q for q in range(6)] + ["lm"], ev.pt_J[k], ev.pt_r[k])
    m = 16
    M = [row[:] + [g[i]] for i, row in enumerate(H)]
    for c in range(m):      # exact elimination: any nonzero pivot will do
        piv = next(i for i in range(c, m) if M[i][c] != 0)
        M[c], M[piv] = M[piv], M[c]
        for i in range(c + 1, P):
            f = M[i][c] / M[c][c]
            if f: M[i] = [x - f * y for x, y in zip(M[i], M[c])]
    A = np.array([[float(M[i][j]) for j in range(m, P)] for i in range(m, P)])
    b = np.array([float(M[i][P]) for i in range(m, P)])
    cols = list(range(15, 30)) + list(range(30, 36)) + [mr.EX + k for k in range(6)]
    return A, b, cols


@pytest.mark.parametrize("seed", [0, 1])
def test_known_answer_to_the_last_bit(seed):
    w, ev = _integer_window(np.random.default_rng(seed))
    A, b, cols = mr.reference(w, ev, 0, None)
    Ax, bx, cx = _exact_schur(w, ev)
    assert cols == cx
    assert np.array_equal(A, Ax) and np.array_equal(b, bx)
    assert np.abs(A).max() > 10 and np.all(np.diag(A) > 0)


@pytest.mark.parametrize("name", ["70", "71", "72", "41"])
def test_against_the_longdouble_reference(oracle, name):
    w, ev, opts = _case(oracle, name)
    Ald, bld, kc = marginalization_reference(w, ev)
    c = mr.compare(Ald, bld, [x if x >= 0 else mr.EX + 6 + x for x in kc], mr.reference(w, ev, 0, opts))
    print("window %s: longdouble reference against 60 digits, scaled: H %.2e b %.2e" % (name, c["eH"], c["eb"]))
    assert c["eH"] <= 1e-7 and c["eb"] <= 1e-7      # measured worst 5.4e-9 (H)


@pytest.mark.parametrize("name", ["71", "72", "41", "73"])
def test_second_new_against_the_oracle(oracle, name):
    w, ev, opts = _case(oracle, name)
    ref = mr.reference(w, ev, 1, opts)
    assert ref is not None and len(ref[2]) == w.prior.n - 6
    c = mr.compare(*prior_information_named(oracle.marginalize(w, 1, opts=opts), 1), ref)
    print("window %s, MARGIN_SECOND_NEW: oracle against 60 digits, scaled: H %.2e b %.2e" % (name, c["eH"], c["eb"]))
    assert c["eH"] <= 1e-11 and c["eb"] <= 1e-10      # measured up to 4.5e-14 / 1.5e-12


@pytest.mark.parametrize("name", ["td89", "ex81"])
def test_second_new_without_a_block_to_drop(oracle, name):
    """A prior that does not reach frame WINDOW_SIZE - 1 has nothing to drop: no reference, the prior comes back as it went in."""
    w, ev, opts = _case(oracle, name)
    assert mr.reference(w, ev, 1, opts) is None
    q = oracle.marginalize(w, 1, opts=opts)
    assert q.n == w.prior.n and np.array_equal(q.J0(), w.prior.J0()) and np.array_equal(q.r0(), w.prior.r0())


@pytest.mark.parametrize("name,flag", [(n, f) for n, c in MARG_REF_CASES.items() for f in ((0, 1) if c[2] is not None else (0,))])
def test_the_oracle_in_the_scaled_metric(oracle, name, flag):
    """Printed, not bounded: the eigen-decomposition pseudo-inverse of A_mm is the reference algorithm's own loss (4e-2 on the window whose prior carries the td
    block).  Asserted is what held before this metric existed: max-relative <= 5e-7 / 1e-8 on windows 70 to 72 (tests/test_marginalization.py)."""
    w, ev, opts = _case(oracle, name)
    ref = mr.reference(w, ev, flag, opts)
    if ref is None: return      # (a prior without a pose block of frame WINDOW_SIZE - 1: test_second_new_without_a_block_to_drop)
    H, b, cols = prior_information_named(oracle.marginalize(w, flag, opts=opts), flag)
    c = mr.compare(H, b, cols, ref)
    lH, lb, _ = mr.fp64_level(w, ev, flag, opts)
    print("case %s flag %d (n = %d): oracle eH %.2e eb %.2e | FP64 level %.2e %.2e | ratio to the bound %.3g %.3g | worst blocks %s"
          % (name, flag, len(cols), c["eH"], c["eb"], lH, lb, c["eH"] / mr.bound(lH), c["eb"] / mr.bound(lb), mr.format_blocks(c, mr.bound(lH))))
    if name in ("70", "71", "72") and flag == 0:
        A, br, kp = ref
        perm = [cols.index(x) for x in kp]
        assert np.abs(H[np.ix_(perm, perm)] - A).max() / np.abs(A).max() <= 5e-7 and np.abs(b[perm] - br).max() / np.abs(br).max() <= 1e-8


@pytest.mark.parametrize("name,least", [("70", 3.0), ("71", 10.0), ("72", 10.0), ("41", 10.0)])
def test_the_gap_is_real(oracle, name, least):
    """The 3 x 3 accelerometer-bias diagonal block of frame 1 times (1 + delta), delta = HALF of what max|H - A| <= 5e-7 max|A| tolerates there: the old metric
    passes, the scaled one fails by a factor >= 10 (>= 3 on window 70, whose FP64 level is itself 1.3e-4)."""
    w, ev, opts = _case(oracle, name)
    A, b, cols = mr.reference(w, ev, 0, opts)
    r = [cols.index(15 + 9 + k) for k in range(3)]
    delta = 0.5 * 5e-7 * np.abs(A).max() / np.abs(A[np.ix_(r, r)]).max()
    Am = A.copy(); Am[np.ix_(r, r)] *= 1 + delta
    old = np.abs(Am - A).max() / np.abs(A).max()
    c = mr.compare(Am, b, cols, (A, b, cols))
    lH, lb, _ = mr.fp64_level(w, ev, 0, opts)
    print("window %s: delta %.3g, old metric %.2e (bound 5e-7), scaled metric %.2e = %.1f x its bound %.2e; worst block %s"
          % (name, delta, old, c["eH"], c["eH"] / mr.bound(lH), mr.bound(lH), max(c["blocks"], key=c["blocks"].get)))
    assert delta > 1e-3
    assert old < 5e-7
    assert c["eH"] / mr.bound(lH) >= least and c["eb"] == 0.0
    assert max(c["blocks"], key=c["blocks"].get) == (1, 1)


@pytest.mark.parametrize("name,flag", [("70", 0), ("71", 0), ("72", 0), ("41", 0), ("71", 1), ("td89", 0), ("ex81", 0)])
def test_the_two_fp64_forms_agree_on_their_level(oracle, name, flag):
    """fp64_level through the same comparison: within its own bound trivially, and neither form degenerates -- both within 100 x of each other.
    (ex80 is not in the list: its kept system has an eigenvalue next to the 1e-8 cut that one form keeps and the other cuts, 3.6e-7 against 1.9e-11 in b -- the rank
    decision marg_ref leaves unpinned; the level is the larger of the two there as everywhere.)"""
    w, ev, opts = _case(oracle, name)
    lH, lb, det = mr.fp64_level(w, ev, flag, opts)
    a, c = det["pivoted"], det["cholesky"]
    assert max(a["eH"], c["eH"]) == lH <= mr.bound(lH) and max(a["eb"], c["eb"]) == lb <= mr.bound(lb)
    for k in ("eH", "eb"):
        assert 0 < a[k] <= 100 * c[k] and 0 < c[k] <= 100 * a[k], (name, flag, k, a[k], c[k])


def test_a_window_on_which_the_eps_cut_acts(oracle):
    """helpers.marg_ref_weak_window: two dropped points with information <= 1e-8 and NO eigenvalue of A_mm (60 digits) in [1e-10, 1e-6], so the cut is unambiguous in FP64;
    the plain reference refuses the window (a pivot under 100 eps), reference_with_cut is the reference's own rule, and the oracle -- that rule in FP64 -- is printed in
    the scaled metric beside the FP64 level of the two forms that cut per landmark block."""
    w = marg_ref_weak_window()
    ev = oracle.evaluate(w, robust=True)
    with pytest.raises(AssertionError, match="eps cut"):
        mr.reference(w, ev, 0, None)
    A, b, cols, lam = mr.reference_with_cut(w, ev, 0, None)
    assert (lam <= 1e-8).sum() == 2 and lam[0] > 0 and lam[1] < 1e-10 and lam[2] > 1e-6, lam[:4]
    H, g, md, kp, _ = mr.assemble(w, ev, 0, None, mr.F64)
    info = np.sort([H[c, c] for c in md if c >= mr.F])
    assert info[1] <= 1e-8 and info[2] > 1e-6
    lH, lb, det = mr.fp64_level(w, ev, 0, None, cut=True)
    c = mr.compare(*prior_information_named(oracle.marginalize(w, 0), 0), (A, b, cols))
    print("weak window: eigenvalues of A_mm %s; FP64 level %.2e %.2e (pivoted %.2e, cholesky %.2e); oracle eH %.2e eb %.2e"
          % (" ".join("%.2e" % x for x in lam[:4]), lH, lb, det["pivoted"]["eH"], det["cholesky"]["eH"], c["eH"], c["eb"]))
    assert 0 < lH < 1e-3 and 0 < lb < 1e-3      # the forms that cut per block are restatements of the same operation, not of another one
