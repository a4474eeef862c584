"""The marginalization prior at 60 digits (mpmath) and the FP64 yardstick that goes with it.  mpmath and numpy only: nothing here comes from csrc, the
oracle, pyref*.py or helpers.marginalization_reference, so a shared slip cannot hide.

reference(w, ev, flag, opts) -> (A, b, cols): the float64 roundings of the Schur complement over the kept columns, every sum and the elimination in mpf.
  flag 0 (MARGIN_OLD, estimator.cpp:1008-1129): the prior, IMU block 0, the points anchored at frame 0 and the line / VP observations j != 0 of lines that
      start at frame 0; dropped = Pose[0], SpeedBias[0] and those landmarks.  Under estimate_td the point factor has ev.pt_Jtd as a 20th column and the
      1-dof td block is a kept block, as the extrinsic is under every option (the solver may hold it constant; the reference's prior carries it anyway).
  flag 1 (MARGIN_SECOND_NEW, estimator.cpp:1160-1200): the only factor is the prior (w.prior.J0(), ev.prior_r); dropped = the pose block of frame
      WINDOW_SIZE - 1.  Returns None when the prior has no such block: the product then hands the prior back unchanged.
  cols name the kept columns in a fixed layout and in the window's ORIGINAL frame numbering: 15 f + k for frame f, EX + k, TD.
  The FP64 entries of the evaluation dump and of the prior's J0 enter mpf exactly.  Partial-pivoted Gaussian elimination; asserted: every kept diagonal is
  positive and no pivot of the dropped block is at or below 100 eps, eps = 1e-8 being the reference's eigenvalue cut -- so the cut's semantics stay out of
  this form (reference_with_cut is the form for a window on which the cut acts: the reference's own rule at 60 digits, mp.eigsy of A_mm, eigenvalues <= 1e-8
  cut, pseudo-inverse; it wants no eigenvalue of A_mm in [1e-10, 1e-6], so that the cut is unambiguous in FP64).

fp64_level(w, ev, flag, opts) -> (lH, lb, detail): what plain numpy FP64 reaches on the same operation, the larger of two restatements
  (a) pivoted Gaussian elimination of the FP64-assembled system, (b) Cholesky block elimination in the product's order, landmark blocks first and then the
  frame block -- each followed by the finish the reference prescribes (marginalization_factor.cpp:265-297): eigh, eigenvalues <= 1e-8 cut,
  J0 = sqrt(S) V^T, r0 = sqrt(S)^-1 V^T b, and back to (J0^T J0, J0^T r0).

The metric (compare): with d_i = sqrt(A_ii) of the reference
    eH = max_ij |H_ij - A_ij| / (d_i d_j)            eb = max_i (|b_i - b*_i| / d_i) / max_i (|b*_i| / d_i)
plus eH per pair of blocks (frame 0..10, 'ex', 'td'), so that a failure names its block.  The bound (bound): e <= max(1e-13, 10 x fp64_level), for H and b
separately -- the rule of tests/test_gpu_lm_step.py.  Ten covers another summation order and FMA contraction, not another algorithm.
Not pinned: the rank decision at the eps cut and the cost constant r0.r0 (the kept systems carry eigenvalues next to 1e-8; which side they fall on is a
round-off decision in every implementation, and the information form moves by 2e-8 absolute with it)."""
import hashlib

import numpy as np
import mpmath as mp

DPS = 60
NF = 11                      # frames of a window (WINDOW_SIZE + 1)
F = 15 * NF                  # the frame columns
EX, TD, NCOLS = F, F + 6, F + 7
KIND_POSE, KIND_SPEEDBIAS, KIND_EX, KIND_TD = range(4)      # uvs_prior.block_kind (tests/test_marg_ref.py holds them against abi)
EPS = 1e-8                   # the reference's eigenvalue cut
PIVOT_FLOOR = 100 * EPS
FLOOR = 1e-13

_cache = {}

_to_mpf = np.frompyfunc(lambda x: mp.mpf(float(x)), 1, 1)


def _mp_zeros(shape):
    a = np.empty(shape, object); a[...] = mp.mpf(0)
    return a


def _to_float(a):
    a = np.asarray(a)
    return np.array([float(x) for x in a.ravel()], np.float64).reshape(a.shape)


MPF = (lambda x: _to_mpf(np.asarray(x, np.float64)), _mp_zeros)
F64 = (lambda x: np.asarray(x, np.float64), lambda shape: np.zeros(shape))


def _td_on(opts):
    return bool(getattr(opts, "estimate_td", 0)) if opts is not None else False


def _prior_columns(p, P0):
    """(columns in the working layout [frames | landmarks | ex | td], columns of J0) of the prior's blocks; a 7-wide pose block has 6 local columns."""
    base = {KIND_POSE: lambda fr: 15 * fr, KIND_SPEEDBIAS: lambda fr: 15 * fr + 6, KIND_EX: lambda fr: P0, KIND_TD: lambda fr: P0 + 6}
    cols, src = [], []
    for b in range(p.n_blocks):
        kind, fr, size, idx = int(p.block_kind[b]), int(p.block_frame[b]), int(p.block_size[b]), int(p.block_idx[b])
        loc = 6 if size == 7 else size
        cols += [base[kind](fr) + k for k in range(loc)]; src += [idx + k for k in range(loc)]
    return cols, src


def assemble(w, ev, flag, opts, arith):
    """(H, g, dropped columns, kept columns, names of the kept columns) with H = sum J^T J, g = sum J^T r in the arithmetic `arith` (MPF or F64)."""
    conv, zeros = arith
    Np, Nl = len(w.inv_depth), len(w.line_orth)
    P0 = F + Np + 4 * Nl
    ex, td, P = P0, P0 + 6, P0 + 7
    H = zeros((P, P)); g = zeros(P)

    def add(cols, J, r):
        cols = np.asarray(cols); J = conv(J); r = conv(r)
        H[np.ix_(cols, cols)] += J.T @ J
        g[cols] += J.T @ r

    name = lambda c: c if c < F else EX + (c - ex)
    have_prior = w.prior is not None and w.prior.n > 0
    if flag == 1:
        assert have_prior, "MARGIN_SECOND_NEW needs a prior"
        p = w.prior; n = p.n
        cols, src = _prior_columns(p, P0)
        add(cols, np.asarray(p.J0())[:, src], np.asarray(ev.prior_r)[:n])
        lo = 15 * (NF - 2)
        md = [c for c in cols if lo <= c < lo + 6]
        kp = [c for c in cols if not lo <= c < lo + 6]
        return H, g, md, kp, [name(c) for c in kp]
    drop = set(range(15))
    if have_prior:
        p = w.prior; n = p.n
        cols, src = _prior_columns(p, P0)
        add(cols, np.asarray(p.J0())[:, src], np.asarray(ev.prior_r)[:n])
    for b, blk in enumerate(w.imu):
        if blk["frame_i"] == 0 and not blk.get("skip", 0):
            add(list(range(30)), ev.imu_J[b], ev.imu_r[b])
    for k in range(len(w.pt_lm)):
        fi, fj, lm = int(w.pt_fi[k]), int(w.pt_fj[k]), int(w.pt_lm[k])
        if fi != 0: continue
        cols = list(range(6)) + list(range(15 * fj, 15 * fj + 6)) + list(range(ex, ex + 6)) + [F + lm]
        J = np.asarray(ev.pt_J[k], np.float64)
        if _td_on(opts):
            cols = cols + [td]; J = np.concatenate([J, np.asarray(ev.pt_Jtd[k], np.float64).reshape(2, 1)], axis=1)
        add(cols, J, ev.pt_r[k]); drop.add(F + lm)
    start = {}
    for k in range(len(w.ln_lm)): start.setdefault(int(w.ln_lm[k]), int(w.ln_fj[k]))
    for k in range(len(w.ln_lm)):
        fj, lm = int(w.ln_fj[k]), int(w.ln_lm[k])
        if start[lm] != 0 or fj == 0: continue
        lc = F + Np + 4 * lm
        cols = list(range(15 * fj, 15 * fj + 6)) + list(range(lc, lc + 4))
        add(cols, ev.ln_J[k], ev.ln_r[k])
        if w.ln_has_vp[k]: add(cols, ev.vp_J[k], ev.vp_r[k])
        drop.update(range(lc, lc + 4))
    used = [c for c in range(P) if H[c, c] != 0]
    md = [c for c in used if c in drop]; kp = [c for c in used if c not in drop]
    assert all(c < F or c >= ex for c in kp)
    return H, g, md, kp, [name(c) for c in kp]


def schur_pivoted(H, g, md, kp, pivot_floor=None):
    """Schur complement over kp by Gaussian elimination of the md block with partial pivoting, in the arithmetic of H."""
    Amm = H[np.ix_(md, md)].copy(); R = np.concatenate([H[np.ix_(md, kp)], g[md][:, None]], axis=1).copy()
    m = len(md)
    for c in range(m):
        piv = c + int(np.argmax(np.abs(Amm[c:, c])))
        if piv != c: Amm[[c, piv]] = Amm[[piv, c]]; R[[c, piv]] = R[[piv, c]]
        if pivot_floor is not None:
            assert abs(Amm[c, c]) > pivot_floor, "pivot %d of the dropped block is %.3g: the reference's eps cut would act here (reference_with_cut)" % (c, float(abs(Amm[c, c])))
        f = Amm[c + 1:, c] / Amm[c, c]
        Amm[c + 1:] -= f[:, None] * Amm[c][None, :]; R[c + 1:] -= f[:, None] * R[c][None, :]
    X = np.zeros_like(R)
    for c in range(m - 1, -1, -1):
        X[c] = (R[c] - Amm[c, c + 1:] @ X[c + 1:]) / Amm[c, c]
    Hkm = H[np.ix_(kp, md)]
    return H[np.ix_(kp, kp)] - Hkm @ X[:, :-1], g[kp] - Hkm @ X[:, -1]


def _key(w, ev, flag, opts, tag):
    h = hashlib.sha1()
    h.update(repr((tag, int(flag), _td_on(opts), len(w.inv_depth), len(w.line_orth))).encode())
    arrays = [w.pt_fi, w.pt_fj, w.pt_lm, w.ln_fj, w.ln_lm, w.ln_has_vp, ev.pt_J, ev.pt_r, ev.ln_J, ev.ln_r, ev.vp_J, ev.vp_r, ev.imu_J, ev.imu_r]
    if _td_on(opts): arrays.append(ev.pt_Jtd)
    if w.prior is not None and w.prior.n > 0:
        p = w.prior; nb = p.n_blocks
        arrays += [p.J0(), np.asarray(ev.prior_r)[:p.n]] + [np.asarray(getattr(p, f)[:nb]) for f in ("block_kind", "block_frame", "block_size", "block_idx")]
    for a in arrays: h.update(np.ascontiguousarray(a).tobytes()); h.update(b"|")
    h.update(repr([(blk["frame_i"], blk.get("skip", 0)) for blk in w.imu]).encode())
    return h.hexdigest()


def _has_block_to_drop(w):
    p = w.prior
    return any(int(p.block_kind[b]) == KIND_POSE and int(p.block_frame[b]) == NF - 2 for b in range(p.n_blocks))


def reference(w, ev, flag, opts=None):
    if flag == 1 and not _has_block_to_drop(w): return None
    key = _key(w, ev, flag, opts, "reference")
    if key not in _cache:
        with mp.workdps(DPS):
            H, g, md, kp, cols = assemble(w, ev, flag, opts, MPF)
            A, b = schur_pivoted(H, g, md, kp, pivot_floor=mp.mpf(PIVOT_FLOOR))
            assert all(A[i, i] > 0 for i in range(len(kp))), "a kept diagonal of the Schur complement is not positive"
            _cache[key] = (_to_float(A), _to_float(b), cols)
    A, b, cols = _cache[key]
    return A.copy(), b.copy(), list(cols)


def reference_with_cut(w, ev, flag, opts=None):
    """The reference's own rule at 60 digits, for a window on which the eps cut acts (marginalization_factor.cpp:234-243): eigen-decomposition of A_mm,
    eigenvalues <= 1e-8 cut, pseudo-inverse.  -> (A, b, cols, eigenvalues of A_mm as floats)."""
    key = _key(w, ev, flag, opts, "reference_with_cut")
    if key not in _cache:
        with mp.workdps(DPS):
            H, g, md, kp, cols = assemble(w, ev, flag, opts, MPF)
            Amm = mp.matrix(H[np.ix_(md, md)].tolist())
            Amm = (Amm + Amm.T) / 2
            E, Q = mp.eigsy(Amm)
            m = len(md)
            Q = np.array(Q.tolist(), object).reshape(m, m)
            inv = np.array([1 / E[i] if E[i] > mp.mpf(EPS) else mp.mpf(0) for i in range(m)], object)
            Ainv = (Q * inv[None, :]) @ Q.T
            Hkm = H[np.ix_(kp, md)]
            A = H[np.ix_(kp, kp)] - Hkm @ Ainv @ H[np.ix_(md, kp)]
            b = g[kp] - Hkm @ Ainv @ g[md]
            assert all(A[i, i] > 0 for i in range(len(kp)))
            _cache[key] = (_to_float(A), _to_float(b), cols, np.array(sorted(float(E[i]) for i in range(m))))
    A, b, cols, lam = _cache[key]
    return A.copy(), b.copy(), list(cols), lam.copy()


def finish(A, b):
    """The finish the reference prescribes, in plain numpy FP64, and back to the information form."""
    lam, V = np.linalg.eigh(0.5 * (A + A.T))
    keep = lam > EPS
    s = np.sqrt(lam[keep])
    J0 = s[:, None] * V[:, keep].T
    r0 = (V[:, keep].T @ b) / s
    return J0.T @ J0, J0.T @ r0


def _schur_cholesky(H, g, md, kp):
    """Cholesky block elimination in the product's order: the landmark blocks of md (block diagonal) first, then its frame block."""
    lm = [c for c in md if c >= F]; fr = [c for c in md if c < F]
    rest = fr + list(kp)
    S = H[np.ix_(rest, rest)].copy(); v = g[rest].copy()
    if lm:
        L = np.linalg.cholesky(H[np.ix_(lm, lm)])
        Y = np.linalg.solve(L, np.concatenate([H[np.ix_(lm, rest)], g[lm][:, None]], axis=1))
        S -= Y[:, :-1].T @ Y[:, :-1]; v -= Y[:, :-1].T @ Y[:, -1]
    m = len(fr)
    L = np.linalg.cholesky(S[:m, :m])
    Y = np.linalg.solve(L, np.concatenate([S[:m, m:], v[:m, None]], axis=1))
    return S[m:, m:] - Y[:, :-1].T @ Y[:, :-1], v[m:] - Y[:, :-1].T @ Y[:, -1]


def _group(c):
    return c // 15 if c < F else "ex" if c < TD else "td"


def compare(H, b, cols, ref):
    """The scaled errors of (H, b) over the columns `cols` against ref = (A, b*, cols*): dict(eH, eb, blocks = {(group, group): eH of that block pair})."""
    A, br, kp = ref
    assert sorted(cols) == sorted(kp), ("kept columns differ", sorted(set(cols) ^ set(kp)))
    perm = [list(cols).index(c) for c in kp]
    H = np.asarray(H, np.float64)[np.ix_(perm, perm)]; b = np.asarray(b, np.float64)[perm]
    d = np.sqrt(np.diag(A))
    E = np.abs(H - A) / np.outer(d, d)
    eb = float(np.abs((b - br) / d).max() / np.abs(br / d).max())
    grp = [_group(c) for c in kp]
    names = sorted(set(grp), key=lambda x: (isinstance(x, str), x))
    idx = {n: [i for i, x in enumerate(grp) if x == n] for n in names}
    blocks = {(p, q): float(E[np.ix_(idx[p], idx[q])].max()) for i, p in enumerate(names) for q in names[i:]}
    return dict(eH=float(E.max()), eb=eb, blocks=blocks)


def bound(level):
    return max(FLOOR, 10 * level)


def fp64_level(w, ev, flag, opts=None, cut=False):
    """(level of H, level of b, {form: compare(...)}) of the two FP64 restatements against reference.
    cut=True: against reference_with_cut, for a window whose dropped POINT landmarks include some with information <= 1e-8; the two forms apply the cut where it acts,
    per landmark block (a 1 x 1 block at or under eps has pseudo-inverse 0: the landmark leaves the system), and eliminate the rest as always."""
    key = _key(w, ev, flag, opts, "fp64_level, cut" if cut else "fp64_level")
    if key not in _cache:
        ref = reference_with_cut(w, ev, flag, opts)[:3] if cut else reference(w, ev, flag, opts)
        H, g, md, kp, cols = assemble(w, ev, flag, opts, F64)
        if cut:
            weak = [c for c in md if F <= c < F + len(w.inv_depth) and H[c, c] <= EPS]
            assert weak and all(H[c, c] > EPS for c in md if c not in weak)
            md = [c for c in md if c not in weak]
        forms = {"pivoted": schur_pivoted(H, g, md, kp), "cholesky": _schur_cholesky(H, g, md, kp)}
        detail = {}
        for nm, (A, b) in forms.items():
            detail[nm] = compare(*finish(A, b), cols, ref)
            detail[nm + ", before the finish"] = compare(A, b, cols, ref)
        lH = max(detail[nm]["eH"] for nm in forms); lb = max(detail[nm]["eb"] for nm in forms)
        _cache[key] = (lH, lb, detail)
    return _cache[key]


def format_blocks(cmp, bH):
    """'e / bound' per block pair, worst first (the printout a failing case is read by)."""
    rows = sorted(cmp["blocks"].items(), key=lambda kv: -kv[1])
    return " ".join("%s-%s:%.2g" % (p, q, e / bH) for (p, q), e in rows[:8])
