"""The 4-DoF pose-graph optimizer of loop closure (uvs_pg_*, csrc/uvs_pose_graph.hip) against tests/pg_ref.py, the numpy restatement of
PoseGraph::optimize4DoF (reference pose_graph/src/pose_graph.cpp:403-579).

CPU tests pin pg_ref itself (Jacobians, a known-answer graph, constant blocks) and the C ABI surface; GPU tests check that the device path
takes the same LM decisions and lands on the same poses, is deterministic, and corrects the drift of an MH_05 trajectory."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pg_cases as pc
import pg_ref
from helpers import abi, uvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- pg_ref (CPU)
def _random_problem(rng, n=6, loops=None, yaw_scale=1.0):
    t = rng.normal(0, 2, (n, 3))
    q = pg_ref.R_to_quat(np.stack([pg_ref.ypr2R(rng.uniform(-180, 180) * yaw_scale, rng.normal(0, 5), rng.normal(0, 5)) for _ in range(n)]))
    const = np.zeros(n, np.int32); const[0] = 1
    return pg_ref.Problem(t, q, np.ones(n, np.int32), const, loops or [])


def _central(pb, x, f, h=1e-6):
    """d f(x) / d x[keyframe of edge side, k] by central differences, per edge: [E, ..., 8]."""
    out = None
    for side, idx in ((0, pb.a), (1, pb.b)):
        for k in range(4):
            for e in range(len(pb.a)):
                xp, xm = x.copy(), x.copy()
                xp[idx[e], k] += h; xm[idx[e], k] -= h
                d = (f(xp)[e] - f(xm)[e]) / (2 * h)
                if out is None:
                    out = np.zeros((len(pb.a),) + np.shape(d) + (8,))
                out[e, ..., 4 * side + k] = d
    return out


@pytest.mark.parametrize("case", ["inlier", "huber", "wrap"])
def test_pg_ref_jacobian_matches_central_differences(case):
    rng = np.random.default_rng(11)
    if case == "inlier":
        pb = _random_problem(rng, loops=[(5, 1, [0.01, -0.02, 0.0], 0.1)])
        pb.rel_t[:] = pg_ref.residuals(pb, pb.x0, jacobian=False)[0][:, :3] * 0 + pb.rel_t     # measurements as built
        x = pb.x0 + rng.normal(0, 1e-3, pb.x0.shape)
        x[pb.b[pb.loop], 1:] = x[pb.a[pb.loop], 1:]         # loop edge near its measurement: inside the Huber threshold
        x[pb.b[pb.loop], 0] = x[pb.a[pb.loop], 0] + 0.1
    elif case == "huber":
        pb = _random_problem(rng, loops=[(5, 1, [3.0, -2.0, 1.0], 40.0), (4, 2, [0.5, 0.5, 0.5], -20.0)])
        x = pb.x0 + rng.normal(0, 0.3, pb.x0.shape)
    else:
        pb = _random_problem(rng, loops=[(5, 0, [0.3, 0.1, 0.0], 175.0)])
        x = pb.x0.copy()
        x[:, 0] = [179.5, -179.0, 178.0, -178.5, 179.9, -179.7]      # yaws across +-180: every difference wraps
    r, J, cost = pg_ref.residuals(pb, x)
    if case == "huber":
        s = (pg_ref.residuals(pb, x, jacobian=False)[0] ** 2).sum(1)
        assert (pb.loop & (s > 0.01)).sum() == 2       # both loop edges on the outer branch
    if case == "wrap":
        raw = x[pb.b, 0] - x[pb.a, 0] - pb.rel_yaw
        assert np.any(np.abs(raw) > 180)
    # the functor's own Jacobian against central differences of its residual
    r_raw, J_raw, _ = pg_ref.residuals(pb, x, robust=False)
    Jn = _central(pb, x, lambda xx: pg_ref.residuals(pb, xx, jacobian=False, robust=False)[0])
    assert np.allclose(J_raw, Jn, rtol=1e-6, atol=1e-7), np.abs(J_raw - Jn).max()
    # the corrected pair (Ceres' corrector, rho'' <= 0: sqrt(rho') scaling) gives the exact gradient of the edge cost 0.5 rho(s)
    gn = _central(pb, x, lambda xx: pg_ref.residuals(pb, xx, jacobian=False)[2])
    assert np.allclose(np.einsum("eik,ei->ek", J, r), gn, rtol=1e-5, atol=1e-8), np.abs(np.einsum("eik,ei->ek", J, r) - gn).max()
    assert np.allclose(J / np.linalg.norm(J, axis=(1, 2), keepdims=True), J_raw / np.linalg.norm(J_raw, axis=(1, 2), keepdims=True))


def test_pg_ref_known_answer_square_loop():
    """A closed square of 16 keyframes.  The first side (keyframes 0-3) is a constant base sequence at its true place; the other three
    sides (sequence 1) carry a pure yaw + translation drift, which is a 4-DoF rigid motion, so their sequential edges are exact.  Loop edges
    4 -> 3 and 15 -> 0 measure the true relative poses: the exact optimum is the true square, with zero cost."""
    n = 16
    side = np.repeat(np.arange(4), 4); s = np.tile(np.arange(4), 4) / 4.0
    corners = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 0]], float)
    p = corners[side] + (corners[side + 1] - corners[side]) * s[:, None]
    yaw = 90.0 * side
    R = pg_ref.ypr2R(yaw, 0.0, 0.0)
    Rd, td = pg_ref.ypr2R(7.0, 0.0, 0.0), np.array([0.3, -0.2, 0.05])
    pv, Rv = p.copy(), R.copy()
    pv[4:] = (Rd @ p[4:].T).T + td; Rv[4:] = Rd @ R[4:]
    true_rel = lambda k, j: (k, j, R[j].T @ (p[k] - p[j]), float(pg_ref.normalize_angle(yaw[k] - yaw[j])))
    seq = (np.arange(n) >= 4).astype(np.int32)
    const = (seq == 0).astype(np.int32)
    x, tr = pg_ref.optimize(pv, pg_ref.R_to_quat(Rv), seq, const, [true_rel(4, 3), true_rel(15, 0)], max_num_iterations=50)
    assert tr.initial_cost > 0.1
    assert tr.final_cost < 1e-12
    assert np.abs(x[:, 1:] - p).max() < 1e-6
    assert np.abs(pg_ref.normalize_angle(x[:, 0] - yaw)).max() < 1e-5


def test_pg_ref_constant_blocks_stay_fixed():
    w = pc.two_sequence_case()
    x, tr = pg_ref.optimize(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
    pb = pg_ref.Problem(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
    c = w["constant"].astype(bool)
    assert c.sum() > 50 and (~c).sum() > 50
    assert np.array_equal(x[c], pb.x0[c])
    assert np.abs(x[~c] - pb.x0[~c]).max() > 0.1
    assert tr.num_iterations >= 1 and tr.final_cost < tr.initial_cost


def test_pg_ref_damped_step_extended_precision():
    """damped_step solves in np.longdouble: it agrees with an FP64 dense solve on a well-conditioned system, and its residual is at the
    extended type's level, far below what FP64 can reach."""
    assert np.finfo(np.longdouble).eps < 1e-18
    w = pc.sized_case(33, 1)
    pb = pg_ref.Problem(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
    M, b, s = pg_ref.damped_system(pb, 1e4)
    assert np.linalg.cond(M) < 1e6
    d = pg_ref.damped_step(pb, 1e4)
    assert d.dtype == np.longdouble and d.shape == (4 * 33,)
    d64 = s * np.linalg.solve(M, b)
    assert np.linalg.norm(d64 - d.astype(np.float64)) <= 1e-13 * np.linalg.norm(d.astype(np.float64))
    y = pg_ref.solve_ld(M, b)
    res = np.asarray(b, np.longdouble) - np.asarray(M, np.longdouble) @ y
    assert float(np.linalg.norm(res) / np.linalg.norm(b)) <= 1e-17


def test_pg_case_structures():
    """Each generator builds the structure its name promises, so the GPU tests below keep testing what they claim to."""
    # constants inside the free run: band pairs whose keyframe distance j differs from the free-index distance d
    w = pc.interleaved_constants_case(); st = pc.structure(w)
    const = w["constant"].astype(bool)
    assert const[0] and const[1:].sum() == 2 + 2 + 3 + 4 + 5
    assert sum(1 for _, d, j in st["band_pairs"] if j != d) >= 10
    assert {j - d for _, d, j in st["band_pairs"]} >= {0, 1, 2, 3}
    assert st["nu"] > 0
    # three sequences: sequence 2 free, no constant keyframe and no loop with one free end; anchored through U columns only
    w = pc.three_sequence_case(); st = pc.structure(w)
    seq, const = w["sequence"], w["constant"].astype(bool)
    assert set(seq.tolist()) == {1, 2} and np.flatnonzero(const).tolist() == [0]
    s2 = seq == 2
    assert not const[s2].any()
    touching = [(k, j) for k, j, _, _ in w["loops"] if s2[k] or s2[j]]
    assert len(touching) == 10 and all(s2[k] and seq[j] == 1 for k, j in touching)
    assert st["nu"] == 10 and st["n_loop_columns"] == 40
    assert all(seq[free_a] == seq[free_b] for free_a, free_b in [(np.flatnonzero(~const)[a], np.flatnonzero(~const)[a - d]) for a, d, _ in st["band_pairs"]])
    # band overlap: loop ends 1..4 keyframes apart, a shared old keyframe, a duplicated loop
    w = pc.band_overlap_case(); st = pc.structure(w)
    gaps = {k - j for k, j in st["two_free"]}
    assert {1, 2, 3, 4} <= gaps
    olds = [j for _, j in st["two_free"]]
    assert max(olds.count(j) for j in set(olds)) >= 4
    assert len(set(st["two_free"])) < len(st["two_free"])
    assert any(w["constant"][j] for _, j, _, _ in w["loops"])
    # sized cases: exactly nf free keyframes and nu loops with two free ends
    for nf, nu in SIZED_STEP + [(222, 256)]:
        st = pc.structure(pc.sized_case(nf, nu))
        assert st["nf"] == nf and st["nu"] == nu and st["n_loop_columns"] == 4 * nu
    ncols = lambda nu: ((4 * nu + 1 + 63) // 64) * 64
    assert ncols(16) == 128 and (4 * 16) % 64 == 0           # the -g column alone in its tile
    assert ncols(256) == 1088                                 # k_pg_capsolve's LDS capacity
    # all constant
    st = pc.structure(pc.all_constant_case())
    assert st["nf"] == 0 and st["nu"] == 0


# ---------------------------------------------------------------- C ABI surface (CPU)
PG_SYMBOLS = ["uvs_pg_create", "uvs_pg_destroy", "uvs_pg_last_error", "uvs_pg_optimize", "uvs_pg_debug_step"]


def test_pose_graph_symbols_exported():
    lib = uvs.api.lib()
    for n in PG_SYMBOLS:
        assert hasattr(lib, n), n
    assert lib.uvs_abi_version() == 7


def test_pose_graph_struct_layouts_match_the_header():
    code = r'''
#include <stdio.h>
#include <stddef.h>
#include "uvs_solver.h"
int main(void) {
  printf("%zu %zu %zu\n", sizeof(uvs_pg_loop), sizeof(uvs_pg_problem), sizeof(uvs_pg_report));
  printf("%zu %zu %zu %zu\n", offsetof(uvs_pg_problem, loops), offsetof(uvs_pg_report, initial_cost), offsetof(uvs_pg_report, radius), offsetof(uvs_pg_report, accepted));
  printf("%d %d\n", UVS_PG_MAX_KEYFRAMES, UVS_PG_MAX_LOOPS);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c"); exe = os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert out[:3] == [C.sizeof(abi.PgLoop), C.sizeof(abi.PgProblem), C.sizeof(abi.PgReport)]
    assert out[3:7] == [abi.PgProblem.loops.offset, abi.PgReport.initial_cost.offset, abi.PgReport.radius.offset, abi.PgReport.accepted.offset]
    assert out[7:] == [abi.PG_MAX_KEYFRAMES, abi.PG_MAX_LOOPS]


def test_pose_graph_create_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        uvs.api.PoseGraphSolver()


# ---------------------------------------------------------------- GPU
def _check_parity(w, pg=None):
    pg = pg or uvs.api.PoseGraphSolver(max_keyframes=max(len(w["t"]), 16), max_loops=max(len(w["loops"]), 1))
    out, rep = pg.optimize(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
    x, tr = pg_ref.optimize(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
    assert rep.status == abi.UVS_OK
    assert rep.num_iterations == tr.num_iterations, (rep.trace()["accepted"], tr.accepted)
    assert list(rep.trace()["accepted"]) == tr.accepted
    assert rep.termination == tr.termination
    assert abs(rep.initial_cost - tr.initial_cost) <= 1e-9 * max(tr.initial_cost, 1e-300) + 1e-18
    assert abs(rep.final_cost - tr.final_cost) <= 1e-9 * max(tr.final_cost, 1e-300) + 1e-18, (rep.final_cost, tr.final_cost)
    # every iteration's cost, candidate cost, model cost change and radius (entry 0 = the initial evaluation)
    trace = rep.trace()
    for key in ("cost", "candidate_cost", "model_cost_change", "radius"):
        ref = np.asarray(getattr(tr, key), dtype=np.float64)
        assert len(ref) == tr.num_iterations + 1, key
        assert np.all(np.abs(trace[key] - ref) <= 1e-9 * np.abs(ref) + 1e-18), (key, trace[key], ref)
    assert np.abs(out[:, 1:] - x[:, 1:]).max() < 1e-7
    assert np.abs(pg_ref.normalize_angle(out[:, 0] - x[:, 0])).max() < 1e-6
    return out, rep


@pytest.mark.gpu
def test_gpu_pose_graph_parity_mh05_2hz():
    w = pc.mh05_case(2.0)
    assert len(w["t"]) == 223 and len(w["loops"]) == 34
    out, rep = _check_parity(w)
    assert pc.positions_ate(out[:, 1:], w["p_true"]) < 0.7 * pc.positions_ate(w["t"], w["p_true"])


@pytest.mark.gpu
def test_gpu_pose_graph_parity_mh05_10hz():
    w = pc.mh05_case(10.0)
    assert len(w["t"]) == 1111 and len(w["loops"]) == 169
    out, rep = _check_parity(w)
    assert rep.n_loop_columns == 4 * 169 - 4 * sum(1 for k, j, _, _ in w["loops"] if j == 0)
    assert pc.positions_ate(out[:, 1:], w["p_true"]) < 0.7 * pc.positions_ate(w["t"], w["p_true"])


@pytest.mark.gpu
def test_gpu_pose_graph_parity_two_sequences():
    w = pc.two_sequence_case()
    out, rep = _check_parity(w)
    c = w["constant"].astype(bool)
    pb = pg_ref.Problem(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
    assert np.array_equal(out[c, 1:], w["t"][c])       # the base sequence does not move: t bit for bit,
    assert np.abs(out[c, 0] - pb.x0[c, 0]).max() < 1e-12   # yaw = R2ypr of the input (device atan2 against numpy's: rounding)


@pytest.mark.gpu
def test_gpu_pose_graph_parity_outliers():
    w = pc.mh05_case(2.0, outliers=6)
    pb = pg_ref.Problem(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
    s = (pg_ref.residuals(pb, pb.x0, jacobian=False)[0] ** 2).sum(1)
    assert (pb.loop & (s > 0.01)).sum() >= 6           # Huber's outer branch is active
    _check_parity(w)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_free", "loop_to_constant", "yaw_wrap", "no_loops"])
def test_gpu_pose_graph_edge_cases(name):
    if name == "one_free":
        w = pc.chain_case(2, 7, n_loops=1)
    elif name == "loop_to_constant":
        w = pc.chain_case(12, 8, n_loops=1)               # the loop's old end is keyframe 0, the constant one
        assert w["loops"][0][1] == 0
    elif name == "yaw_wrap":
        w = pc.chain_case(24, 9, yaw0=170.0)
    else:
        w = pc.chain_case(20, 10); w["loops"] = []
    assert (w["constant"] == 0).sum() >= 1
    _check_parity(w)


@pytest.mark.gpu
def test_gpu_pose_graph_is_deterministic():
    w = pc.mh05_case(10.0)
    pg = uvs.api.PoseGraphSolver(max_keyframes=2048, max_loops=256)
    a, ra = pg.optimize(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
    b, rb = pg.optimize(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
    assert a.tobytes() == b.tobytes()
    assert bytes(ra) == bytes(rb)


@pytest.mark.gpu
def test_gpu_pose_graph_argument_checks():
    w = pc.chain_case(12, 8)
    pg = uvs.api.PoseGraphSolver(max_keyframes=12, max_loops=2)
    rc, _, _ = pg.optimize_raw(w["t"], w["q"], w["sequence"], w["constant"], [(3, 5, [0, 0, 0], 0.0)])      # old > cur
    assert rc == abi.UVS_ERR_INVALID_ARG
    rc, _, _ = pg.optimize_raw(w["t"], w["q"], w["sequence"], w["constant"], [(12, 0, [0, 0, 0], 0.0)])     # outside the problem
    assert rc == abi.UVS_ERR_INVALID_ARG
    rc, _, _ = pg.optimize_raw(w["t"], w["q"], w["sequence"], w["constant"], [(5, 0, [0, 0, 0], 0.0)] * 3)  # 3 loops > capacity 2
    assert rc == abi.UVS_ERR_CAPACITY
    big = pc.chain_case(13, 8)
    rc, _, _ = pg.optimize_raw(big["t"], big["q"], big["sequence"], big["constant"], big["loops"])
    assert rc == abi.UVS_ERR_CAPACITY
    rc, _, _ = pg.optimize_raw(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])                    # the handle still works
    assert rc == abi.UVS_OK


# ---------------------------------------------------------------- one damped solve against the extended-precision reference (GPU)
STEP_RADII = [1e-2, 1.0, 1e4, 8.1e5]            # 8.1e5 = 1e4 * 3^4: the largest radius the LM controller reaches in five iterations
# (nf, nu): the 32-row chunk edges of k_pg_factor / k_pg_back, the 64-column U tiles (16 loops: the -g column alone in its tile), capacity
SIZED_STEP = [(1, 0), (2, 1), (3, 0), (4, 15), (5, 16), (31, 17), (32, 0), (33, 1), (36, 16), (37, 64), (64, 17), (65, 15), (65, 256),
              (222, 0), (222, 256)]


def _step_cases():
    cases = {"interleaved_constants": pc.interleaved_constants_case, "three_sequence": pc.three_sequence_case,
             "band_overlap": pc.band_overlap_case, "mh05_2hz": lambda: pc.mh05_case(2.0), "outliers": lambda: pc.mh05_case(2.0, outliers=6),
             "two_sequences": pc.two_sequence_case}
    cases.update({f"sized_{nf}_{nu}": (lambda nf=nf, nu=nu: pc.sized_case(nf, nu)) for nf, nu in SIZED_STEP})
    return cases


STEP_CASES = _step_cases()


@pytest.fixture(scope="module")
def pg_big():
    pg = uvs.api.PoseGraphSolver(max_keyframes=2048, max_loops=256)
    yield pg
    pg.close()


def _dense_fp64_error(M, b, s, ref):
    """Relative error of FP64 dense solves (np.linalg.solve) of the same system, the largest over three elimination orders of the unknowns
    (natural, reversed, one fixed shuffle): one order alone can land far below the usual level by luck of rounding."""
    m = len(b)
    worst = 0.0
    for perm in (np.arange(m), np.arange(m)[::-1], np.random.default_rng(0).permutation(m)):
        y = np.empty(m)
        y[perm] = np.linalg.solve(M[np.ix_(perm, perm)], b[perm])
        worst = max(worst, np.linalg.norm(s * y - ref) / np.linalg.norm(ref))
    return worst


def _check_step(pg, w, radii):
    """uvs_pg_debug_step against pg_ref.damped_step: relative error <= max(10 x the error of an FP64 dense solve of the same system, 1e-12).
    The floor is that of the linearization, not of the solve: the device and numpy round the residuals of the sequential edges at the initial
    poses (exact cancellations, ~1e-16 m) differently, so the two systems differ in g at that level; at small radii the step is about
    radius D^-1 g, and the two steps differ by up to ~2e-13 relative (MI355X, no loop column at all) however exact the solves."""
    pb = pg_ref.Problem(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
    st = pc.structure(w)
    rows = []
    for radius in radii:
        delta, info = pg.debug_step(w["t"], w["q"], w["sequence"], w["constant"], w["loops"], radius)
        assert info["factor_fail"] == 0 and info["capacitance_fail"] == 0, (radius, info)
        assert info["n_free"] == st["nf"] and info["n_loop_columns"] == st["n_loop_columns"]
        M, b, s = pg_ref.damped_system(pb, radius)
        ref = (s.astype(np.longdouble) * pg_ref.solve_ld(M, b)).astype(np.float64)
        err = np.linalg.norm(delta - ref) / np.linalg.norm(ref)
        err64 = _dense_fp64_error(M, b, s, ref)
        rows.append((radius, err, err64))
        assert err <= max(10.0 * err64, 1e-12), (radius, err, err64)
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STEP_CASES))
def test_gpu_pose_graph_step_matches_extended_reference(pg_big, name):
    _check_step(pg_big, STEP_CASES[name](), STEP_RADII)


@pytest.mark.gpu
def test_gpu_pose_graph_step_three_sequences_large_radius(pg_big):
    """Sequence 2 hangs on U alone: cond(A) grows with the radius while cond(A + U U^T + D / radius) does not.  The plain Woodbury solve
    loses accuracy in proportion to cond(A); the refinement step must hold the dense-solve level."""
    _check_step(pg_big, pc.three_sequence_case(), [1e8, 1e10, 1e12])


@pytest.mark.gpu
def test_gpu_pose_graph_step_argument_checks(pg_big):
    w = pc.sized_case(5, 1)
    for radius in (0.0, -1.0, float("inf"), float("nan")):
        rc, _, _ = pg_big.debug_step_raw(w["t"], w["q"], w["sequence"], w["constant"], w["loops"], radius)
        assert rc == abi.UVS_ERR_INVALID_ARG, radius
    rc, _, _ = pg_big.debug_step_raw(w["t"], w["q"], w["sequence"], w["constant"], [(3, 5, [0, 0, 0], 0.0)], 1e4)
    assert rc == abi.UVS_ERR_INVALID_ARG
    rc, delta, scal = pg_big.debug_step_raw(w["t"], w["q"], w["sequence"], w["constant"], w["loops"], 1e4)
    assert rc == abi.UVS_OK and len(delta) == 20 and scal[3] == 5 and scal[2] == 4
    a = pc.all_constant_case()
    delta, info = pg_big.debug_step(a["t"], a["q"], a["sequence"], a["constant"], a["loops"], 1e4)
    assert len(delta) == 0 and info["n_free"] == 0


# ---------------------------------------------------------------- full parity of the new structures (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["interleaved_constants", "three_sequence", "band_overlap", "sized_1_0", "sized_33_1", "sized_36_16",
                                  "sized_64_17", "sized_222_256"])
def test_gpu_pose_graph_parity_structures(pg_big, name):
    w = STEP_CASES[name]()
    _, rep = _check_parity(w, pg_big)
    assert rep.n_loop_columns == pc.structure(w)["n_loop_columns"]


@pytest.mark.gpu
def test_gpu_pose_graph_all_constant():
    w = pc.all_constant_case()
    pg = uvs.api.PoseGraphSolver(max_keyframes=16, max_loops=4)
    out, rep = pg.optimize(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
    x, tr = pg_ref.optimize(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
    pb = pg_ref.Problem(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
    assert rep.status == abi.UVS_OK and rep.n_free == 0 and rep.n_edges == 0 and rep.n_loop_columns == 0
    assert rep.num_iterations == 0 and rep.termination == pg_ref.TERM["FUNCTION_TOL"] == tr.termination
    assert np.array_equal(out[:, 1:], w["t"])
    assert np.abs(out[:, 0] - pb.x0[:, 0]).max() < 1e-12
    assert rep.initial_cost == tr.initial_cost == 0.0 and rep.final_cost == tr.final_cost == 0.0


@pytest.mark.gpu
def test_gpu_pose_graph_handle_reuse_is_bitwise_fresh():
    """One handle through problems of different n and ncols (rows of W before a wave's start are never written and stay from the call
    before): every output and report equals that of a fresh handle, bit for bit."""
    seqs = [pc.mh05_case(10.0), pc.chain_case(12, 8), pc.sized_case(40, 0), pc.sized_case(36, 16), pc.mh05_case(10.0)]
    pg = uvs.api.PoseGraphSolver(max_keyframes=2048, max_loops=256)
    for w in seqs:
        a, ra = pg.optimize(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
        fresh = uvs.api.PoseGraphSolver(max_keyframes=2048, max_loops=256)
        b, rb = fresh.optimize(w["t"], w["q"], w["sequence"], w["constant"], w["loops"])
        fresh.close()
        assert a.tobytes() == b.tobytes()
        assert bytes(ra) == bytes(rb)
    # a handle without loop capacity on a problem without loops
    w = pc.chain_case(20, 10); w["loops"] = []
    pg0 = uvs.api.PoseGraphSolver(max_keyframes=32, max_loops=0)
    _check_parity(w, pg0)
