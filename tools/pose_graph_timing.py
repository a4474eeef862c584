"""Call latency of uvs_pg_optimize (the 4-DoF pose-graph solve of loop closure) for N keyframes x L loop edges.

Each call is synchronous (upload, every LM iteration with its per-iteration scalar read-back, download), so a host clock around it is a
device-synchronized time.  Problems are synthetic and seeded: a drifted multi-lap circuit of N keyframes, one sequence, keyframe 0 constant,
and L loop edges between keyframes one lap apart (true relative pose plus small noise).  The kernel breakdown comes from a separate run
under `rocprofv3 --kernel-trace --stats`.

    python tools/pose_graph_timing.py [--reps 10] [--sizes 250,1000,4000,16000] [--loops 16,64,256] [--out results.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
uvs = importlib.import_module("uv-slam_amd")
import pg_ref  # noqa: E402


def problem(n, n_loops, seed=0, per_lap=None):
    per_lap = per_lap or max(20, min(200, n // 4))       # a lap: 200 keyframes, shorter for small N so that the loops fit
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    ang = 2 * np.pi * k / per_lap
    rad = 5.0 + 0.3 * (k // per_lap)
    p = np.stack([rad * np.cos(ang), rad * np.sin(ang), 0.2 * np.sin(3 * ang)], 1)
    yaw = np.degrees(ang) + 90.0
    R = pg_ref.ypr2R(yaw, rng.normal(0, 1, n), rng.normal(0, 1, n))
    psi = np.cumsum(rng.normal(0, 0.05, n)); dt = np.cumsum(rng.normal(0, 0.003, (n, 3)), 0)
    pv, Rv = p.copy(), R.copy()
    for i in range(1, n):
        Rz = pg_ref.ypr2R(psi[i], 0.0, 0.0)
        pv[i] = pv[i - 1] + Rz @ (p[i] - p[i - 1]) + dt[i] - dt[i - 1]; Rv[i] = Rz @ R[i]
    ypr = pg_ref.R2ypr(R)
    cur = np.sort(rng.choice(np.arange(per_lap, n), size=min(n_loops, n - per_lap), replace=False))
    loops = []
    for c in cur:
        o = int(c - per_lap * rng.integers(1, c // per_lap + 1))
        loops.append((int(c), o, R[o].T @ (p[c] - p[o]) + rng.normal(0, 0.01, 3), float(pg_ref.normalize_angle(ypr[c, 0] - ypr[o, 0]))))
    const = np.zeros(n, np.int32); const[0] = 1
    return pv, pg_ref.R_to_quat(Rv), np.ones(n, np.int32), const, loops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="250,1000,4000,16000")
    ap.add_argument("--loops", default="16,64,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(v) for v in a.sizes.split(",")]; lps = [int(v) for v in a.loops.split(",")]
    pg = uvs.api.PoseGraphSolver(max_keyframes=max(sizes), max_loops=max(lps))
    rows = []
    for n in sizes:
        for L in lps:
            t, q, seq, const, loops = problem(n, L)
            for _ in range(2):                      # warm-up: code objects, first-touch of the buffers
                pg.optimize(t, q, seq, const, loops)
            ms = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                _, rep = pg.optimize(t, q, seq, const, loops)
                ms.append((time.perf_counter() - t0) * 1e3)
            row = dict(n=n, loops=len(loops), loop_columns=rep.n_loop_columns, iterations=rep.num_iterations, median_ms=float(np.median(ms)),
                       min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), ms_per_iteration=float(np.median(ms) / max(rep.num_iterations, 1)))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
