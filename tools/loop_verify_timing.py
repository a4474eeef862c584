"""Call latency of uvs_lc_verify (loop verification: BRIEF matching + PnP-RANSAC of KeyFrame::findConnection) for B pairs x 150 queries x N
old keypoints.

Each call is synchronous (packing into pinned memory, one upload, k_lc_verify, one download), so a host clock around it is a
device-synchronized time; the table reports the median after warm-up.  Pairs are seeded planted pairs from tests/lc_cases.py: 150 window
points of which 120 match consistent geometry and 30 match with random uv, the rest of the old keypoints distractors.  The kernel time comes
from a separate run under `rocprofv3 --kernel-trace --stats`.

    python tools/loop_verify_timing.py [--reps 50] [--batches 1,64] [--olds 500,1000,4000] [--out results.json]
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
import lc_cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--olds", default="500,1000,4000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    batches = [int(v) for v in a.batches.split(",")]; olds = [int(v) for v in a.olds.split(",")]
    v = uvs.api.LoopVerifier(max_pairs=max(batches), max_query=1024, max_old=max(olds))
    tic, qic = lc_cases.extrinsic()
    rows = []
    for n_old in olds:
        base = [lc_cases.planted_pair(100 + s, n_in=120, n_out=30, n_distract=n_old - 150)[0] for s in range(max(batches))]
        for B in batches:
            pairs = base[:B]
            for _ in range(3):                      # warm-up: code object load, first touch of the buffers
                v.verify(pairs, tic, qic)
            ms = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                res, _, _ = v.verify(pairs, tic, qic)
                ms.append((time.perf_counter() - t0) * 1e3)
            row = dict(pairs=B, queries=150, old=n_old, accepted=int(sum(r["accepted"] for r in res)), median_ms=float(np.median(ms)),
                       min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), ms_per_pair=float(np.median(ms) / B))
            rows.append(row)
            print(json.dumps(row), flush=True)
    v.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
