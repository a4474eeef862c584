"""Call latency of uvs_ft_reject (outlier rejection of the point front end: fundamental-matrix RANSAC over 7-point samples) for B items of 150
tracks each, at 10 % and at 50 % gross outliers: the stopping rule ends the loop within the first round of 256 hypotheses at 10 %, and after up
to four rounds at 50 %.

Every item is a seeded scene of tests/fr_cases.py (general motion, 0.3 px of noise at focal length 460), a different seed per item.

Two clocks per call: a host clock around the synchronous call (packing, upload of the points, the kernel, download) and the HIP events the
library records on its stream (uvs_ft_last_reject_device_ms).  The table reports the median of --reps synchronous calls after --warmup calls of
every shape, and the iteration counts seen.

Per-kernel times come from a SEPARATE run of this file under `rocprofv3 --kernel-trace --stats` (no counters in that run; tracing slows the
host, so the table above is taken with the profiler off):

    python tools/feature_reject_timing.py [--items 1,4,16] [--outliers 0.1,0.5] [--reps 50] [--warmup 3] [--out results.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/feature_reject_timing.py --items 1 --reps 50
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
import fr_cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", default="1,4,16")
    ap.add_argument("--outliers", default="0.1,0.5")
    ap.add_argument("--tracks", type=int, default=150)
    ap.add_argument("--noise", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    batches = [int(v) for v in a.items.split(",")]
    shares = [float(v) for v in a.outliers.split(",")]
    S = max(batches)
    ft = uvs.api.FeatureTracker(max_streams=S, max_width=96, max_height=80, levels=1, max_points=a.tracks)
    rows = []
    for share in shares:
        scenes = [fr_cases.scene("general", a.tracks, share, a.noise, 100 + s) for s in range(S)]
        for B in batches:
            items = [dict(prev=sc["prev"], next=sc["next"], seed=sc["seed"]) for sc in scenes[:B]]
            wall, dev, out = [], [], None
            for k in range(a.warmup + a.reps):      # the warm-up: code object load, the first call's allocations
                t0 = time.perf_counter()
                out = ft.reject(items, fr_cases.THRESHOLD, fr_cases.CONFIDENCE)
                if k >= a.warmup:
                    wall.append((time.perf_counter() - t0) * 1e3); dev.append(ft.last_reject_device_ms())
            its = [d["iterations"] for d in out]
            row = dict(items=B, tracks=a.tracks, outlier_share=share, noise_px=a.noise, reps=len(wall), iterations_min=int(min(its)),
                       iterations_max=int(max(its)), rounds_max=int((max(its) + 255) // 256), kept_mean=float(np.mean([d["n_inliers"] for d in out])),
                       wall_median_ms=float(np.median(wall)), wall_min_ms=float(np.min(wall)), wall_max_ms=float(np.max(wall)),
                       device_median_ms=float(np.median(dev)), device_min_ms=float(np.min(dev)), device_max_ms=float(np.max(dev)),
                       device_ms_per_item=float(np.median(dev) / B))
            rows.append(row)
            print(json.dumps(row), flush=True)
    ft.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
