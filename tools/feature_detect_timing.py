"""Call latency of uvs_ft_detect (new points of the point front end: Shi-Tomasi score, mask of the occupied points, candidates, ranking, the
minimum distance, normalized points) for S streams of 752 x 480 with about 100 occupied points each, max_new = 50, min_distance = 30.

Every stream holds a seeded scene of tests/kf_cases.py (stored once by uvs_ft_track; detection uploads no image).  The occupied points are
the first --occupied points uvs_ft_detect itself returns on the scene with min_distance --radius, as a tracker's own points would be; the
timed calls then ask for 50 more.

Two clocks per call: a host clock around the synchronous call (packing, upload of the occupied points, the kernels, download) and the HIP events
the library records on its stream (uvs_ft_last_detect_device_ms).  The table reports the median of --reps synchronous calls after --warmup
calls of every shape, and the candidate counts seen.

Per-kernel times come from a SEPARATE run of this file under `rocprofv3 --kernel-trace --stats` (no counters in that run; tracing slows the
host, so the table above is taken with the profiler off):

    python tools/feature_detect_timing.py [--streams 1,4,16] [--reps 50] [--warmup 3] [--out results.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/feature_detect_timing.py --streams 1 --reps 50
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
import kf_cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,4,16")
    ap.add_argument("--occupied", type=int, default=100)
    ap.add_argument("--max-new", type=int, default=50)
    ap.add_argument("--radius", type=int, default=30)
    ap.add_argument("--quality", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    streams = [int(v) for v in a.streams.split(",")]
    S = max(streams)
    W, H = kf_cases.W, kf_cases.H
    cam = kf_cases.CAM_DIST
    ft = uvs.api.FeatureTracker(max_streams=S, max_width=W, max_height=H, levels=4, max_points=max(a.occupied, a.max_new))
    ft.track([dict(stream=s, image=kf_cases.texture(s)) for s in range(S)], cam)
    first = ft.detect([dict(stream=s, max_new=a.occupied) for s in range(S)], cam, a.quality, a.radius)
    occ = [d["xy"].astype(np.float64) + 0.25 for d in first]      # sub-pixel, as tracked points are
    rows = []
    for B in streams:
        items = [dict(stream=s, occupied=occ[s], max_new=a.max_new) for s in range(B)]
        wall, dev, out = [], [], None
        for k in range(a.warmup + a.reps):          # the warm-up: code object load, the first call's allocations
            t0 = time.perf_counter()
            out = ft.detect(items, cam, a.quality, a.radius)
            if k >= a.warmup:
                wall.append((time.perf_counter() - t0) * 1e3); dev.append(ft.last_detect_device_ms())
        row = dict(streams=B, width=W, height=H, occupied_mean=float(np.mean([len(o) for o in occ[:B]])), max_new=a.max_new, radius=a.radius,
                   reps=len(wall), candidates_min=int(min(d["n_candidates"] for d in out)), candidates_max=int(max(d["n_candidates"] for d in out)),
                   new_mean=float(np.mean([d["n_new"] for d in out])),
                   wall_median_ms=float(np.median(wall)), wall_min_ms=float(np.min(wall)), wall_max_ms=float(np.max(wall)),
                   device_median_ms=float(np.median(dev)), device_min_ms=float(np.min(dev)), device_max_ms=float(np.max(dev)),
                   device_ms_per_stream=float(np.median(dev) / B))
        rows.append(row)
        print(json.dumps(row), flush=True)
    ft.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
