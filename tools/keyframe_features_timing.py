"""Call latency of uvs_kf_extract (keyframe features of loop closure: blur, FAST corners, BRIEF descriptors, normalized keypoints) for B frames
of 752 x 480 with 150 window points each.

Two clocks per call: a host clock around the synchronous call (repacking into pinned memory, upload, six kernels, download, unpacking) and the
HIP events the library records on its stream around the upload, the kernels and the download (uvs_kf_last_device_ms).  The table reports the
median of --reps synchronous calls after --warmup calls of every shape.  Frames are the seeded scenes of tests/kf_cases.py (a few hundred
keypoints of a few thousand corners each), reused with other seeds beyond the four pinned ones.

Per-kernel times come from a SEPARATE run of this file under `rocprofv3 --kernel-trace --stats` (no counters in that run; tracing slows the
host, so the table above is taken with the profiler off):

    python tools/keyframe_features_timing.py [--batches 1,4,16] [--reps 50] [--warmup 3] [--out results.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/keyframe_features_timing.py --batches 1 --reps 50
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
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--window", type=int, default=150)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    batches = [int(v) for v in a.batches.split(",")]
    x = uvs.api.KeyframeExtractor(kf_cases.pattern(), max_frames=max(batches), max_width=kf_cases.W, max_height=kf_cases.H, max_keypoints=4096,
                                  max_window=max(a.window, 1))
    base = [dict(image=kf_cases.texture(s), window_uv=kf_cases.window_points(s, a.window, kf_cases.W, kf_cases.H)) for s in range(max(batches))]
    rows = []
    for B in batches:
        frames = base[:B]
        for _ in range(a.warmup):                   # code object load, first touch of the buffers
            out = x.extract(frames, kf_cases.CAM_DIST)
        wall, dev = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = x.extract(frames, kf_cases.CAM_DIST)
            wall.append((time.perf_counter() - t0) * 1e3); dev.append(x.last_device_ms)
        row = dict(frames=B, width=kf_cases.W, height=kf_cases.H, window=a.window, reps=len(wall),
                   keypoints_mean=float(np.mean([d["n_keypoints"] for d in out])), corners_mean=float(np.mean([d["n_corners_before_nms"] for d in out])),
                   wall_median_ms=float(np.median(wall)), wall_min_ms=float(np.min(wall)), wall_max_ms=float(np.max(wall)),
                   device_median_ms=float(np.median(dev)), device_min_ms=float(np.min(dev)), device_max_ms=float(np.max(dev)),
                   device_ms_per_frame=float(np.median(dev) / B))
        rows.append(row)
        print(json.dumps(row), flush=True)
    x.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
