"""Call latency of uvs_ft_track (point tracking of the point front end: image pyramid, pyramidal Lucas-Kanade, inBorder, normalized points) for
S streams of 752 x 480 with 150 points each and 4 levels.

Every stream alternates between a seeded scene of tests/kf_cases.py and the same scene moved by (3, -2) px with fresh pixel noise, so that every
call uploads one image per stream, builds its pyramid and follows 150 points over a real motion; the points are the 150 strongest FAST corners
of uvs_kf_extract on the scene.

Two clocks per call: a host clock around the synchronous call (repacking into pinned memory, upload, the kernels, download, unpacking) and the
HIP events the library records on its stream around the upload, the kernels and the download (uvs_ft_last_device_ms).  The table reports the
median of --reps synchronous calls after --warmup calls of every shape.

Per-kernel times come from a SEPARATE run of this file under `rocprofv3 --kernel-trace --stats` (no counters in that run; tracing slows the
host, so the table above is taken with the profiler off):

    python tools/feature_track_timing.py [--streams 1,4,16] [--reps 50] [--warmup 3] [--out results.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/feature_track_timing.py --streams 1 --reps 50
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

SHIFT = (3, -2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,4,16")
    ap.add_argument("--points", type=int, default=150)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    streams = [int(v) for v in a.streams.split(",")]
    S = max(streams)
    W, H = kf_cases.W, kf_cases.H
    kf = uvs.api.KeyframeExtractor(kf_cases.pattern(), max_frames=1, max_width=W, max_height=H)
    pair, pts = [], []
    for s in range(S):
        img = kf_cases.texture(s)
        moved = np.roll(img, (SHIFT[1], SHIFT[0]), axis=(0, 1)).astype(np.float64) + np.random.default_rng(s).normal(0.0, 1.5, img.shape)
        pair.append((img, np.clip(np.rint(moved), 0, 255).astype(np.uint8)))
        fr = kf.extract([dict(image=img)], kf_cases.CAM_DIST)[0]
        p = fr["xy"][kf_cases.strongest(fr, a.points)].astype(np.float64)
        pts.append((p, p + np.array(SHIFT, np.float64)))          # where the corners are in the scene / in the moved scene
    kf.close()
    ft = uvs.api.FeatureTracker(max_streams=S, max_width=W, max_height=H, levels=a.levels, max_points=a.points)
    rows = []
    for B in streams:
        for s in range(B):
            ft.reset(s)
        ft.track([dict(stream=s, image=pair[s][0]) for s in range(B)], kf_cases.CAM_DIST)
        wall, dev, tracked, iters = [], [], [], []
        for k in range(a.warmup + a.reps):          # the warm-up: code object load, first touch of the buffers
            cur = k % 2                              # the stored image; the call brings the other one
            items = [dict(stream=s, image=pair[s][1 - cur], points=pts[s][cur]) for s in range(B)]
            t0 = time.perf_counter()
            out = ft.track(items, kf_cases.CAM_DIST)
            if k >= a.warmup:
                wall.append((time.perf_counter() - t0) * 1e3); dev.append(ft.last_device_ms)
                tracked.append(np.mean([d["n_tracked"] for d in out])); iters.append(np.mean([d["iterations"].mean() for d in out]))
        row = dict(streams=B, width=W, height=H, points=a.points, levels=a.levels, reps=len(wall), tracked_mean=float(np.mean(tracked)),
                   iterations_level0_mean=float(np.mean(iters)),
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
