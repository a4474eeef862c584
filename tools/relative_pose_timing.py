"""Call latency of uvs_rp_relative_pose (the bootstrap's choice of its reference frame: gates, fundamental-matrix RANSAC, recoverPose) for W
windows of ten frame pairs with n correspondences each, and what it adds to the part that existed before it: uvs_ft_reject on the same rounded
items in the same process, in chunks of the tracker handle's max_streams.

Every item is a seeded two-view scene of tests/rp_cases.py (a metre and a half of sideways motion with a 5 degree turn that adds to its parallax, points 2 .. 40 m
away, 0.1 px of noise at focal length 460), a different seed per item; every item passes the gates, so every item runs all three kernels.

Three clocks per call: a host clock around the synchronous call (checks, packing, upload, the kernels, download), the HIP events of the library
around each of its kernels (uvs_rp_last_device_ms: gate, RANSAC, recover), and for the comparator the host clock around its chunked calls with
the sum of uvs_ft_last_reject_device_ms.  The table reports medians of --reps calls after --warmup calls of every shape.

    python tools/relative_pose_timing.py [--shapes 1x150,256x150,1x1000] [--reps 30] [--warmup 3] [--out results.json]
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
import rp_cases  # noqa: E402
import rp_ref  # noqa: E402

FT_STREAMS = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x150,256x150,1x1000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    max_items = max(w for w, _ in shapes) * 10; max_points = max(n for _, n in shapes)
    rp = uvs.api.RelativePose(max_items=max_items, max_points=max_points)
    ft = uvs.api.FeatureTracker(max_streams=FT_STREAMS, max_width=96, max_height=80, levels=1, max_points=max_points)
    R = rp_cases.rot((0, 1, 0), -5.0)
    rows = []
    for W, n in shapes:
        items, rej = [], []
        for k in range(W * 10):
            left, right, _ = rp_cases.two_views(np.random.default_rng(1000 + k), n, R, (-1.5, 0.05, 0.1))
            items.append(dict(window=k // 10, frame_l=k % 10, seed=k, left=left, right=right))
            rej.append(dict(prev=rp_ref.round32(left), next=rp_ref.round32(right), seed=k))
        wall, dev, cmp_wall, cmp_dev, res = [], [], [], [], None
        for k in range(a.warmup + a.reps):          # the warm-up: code object load, the first call's allocations
            t0 = time.perf_counter()
            res, _, win = rp.solve(items, n_windows=W)
            t1 = time.perf_counter()
            d = 0.0
            for c in range(0, len(rej), FT_STREAMS):
                ft.reject(rej[c:c + FT_STREAMS], rp_ref.PARAMS["f_threshold"], rp_ref.PARAMS["confidence"])
                d += ft.last_reject_device_ms()
            t2 = time.perf_counter()
            if k >= a.warmup:
                wall.append((t1 - t0) * 1e3); dev.append(rp.last_device_ms); cmp_wall.append((t2 - t1) * 1e3); cmp_dev.append(d)
        dev = np.median(np.array(dev), axis=0)
        row = dict(windows=W, items=W * 10, points=n, reps=len(wall), gated_items=int((res["ransac_status"] == 1).sum()), ok_items=int(res["ok"].sum()),
                   l_found=int((win["l"] >= 0).sum()),
                   iterations_max=int(res["iterations"].max()), wall_median_ms=float(np.median(wall)), wall_min_ms=float(np.min(wall)),
                   gate_ms=float(dev[0]), ransac_ms=float(dev[1]), recover_ms=float(dev[2]),
                   reject_chunks=(len(rej) + FT_STREAMS - 1) // FT_STREAMS, reject_wall_median_ms=float(np.median(cmp_wall)),
                   reject_device_median_ms=float(np.median(cmp_dev)),      # upload + kernel + download of every chunk
                   added_wall_ms=float(np.median(wall) - np.median(cmp_wall)), added_kernel_ms=float(dev[0] + dev[2]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    rp.close(); ft.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
