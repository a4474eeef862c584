"""Call latency of uvs_ft_track with the slots' equalization off and on, and of uvs_ft_equalize alone (CLAHE 3.0, 8 x 8 of 752 x 480 images), for
S streams with 150 points each and 4 levels.  The method is tools/feature_track_timing.py's: every stream alternates between a seeded scene of
tests/kf_cases.py and the same scene moved by (3, -2) px with fresh pixel noise, the points are the 150 strongest FAST corners of uvs_kf_extract,
and the table reports the median, the minimum and the maximum of --reps synchronous calls after --warmup calls, by a host clock around the call
and by the HIP events the library records on its stream (uvs_ft_last_device_ms, uvs_ft_last_equalize_device_ms).  Profiler off.

Two trackers live in one process, one with every slot plain and one with every slot equalized, and their calls ALTERNATE (off, on, off, on, ..),
so that a drift of the clocks or of the box hits both alike.  The equalized tracker is given the dimmed frames (contrast about 128 cut to a
quarter), which is what the equalization is for; its points are the same corners.  uvs_ft_equalize is timed on the same dimmed frames in a loop
of its own afterwards.

--off-only times the plain tracker alone and touches nothing this feature added: that mode runs unchanged on the commit before it, which is how
the off path is compared (the only timing condition of the feature: its median within the other build's min .. max on the same box).

    python tools/feature_equalize_timing.py [--streams 1,4,16] [--reps 50] [--warmup 3] [--off-only] [--out results.json]
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


def dim(img):
    return np.clip(np.rint(100.0 + 0.25 * (img.astype(np.float64) - 128.0)), 0, 255).astype(np.uint8)


def stats(prefix, v):
    return {prefix + "_median_ms": float(np.median(v)), prefix + "_min_ms": float(np.min(v)), prefix + "_max_ms": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,4,16")
    ap.add_argument("--points", type=int, default=150)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--label", default="")
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
        pts.append((p, p + np.array(SHIFT, np.float64)))
    kf.close()
    modes = ["off"] if a.off_only else ["off", "on"]
    images = dict(off=pair, on=[(dim(p[0]), dim(p[1])) for p in pair])
    make = lambda: uvs.api.FeatureTracker(max_streams=S, max_width=W, max_height=H, levels=a.levels, max_points=a.points)
    ft = {m: make() for m in modes}
    rows = []
    for B in streams:
        for m in modes:
            for s in range(B):
                ft[m].reset(s)
                if m == "on":
                    ft[m].set_equalize(s, 3.0, 8)
            ft[m].track([dict(stream=s, image=images[m][s][0]) for s in range(B)], kf_cases.CAM_DIST)
        wall = {m: [] for m in modes}; dev = {m: [] for m in modes}; tracked = {m: [] for m in modes}
        for k in range(a.warmup + a.reps):
            cur = k % 2
            for m in modes:                          # off, on, off, on, ..
                items = [dict(stream=s, image=images[m][s][1 - cur], points=pts[s][cur]) for s in range(B)]
                t0 = time.perf_counter()
                out = ft[m].track(items, kf_cases.CAM_DIST)
                if k >= a.warmup:
                    wall[m].append((time.perf_counter() - t0) * 1e3); dev[m].append(ft[m].last_device_ms)
                    tracked[m].append(np.mean([d["n_tracked"] for d in out]))
        for m in modes:
            row = dict(label=a.label, call="uvs_ft_track", equalize=m, streams=B, width=W, height=H, points=a.points, levels=a.levels, reps=len(wall[m]),
                       tracked_mean=float(np.mean(tracked[m])), **stats("wall", wall[m]), **stats("device", dev[m]))
            rows.append(row)
            print(json.dumps(row), flush=True)
        if not a.off_only:
            wall_e, dev_e = [], []
            for k in range(a.warmup + a.reps):
                imgs = [images["on"][s][k % 2] for s in range(B)]
                t0 = time.perf_counter()
                ft["on"].equalize(imgs, 3.0, 8)
                if k >= a.warmup:
                    wall_e.append((time.perf_counter() - t0) * 1e3); dev_e.append(ft["on"].last_equalize_device_ms())
            row = dict(label=a.label, call="uvs_ft_equalize", streams=B, width=W, height=H, reps=len(wall_e), **stats("wall", wall_e), **stats("device", dev_e))
            rows.append(row)
            print(json.dumps(row), flush=True)
    for t in ft.values():
        t.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
