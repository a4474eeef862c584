"""Call latency of uvs_lt_track (LBD descriptors of caller-supplied segments, the Hamming match against the slot's previous lines) for S streams
of 752 x 480 frames with 150 segments of 40 .. 160 px each.  The method is tools/feature_equalize_timing.py's: every stream alternates between a
seeded scene of tests/kf_cases.py and the same scene moved by (3, -2) px with fresh pixel noise, the segments are seeded random ones that move
with the scene (the detector is the caller's and is not timed), and the table reports the median, the minimum and the maximum of --reps
synchronous calls after --warmup calls, by a host clock around the call and by the HIP events the library records on its stream
(uvs_lt_last_device_ms: upload, kernels, download).  Profiler off.  uvs_lt_match alone (150 x 150 and 1024 x 1024 descriptors) follows by the
host clock.

    python tools/line_track_timing.py [--streams 1,16] [--lines 150] [--reps 50] [--warmup 3] [--out results.json]
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


def stats(prefix, v):
    return {prefix + "_median_ms": float(np.median(v)), prefix + "_min_ms": float(np.min(v)), prefix + "_max_ms": float(np.max(v))}


def segments(seed, n, W, H, lo=40.0, hi=160.0):
    """n seeded segments of length lo .. hi whose ends lie at least 8 px inside the image."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        c = rng.uniform([8, 8], [W - 8, H - 8]); th = rng.uniform(0, np.pi); hl = rng.uniform(lo, hi) / 2
        d = hl * np.array([np.cos(th), np.sin(th)])
        a, b = c - d, c + d
        if min(a[0], b[0]) >= 8 and max(a[0], b[0]) <= W - 8 and min(a[1], b[1]) >= 8 and max(a[1], b[1]) <= H - 8:
            out.append([a[0], a[1], b[0], b[1]])
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,16")
    ap.add_argument("--lines", type=int, default=150)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    streams = [int(v) for v in a.streams.split(",")]
    S = max(streams)
    W, H = kf_cases.W, kf_cases.H
    frames = []
    for s in range(S):
        img = kf_cases.texture(s)
        moved = np.roll(img, (SHIFT[1], SHIFT[0]), axis=(0, 1)).astype(np.float64) + np.random.default_rng(s).normal(0.0, 1.5, img.shape)
        seg = segments(100 + s, a.lines, W, H)
        frames.append(((img, seg), (np.clip(np.rint(moved), 0, 255).astype(np.uint8), seg + np.tile(np.array(SHIFT, np.float64), 2))))
    lt = uvs.api.LineTracker(max_streams=S, max_width=W, max_height=H, max_lines=max(a.lines, 1024), max_length=256)
    rows = []
    for B in streams:
        for s in range(B):
            lt.reset(s)
        lt.track([dict(stream=s, image=frames[s][0][0], segs=frames[s][0][1]) for s in range(B)])
        wall, dev, matched, samples = [], [], [], 0
        for k in range(a.warmup + a.reps):
            cur = 1 - k % 2
            items = [dict(stream=s, image=frames[s][cur][0], segs=frames[s][cur][1]) for s in range(B)]
            t0 = time.perf_counter()
            out = lt.track(items)
            if k >= a.warmup:
                wall.append((time.perf_counter() - t0) * 1e3); dev.append(lt.last_device_ms)
                matched.append(np.mean([d["n_matched"] for d in out]))
        L = np.floor(np.hypot(frames[0][0][1][:, 2] - frames[0][0][1][:, 0], frames[0][0][1][:, 3] - frames[0][0][1][:, 1]))
        row = dict(label=a.label, call="uvs_lt_track", streams=B, width=W, height=H, lines=a.lines, samples_per_frame=int(63 * L.sum()), reps=len(wall),
                   matched_mean=float(np.mean(matched)), **stats("wall", wall), **stats("device", dev))
        rows.append(row)
        print(json.dumps(row), flush=True)
    rng = np.random.default_rng(1)
    for n in (a.lines, 1024):
        pd = rng.integers(0, 256, (n, 32)).astype(np.uint8); cd = rng.integers(0, 256, (n, 32)).astype(np.uint8)
        pe = rng.integers(0, 700, (n, 4)).astype(np.int32); ce = pe + rng.integers(-20, 21, (n, 4)).astype(np.int32)
        wall = []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            lt.match(pd, pe, cd, ce)
            if k >= a.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
        row = dict(label=a.label, call="uvs_lt_match", n_prev=n, n_cur=n, reps=len(wall), **stats("wall", wall))
        rows.append(row)
        print(json.dumps(row), flush=True)
    lt.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
