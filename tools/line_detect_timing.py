"""Call latency of uvs_lt_detect and uvs_lt_detect_track (line-support regions: blur, Sobel, two sector maps, union-find labelling, the vote,
the moment fit, the ranking; then LBD descriptors and the match) for S items of 752 x 480.  The method is tools/line_track_timing.py's: every
stream alternates between a seeded scene of tests/kf_cases.py and the same scene moved by (3, -2) px with fresh pixel noise, and the table
reports the median, the minimum and the maximum of --reps synchronous calls after --warmup calls, by a host clock around the C-ABI call
(LineTracker.last_ms) and by the HIP events the library records on its stream (uvs_lt_last_detect_device_ms: upload, kernels, download; for
uvs_lt_detect_track the detection's and the tracking's added).  Profiler off.  The last rows are the atomic-contention worst case: a
horizontal ramp of one grey level per pixel.  8 bits carry such a ramp over 256 columns only (a flatter one has columns without gradient
after the blur), so the image is three ramps side by side: three regions of some 120 000 pixels each in both partitions, every pixel of a
region adding to the same record.

    python tools/line_detect_timing.py [--streams 1,16] [--reps 50] [--warmup 3] [--out results.json]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
uvs = importlib.import_module("uv-slam_amd")
import kf_cases  # noqa: E402

SHIFT = (3, -2)
PARAMS = dict(grad_threshold=40, min_pixels=10, min_length=12.0)


def stats(prefix, v):
    return {prefix + "_median_ms": float(np.median(v)), prefix + "_min_ms": float(np.min(v)), prefix + "_max_ms": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,16")
    ap.add_argument("--max-lines", type=int, default=256)
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
        frames.append((img, np.clip(np.rint(moved), 0, 255).astype(np.uint8)))
    ramp = np.ascontiguousarray(np.broadcast_to((np.arange(W) % 256)[None, :], (H, W)).astype(np.uint8))
    lt = uvs.api.LineTracker(max_streams=S, max_width=W, max_height=H, max_lines=a.max_lines, max_length=256)
    rows = []
    for image_kind, params in (("texture", PARAMS), ("ramp", dict(PARAMS, grad_threshold=8))):
        for call in ("uvs_lt_detect", "uvs_lt_detect_track"):
            for B in (streams if image_kind == "texture" else streams[:1]):
                for s in range(B):
                    lt.reset(s)
                fn = lt.detect if call == "uvs_lt_detect" else lt.detect_track
                wall, dev, out = [], [], None
                for k in range(a.warmup + a.reps):
                    cur = k % 2
                    items = [dict(stream=s, image=frames[s][cur] if image_kind == "texture" else ramp) for s in range(B)]
                    out = fn(items, **params)
                    if k >= a.warmup:
                        wall.append(lt.last_ms); dev.append(lt.last_detect_device_ms)
                row = dict(label=a.label, call=call, image=image_kind, items=B, width=W, height=H, max_lines=a.max_lines, reps=len(wall),
                           n_support_mean=float(np.mean([d["n_support"] for d in out])), n_regions_mean=float(np.mean([sum(d["n_regions"]) for d in out])),
                           n_found_mean=float(np.mean([d["n_found"] for d in out])), largest_region=int(max(d["info"][:, 2].max() if len(d["info"]) else 0 for d in out)),
                           n_matched_mean=float(np.mean([d.get("n_matched", 0) for d in out])), **stats("wall", wall), **stats("device", dev))
                rows.append(row)
                print(json.dumps(row), flush=True)
    lt.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
