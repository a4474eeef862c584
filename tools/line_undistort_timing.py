"""Call latency of uvs_lt_undistort (the remap of raw frames through a slot's map) and of uvs_lt_detect_track with and without a mapped slot,
for S items of 752 x 480 under EuRoC cam0's camera.  The method is tools/line_detect_timing.py's: every stream alternates between a seeded
scene of tests/kf_cases.py and the same scene moved by (3, -2) px with fresh pixel noise, and the table reports the median, the minimum and
the maximum of --reps synchronous calls after --warmup calls, by a host clock around the C-ABI call (LineTracker.last_ms) and by the HIP
events the library records on its stream (uvs_lt_last_undistort_device_ms, uvs_lt_last_detect_device_ms: upload, kernels, download).
Profiler off.  Three trackers take uvs_lt_detect_track calls in turn, so that a drift of the machine meets all: "mapped" takes the frames as raw
frames (margins 0, so it detects in 752 x 480 pixels), "plain" the same frames as they are (the library's call before the undistortion
existed; the content differs from what "mapped" detects in), and "plain, undistorted" the images uvs_lt_undistort returned for those frames:
the same detection as "mapped" bit for bit, without the remap kernel.  The one-off uvs_lt_set_undistort (allocation, the map
kernel, a wait) is timed by the host clock.

    python tools/line_undistort_timing.py [--streams 1,16] [--reps 30] [--warmup 3] [--out results.json]
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
PARAMS = dict(grad_threshold=40, min_pixels=10, min_length=12.0)
CAM = (458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)      # EuRoC cam0


def stats(prefix, v):
    return {prefix + "_median_ms": float(np.median(v)), prefix + "_min_ms": float(np.min(v)), prefix + "_max_ms": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,16")
    ap.add_argument("--max-lines", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
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
    mapped = uvs.api.LineTracker(max_streams=S, max_width=W, max_height=H, max_lines=a.max_lines, max_length=256)
    plain = uvs.api.LineTracker(max_streams=S, max_width=W, max_height=H, max_lines=a.max_lines, max_length=256)
    plain_u = uvs.api.LineTracker(max_streams=S, max_width=W, max_height=H, max_lines=a.max_lines, max_length=256)
    set_ms = []
    for s in range(S):
        t0 = time.perf_counter()
        mapped.set_undistort(s, CAM, W, H)
        set_ms.append((time.perf_counter() - t0) * 1e3)
    rows = [dict(label=a.label, call="uvs_lt_set_undistort", items=1, width=W, height=H, reps=len(set_ms), first_ms=set_ms[0], **stats("wall", set_ms[1:] or set_ms))]
    print(json.dumps(rows[0]), flush=True)
    for B in streams:
        wall, dev = [], []
        for k in range(a.warmup + a.reps):
            mapped.undistort([dict(stream=s, image=frames[s][k % 2]) for s in range(B)])
            if k >= a.warmup:
                wall.append(mapped.last_ms); dev.append(mapped.last_undistort_device_ms)
        rows.append(dict(label=a.label, call="uvs_lt_undistort", items=B, width=W, height=H, reps=len(wall), **stats("wall", wall), **stats("device", dev)))
        print(json.dumps(rows[-1]), flush=True)
    und = [[mapped.undistort([dict(stream=s, image=frames[s][c])])[0] for c in range(2)] for s in range(S)]
    for B in streams:
        for s in range(B):
            mapped.reset(s); plain.reset(s); plain_u.reset(s)
        t = {"mapped": ([], [], None), "plain": ([], [], None), "plain, undistorted": ([], [], None)}
        for k in range(a.warmup + a.reps):
            items = [dict(stream=s, image=frames[s][k % 2]) for s in range(B)]
            items_u = [dict(stream=s, image=und[s][k % 2]) for s in range(B)]
            for kind, lt in (("mapped", mapped), ("plain", plain), ("plain, undistorted", plain_u)):
                out = lt.detect_track(items_u if kind == "plain, undistorted" else items, **PARAMS)
                if k >= a.warmup:
                    t[kind][0].append(lt.last_ms); t[kind][1].append(lt.last_detect_device_ms)
                t[kind] = (t[kind][0], t[kind][1], out)
        assert all(np.array_equal(m["seg"], u["seg"]) and np.array_equal(m["desc"], u["desc"]) for m, u in zip(t["mapped"][2], t["plain, undistorted"][2]))
        for kind in ("plain", "plain, undistorted", "mapped"):
            wall, dev, out = t[kind]
            rows.append(dict(label=a.label, call="uvs_lt_detect_track", slot=kind, items=B, width=W, height=H, max_lines=a.max_lines, reps=len(wall),
                             n_support_mean=float(np.mean([d["n_support"] for d in out])), n_found_mean=float(np.mean([d["n_found"] for d in out])),
                             n_matched_mean=float(np.mean([d["n_matched"] for d in out])), **stats("wall", wall), **stats("device", dev)))
            print(json.dumps(rows[-1]), flush=True)
    mapped.close(); plain.close(); plain_u.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
