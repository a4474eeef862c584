"""What a camera model costs (uvs_ft_set_camera_model, uvs_kf_set_camera_model, uvs_ft_lift, uvs_lt_set_undistort_model) against the pinhole:

  * uvs_ft_track of one 752 x 480 frame with 150 points and uvs_kf_extract of one 752 x 480 frame, each with the plain uvs_kf_camera, with a
    Kannala-Brandt model (TUM-VI's coefficients, scaled to the frame) and with a MEI model on the handle.  The three variants are INTERLEAVED
    call by call in one process on one device, so they see the same clocks; the table reports medians of the HIP-event times the library
    records (uvs_ft_last_device_ms, uvs_kf_last_device_ms) and of the host clock around the call.
  * uvs_ft_lift of n loose points per model: the host clock around the synchronous call (upload, kernel, download).
  * uvs_lt_set_undistort_model for 752 x 480 per model against uvs_lt_set_undistort (both build the map on the device and wait for it).

The pinhole rows are also what to compare with the same calls of an earlier build (tools/feature_track_timing.py and
tools/keyframe_features_timing.py run there and here, alternately, on the same box).

    python tools/camera_models_timing.py [--reps 50] [--warmup 3] [--out results.json]
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
abi = uvs.abi
import kf_cases  # noqa: E402
import lt_cases  # noqa: E402

SHIFT = (3, -2)
CAMERAS = os.path.join(ROOT, "tests", "golden", "cameras")


def scaled(name, width):
    """A shipped configuration's camera for a frame `width` wide: the scales and the centre multiplied by width / its own width."""
    f = abi.load_camera_calibration(os.path.join(CAMERAS, name + "_config.yaml"))
    s = width / f["width"]
    k = len(f["params"]) - 4
    return abi.camera_model(f["model"], tuple(f["params"][:k]) + tuple(v * s for v in f["params"][k:]))


def med(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = kf_cases.W, kf_cases.H
    variants = [("pinhole", None), ("kannala_brandt", scaled("tum", W)), ("mei", scaled("black_box", W))]
    rows = []

    def report(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- uvs_kf_extract and uvs_ft_track, a handle per variant, the calls interleaved
    img = kf_cases.texture(0)
    moved = np.roll(img, (SHIFT[1], SHIFT[0]), axis=(0, 1)).astype(np.float64) + np.random.default_rng(0).normal(0.0, 1.5, img.shape)
    pair = (img, np.clip(np.rint(moved), 0, 255).astype(np.uint8))
    kfs, fts = {}, {}
    for name, model in variants:
        kfs[name] = uvs.api.KeyframeExtractor(kf_cases.pattern(), max_frames=1, max_width=W, max_height=H)
        fts[name] = uvs.api.FeatureTracker(max_streams=1, max_width=W, max_height=H, levels=4, max_points=a.points)
        if model is not None:
            kfs[name].set_camera_model(model); fts[name].set_camera_model(model)
    fr = kfs["pinhole"].extract([dict(image=img)], kf_cases.CAM_DIST)[0]
    p = fr["xy"][kf_cases.strongest(fr, a.points)].astype(np.float64)
    pts = (p, p + np.array(SHIFT, np.float64))
    t_kf = {n: ([], []) for n, _ in variants}; t_ft = {n: ([], []) for n, _ in variants}
    for name, _ in variants:
        fts[name].track([dict(stream=0, image=pair[0])], kf_cases.CAM_DIST)
    n_kp = n_tr = 0
    for k in range(a.warmup + a.reps):
        cur = k % 2
        for name, model in variants:
            camera = kf_cases.CAM_DIST if model is None else None
            t0 = time.perf_counter()
            out = kfs[name].extract([dict(image=pair[cur])], camera)[0]
            t1 = time.perf_counter()
            tr = fts[name].track([dict(stream=0, image=pair[1 - cur], points=pts[cur])], camera)[0]
            t2 = time.perf_counter()
            if k >= a.warmup:
                t_kf[name][0].append((t1 - t0) * 1e3); t_kf[name][1].append(kfs[name].last_device_ms)
                t_ft[name][0].append((t2 - t1) * 1e3); t_ft[name][1].append(fts[name].last_device_ms)
                n_kp, n_tr = out["n_returned"], tr["n_tracked"]
    for name, _ in variants:
        report(call="uvs_kf_extract", camera=name, width=W, height=H, keypoints=int(n_kp), reps=len(t_kf[name][0]), wall_median_ms=med(t_kf[name][0]),
               device_median_ms=med(t_kf[name][1]), device_min_ms=float(np.min(t_kf[name][1])))
    for name, _ in variants:
        report(call="uvs_ft_track", camera=name, width=W, height=H, points=a.points, tracked=int(n_tr), reps=len(t_ft[name][0]),
               wall_median_ms=med(t_ft[name][0]), device_median_ms=med(t_ft[name][1]), device_min_ms=float(np.min(t_ft[name][1])))
    for h in list(kfs.values()):
        h.close()

    # ---- uvs_ft_lift: loose points
    ft = fts["pinhole"]
    models = [("pinhole", abi.camera_model(abi.CAM_PINHOLE, kf_cases.CAM_DIST))] + variants[1:]
    rng = np.random.default_rng(1)
    for n in (150, 100000):
        xy = np.stack([rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)], 1)
        t = {name: [] for name, _ in models}
        for k in range(a.warmup + a.reps):
            for name, model in models:
                t0 = time.perf_counter()
                ft.lift(model, xy)
                if k >= a.warmup:
                    t[name].append((time.perf_counter() - t0) * 1e3)
        for name, _ in models:
            report(call="uvs_ft_lift", camera=name, n=n, reps=len(t[name]), wall_median_ms=med(t[name]), wall_min_ms=float(np.min(t[name])))
    for h in fts.values():
        h.close()

    # ---- the undistortion map of a 752 x 480 frame
    lt = uvs.api.LineTracker(max_streams=1, max_width=W, max_height=H, max_lines=8, max_length=lt_cases.MAX_LENGTH)
    out_cam = (0.5 * W, 0.5 * W, 0.5 * W, 0.5 * H)
    t = {name: [] for name, _ in models}; t["uvs_lt_set_undistort"] = []
    for k in range(a.warmup + a.reps):
        for name, model in models:
            t0 = time.perf_counter()
            lt.set_undistort_model(0, model, W, H, out_cam)
            if k >= a.warmup:
                t[name].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        lt.set_undistort(0, kf_cases.CAM_DIST, W, H)
        if k >= a.warmup:
            t["uvs_lt_set_undistort"].append((time.perf_counter() - t0) * 1e3)
    for name, v in t.items():
        report(call="uvs_lt_set_undistort_model" if name != "uvs_lt_set_undistort" else name, camera=name if name != "uvs_lt_set_undistort" else "pinhole",
               width=W, height=H, reps=len(v), wall_median_ms=med(v), wall_min_ms=float(np.min(v)))
    lt.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
