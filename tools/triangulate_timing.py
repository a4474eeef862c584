"""Call latency of uvs_tri_triangulate (the DLT of point tracks, the Pluecker line of two views) at the project's scale points, beside the host
mirror's serial loop on the same tracks.

Per shape `B x (points, lines)`: B windows of that many landmarks in ONE uvs_tri_triangulate call.  Three clocks, medians over --reps calls after
warm-up: a host clock around the synchronous C call (packing into pinned memory, upload, kernels, download, unpacking), the HIP events the
library records around the kernels alone (uvs_tri_last_device_ms), and a host clock around the comparator -- the unchanged
uvs_host_triangulate of libuvs_host.so (FeatureManager::triangulate + triangulateLine, one thread), called once per window in a loop.  Device
and host calls alternate in the same process.  The host hook also builds its std::list tracks from the flat arrays inside the timed call, as
the device call packs its staging buffer inside its own.

Tracks are seeded scenes in the style of tests/tri_cases.py (0.2 m per frame, 1e-3 of noise), every point starting in frames 0 .. 7 so that
the host's selection rule takes all of them; 8 distinct windows (a tenth of the landmarks of a window above 2 000) are repeated to fill a shape.

    python tools/triangulate_timing.py [--shapes 1x150x40,256x150x40,1x20000x5000] [--reps 30] [--out results.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
uvs = importlib.import_module("uv-slam_amd")
import tri_cases  # noqa: E402
import tri_ref  # noqa: E402

NF = 11


def make_window(seed, n_points, n_lines):
    """-> dict: pose, ex, point tracks (start, nobs, obs) and line tracks (start, nobs, sp, ep over consecutive frames), the layout of uvs_host_triangulate."""
    rng = np.random.default_rng(seed)
    pose, ex = tri_cases._window(rng, 0.2)
    cams = tri_ref.cameras(pose, ex)
    pt_start, pt_nobs, pt_obs = [], [], []
    for _ in range(n_points):
        s = int(rng.integers(0, 8)); n = int(rng.integers(2, NF - s + 1))
        X = cams[1][s] + cams[0][s] @ np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4), 1.0]) * rng.uniform(1.5, 12.0)
        pt_start.append(s); pt_nobs.append(n)
        pt_obs += [tri_cases._noisy(rng, tri_cases._view(cams, s + j, X), tri_cases.NOISE) for j in range(n)]
    ln_start, ln_nobs, ln_sp, ln_ep = [], [], [], []
    for _ in range(n_lines):
        s = int(rng.integers(0, 6)); n = int(rng.integers(5, NF - s + 1))
        A = cams[1][s] + cams[0][s] @ np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(4.0, 9.0)])
        d = rng.standard_normal(3); d[2] *= 0.3; d /= np.linalg.norm(d)
        ln_start.append(s); ln_nobs.append(n)
        for j in range(n):
            ln_sp.append(tri_cases._noisy(rng, tri_cases._view(cams, s + j, A - rng.uniform(0.3, 1.0) * d), tri_cases.NOISE))
            ln_ep.append(tri_cases._noisy(rng, tri_cases._view(cams, s + j, A + rng.uniform(0.3, 1.0) * d), tri_cases.NOISE))
    i32 = lambda v: np.asarray(v, np.int32)
    f3 = lambda v: np.ascontiguousarray(np.asarray(v, np.float64).reshape(-1, 3))
    return dict(pose=pose, ex=ex, pt_start=i32(pt_start), pt_nobs=i32(pt_nobs), pt_obs=f3(pt_obs), ln_start=i32(ln_start), ln_nobs=i32(ln_nobs),
                ln_sp=f3(ln_sp), ln_ep=f3(ln_ep))


def repeat(w, times):
    """The landmarks of a window `times` times over (the same frames)."""
    out = dict(pose=w["pose"], ex=w["ex"])
    for k in ("pt_start", "pt_nobs", "pt_obs", "ln_start", "ln_nobs", "ln_sp", "ln_ep"):
        out[k] = np.ascontiguousarray(np.concatenate([w[k]] * times))
    return out


def device_batch(windows):
    """The uvs_tri_batch dict of a list of host-layout windows: all views of a point, the first and the last view of a line."""
    b = dict(pose=np.stack([w["pose"] for w in windows]), ex_pose=np.stack([w["ex"] for w in windows]))
    b["pt_window"] = np.concatenate([np.full(len(w["pt_start"]), i, np.int32) for i, w in enumerate(windows)])
    b["pt_start"] = np.concatenate([w["pt_start"] for w in windows])
    b["pt_obs_begin"] = np.r_[0, np.cumsum(np.concatenate([w["pt_nobs"] for w in windows]))].astype(np.int32)
    b["pt_obs"] = np.concatenate([w["pt_obs"] for w in windows])
    b["ln_window"] = np.concatenate([np.full(len(w["ln_start"]), i, np.int32) for i, w in enumerate(windows)])
    b["ln_fi"] = np.concatenate([w["ln_start"] for w in windows])
    b["ln_fj"] = np.concatenate([w["ln_start"] + w["ln_nobs"] - 1 for w in windows]).astype(np.int32)
    first = [np.r_[0, np.cumsum(w["ln_nobs"])[:-1]] for w in windows]; last = [np.cumsum(w["ln_nobs"]) - 1 for w in windows]
    b["ln_sp_i"] = np.concatenate([w["ln_sp"][f] for w, f in zip(windows, first)]); b["ln_ep_i"] = np.concatenate([w["ln_ep"][f] for w, f in zip(windows, first)])
    b["ln_sp_j"] = np.concatenate([w["ln_sp"][l] for w, l in zip(windows, last)]); b["ln_ep_j"] = np.concatenate([w["ln_ep"][l] for w, l in zip(windows, last)])
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x150x40,256x150x40,1x20000x5000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    host = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double)); ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int))
    rows = []
    for shape in a.shapes.split(","):
        B, n_pt, n_ln = (int(v) for v in shape.split("x"))
        tile = 10 if n_pt >= 2000 and n_pt % 10 == 0 and n_ln % 10 == 0 else 1
        distinct = [repeat(make_window(7000 + s, n_pt // tile, n_ln // tile), tile) for s in range(min(B, 8))]
        windows = [distinct[i % len(distinct)] for i in range(B)]
        batch = device_batch(windows)
        tri = uvs.api.Triangulator(max_windows=B, max_points=B * n_pt, max_lines=B * n_ln)
        host_args = [(dp(w["pose"]), dp(w["ex"]), n_pt, ip(w["pt_start"]), ip(w["pt_nobs"]), dp(w["pt_obs"]), n_ln, ip(w["ln_start"]), ip(w["ln_nobs"]),
                      dp(w["ln_sp"]), dp(w["ln_ep"])) for w in distinct]
        depth_h = np.zeros(n_pt); orth_h = np.zeros((n_ln, 4))

        def host_call():
            t0 = time.perf_counter()
            for i in range(B):
                depth_h[:] = -1.0; orth_h[:] = 0.0
                if host.uvs_host_triangulate(*host_args[i % len(distinct)], dp(depth_h), dp(orth_h)) != 0:
                    raise RuntimeError("uvs_host_triangulate failed")
            return (time.perf_counter() - t0) * 1e3

        for _ in range(3):                      # warm-up: code object load, first touch of the buffers
            depth, pf, orth, lf = tri.triangulate(batch); host_call()
        wall, dev, cpu = [], [], []
        for _ in range(a.reps):
            depth, pf, orth, lf = tri.triangulate(batch)
            wall.append(tri.last_ms); dev.append(tri.last_device_ms)
            cpu.append(host_call())
        # the last window of the batch is the one the host loop ended on: the two routes agree there (0.2 m class)
        n_last = len(windows[-1]["pt_start"])
        agree = float(np.abs(depth[-n_last:] / depth_h - 1).max())
        row = dict(windows=B, points=n_pt, lines=n_ln, reps=a.reps, flags_pt=np.bincount(pf, minlength=3).tolist(), flags_ln=np.bincount(lf, minlength=3).tolist(),
                   device_call_median_ms=float(np.median(wall)), device_call_min_ms=float(np.min(wall)), device_call_max_ms=float(np.max(wall)),
                   kernels_median_ms=float(np.median(dev)), kernels_min_ms=float(np.min(dev)),
                   host_loop_median_ms=float(np.median(cpu)), host_loop_min_ms=float(np.min(cpu)), host_loop_max_ms=float(np.max(cpu)),
                   host_over_device=float(np.median(cpu) / np.median(wall)), last_window_depth_agreement=agree)
        rows.append(row)
        print(json.dumps(row), flush=True)
        tri.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
