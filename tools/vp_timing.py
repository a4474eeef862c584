"""Call latency of uvs_vp_estimate (vanishing points of the line front end: hypotheses, sphere-grid voting, selection, line tags) for B frames
of N lines.

Two clocks per call: a host clock around the synchronous call (packing into pinned memory, upload, five kernels, download, unpacking) and
the HIP events the library records on its stream around the upload, the kernels and the download (uvs_vp_last_device_ms).  The table reports
medians after warm-up of every shape; calls are repeated until each shape has run for at least --min-seconds.  Frames are seeded Manhattan
scenes of tests/vp_cases.py scaled to N lines (5/16, 4/16, 3/16 of them along the three directions, the rest free), each with its own seed.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats`.

    python tools/vp_timing.py [--batches 1,16,64,256] [--lines 40,150,600] [--min-seconds 1.0] [--out results.json]
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
import vp_cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64,256")
    ap.add_argument("--lines", default="40,150,600")
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--min-reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    batches = [int(v) for v in a.batches.split(",")]; lines = [int(v) for v in a.lines.split(",")]
    v = uvs.api.VanishingPointEstimator(max_frames=max(batches), max_lines=max(lines))
    rows = []
    for n in lines:
        per = (5 * n // 16, 4 * n // 16, 3 * n // 16)
        distinct = [vp_cases.scene(500 + s, n_per=per, n_free=n - sum(per))[0] for s in range(min(max(batches), 16))]      # 16 scenes, reused with other seeds
        base = [dict(segs=distinct[s % len(distinct)], seed=9000 + s) for s in range(max(batches))]
        for B in batches:
            frames = base[:B]
            for _ in range(3):                      # warm-up: code object load, first touch of the buffers
                res, _, _ = v.estimate(frames, vp_cases.CAM)
            wall, dev = [], []
            t_start = time.perf_counter()
            while len(wall) < a.min_reps or time.perf_counter() - t_start < a.min_seconds:
                t0 = time.perf_counter()
                res, tag, _ = v.estimate(frames, vp_cases.CAM)
                wall.append((time.perf_counter() - t0) * 1e3); dev.append(v.last_device_ms)
            row = dict(frames=B, lines=n, reps=len(wall), ok=int(sum(r["status"] == 0 for r in res)), tagged=float(np.mean(np.concatenate(tag) < 3)),
                       wall_median_ms=float(np.median(wall)), wall_min_ms=float(np.min(wall)), wall_max_ms=float(np.max(wall)),
                       device_median_ms=float(np.median(dev)), device_min_ms=float(np.min(dev)), device_max_ms=float(np.max(dev)),
                       device_ms_per_frame=float(np.median(dev) / B))
            rows.append(row)
            print(json.dumps(row), flush=True)
    v.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
