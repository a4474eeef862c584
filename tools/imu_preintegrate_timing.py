"""Call latency of uvs_imu_preintegrate (IntegrationBase's pre-integration for a batch of intervals) at the project's scale points, beside the host
mirror's serial loop on the same samples and beside the solve the blocks feed.

Per shape `B x S` (S one number or lo-hi): B windows of 10 intervals, each of S samples, in ONE uvs_imu_preintegrate call.  Clocks, medians over
--reps calls after warm-up: a host clock around the synchronous C call (checks, packing into pinned memory, upload, kernel, download), the HIP
events the library records around the kernel alone (uvs_imu_last_device_ms), and a host clock around the comparator -- uvs_host_imu_integrate of
libuvs_host.so (IntegrationBase::push_back sample by sample, one thread), called once per interval in a loop.  The yardstick for "fast enough" is the
k_solve launch of a batch of --solve-batch windows (HIP events, as bench.py's kernel time), measured in the same process.  Device call, host loop
and solve launch alternate.

Samples are the seeded intervals of tests/imu_cases.py's style (200 Hz, gravity plus excitation, biases); 16 distinct intervals per length are
repeated to fill a shape.

    python tools/imu_preintegrate_timing.py [--shapes 1x20-60,256x20-60,1x400] [--reps 30] [--solve-batch 256] [--out results.json]
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
abi = uvs.abi


def make_interval(seed, n):
    rng = np.random.default_rng([911, seed, n])
    t = 0.005 * np.arange(n + 1)
    amp_a, amp_g = rng.uniform(1.0, 1.5, 3), rng.uniform(0.3, 0.5, 3)
    fa, fg, pa, pg = rng.uniform(0.3, 1.5, 3), rng.uniform(0.3, 1.5, 3), rng.uniform(0, 2 * np.pi, 3), rng.uniform(0, 2 * np.pi, 3)
    a = np.array([0.0, 0.0, 9.81007]) + amp_a * np.sin(2 * np.pi * fa * t[:, None] + pa); g = amp_g * np.sin(2 * np.pi * fg * t[:, None] + pg)
    return dict(acc_0=a[0], gyr_0=g[0], ba=rng.normal(0, 0.1, 3), bg=rng.normal(0, 0.01, 3), dt=np.full(n, 0.005), acc=a[1:], gyr=g[1:], frame_i=seed % 10)


def shape_intervals(B, lo, hi):
    rng = np.random.default_rng([912, B, lo, hi])
    pool = {}
    out = []
    for k in range(10 * B):
        n = int(rng.integers(lo, hi + 1)); key = (k % 16, n)
        if key not in pool:
            pool[key] = make_interval(*key)
        out.append(pool[key])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x20-60,256x20-60,1x400")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--solve-batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    host = C.CDLL(os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so"))
    host.uvs_host_imu_integrate.argtypes = [C.c_int] + [abi.c_double_p] * 9 + [C.c_void_p]; host.uvs_host_imu_integrate.restype = C.c_int
    solver = None
    if args.solve_batch > 0:
        solver = uvs.api.Solver(device=0, max_batch=args.solve_batch)
        solver.upload([uvs.synth.make_window(i) for i in range(args.solve_batch)])
    results = []
    for shape in args.shapes.split(","):
        B, S = shape.split("x"); B = int(B)
        lo, hi = (int(v) for v in S.split("-")) if "-" in S else (int(S), int(S))
        ivs = shape_intervals(B, lo, hi)
        batch = abi.imu_batch_of(ivs)
        n_samples = int(batch["sample_begin"][-1])
        imu = uvs.api.ImuPreintegrator(device=0, max_intervals=len(ivs), max_samples=max(n_samples, 1))
        f = lambda a: np.ascontiguousarray(a, np.float64).reshape(-1)
        keep = [[f(iv[k]) for k in ("acc_0", "gyr_0", "ba", "bg", "dt", "acc", "gyr")] for iv in ivs]
        host_args = [[abi._dp(a) for a in row] for row in keep]
        out = np.zeros(1, abi.IMU_BLOCK_DTYPE)

        def host_loop():
            t0 = time.perf_counter()
            for iv, row in zip(ivs, host_args):
                host.uvs_host_imu_integrate(len(iv["dt"]), *row, None, None, C.c_void_p(out.ctypes.data))
            return (time.perf_counter() - t0) * 1e3

        call, kern, hst, slv = [], [], [], []
        for r in range(args.warmup + args.reps):
            blocks = imu.preintegrate(batch)
            h = host_loop()
            s = solver.solve_resident() if solver else float("nan")
            if r >= args.warmup:
                call.append(imu.last_ms); kern.append(imu.last_device_ms); hst.append(h); slv.append(s)
        assert abs(blocks[-1]["delta_p"] - out[0]["delta_p"]).max() < 1e-9          # both integrated the same last interval
        imu.close()
        res = dict(shape=shape, intervals=len(ivs), samples=n_samples, call_ms=float(np.median(call)), kernel_ms=float(np.median(kern)),
                   copies_and_host_ms=float(np.median(call) - np.median(kern)), host_loop_ms=float(np.median(hst)),
                   k_solve_launch_ms=float(np.median(slv)), download_bytes=len(ivs) * abi.IMU_BLOCK_DTYPE.itemsize, reps=args.reps)
        print(json.dumps(res))
        results.append(res)
    if solver:
        solver.close()
    if args.out:
        with open(args.out, "w") as fo:
            json.dump(results, fo, indent=1)


if __name__ == "__main__":
    main()
