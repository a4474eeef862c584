"""Call latency of uvs_pr_detect (place recognition of loop closure: the vocabulary tree's descent, the bag-of-words vector, the L1 query of the
database, the add) for one keyframe of N descriptors against a database of E entries.

The vocabulary is a synthetic full-size tree (k = 10, L = 6: 1 111 110 nodes, random centres and weights, generated here in numpy; nothing is
stored), the descriptors are random, and every database entry has as many descriptors as the query.  Two clocks per call: a host clock around
the synchronous call and the HIP events the library records on its stream (uvs_pr_last_device_ms: the whole call, the transform = upload,
descent and vector, the query = scoring and download).  The table reports the median of --reps calls after --warmup calls, with the least and
the greatest; the database grows by one entry per call, which is part of detectLoop.

    python tools/place_recognition_timing.py [--features 500,2000] [--entries 100,1000,10000] [--reps 30] [--warmup 5] [--out results.json]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
uvs = importlib.import_module("uv-slam_amd")


def synthetic_vocabulary(k, L, seed=1):
    """A full k-ary tree in breadth-first ids (the children of node p are k p + 1 .. k p + k), random centres, weights in (0.5, 8)."""
    rng = np.random.default_rng(seed)
    n = sum(k ** l for l in range(1, L + 1))
    ids = np.arange(1, n + 1, dtype=np.int32)
    first_leaf = n - k ** L + 1
    leaves = ids[first_leaf - 1:]
    return dict(k=k, L=L, scoring=0, weighting=0, node_id=ids, parent_id=((ids - 1) // k).astype(np.int32), weight=rng.uniform(0.5, 8.0, n),
                descriptor=rng.integers(0, 2 ** 64, (n, 4), dtype=np.uint64), word_node_id=leaves, word_id=np.arange(len(leaves), dtype=np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", default="500,2000")
    ap.add_argument("--entries", default="100,1000,10000")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    voc = synthetic_vocabulary(a.k, a.levels)
    rng = np.random.default_rng(2)
    rows = []
    for nf in [int(v) for v in a.features.split(",")]:
        pr = uvs.api.PlaceRecognizer(voc, max_features=max(nf, 1), initial_entries=1024)
        for ne in sorted(int(v) for v in a.entries.split(",")):
            while pr.size() < ne:                   # the database: batches of random keyframes
                b = min(uvs.abi.PR_MAX_FRAMES, ne - pr.size())
                pr.add([rng.integers(0, 2 ** 64, (nf, 4), dtype=np.uint64) for _ in range(b)])
            size = pr.size()
            wall, dev, tr, qu, hits = [], [], [], [], []
            for i in range(a.warmup + a.reps):
                _, ids, _ = pr.detect(rng.integers(0, 2 ** 64, (nf, 4), dtype=np.uint64), size + 60 + i)
                if i >= a.warmup:
                    wall.append(pr.last_ms); dev.append(pr.last_device_ms["total"]); tr.append(pr.last_device_ms["transform"])
                    qu.append(pr.last_device_ms["query"]); hits.append(len(ids))
            row = dict(features=nf, entries=size, nodes=len(voc["node_id"]), reps=len(wall), results_mean=float(np.mean(hits)))
            for name, v in (("wall", wall), ("device", dev), ("transform", tr), ("query", qu)):
                row.update({f"{name}_median_ms": float(np.median(v)), f"{name}_min_ms": float(np.min(v)), f"{name}_max_ms": float(np.max(v))})
            rows.append(row)
            print(json.dumps(row), flush=True)
        pr.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
