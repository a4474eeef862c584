#!/bin/bash
# A/B of two BUILT checkouts on ONE box for code that moved between front-end units: bash tools/ab/run_ab_front_end.sh <other checkout>
# uvs_tri_triangulate and uvs_ft_reject at their README shapes through each tree's own tools/ and library, this tree ("cur") and the other one
# alternating REPS times (default 3); every run has its own time limit and the first one that fails ends the comparison.
# Prints per run the call and kernel medians (ms) of every shape.
set -u -o pipefail
other=${1:?the other checkout (built)}
out=$(mktemp -d)
for rep in $(seq 1 ${REPS:-3}); do
for tree in . "$other"; do
  name=$([ "$tree" = "." ] && echo cur || echo other)
  timeout -k 10 200 python "$tree/tools/triangulate_timing.py" --shapes 1x150x40,256x150x40,1x20000x5000 --reps 30 > "$out/tri_${name}_$rep.log" 2>/dev/null || { echo "$name: triangulate_timing failed, stopping"; exit 1; }
  timeout -k 10 200 python "$tree/tools/feature_reject_timing.py" --items 1,4,16 --outliers 0.1,0.5 --reps 50 > "$out/fr_${name}_$rep.log" 2>/dev/null || { echo "$name: feature_reject_timing failed, stopping"; exit 1; }
done; done
python - "$out" <<'PY'
import glob, json, sys
for kind, keys in (("tri", ("device_call_median_ms", "kernels_median_ms")), ("fr", ("wall_median_ms", "device_median_ms"))):
    for name in ("cur", "other"):
        for f in sorted(glob.glob(f"{sys.argv[1]}/{kind}_{name}_*.log")):
            rows = [json.loads(l) for l in open(f) if l.startswith("{")]
            print(kind, name, f[-5], " | ".join(" ".join("%.4f" % r[k] for k in keys) for r in rows))
PY
