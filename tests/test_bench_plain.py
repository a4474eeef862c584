"""bench.py without --full: the headline line only (no secondary legs), --steps timed launches, and --dump-outputs writing the last step's
results as float64 .npy files that match the solver's own download of the same windows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_run_line_and_dumped_outputs(tmp_path, gpu_api, uvs):
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--batch", "8", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{") and '"metric"' in l]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 4 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["unit"] == "solves/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert abs(d["value"] - 8 * 4 / (d["ms_per_step"] * 4e-3)) <= 1e-6 * d["value"]
    for k in ("roofline", "single_window", "end_to_end", "large_window", "replay", "marginalization_batch", "cpu_baseline"):
        assert k not in d, k                                        # secondary legs run with --full only

    files = sorted(p.name for p in out_dir.iterdir())
    assert "pose.npy" in files and "final_cost.npy" in files and "inv_depth.npy" in files
    assert sum(p.stat().st_size for p in out_dir.iterdir()) <= 64 << 20
    arrays = {f[:-4]: np.load(out_dir / f) for f in files}
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert arrays["pose"].shape == (8, 11, 7) and arrays["final_cost"].shape == (8,)
    assert np.all(arrays["status"] == 0) and abs(arrays["final_cost"].mean() - d["final_cost_mean"]) <= 1e-12 * d["final_cost_mean"]

    # the same windows (bench.py's seeds and prior) solved in this process: the dump is what the resident batch path returns
    s = gpu_api.Solver(device=0, max_batch=8)
    ws = [uvs.synth.make_window(i, with_prior=True, marginalize_fn=lambda win, flag: s.marginalize(win, flag)) for i in range(8)]
    s.upload(ws)
    s.solve_resident()
    states, reps = s.download()
    s.close()
    assert np.array_equal(arrays["num_iterations"], np.array([r.num_iterations for r in reps], dtype=np.float64))
    np.testing.assert_allclose(arrays["pose"], np.stack([st.pose for st in states]), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(arrays["inv_depth"], np.concatenate([st.inv_depth for st in states]), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(arrays["final_cost"], np.array([r.final_cost for r in reps]), rtol=1e-9)
