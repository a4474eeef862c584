"""A Solver handle returns every device allocation when it is closed, the large-window buffers included.

A fresh child process repeats create -> large_solve_fused -> large_solve (step-wise) -> close on a window whose chunk count fills the
persistent grid of the large-window kernels (compute units - 1 workgroups), then compares the device's free memory with its value after
one warm-up cycle.  That figure covers the whole device, which other processes may share, so the margin sits well below the leak it
guards against.  Measured on an MI355X (256 compute units, 255 chunks, two runs each): a library that kept the large-window buffers
(k_large_chunks' partial rows alone are grid x LG_ROW x 8 bytes) lost 86 MiB over the 6 cycles, 14.3 MiB per cycle; one that frees
them lost 2 MiB over 6 cycles, 0 over 2 and 2 MiB over 12: one allocation granule of the runtime, not a loss per cycle."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CYCLES = 6
MARGIN_BYTES = 24 << 20

CHILD = r"""
import ctypes as C, importlib, json, os, sys
sys.path.insert(0, sys.argv[1])
import torch
u = importlib.import_module("uv-slam_amd")
abi = u.abi
w = u.synth.make_window(3, n_points=3000, n_lines=400)
cus = torch.cuda.get_device_properties(0).multi_processor_count
L = u.api.lib()
L.uvs_debug_pack_layout.argtypes = [C.POINTER(abi.Options), C.POINTER(abi.WindowC), C.POINTER(C.c_int32)]
os.environ["UVS_DEBUG_CHUNK_GRID"] = str(cus - 1)      # the grid uvs_large_begin / uvs_large_solve_fused pack for
wc, keep = w.to_c(); info = (C.c_int32 * 12)()
assert L.uvs_debug_pack_layout(C.byref(abi.default_options()), C.byref(wc), info) == abi.UVS_OK
del os.environ["UVS_DEBUG_CHUNK_GRID"]

def cycle():
    s = u.api.Solver(max_batch=1, max_points=len(w.inv_depth), max_point_obs=len(w.pt_lm), max_lines=len(w.line_orth), max_line_obs=len(w.ln_lm))
    s.large_solve_fused(w)
    s.large_solve(w)
    s.close()

cycle()      # warm-up: the runtime's own first-use allocations
torch.cuda.synchronize()
free0 = torch.cuda.mem_get_info(0)[0]
for _ in range(int(sys.argv[2])):
    cycle()
torch.cuda.synchronize()
free1 = torch.cuda.mem_get_info(0)[0]
print(json.dumps({"cus": cus, "n_chunks": info[2], "drop_bytes": free0 - free1}))
"""


def run_cycles(cycles=CYCLES, env=None):
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(cycles)], env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_solver_close_frees_the_large_window_buffers():
    res = run_cycles()
    assert res["n_chunks"] >= res["cus"] - 1, res      # every chunk workgroup has a partial row
    assert res["drop_bytes"] < MARGIN_BYTES, res
