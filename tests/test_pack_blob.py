"""The host packing (csrc/uvs_pack.cpp: uvs_window -> the blob every back-end kernel reads) as a stand-alone program, without HIP and without a device.

tools/pack_dump.cpp is compiled with the plain host compiler against the packing unit alone; it packs window files and writes the blobs.  Their SHA-256
must equal tests/golden/pack_blob_digests.json, recorded from the commit BEFORE the packing moved out of uvs_solver.hip (one function of 520 lines then):
every blob stays byte for byte what that commit packed.  The same program must agree with the shipped library's uvs_debug_pack_layout on the twelve
header integers, which ties the stand-alone build to the library's, and every rejection keeps its status and its text."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from helpers import uvs, abi
from test_golden import load as load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pack_blob_digests.json")
BIG = dict(n_points=4000, n_lines=1000, n_tagged=700)      # 27 000 observations: the inner packing threads and the structure cache start at 20 000


def build_driver(directory):
    exe = os.path.join(str(directory), "pack_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tools", "pack_dump.cpp"), os.path.join(ROOT, "uv-slam_amd", "csrc", "uvs_pack.cpp"),
                           "-o", exe, "-pthread"])
    return exe


def pack(exe, directory, name, w, switches=(), env=None):
    """Saves `w`, packs it with the program; -> dict(info = the twelve integers, sha256, out_host, cur_sel, hit, placed) or dict(status, text)."""
    path = os.path.join(str(directory), name + ".win"); blob = os.path.join(str(directory), name + ".blob")
    if w is not None: w.save(path)
    out = subprocess.check_output([exe, path, blob] + list(switches), env=dict(os.environ, **(env or {}))).decode().strip()
    if out.startswith("error "):
        _, status, text = out.split(" ", 2)
        return dict(status=int(status), text=text)
    v = [int(x) for x in out.split()[1:]]
    with open(blob, "rb") as f: raw = f.read()
    os.remove(blob)
    assert len(raw) == v[0]
    return dict(status=0, info=v[:12], out_host=v[12], cur_sel=v[13], hit=v[14], placed=v[15], sha256=hashlib.sha256(raw).hexdigest())


def small_cases():
    """(name, window, switches of the program) of every small case; the rng and the windows are those of test_abi.py::test_pack_layout_host_only."""
    synth = uvs.synth
    rng = np.random.default_rng(5)
    for i in range(24):
        npt, nln = int(rng.integers(20, 300)), int(rng.integers(0, 80))
        w = synth.make_window(24000 + i, n_points=npt, n_lines=nln, n_tagged=int(rng.integers(0, nln + 1)), pt_track=int(rng.integers(3, 10)), ln_track=int(rng.integers(5, 10)))
        mode = i % 4
        if mode in (1, 2): w = synth.add_time_offset(w)
        if mode == 3: w = synth.add_relocalization(w, relo_frame=int(rng.integers(0, 10)), fraction=1.0, seed=i)
        yield f"mix{i:02d}_" + ("plain", "td", "td_ex", "relo")[mode], w, [[], ["td"], ["td", "ex"], []][mode]
    w = synth.add_relocalization(synth.make_window(3), seed=3)
    yield "relo_free_ex", w, ["ex"]
    yield "relo_free_ex_grid64", w, ["ex", "grid=64"]
    for name in ("small_prior", "small_noprior", "small_relo", "canonical_prior", "canonical_vp_heavy", "points_only"):
        yield "golden_" + name, load_golden(name)[1], []
    w = load_golden("canonical_prior")[1]
    yield "canonical_prior_grid8", w, ["grid=8"]
    yield "canonical_prior_grid8_all_blocks", w, ["grid=8", "all"]


def big_windows():
    """The large window, the same one with other values, and the same one with one pt_fj moved (another structure)."""
    a = uvs.synth.make_window(70, **BIG)
    assert len(a.pt_lm) + len(a.ln_lm) >= 20000
    b = a.copy(); b.inv_depth = b.inv_depth * 1.01; b.pose[3, 0] += 0.01; b.speedbias[5, 2] -= 0.02; b.pt_pj[:, 0] += 1e-3; b.ln_sp[:, 1] -= 1e-3; b.line_orth[:, 2] += 1e-3
    c = a.copy()
    last = np.flatnonzero((np.append(c.pt_lm[1:], -1) != c.pt_lm) & (c.pt_fj < 10))[0]      # a landmark's last observation, one frame later: still a valid window
    c.pt_fj[last] += 1
    return a, b, c


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("pack_dump"))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return {row["case"]: row for row in json.load(f)}


def check(got, want):
    assert got["status"] == 0, got
    assert (got["info"][0], got["info"][1], got["info"][2]) == (want["blob_bytes"], want["ws_doubles"], want["n_chunks"])
    assert got["sha256"] == want["sha256"]
    assert got["out_host"] == 0 and got["cur_sel"] == 0      # written later: by upload_windows into the staged header, by the kernel


def test_small_blobs_are_the_parents_bytes_and_the_librarys_header(driver, golden, tmp_path, monkeypatch):
    lib = uvs.api.lib()
    lib.uvs_debug_pack_layout.argtypes = [C.POINTER(abi.Options), C.POINTER(abi.WindowC), C.POINTER(C.c_int32)]
    seen = {}
    for name, w, sw in small_cases():
        got = pack(driver, tmp_path, name, w, sw)
        check(got, golden[name])
        placed = pack(driver, tmp_path, name, None, sw + ["dst"])      # through a PackDst over a heap buffer: the same bytes as in the vector
        assert placed["placed"] == 1 and placed["sha256"] == got["sha256"] and placed["info"] == got["info"]
        seen[name] = got
        # the library's own packing (hipcc's host compiler, inside libuvs_solver.so) reports the same header
        o = abi.default_options(); o.estimate_td = int("td" in sw); o.estimate_extrinsic = int("ex" in sw)
        grid = [s[5:] for s in sw if s.startswith("grid=")]
        if grid: monkeypatch.setenv("UVS_DEBUG_CHUNK_GRID", grid[0])
        else: monkeypatch.delenv("UVS_DEBUG_CHUNK_GRID", raising=False)
        wc, keep = w.to_c(); info = (C.c_int32 * 12)()
        assert lib.uvs_debug_pack_layout(C.byref(o), C.byref(wc), info) == abi.UVS_OK
        # (the export has no all_blocks switch: there the group assignment differs, which of the twelve only n_parts, index 9, can show)
        skip = {9} if "all" in sw else set()
        assert [v for k, v in enumerate(info) if k not in skip] == [v for k, v in enumerate(got["info"]) if k not in skip], name
    monkeypatch.delenv("UVS_DEBUG_CHUNK_GRID", raising=False)
    assert len(seen) == 34 == len([c for c in golden if not c.startswith("big_")])
    # some block of the canonical window has no work: it gets a group under all_blocks only
    assert seen["canonical_prior_grid8"]["sha256"] != seen["canonical_prior_grid8_all_blocks"]["sha256"]
    assert seen["relo_free_ex_grid64"]["info"][2] >= seen["relo_free_ex"]["info"][2] and seen["golden_small_prior"]["info"][10] > 0


def test_large_window_threads_and_structure_cache(driver, golden, tmp_path):
    a, b, c = big_windows()
    fresh = {}
    for name, w in (("big_a", a), ("big_b_values_moved", b), ("big_c_one_fj_moved", c)):
        fresh[name] = pack(driver, tmp_path, name, w, [], env={"UVS_PACK_THREADS": "1"})
        check(fresh[name], golden[name])
    assert fresh["big_a"]["sha256"] != fresh["big_b_values_moved"]["sha256"] != fresh["big_c_one_fj_moved"]["sha256"]
    eight = pack(driver, tmp_path, "big_a", None, [], env={"UVS_PACK_THREADS": "8"})      # the lists do not depend on the thread count
    assert eight["sha256"] == fresh["big_a"]["sha256"] and eight["info"] == fresh["big_a"]["info"]
    first = "cache=" + os.path.join(str(tmp_path), "big_a.win")
    for threads in ("1", "8"):
        hit = pack(driver, tmp_path, "big_b_values_moved", None, [first], env={"UVS_PACK_THREADS": threads})      # same structure: only the value sections are rewritten
        assert hit["hit"] == 1 and hit["sha256"] == fresh["big_b_values_moved"]["sha256"] and hit["info"] == fresh["big_b_values_moved"]["info"]
    miss = pack(driver, tmp_path, "big_c_one_fj_moved", None, [first], env={"UVS_PACK_THREADS": "8"})
    assert miss["hit"] == 0 and miss["sha256"] == fresh["big_c_one_fj_moved"]["sha256"]
    placed = pack(driver, tmp_path, "big_a", None, ["dst"], env={"UVS_PACK_THREADS": "8"})
    assert placed["placed"] == 1 and placed["sha256"] == fresh["big_a"]["sha256"]


def rejections():
    """(name, window, switches, status, text): every rejection of validate_window / pack_window a window file can carry, with the status and the text of the
    commit before the move.  ("single ... landmark exceeds LDS staging" is not among them: a landmark that passes validate_window has at most 11
    observations, and one landmark per chunk always fits.)"""
    base = uvs.synth.make_window(11, n_points=30, n_lines=8, n_tagged=4)
    w = base.copy(); w.pt_lm[0] = w.pt_lm[-1]
    yield "ungrouped", w, [], abi.UVS_ERR_INVALID_ARG, "point observations must be grouped by non-decreasing landmark index"
    w = base.copy(); k = int(np.flatnonzero(w.pt_lm[1:] == w.pt_lm[:-1])[0]); w.pt_fj[k + 1] = w.pt_fj[k]
    yield "frame_order", w, [], abi.UVS_ERR_INVALID_ARG, "point observations of one landmark must share imu_i and have increasing imu_j"
    w = base.copy(); w.ln_fj[0] = 11
    yield "line_frame", w, [], abi.UVS_ERR_INVALID_ARG, "line observation frame out of range"
    w = uvs.synth.add_relocalization(base.copy(), seed=1); assert len(w.relo_lm) >= 2; w.relo_lm[1] = w.relo_lm[0]
    yield "relo_lm_order", w, [], abi.UVS_ERR_INVALID_ARG, "relo_lm must be strictly increasing and name landmarks that have observations"
    yield "td_arrays_missing", base, ["td"], abi.UVS_ERR_INVALID_ARG, "estimate_td needs pt_vel_i / pt_vel_j / pt_td_i / pt_td_j"

    def with_prior(mutate):
        w = base.copy(); p = abi.Prior(); p.n = 15; p.n_blocks = 2
        p.block_kind[0] = abi.BLOCK_POSE; p.block_frame[0] = 0; p.block_size[0] = 7; p.block_idx[0] = 0; p.x0_off[0] = 0
        p.block_kind[1] = abi.BLOCK_SPEEDBIAS; p.block_frame[1] = 0; p.block_size[1] = 9; p.block_idx[1] = 6; p.x0_off[1] = 7
        p.x0[6] = 1.0
        for k in range(15): p.linearized_jacobians[k * 15 + k] = 1.0
        mutate(p); w.prior = p
        return w
    yield "prior_ok", with_prior(lambda p: None), [], abi.UVS_OK, ""
    yield "prior_kind_size", with_prior(lambda p: p.block_size.__setitem__(0, 9)), [], abi.UVS_ERR_INVALID_ARG, "prior block kind / size mismatch"
    yield "prior_x0_off", with_prior(lambda p: p.x0_off.__setitem__(1, 144 - 8)), [], abi.UVS_ERR_INVALID_ARG, "prior x0 offset out of range"
    yield "prior_overlap", with_prior(lambda p: p.block_idx.__setitem__(1, 3)), [], abi.UVS_ERR_INVALID_ARG, "prior keeps a parameter block twice / its blocks overlap"
    yield "prior_twice", with_prior(lambda p: (p.block_kind.__setitem__(1, abi.BLOCK_POSE), p.block_size.__setitem__(1, 7))), [], abi.UVS_ERR_INVALID_ARG, "prior keeps a parameter block twice / its blocks overlap"


def test_rejections_keep_status_and_text(driver, tmp_path):
    for name, w, sw, status, text in rejections():
        got = pack(driver, tmp_path, name, w, sw)
        assert got["status"] == status and got.get("text", "") == text, (name, got)
