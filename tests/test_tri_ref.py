"""The references of the triangulation of landmarks (tests/tri_ref.py, tests/tri_cases.py), on the CPU: the 60-digit evaluation is the truth on
noise-free scenes, the numpy restatement stays within its measured error of it, and the bounds tests/test_triangulate.py holds the device to
catch the defects planted here -- above all the normal-equation shortcut on the low-parallax classes.

E_ref, the largest error of the numpy SVD restatement against the 60-digit values, as measured on the committed seeds:
    class       points (relative depth)   lines (entries of U(psi), phi)
    0.2 m       1.2e-13                   1.8e-14
    0.02 m      9.8e-13                   5.2e-14
    0.002 m     3.9e-12                   1.6e-13
The normal-equation route reaches 1.1e-13, 1.8e-11 and 4.5e-10: 0.9, 18 and 113 times E_ref, so the 8 E_ref bound separates it on the two
low-parallax classes and, as it should, not on the 0.2 m class where the two routes agree."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import tri_cases as tc
import tri_ref
from helpers import abi, uvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 8.0          # the multiple of E_ref the device is held to (tests/test_triangulate.py)
CLASSES = tuple(tc.BASELINES)


def test_scenes_cover_the_shapes_they_promise():
    for cls in CLASSES:
        b = tc.scene(cls)
        views = np.diff(b["pt_obs_begin"])
        assert [int((b["pt_window"] == w).sum()) for w in range(3)] == list(tc.COUNTS) == [int((b["ln_window"] == w).sum()) for w in range(3)]
        assert views.min() == 2 and views.max() == 11 and b["pt_start"].min() == 0 and b["pt_start"].max() == 9
        assert np.all(b["pt_start"] + views <= 11) and np.all(np.diff(b["pt_window"]) >= 0)
        gap = b["ln_fj"] - b["ln_fi"]
        assert gap.min() == 1 and gap.max() == 10 and b["ln_fj"].max() == 10
        assert 1.5 <= b["true_depth"].min() and b["true_depth"].max() <= 12.0


def test_sixty_digits_recover_the_truth_on_noise_free_scenes():
    for cls in CLASSES:
        b = tc.scene(cls, 0.0)
        _, hp = tc.refs(cls, 0.0)
        assert np.all(hp["pt_flag"] == 0) and np.all(hp["ln_flag"] == 0)
        # the FP64 observations of an exact point are themselves rounded: 1e-16 of bearing over a parallax of baseline / depth
        assert np.abs(hp["raw"] / b["true_depth"] - 1).max() < 1e-16 * 12.0 / tc.BASELINES[cls] * 100
        for U, phi, L in zip(hp["U"], hp["phi"], b["true_plucker"]):
            P = np.r_[np.cos(phi) * U[:, 0], np.sin(phi) * U[:, 1]]
            Ln = L / np.linalg.norm(L)
            assert min(np.abs(P - Ln).max(), np.abs(P + Ln).max()) < 1e-16 * 12.0 / tc.BASELINES[cls] * 1000


def test_numpy_restatement_stays_within_its_measured_error():
    measured = {"0.2": (1.2e-13, 1.8e-14), "0.02": (9.8e-13, 5.2e-14), "0.002": (3.9e-12, 1.6e-13)}      # the table of the docstring
    for cls in CLASSES:
        (_, pf, _, lf), hp = tc.refs(cls)
        ep, keep = tc.e_ref_points(cls)
        el, ok = tc.e_ref_lines(cls)
        print(f"class {cls}: E_ref points {ep:.2e} ({int(keep.sum())} of {len(keep)} compared), lines {el:.2e}")
        assert keep.all() and ok.all()          # the seeds put no depth within 1e-9 of the threshold and no NaN
        assert np.array_equal(pf, hp["pt_flag"]) and np.array_equal(lf, hp["ln_flag"])
        assert ep <= 2 * measured[cls][0] and el <= 2 * measured[cls][1]
        assert np.abs(hp["raw"] - tri_ref.THRESHOLD).min() > 1e-6
    assert (tc.refs("0.002")[1]["pt_flag"] == 1).sum() >= 5          # hand-held parallax under this noise does throw depths below the threshold


def test_edge_cases_get_their_flags_in_both_references():
    b = tc.edge()
    (depth, pf, orth, lf), hp = tc.refs("edge")
    assert np.array_equal(pf, b["expect_pt_flag"]) and np.array_equal(hp["pt_flag"], b["expect_pt_flag"])
    assert np.array_equal(lf, b["expect_ln_flag"]) and np.array_equal(hp["ln_flag"], b["expect_ln_flag"])
    assert depth[1] == depth[2] == tc.INIT_DEPTH and hp["raw"][1] < 0 and hp["raw"][2] == 0.0 and np.all(orth[1] == 0)


def _planted_point_errors(cls, fn):
    b = tc.scene(cls)
    _, hp = tc.refs(cls)
    depth = tri_ref.triangulate(dict(b, ln_window=np.zeros(0, np.int32)), tc.INIT_DEPTH, point_fn=fn)[0]
    e, keep = tc.e_ref_points(cls)
    return float(tri_ref.depth_errors(depth[keep], hp["depth"][keep]).max()), e


def test_bound_catches_the_normal_equations_on_the_low_parallax_classes():
    for cls in ("0.02", "0.002"):
        err, e = _planted_point_errors(cls, tri_ref.point_depth_normal_equations)
        print(f"class {cls}: normal equations {err:.2e} = {err / e:.1f} E_ref")
        assert err > BOUND * e
    err, e = _planted_point_errors("0.2", tri_ref.point_depth_normal_equations)
    assert err <= BOUND * e          # ... and at 0.2 m the two routes agree, which the host-route comparison of the GPU tests relies on


def test_bound_catches_the_planted_line_defects():
    for cls in CLASSES:
        b = tc.scene(cls)
        _, hp = tc.refs(cls)
        el, ok = tc.e_ref_lines(cls)
        # beta with the wrong sign: the moment flips against the direction
        orth = tri_ref.triangulate(dict(b, pt_window=np.zeros(0, np.int32)), tc.INIT_DEPTH, line_defect="beta_sign")[2]
        assert tri_ref.line_errors(orth[ok], hp["U"][ok], hp["phi"][ok]).max() > BOUND * el
        # the other Euler branch stands for the same U: the range check of the first angle is what catches it
        orth = tri_ref.triangulate(dict(b, pt_window=np.zeros(0, np.int32)), tc.INIT_DEPTH, line_defect="euler_branch")[2]
        assert tri_ref.line_errors(orth[ok], hp["U"][ok], hp["phi"][ok]).max() <= BOUND * el
        assert not np.all((orth[:, 0] >= 0) & (orth[:, 0] <= np.pi)) and np.all((tc.refs(cls)[0][2][:, 0] >= 0) & (tc.refs(cls)[0][2][:, 0] <= np.pi))


def test_bound_catches_the_second_last_line_observation():
    """A line seen in three frames, triangulated from the first and the SECOND one instead of the last: under noise that is another line."""
    rng = np.random.default_rng(9240)
    b = tc.scene("0.2")
    cams = tri_ref.cameras(b["pose"][1], b["ex_pose"][1]); hp_cams = tri_ref.cameras_hp(b["pose"][1], b["ex_pose"][1])
    el, _ = tc.e_ref_lines("0.2")
    caught = 0
    for _ in range(8):
        A = cams[1][2] + cams[0][2] @ np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4, 9)])
        d = rng.standard_normal(3); d /= np.linalg.norm(d)
        ends = {f: [tc._noisy(rng, tc._view(cams, f, A + s * d), tc.NOISE) for s in (-0.7, 0.6)] for f in (2, 5, 8)}
        U, phi, flag = tri_ref.line_hp(hp_cams, 2, 8, *ends[2], *ends[8])
        wrong, _ = tri_ref.line_orth(cams, 2, 5, *ends[2], *ends[5])
        caught += flag == 0 and tri_ref.line_errors(wrong[None], U[None], np.array([phi]))[0] > BOUND * el
    assert caught == 8


def test_check_and_shift_references_agree_and_cover_their_cases():
    f64, hp, z = tc.check_refs()
    kind = tc.check_scene()["kind"]
    assert np.array_equal(f64, hp) and np.abs(z).min() > 1e-9
    assert np.all(hp[kind == 0] == 1) and np.all(hp[kind != 0] == 2) and all((kind == k).sum() >= 40 for k in range(3))
    assert np.all((z[kind == 1] < 0).all(axis=1)) and np.all((z[kind == 2] < 0).sum(axis=1) == 1)
    (out, flag, _), zh, (out_hp, flag_hp) = tc.shift_refs()
    assert np.array_equal(flag, flag_hp) and np.abs(zh).min() > 1e-9 and (flag_hp == 1).sum() >= 20 and (flag_hp == 0).sum() >= 100
    e = np.abs(out - out_hp) / np.abs(out_hp)
    print(f"shift_depth: E_ref {e.max():.2e}")
    assert e.max() < 2e-15


def test_ctypes_mirror_and_exports():
    lib = uvs.api.lib()
    hdr = open(os.path.join(ROOT, "include", "uvs_solver.h")).read()
    for s in ("uvs_tri_create", "uvs_tri_destroy", "uvs_tri_last_error", "uvs_tri_set_init_depth", "uvs_tri_triangulate", "uvs_tri_check_lines",
              "uvs_tri_shift_depth", "uvs_tri_last_device_ms"):
        assert s + "(" in hdr and s in uvs.api.EXPORTS and hasattr(lib, s), s
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "uvs_solver.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(uvs_tri_batch), '
            'offsetof(uvs_tri_batch, pose), offsetof(uvs_tri_batch, pt_obs), offsetof(uvs_tri_batch, ln_ep_j)); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(code)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])      # the header is plain C
        want = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert [C.sizeof(abi.TriBatch), abi.TriBatch.pose.offset, abi.TriBatch.pt_obs.offset, abi.TriBatch.ln_ep_j.offset] == want
    b, keep = abi.tri_batch(tc.scene("0.2"))
    assert (b.n_windows, b.n_points, b.n_lines) == (3, 130, 130)
    # without a GPU the handle refuses to exist (on a GPU machine it is made: the GPU tests take it from there)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            uvs.api.Triangulator()


def test_tracks_of_windows_match_an_independent_restatement():
    ws = [uvs.synth.make_window(31, n_points=30, n_lines=8, n_tagged=4), uvs.synth.make_window(32, n_points=17, n_lines=5, n_tagged=2, pt_track=4)]
    got, want = uvs.api.Triangulator.tracks_of(ws), tc.tracks_of_windows(ws)
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]), v), k
    bad = ws[0].copy(); bad.pt_fj = bad.pt_fj.copy(); bad.pt_fj[1] += 1
    with pytest.raises(ValueError):
        uvs.api.Triangulator.tracks_of([bad])
