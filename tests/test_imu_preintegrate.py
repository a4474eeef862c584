"""IMU pre-integration on the GPU (uvs_imu_*, csrc/uvs_imu_preintegrate.hip) against the 60-digit values of tests/imu_ref.py.

The bound is never a literal: for every class of interval length E_ref is the largest error of synth.PreIntegration (dead reckoning: its numpy
restatement) against the 60-digit values over the class's cases (tests/imu_cases.py), and the device is held to 8 * max(E_ref, 2^-53) in every
metric of imu_ref.errors -- tests/test_imu_ref.py shows that six planted defects miss that bound.  sum_dt may be one rounding per sample away
from the 60-digit sum; skip, frame_i and the structural zeros and ones of the Jacobian are exact.  Each test prints what it measured before it asserts."""
import ctypes as C
import os

import numpy as np
import pytest

import imu_cases as ic
import imu_ref
from helpers import abi, pose_deltas, synth, uvs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so")
ALL = [(n, c) for n in ic.CLASSES for c in range(ic.N_CASES[n])]


def fmt(err):
    return {k: (f"{v:.1e}" if isinstance(v, float) else v) for k, v in err.items()}


def same_bytes(a, b):
    return a.tobytes() == b.tobytes()


def case(k):
    return ic.cases(ALL[k][0])[ALL[k][1]]


@pytest.fixture(scope="module")
def imu():
    h = uvs.api.ImuPreintegrator(device=0, max_intervals=2600, max_samples=120000)
    yield h
    h.close()


@pytest.fixture(scope="module")
def mixed(imu):
    """ONE call over every case of every class, lengths mixed, with the dead reckoning -> (blocks, pred_p, pred_R, pred_v), indexed like ALL."""
    ivs = [ic.cases(n)[c] for n, c in ALL]; sts = [ic.states(n)[c] for n, c in ALL]
    return imu.preintegrate(abi.imu_batch_of(ivs, sts, ic.GRAVITY))


@pytest.mark.parametrize("n", ic.CLASSES)
def test_blocks_against_sixty_digits(mixed, n):
    blocks = mixed[0]
    for k, (cls, c) in enumerate(ALL):
        if cls != n:
            continue
        iv, h, blk = ic.cases(n)[c], ic.hp(n, c), blocks[k]
        err = imu_ref.errors(blk, h)
        print(f"class {n} case {c}: device {fmt(err)}; E_ref {fmt(ic.e_ref(n))}")
        assert not imu_ref.within(err, ic.e_ref(n), n)
        assert int(blk["skip"]) == int(float(h["sum_dt"]) > 10.0) == int(n == 2001) and int(blk["frame_i"]) == iv["frame_i"]
        assert np.array_equal(blk["linearized_ba"], iv["ba"]) and np.array_equal(blk["linearized_bg"], iv["bg"])
        J = blk["jacobian"]
        assert np.array_equal(J[0:3, 6:9], blk["sum_dt"] * np.eye(3))          # sum_dt * I, to the bit
        if n >= 2:
            np.linalg.cholesky(blk["covariance"])
        if n == 0:
            assert np.array_equal(J, np.eye(15)) and not blk["covariance"].any() and blk["sum_dt"] == 0.0
            assert np.array_equal(blk["delta_q"], [0, 0, 0, 1]) and not blk["delta_p"].any() and not blk["delta_v"].any()


@pytest.mark.parametrize("n", ic.CLASSES)
def test_dead_reckoning_against_sixty_digits(mixed, n):
    _, pp, pR, pv = mixed
    for k, (cls, c) in enumerate(ALL):
        if cls != n:
            continue
        err = imu_ref.dr_errors(pp[k], pR[k], pv[k], ic.hp(n, c))
        print(f"class {n} case {c}: device {fmt(err)}; E_ref {fmt({m: ic.e_ref(n)[m] for m in imu_ref.DR_METRICS})}")
        assert not imu_ref.within(err, ic.e_ref(n), n)
        if n == 0:
            st = ic.states(n)[c]
            assert np.array_equal(pp[k], st[0]) and np.array_equal(pR[k], st[1]) and np.array_equal(pv[k], st[2])


def test_predictions_untouched_without_dead_reckoning(imu, mixed):
    ivs = [ic.cases(20)[0], ic.cases(2)[1]]
    rc, blocks, pp, pR, pv = imu.preintegrate_raw(abi.imu_batch_of(ivs))
    assert rc == abi.UVS_OK
    assert np.all(pp == imu.FILL) and np.all(pR == imu.FILL) and np.all(pv == imu.FILL)
    assert same_bytes(blocks[0], mixed[0][ALL.index((20, 0))]) and same_bytes(blocks[1], mixed[0][ALL.index((2, 1))])      # and the blocks do not depend on it


def test_every_interval_alone_and_in_a_crowd(imu, mixed):
    """A block does not depend on its neighbours: alone, in the mixed call, and among 2 561 intervals (more waves than one round of the machine)."""
    blocks = mixed[0]
    for k, (n, c) in enumerate(ALL):
        alone = imu.preintegrate(abi.imu_batch_of([ic.cases(n)[c]]))
        assert same_bytes(alone[0], blocks[k]), (n, c)
    short = [k for k, (n, c) in enumerate(ALL) if n <= ic.CHUNK + 1]
    pick = [short[j % len(short)] for j in range(2561)]
    crowd = imu.preintegrate(abi.imu_batch_of([case(k) for k in pick]))
    bad = [j for j, k in enumerate(pick) if not same_bytes(crowd[j], blocks[k])]
    print(f"2561 intervals, {sum(ALL[k][0] for k in pick)} samples: {len(bad)} blocks differ; kernel {imu.last_device_ms:.3f} ms, call {imu.last_ms:.3f} ms")
    assert not bad


@pytest.mark.parametrize("n", [20, ic.CHUNK + 1])
def test_repropagation_is_a_fresh_integration(imu, n):
    for c, iv in enumerate(ic.cases(n)):
        re = ic.other_biases(iv)
        old, new = imu.preintegrate(abi.imu_batch_of([iv, re]))
        h = ic.hp(n, c, rebias=True)
        err = imu_ref.errors(new, h)
        J = old["jacobian"]; dba, dbg = re["ba"] - iv["ba"], re["bg"] - iv["bg"]
        corrected = dict(imu_ref.preintegrate_synth(re), delta_p=old["delta_p"] + J[0:3, 9:12] @ dba + J[0:3, 12:15] @ dbg,
                         delta_v=old["delta_v"] + J[6:9, 9:12] @ dba + J[6:9, 12:15] @ dbg)
        first = imu_ref.errors(corrected, h)
        print(f"class {n} case {c}: re-propagated {fmt(err)}; first-order correction instead: dp {first['dp']:.1e}, dv {first['dv']:.1e}")
        assert not imu_ref.within(err, ic.e_ref(n), n)
        assert np.array_equal(new["linearized_ba"], re["ba"]) and np.array_equal(new["linearized_bg"], re["bg"])
        assert {"dp", "dv"} <= set(imu_ref.within(first, ic.e_ref(n), n))          # jacobian * dbias is NOT the expected value


def test_set_noise_changes_the_covariance_and_nothing_else(imu, mixed):
    n, c = 20, 1
    iv, before = ic.cases(n)[c], mixed[0][ALL.index((n, c))]
    noise = (0.2, 0.05, 0.002, 4.0e-5)
    imu.set_noise(*noise)
    try:
        got = imu.preintegrate(abi.imu_batch_of([iv]))[0]
    finally:
        imu.set_noise(*imu_ref.NOISE)
    h = imu_ref.preintegrate_hp(iv, noise=noise)
    err = imu_ref.errors(got, h)
    print(f"other noise: {fmt(err)}; covariance diagonal changed by factors of {(np.diag(got['covariance']) / np.diag(before['covariance'])).min():.1f} .. {(np.diag(got['covariance']) / np.diag(before['covariance'])).max():.1f}")
    assert not imu_ref.within(err, ic.e_ref(n), n)
    for name in abi.IMU_BLOCK_DTYPE.names:
        assert same_bytes(got[name], before[name]) == (name != "covariance"), name
    assert same_bytes(imu.preintegrate(abi.imu_batch_of([iv]))[0], before)          # and the EuRoC values are back


def _refusals():
    iv = lambda: [dict(ic.cases(20)[0]), dict(ic.cases(2)[0])]
    st = lambda: [ic.states(20)[0], ic.states(2)[0]]
    plain = lambda: abi.imu_batch_of(iv())
    reck = lambda: abi.imu_batch_of(iv(), st(), ic.GRAVITY)

    def put(field, index, value, b=None):
        b = b or plain()
        a = np.array(b[field], copy=True); a.reshape(-1)[index] = value; b[field] = a
        return b

    cases = [("null batch", plain(), dict(null=("batch",)), abi.UVS_ERR_INVALID_ARG, "null batch"),
             ("null blocks", plain(), dict(null=("blocks",)), abi.UVS_ERR_INVALID_ARG, "null pointer"),
             ("negative count", plain(), dict(n_intervals=-1), abi.UVS_ERR_INVALID_ARG, "negative"),
             ("sample_begin[0] != 0", put("sample_begin", 0, 1), {}, abi.UVS_ERR_INVALID_ARG, "sample_begin[0]"),
             ("decreasing sample_begin", put("sample_begin", 1, 30), {}, abi.UVS_ERR_INVALID_ARG, "decreases"),
             ("too many intervals", plain(), dict(n_intervals=2601), abi.UVS_ERR_CAPACITY, "intervals"),
             ("too many samples", put("sample_begin", 2, 120001), {}, abi.UVS_ERR_CAPACITY, "samples"),
             ("negative dt", put("dt", 3, -0.005), {}, abi.UVS_ERR_INVALID_ARG, "dt"),
             ("dt not finite", put("dt", 21, np.inf), {}, abi.UVS_ERR_INVALID_ARG, "dt"),
             ("sample not finite", put("gyr", 5, np.nan), {}, abi.UVS_ERR_INVALID_ARG, "sample"),
             ("start sample not finite", put("acc_0", 4, np.inf), {}, abi.UVS_ERR_INVALID_ARG, "sample"),
             ("bias not finite", put("bg", 1, np.nan), {}, abi.UVS_ERR_INVALID_ARG, "bias"),
             ("state set in part", reck(), dict(null=("state_R",)), abi.UVS_ERR_INVALID_ARG, "all null or all set"),
             ("prediction output missing", reck(), dict(null=("pred_v",)), abi.UVS_ERR_INVALID_ARG, "pred_p, pred_R and pred_v")]
    for name in ("sample_begin", "acc_0", "gyr_0", "ba", "bg", "dt", "acc", "gyr"):
        cases.append(("null " + name, plain(), dict(null=(name,)), abi.UVS_ERR_INVALID_ARG, "null"))
    return cases


@pytest.mark.parametrize("case", _refusals(), ids=lambda c: c[0])
def test_refusals(imu, mixed, case):
    name, batch, kw, want_rc, text = case
    rc, blocks, pp, pR, pv = imu.preintegrate_raw(batch, **kw)
    print(name, "->", rc, imu.last_error())
    assert rc == want_rc and text in imu.last_error()
    assert blocks.tobytes() == b"\xa5" * blocks.nbytes and np.all(pp == imu.FILL) and np.all(pR == imu.FILL) and np.all(pv == imu.FILL)      # nothing written
    again = imu.preintegrate(abi.imu_batch_of([ic.cases(20)[0]]))                      # and the handle still works
    assert imu.last_error() == "" and same_bytes(again[0], mixed[0][ALL.index((20, 0))])


def test_noise_refusals_and_empty_call(imu, mixed):
    for bad in ((0.0, 1, 1, 1), (1, -1.0, 1, 1), (1, 1, np.inf, 1), (1, 1, 1, np.nan)):
        assert imu.set_noise_raw(*bad) == abi.UVS_ERR_INVALID_ARG and "positive and finite" in imu.last_error()
    assert same_bytes(imu.preintegrate(abi.imu_batch_of([ic.cases(20)[0]]))[0], mixed[0][ALL.index((20, 0))])          # the values stayed as they were
    rc, blocks, *_ = imu.preintegrate_raw(abi.imu_batch_of([]))
    assert rc == abi.UVS_OK and len(blocks) == 0
    L = uvs.api.lib(); h = C.c_void_p()
    assert L.uvs_imu_create(0, 0, 10, C.byref(h)) == abi.UVS_ERR_INVALID_ARG and L.uvs_imu_create(0, 10, abi.IMU_MAX_SAMPLES + 1, C.byref(h)) == abi.UVS_ERR_CAPACITY
    assert L.uvs_imu_create(0, abi.IMU_MAX_INTERVALS + 1, 10, C.byref(h)) == abi.UVS_ERR_CAPACITY and not h


def test_symbols_and_abi_version():
    L = uvs.api.lib()
    hdr = open(os.path.join(ROOT, "include", "uvs_solver.h")).read()
    for s in ("uvs_imu_create", "uvs_imu_destroy", "uvs_imu_last_error", "uvs_imu_set_noise", "uvs_imu_preintegrate", "uvs_imu_last_device_ms"):
        assert s + "(" in hdr and s in uvs.api.EXPORTS and hasattr(L, s), s
    assert L.uvs_abi_version() == 7 and "#define UVS_ABI_VERSION 7" in hdr
    assert f"#define UVS_IMU_STAGE_CHUNK {abi.IMU_STAGE_CHUNK}" in hdr and C.sizeof(abi.ImuBlock) == abi.IMU_BLOCK_DTYPE.itemsize


def _window_with_samples(index):
    """synth.make_window(index) and the raw IMU messages its blocks were made from (synth._simulate_frames(..., samples=), the route sequence.py uses)."""
    w = synth.make_window(index, n_points=60, n_lines=16, n_tagged=12)
    for attempt in range(50):
        samples = []
        blocks = synth._simulate_frames(np.random.default_rng([1000 + index, attempt]), abi.NUM_FRAMES, samples)[5]
        if all(np.array_equal(b.delta_p, i["delta_p"]) for b, i in zip(blocks, w.imu)):
            return w, samples
    raise AssertionError("the window's IMU samples could not be reproduced")


def test_batch_solve_with_device_blocks(imu):
    """Three windows solved through uvs_batch_* with synth's blocks and with ImuPreintegrator.preintegrate_windows: same terminations and iteration
    counts, poses within the parity bound of tests/test_gpu_parity.py (1e-4 m / 1e-4 rad)."""
    ws, samples = zip(*[_window_with_samples(i) for i in (7, 8, 9)])
    lists = imu.preintegrate_windows(samples, [w.imu[0]["linearized_ba"] for w in ws], [w.imu[0]["linearized_bg"] for w in ws])
    ours = []
    for w, blocks in zip(ws, lists):
        o = w.copy(); o.imu = blocks
        assert len(blocks) == len(w.imu) and [b["frame_i"] for b in blocks] == [b["frame_i"] for b in w.imu]
        ours.append(o)
    s = uvs.api.Solver(device=0, max_batch=4)
    try:
        out = []
        for batch in (list(ws), ours):
            s.upload(batch); s.solve_resident()
            out.append(s.download())
    finally:
        s.close()
    for k, ((sa, ra), (sb, rb)) in enumerate(zip(zip(*out[0]), zip(*out[1]))):
        dp, da = pose_deltas(sa.pose, sb.pose)
        print(f"window {k}: termination {ra.termination} / {rb.termination}, iterations {ra.num_iterations} / {rb.num_iterations}, pose difference {dp:.2e} m, {da:.2e} rad")
        assert ra.termination == rb.termination and ra.num_iterations == rb.num_iterations and ra.status == rb.status == 0
        assert dp < 1e-4 and da < 1e-4


def _segment(path, n_images, use_device):
    lib = C.CDLL(HOST)
    lib.uvs_host_imu_segment.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, abi.c_double_p, abi.c_i32_p, abi.c_double_p, C.c_int, abi.c_i32_p]
    lib.uvs_host_imu_segment.restype = C.c_int
    W, cap = abi.WINDOW_SIZE, 400
    blocks = np.zeros(W, abi.IMU_BLOCK_DTYPE); start = np.zeros((W, 6)); ns = np.zeros(W, np.int32); smp = np.zeros((W, cap, 7)); flags = np.zeros(n_images, np.int32)
    rc = lib.uvs_host_imu_segment(path.encode(), n_images, int(use_device), C.c_void_p(blocks.ctypes.data), abi._dp(start), ns.ctypes.data_as(abi.c_i32_p), abi._dp(smp), cap,
                                  flags.ctypes.data_as(abi.c_i32_p))
    assert rc == 0, rc
    ivs = [dict(acc_0=start[i, :3], gyr_0=start[i, 3:], ba=blocks[i]["linearized_ba"], bg=blocks[i]["linearized_bg"], dt=smp[i, :ns[i], 0], acc=smp[i, :ns[i], 1:4],
                gyr=smp[i, :ns[i], 4:7]) for i in range(W)]
    return blocks, ivs, flags


def test_host_mirror_device_route(tmp_path):
    """A short Estimator segment -- the window filled, the initialStructure stand-in with its re-propagation, a dozen images with both marginalization
    kinds -- with setDeviceIntegration on and off: every pre_integrations[i] of both runs within the bound of the 60-digit values of its own sample
    buffer; off is IntegrationBase's own serial loop to the bit; the switch makes and frees the handle."""
    seq = uvs.sequence.make_sequence(0, n_frames=23)
    path = str(tmp_path / "seq.bin")
    uvs.sequence.save(seq, path)
    off, ivs_off, flags = _segment(path, 23, False)
    on, ivs_on, flags_on = _segment(path, 23, True)
    print("marginalization flags:", flags.tolist())
    assert list(flags[:10]) == [-1] * 10 and {0, 1} <= set(flags[10:]) and len(flags) - 10 >= 12 and np.array_equal(flags, flags_on)
    import test_imu_ref
    for i in range(abi.WINDOW_SIZE):
        n = len(ivs_off[i]["dt"])
        assert n == len(ivs_on[i]["dt"]) and all(np.array_equal(ivs_off[i][k], ivs_on[i][k]) for k in ("acc_0", "gyr_0", "dt", "acc", "gyr"))
        cls = max(c for c in ic.CLASSES if c <= n)          # E_ref grows with the length: the class at or below n samples gives the tighter bound
        for name, blocks, ivs in (("off", off, ivs_off), ("on", on, ivs_on)):
            h = imu_ref.preintegrate_hp(ivs[i])
            err = imu_ref.errors(blocks[i], h)
            print(f"pre_integrations[{i + 1}] ({n} samples, E_ref of class {cls}) {name}: {fmt(err)}")
            assert not imu_ref.within(err, ic.e_ref(cls), n)
            assert int(blocks[i]["frame_i"]) == i and int(blocks[i]["skip"]) == 0
        alone = test_imu_ref.host_integrate(ivs_off[i])                             # off: what IntegrationBase has always computed, to the bit
        assert all(same_bytes(off[i][name], alone[name]) for name in abi.IMU_BLOCK_DTYPE.names if name != "frame_i")
    lib = C.CDLL(HOST)
    assert lib.uvs_host_device_integration_switch() == 7
