"""The reference of the IMU pre-integration tests (tests/imu_ref.py, tests/imu_cases.py) has teeth, and the host mirror's IntegrationBase meets it.

No bound is a literal: for each class of interval length E_ref is the largest error of synth.PreIntegration against the 60-digit values over the
class's cases, and a statement of the rule passes when every metric is within 8 * max(E_ref, 2^-53) (imu_ref.within).  Here: E_ref is finite and
positive, the 60-digit engine equals an mpmath evaluation, the structural zeros and ones hold in the reference, six planted defects in a copy of
the numpy restatement each miss the bound, and IntegrationBase of the host mirror (push_back, and repropagate with other biases), driven
through uvs_host_imu_integrate, lies within the bound -- which holds IntegrationBase to an independent value for the first time.
No GPU is needed."""
import ctypes as C
import decimal
import os

import numpy as np
import pytest

import imu_cases as ic
import imu_ref
from helpers import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "uv-slam_amd", "libuvs_host.so")


def host_integrate(iv, rebias=None):
    """IntegrationBase over the interval through the hook -> one record of abi.IMU_BLOCK_DTYPE."""
    lib = C.CDLL(HOST)
    lib.uvs_host_imu_integrate.argtypes = [C.c_int] + [abi.c_double_p] * 9 + [C.c_void_p]; lib.uvs_host_imu_integrate.restype = C.c_int
    f = lambda a: np.ascontiguousarray(a, np.float64).reshape(-1)
    arrs = [f(iv[k]) for k in ("acc_0", "gyr_0", "ba", "bg", "dt", "acc", "gyr")]
    arrs = [a if a.size else np.zeros(3) for a in arrs]
    re = [f(rebias["ba"]), f(rebias["bg"])] if rebias is not None else [None, None]
    out = np.zeros(1, abi.IMU_BLOCK_DTYPE)
    rc = lib.uvs_host_imu_integrate(len(np.atleast_1d(iv["dt"])), *[abi._dp(a) for a in arrs], *[None if a is None else abi._dp(a) for a in re], C.c_void_p(out.ctypes.data))
    assert rc == 0, rc
    return out[0]


@pytest.mark.parametrize("n", ic.CLASSES)
def test_e_ref_is_finite_and_positive(n):
    e = ic.e_ref(n)
    print(n, {k: f"{v:.1e}" for k, v in e.items()})
    assert all(np.isfinite(v) and v >= 0 for v in e.values())
    if n == 0:          # nothing is computed: every error is exactly zero, and the bound is its floor
        assert all(v == 0 for v in e.values()) and 8.0 * max(e["J"], imu_ref.EPS) > 0
    else:
        assert all(v > 0 for v in e.values()), e


def test_sixty_digit_engine_equals_mpmath():
    iv = ic.cases(20)[3]                                       # irregular dt, one dt == 0
    h, m = ic.hp(20, 3), imu_ref.preintegrate_mpmath(iv)
    worst = 0.0
    with decimal.localcontext() as ctx:
        ctx.prec = 80
        for key in ("dp", "dq", "dv", "J", "C"):
            a = np.asarray(h[key], object).reshape(-1); b = np.asarray(m[key], object).reshape(-1)
            for x, y in zip(a, b):
                y = decimal.Decimal(y)
                assert (x == 0) == (y == 0)
                if x != 0:
                    worst = max(worst, float(abs((x - y) / x)))
        assert decimal.Decimal(m["sum_dt"]) == h["sum_dt"]
    print(f"Decimal engine against mpmath at {imu_ref.DPS} digits: largest relative difference {worst:.1e}")
    assert worst < 1e-50          # both carry 60 digits; ten are left for the cancellation inside the sums


@pytest.mark.parametrize("n", [c for c in ic.CLASSES if c > 0])
def test_structural_zeros_and_ones_of_the_reference(n):
    for c, iv in enumerate(ic.cases(n)):
        h = ic.hp(n, c)
        J = h["J"]
        for i in range(15):
            for j in range(15):
                if i >= 9 or j < 3:
                    assert J[i][j] == (1 if i == j else 0), (i, j)
        for (rb, cb) in ((1, 2), (1, 3), (3, 4), (4, 3)):
            assert all(J[3 * rb + a][3 * cb + b] == 0 for a in range(3) for b in range(3))
        for a in range(3):
            for b in range(3):
                assert J[a][6 + b] == (h["sum_dt"] if a == b else 0) and J[6 + a][6 + b] == (1 if a == b else 0)
        assert imu_ref.errors(imu_ref.preintegrate_synth(iv), h)["structure"] == 0


def test_the_copy_is_the_restatement():
    for n in (2, 20, ic.CHUNK + 1):
        for iv in ic.cases(n):
            a, b = imu_ref.preintegrate_np(iv), imu_ref.preintegrate_synth(iv)
            assert all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


@pytest.mark.parametrize("defect", imu_ref.DEFECTS)
def test_planted_defects_miss_the_bound(defect):
    for n in (2, 20, 200):
        for c, iv in enumerate(ic.cases(n)):
            err = imu_ref.errors(imu_ref.preintegrate_np(iv, defect=defect), ic.hp(n, c))
            bad = imu_ref.within(err, ic.e_ref(n), n)
            print(defect, n, c, bad, {k: f"{err[k]:.1e}" for k in bad if k in err})
            assert bad, (defect, n, c)


@pytest.mark.parametrize("n", ic.CLASSES)
def test_host_mirror_integration_base(n):
    for c, iv in enumerate(ic.cases(n)):
        blk = host_integrate(iv)
        err = imu_ref.errors(blk, ic.hp(n, c))
        print(n, c, {k: (f"{v:.1e}" if isinstance(v, float) else v) for k, v in err.items()})
        assert not imu_ref.within(err, ic.e_ref(n), n)
        assert int(blk["skip"]) == int(float(ic.hp(n, c)["sum_dt"]) > 10.0) == int(n == 2001)
        assert np.array_equal(blk["linearized_ba"], iv["ba"]) and np.array_equal(blk["linearized_bg"], iv["bg"])
        if n >= 2:
            np.linalg.cholesky(blk["covariance"])


@pytest.mark.parametrize("n", [20, ic.CHUNK + 1])
def test_host_mirror_repropagate(n):
    for c, iv in enumerate(ic.cases(n)):
        re = ic.other_biases(iv)
        blk = host_integrate(iv, rebias=re)
        h = ic.hp(n, c, rebias=True)
        err = imu_ref.errors(blk, h)
        first_order = imu_ref.errors(dict(imu_ref.preintegrate_synth(iv), sum_dt=blk["sum_dt"]), h)
        print(n, c, {k: (f"{v:.1e}" if isinstance(v, float) else v) for k, v in err.items()}, "unchanged block:", f"{first_order['dp']:.1e}")
        assert not imu_ref.within(err, ic.e_ref(n), n)
        assert np.array_equal(blk["linearized_ba"], re["ba"]) and np.array_equal(blk["linearized_bg"], re["bg"])
        assert imu_ref.within(first_order, ic.e_ref(n), n)          # the block at the old biases is not the answer
