"""Seeded intervals for the IMU pre-integration (tests/test_imu_ref.py on the CPU, tests/test_imu_preintegrate.py on the GPU), their 60-digit
values and E_ref (computed once per process and shared: nothing modifies them; the 60-digit run of the long cases is what costs time, a few
seconds, so it is cached here and never stored in git).

Every interval: 200 Hz, the accelerometer reads gravity plus 1 .. 1.5 m/s^2 of excitation (so no compared vector is near zero), the gyroscope
0.3 .. 0.5 rad/s, biases of 0.1 m/s^2 and 0.01 rad/s, EuRoC noise.  Classes by sample count: 0, 1, 2, 20, 61, the kernel's staging chunk plus
one (65), 200, 1 980 (9.9 s: skip == 0) and 2 001 (sum_dt > 10: skip == 1).  The short classes hold four cases -- the last one of each
with irregular dt in 0.004 .. 0.006 and one sample of dt == 0 where the class has three samples or more -- the classes of 200 and more two;
a case of 1 980 samples is the first 1 980 samples of the case of 2 001 with the same number, so one 60-digit run serves both.

E_ref[class][metric]: the largest error of synth.PreIntegration (dead reckoning: imu_ref.dead_reckon_np) against the 60-digit values over the
class's cases.  The class of 0 samples has E_ref = 0 in every metric by construction (nothing is computed); the bound's floor 2^-53 covers it.

TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import imu_ref
from helpers import abi

CHUNK = abi.IMU_STAGE_CHUNK
CLASSES = (0, 1, 2, 20, 61, CHUNK + 1, 200, 1980, 2001)
N_CASES = {n: (1 if n == 0 else 4 if n < 200 else 2) for n in CLASSES}
GRAVITY = np.array([0.0, 0.0, 9.81007])
SEED = 7300


def _rotation(rng):
    q = rng.standard_normal(4); q /= np.linalg.norm(q)
    return np.array(imu_ref.quat_R(q), float)


@functools.lru_cache(maxsize=None)
def _trajectory(n, c):
    """(interval, dead-reckoning state) of case c of the class of n samples (n = 1 980: a prefix of the case of 2 001)."""
    if n == 1980:
        iv, st = _trajectory(2001, c)
        return dict(iv, dt=iv["dt"][:n], acc=iv["acc"][:n], gyr=iv["gyr"][:n]), st
    rng = np.random.default_rng([SEED, n, c])
    amp_a, amp_g = rng.uniform(1.0, 1.5, 3), rng.uniform(0.3, 0.5, 3)
    fa, fg, pa, pg = rng.uniform(0.3, 1.5, 3), rng.uniform(0.3, 1.5, 3), rng.uniform(0, 2 * np.pi, 3), rng.uniform(0, 2 * np.pi, 3)
    tilt = _rotation(rng)
    irregular = n < 200 and c == N_CASES[n] - 1 and n > 0
    dt = rng.uniform(0.004, 0.006, n) if irregular else np.full(n, 0.005)
    if irregular and n >= 3:
        dt[n // 2] = 0.0
    t = np.r_[0.0, np.cumsum(dt)]
    meas = lambda tt: (tilt @ GRAVITY + amp_a * np.sin(2 * np.pi * fa * tt + pa), amp_g * np.sin(2 * np.pi * fg * tt + pg))
    a, g = zip(*[meas(tt) for tt in t])
    a, g = np.array(a), np.array(g)
    ba = 0.1 * np.sign(rng.standard_normal(3)) * rng.uniform(0.8, 1.0, 3); bg = 0.01 * np.sign(rng.standard_normal(3)) * rng.uniform(0.8, 1.0, 3)
    iv = dict(acc_0=a[0], gyr_0=g[0], ba=ba, bg=bg, dt=dt, acc=a[1:].reshape(-1, 3), gyr=g[1:].reshape(-1, 3), frame_i=int(rng.integers(0, 10)))
    state = (rng.uniform(-5, 5, 3), _rotation(rng), rng.uniform(-1.5, 1.5, 3) + np.array([1.0, 0.0, 0.0]))
    return iv, state


def cases(n):
    """The intervals of the class of n samples."""
    return [_trajectory(n, c)[0] for c in range(N_CASES[n])]


def states(n):
    return [_trajectory(n, c)[1] for c in range(N_CASES[n])]


def other_biases(iv):
    """The interval with other biases (re-propagation): 0.02 m/s^2 and 0.003 rad/s away."""
    return dict(iv, ba=iv["ba"] + np.array([0.02, -0.02, 0.01]), bg=iv["bg"] + np.array([-0.003, 0.002, 0.003]))


def hp(n, c, rebias=False):
    """The 60-digit values of case c of class n, with its dead reckoning (rebias: with other_biases)."""
    return _hp(int(n), int(c), bool(rebias))


@functools.lru_cache(maxsize=None)
def _hp(n, c, rebias):
    if n == 1980:
        return _hp(2001, c, rebias)["at"][1980]
    iv, st = _trajectory(n, c)
    return imu_ref.preintegrate_hp(other_biases(iv) if rebias else iv, state=st, gravity=GRAVITY, snapshots=(1980,) if n == 2001 else ())


@functools.lru_cache(maxsize=None)
def e_ref(n):
    """E_ref of the class: per metric the largest error of the numpy restatement over the class's cases."""
    out = dict.fromkeys(imu_ref.METRICS + imu_ref.DR_METRICS, 0.0)
    for c, (iv, st) in enumerate(zip(cases(n), states(n))):
        h = hp(n, c)
        err = imu_ref.errors(imu_ref.preintegrate_synth(iv), h)
        if n > 0:
            err.update(imu_ref.dr_errors(*imu_ref.dead_reckon_np(iv, st, GRAVITY), h))
        for m in out:
            out[m] = max(out[m], err.get(m, 0.0))
    return out
