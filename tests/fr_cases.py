"""Scenes for the tests of uvs_ft_reject: synthetic 3-D points seen from two poses, as normalized points, with Gaussian noise given in pixels at
focal length 460 and a share of gross outliers displaced by 5 .. 35 px.  TEST INFRASTRUCTURE ONLY.  ref(name) is the numpy restatement's answer
(tests/fr_ref.py), computed once per process and shared."""
import functools

import numpy as np

import fr_ref

FOCAL = 460.0
THRESHOLD = 1.0 / FOCAL             # F_THRESHOLD / FOCAL_LENGTH
CONFIDENCE = 0.99

MOTIONS = {                          # rotation vector (rad), translation (m) of the second camera: X2 = R X1 + t
    "general": ((0.02, -0.03, 0.01), (0.15, -0.05, 0.04)),
    "forward": ((0.0, 0.0, 0.0), (0.01, -0.005, 0.30)),
    "rotation": ((0.03, -0.04, 0.02), (0.0, 0.0, 0.0)),
    "rest": ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
}


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def scene(motion, n, outlier_share=0.0, noise_px=0.0, seed=1):
    """-> dict(prev [n, 2], next [n, 2], outlier [n] bool, E [3, 3] the true essential matrix (x2' E x1 = 0), seed)."""
    rng = np.random.default_rng(seed)
    w, t = MOTIONS[motion]
    R = rodrigues(w); t = np.asarray(t, np.float64)
    X = np.c_[rng.uniform(-2.5, 2.5, n), rng.uniform(-1.6, 1.6, n), rng.uniform(3.0, 9.0, n)]
    prev = X[:, :2] / X[:, 2:]
    if motion == "rest":
        nxt = prev.copy()
    else:
        X2 = X @ R.T + t
        nxt = X2[:, :2] / X2[:, 2:]
    if noise_px > 0:
        nxt = nxt + rng.normal(0.0, noise_px / FOCAL, nxt.shape)
    outlier = np.zeros(n, bool)
    m = int(round(outlier_share * n))
    if m:
        pick = rng.choice(n, m, replace=False)
        ang = rng.uniform(0, 2 * np.pi, m); mag = rng.uniform(5.0, 35.0, m) / FOCAL
        nxt[pick] += np.c_[mag * np.cos(ang), mag * np.sin(ang)]
        outlier[pick] = True
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return dict(prev=np.ascontiguousarray(prev), next=np.ascontiguousarray(nxt), outlier=outlier, E=tx @ R, seed=1000 + seed)


# name -> (motion, n, outlier share, noise px, seed).  n = 8, 9, 12: the smallest items; 300: more tracks than a round has hypotheses; the shares
# make the loop end in the first round (0 %, 20 %), in a later round (50 % with 0.3 px of noise) and at 1 000 (50 % with 0.5 px)
CASES = {
    "general_8": ("general", 8, 0.0, 0.0, 3),
    "general_9": ("general", 9, 0.0, 0.1, 4),
    "general_12": ("general", 12, 0.0, 0.3, 5),
    "forward_40": ("forward", 40, 0.2, 0.3, 6),
    "general_150": ("general", 150, 0.0, 0.0, 7),
    "general_150_o20": ("general", 150, 0.2, 0.3, 8),
    "general_150_o50": ("general", 150, 0.5, 0.3, 9),
    "general_150_o50_n05": ("general", 150, 0.5, 0.5, 21),
    "general_150_o20_clean": ("general", 150, 0.2, 0.0, 14),
    "forward_150_o20": ("forward", 150, 0.2, 0.0, 33),
    "rotation_150": ("rotation", 150, 0.2, 0.3, 11),
    "rest_150": ("rest", 150, 0.0, 0.0, 12),
    "general_300_o20": ("general", 300, 0.2, 0.3, 13),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return scene(*CASES[name])


@functools.lru_cache(maxsize=None)
def ref(name):
    """fr_ref's answer for the case; shared, so leave it unchanged."""
    sc = case(name)
    return fr_ref.reject(sc["prev"], sc["next"], sc["seed"], THRESHOLD, CONFIDENCE)
