"""Seeded cases of the vanishing-point tests (tests/test_vanishing_points.py): Manhattan scenes with free lines and pixel noise, and the edge cases
of the estimator.  A case is a dict: segs [n, 4] (x1, y1, x2, y2 in pixels), seed, th (the tag threshold, radians)."""
import math

import numpy as np

import vp_ref

CAM = (461.6, 460.3, 363.0, 248.1)          # fx, fy, cx, cy (EuRoC cam0, config/euroc/euroc_config.yaml)
W, H = 752, 480
# Seeds of the scene cases: the first twelve of 0 .. 21 under which vp_ref's argmax is decided against EVERY other ordered cell triple
# (vp_ref.best_margin, asserted by test_scene_margins_under_the_reference).  In 9 of the 22 scenes two hypotheses with the same three cells
# in another order score equal to the last bit or one ulp apart -- (g0 + g1) + g2 against (g0 + g2) + g1 -- and rounding alone decides
# between them: float64 and longdouble evaluations of vp_ref itself then pick different ones (seeds 8 and 11).  Such a pair names the same
# three directions in another order, so line_vp is unaffected, but the tag numbers are permuted; those scenes cannot pin an implementation.
SCENE_SEEDS = (3, 4, 5, 6, 9, 10, 12, 13, 15, 16, 20, 21)


def scene(seed, n_per=(25, 20, 15), n_free=20, noise=0.5):
    """Segments of a box world seen by a randomly rotated camera: n_per lines along each Manhattan direction, n_free free lines.
    -> segs, label (0..2 the direction, 3 free), R (columns: the three directions in the camera frame)."""
    fx, fy, cx, cy = CAM
    rng = np.random.default_rng([9090, seed])
    a = rng.normal(0, 0.4, 3); th = np.linalg.norm(a); k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
    segs, lab = [], []

    def proj(P):
        return np.array([fx * P[0] / P[2] + cx, fy * P[1] / P[2] + cy])

    for d in range(3):
        c = 0
        while c < n_per[d]:
            P = np.array([rng.uniform(-4, 4), rng.uniform(-2.5, 2.5), rng.uniform(3, 10)])
            Q = P + rng.uniform(0.5, 3.0) * R[:, d]
            if Q[2] < 1: continue
            p, q = proj(P), proj(Q)
            if not (0 <= p[0] < W and 0 <= p[1] < H and 0 <= q[0] < W and 0 <= q[1] < H): continue
            if np.linalg.norm(p - q) < 30: continue
            segs.append(np.r_[p + rng.normal(0, noise, 2), q + rng.normal(0, noise, 2)]); lab.append(d); c += 1
    c = 0
    while c < n_free:
        p = np.array([rng.uniform(0, W), rng.uniform(0, H)]); ang = rng.uniform(0, math.pi); L = rng.uniform(30, 150)
        q = p + L * np.array([math.cos(ang), math.sin(ang)])
        if not (0 <= q[0] < W and 0 <= q[1] < H): continue
        segs.append(np.r_[p, q]); lab.append(3); c += 1
    segs, lab = np.array(segs), np.array(lab)
    perm = rng.permutation(len(segs))
    return segs[perm], lab[perm], R


def scene_cases():
    return {f"scene_{s}": dict(segs=scene(s)[0], seed=1234 + s, th=vp_ref.DEG) for s in SCENE_SEEDS}


def edge_cases():
    out = {}
    base = scene(3, n_per=(10, 8, 6), n_free=6)[0]
    out["n0"] = dict(segs=np.zeros((0, 4)), seed=5, th=vp_ref.DEG)
    out["n1"] = dict(segs=base[:1], seed=6, th=vp_ref.DEG)
    out["n2"] = dict(segs=np.array([[100.0, 100.0, 300.0, 140.0], [120.0, 300.0, 330.0, 250.0]]), seed=7, th=vp_ref.DEG)
    # two lines at a right angle: their orientations differ by more than 60 degrees, nothing votes, every score is 0, hypothesis 0 is the best
    out["empty_grid"] = dict(segs=np.array([[100.0, 100.0, 300.0, 110.0], [200.0, 50.0, 190.0, 400.0]]), seed=8, th=vp_ref.DEG)
    # horizontal lines: para.x == 0 exactly, so every pair has (para_a x para_b).z == 0 and no sample finds a pair
    out["all_parallel"] = dict(segs=np.array([[50.0 + 7 * k, 40.0 + 30 * k, 400.0 + 5 * k, 40.0 + 30 * k] for k in range(12)]), seed=9, th=vp_ref.DEG)
    # a scene that also holds two exactly parallel lines: that pair does not vote and is never a sample
    out["with_z0_pair"] = dict(segs=np.vstack([base, [[60.0, 100.0, 260.0, 100.0], [90.0, 333.0, 410.0, 333.0]]]), seed=10, th=vp_ref.DEG)
    # the tag threshold put 1e-7 rad above / below the angle of a tagged line (1e-9 rad is what the comparison excuses)
    r = vp_ref.estimate(base, 11, CAM)
    mn = np.asarray(r["angles"], dtype=np.float64).min(axis=1)
    k = int(np.argmax(np.where(r["tag"] < 3, mn, -1.0)))          # the tagged line furthest from its vanishing point
    out["threshold_above"] = dict(segs=base, seed=11, th=float(mn[k]) + 1e-7, line=k)
    out["threshold_below"] = dict(segs=base, seed=11, th=float(mn[k]) - 1e-7, line=k)
    return out


def all_cases():
    c = scene_cases(); c.update(edge_cases())
    return c


def recovery(seed, r):
    """Largest angle (degrees) between a true Manhattan direction of scene `seed` and the nearest estimated vanishing point.  (fx ~ fy.)"""
    R = scene(seed)[2]
    c = np.abs(np.asarray(r["vps"], dtype=np.float64) @ R)
    return float(np.degrees(np.arccos(np.clip(c.max(0), 0, 1))).max())
