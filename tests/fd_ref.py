"""The numpy restatement of uvs_ft_detect (include/uvs_solver.h states the rules; csrc/uvs_feature_detect.hip is held to this file bit for bit)
and of the host mirror's setMask (host/feature_tracker.h).  Integer sums in int64, one FP64 sqrt and one subtraction per pixel, one FP64 product
for the threshold; numpy's sqrt is correctly rounded, as the device's is."""
import numpy as np

import kf_ref

DETECT_OK, DETECT_OVERFLOW = 0, 1
DEFAULT_CANDIDATES = 65536
MAX_CANDIDATES = 1 << 20
MAX_MIN_DISTANCE = 1024


def sobel(img):
    """gx, gy [H, W] int64: the 3 x 3 Sobel of the image, every read through reflect-101 (numpy's 'reflect')."""
    p = np.pad(np.asarray(img).astype(np.int64), 1, mode="reflect")
    gx = (p[:-2, 2:] - p[:-2, :-2]) + 2 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])
    gy = (p[2:, :-2] - p[:-2, :-2]) + 2 * (p[2:, 1:-1] - p[:-2, 1:-1]) + (p[2:, 2:] - p[:-2, 2:])
    return gx, gy


def box3(a):
    """The 3 x 3 sum of a, a itself read through reflect-101 (the products are reflected, not the image a second time)."""
    p = np.pad(a, 1, mode="reflect")
    H, W = a.shape
    return sum(p[j:j + H, i:i + W] for j in range(3) for i in range(3))


def sums(img):
    """A, B, C [H, W] int64 (they fit int32: at most 9 x 1020^2)."""
    gx, gy = sobel(img)
    return box3(gx * gx), box3(gx * gy), box3(gy * gy)


def score_map(img):
    A, B, C = sums(img)
    S = (A - C) * (A - C) + 4 * B * B                          # int64, at most 4.4e14: exact in FP64
    return (A + C).astype(np.float64) - np.sqrt(S.astype(np.float64))


def allowed_map(shape, occupied=(), R=30, mask=None):
    """[H, W] bool: the mask is absent or non-zero, and no occupied point's rint centre lies within R (<=)."""
    H, W = shape
    al = np.ones((H, W), bool) if mask is None else (np.asarray(mask) != 0)
    y, x = np.mgrid[0:H, 0:W]
    for ox, oy in np.asarray(occupied, np.float64).reshape(-1, 2):
        xr, yr = int(np.rint(ox)), int(np.rint(oy))
        al = al & ~((x - xr) ** 2 + (y - yr) ** 2 <= R * R)
    return al


def detect(img, cam, occupied=(), max_new=50, quality_level=0.01, min_distance=30, mask=None, max_candidates=DEFAULT_CANDIDATES):
    """-> dict: score_map, allowed, max_score, threshold, n_candidates, status, cand_index / cand_score (the ranked candidates), and the taken
    points xy [n_new, 2] int32, score, norm in taking order."""
    img = np.asarray(img)
    H, W = img.shape
    R = int(min_distance)
    score = score_map(img)
    al = allowed_map((H, W), occupied, R, mask)
    mx = float(score[al].max()) if al.any() else 0.0
    thr = np.float64(quality_level) * np.float64(mx)
    cand = np.zeros((H, W), bool)
    if mx > 0.0:
        p = np.pad(score, 1, mode="constant", constant_values=0.0)       # the ring is no candidate, so the padding is never the deciding neighbour
        nmax = np.max([p[j:j + H, i:i + W] for j in range(3) for i in range(3) if (i, j) != (1, 1)], axis=0)
        cand = al & (score > thr) & (score >= nmax)
        cand[0, :] = cand[-1, :] = False; cand[:, 0] = cand[:, -1] = False
    idx = np.flatnonzero(cand.ravel())                         # row-major
    n_cand = len(idx)
    status = DETECT_OVERFLOW if n_cand > max_candidates else DETECT_OK
    idx = idx[:max_candidates]
    cs = score.ravel()[idx]
    order = np.lexsort((-idx, -cs))                            # the score descending, equal scores by the index descending
    idx, cs = idx[order].astype(np.int32), cs[order]
    taken = []
    for k in range(len(idx)):
        if len(taken) >= max_new:
            break
        x, y = int(idx[k]) % W, int(idx[k]) // W
        if all((x - tx) ** 2 + (y - ty) ** 2 >= R * R for tx, ty, _ in taken):
            taken.append((x, y, k))
    xy = np.array([(t[0], t[1]) for t in taken], np.int32).reshape(-1, 2)
    sc = np.array([cs[t[2]] for t in taken], np.float64)
    norm = kf_ref.lift(cam, xy.astype(np.float64)) if len(xy) else np.zeros((0, 2))
    return dict(score_map=score, allowed=al.astype(np.uint8), max_score=mx, threshold=float(thr), n_candidates=n_cand, status=status,
                cand_index=idx, cand_score=cs, xy=xy, score=sc, norm=norm, n_new=len(xy))


def set_mask(pts, ids, track_cnt, norm, min_dist):
    """The host mirror's setMask: a STABLE order by track_cnt descending; a point is kept iff no point kept before it lies within min_dist (<=)
    on the rint centres.  -> the four arrays, permuted alike."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    order = np.argsort(-np.asarray(track_cnt, np.int64), kind="stable")
    kept, centres = [], []
    for i in order:
        c = (int(np.rint(pts[i, 0])), int(np.rint(pts[i, 1])))
        if all((c[0] - k[0]) ** 2 + (c[1] - k[1]) ** 2 > min_dist * min_dist for k in centres):
            kept.append(int(i)); centres.append(c)
    kept = np.array(kept, int)
    return pts[kept], np.asarray(ids)[kept], np.asarray(track_cnt)[kept], np.asarray(norm, np.float64).reshape(-1, 2)[kept]
