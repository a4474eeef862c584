"""The numpy restatement of uvs_lt_detect (include/uvs_solver.h states the rule; csrc/uvs_line_detect.hip is held to this file bit for bit):
Burns-style line-support regions.  Blur, Sobel, two integer sector maps, the connected regions of like sector in each partition, the vote
between the partitions, the weighted moment fit, the extent and the ranking.  Everything up to the six moment sums is integer arithmetic; the
FP64 of the fit is written operation by operation, in the header's order.  The stages come twice: vectorized (what the tests use) and as plain
loops (`*_loops`), held to each other value by value.  `variant` plants one misreading for the tests that the cases tell each from the rule;
None is the rule."""
import math

import numpy as np

import fd_ref

OK, OVERFLOW = 0, 1
NONE = 255                 # sector of a pixel without support
VARIANTS = ("four_connected", "tie_to_b", "half_support", "fit_voters", "unweighted", "gt_boundary")
NB8 = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
NB4 = ((-1, 0), (0, -1), (0, 1), (1, 0))


def blur(img):
    """[H, W] int64: taps 1 4 6 4 1 along the rows, then along the columns, reflect-101, (sum + 128) >> 8."""
    k = (1, 4, 6, 4, 1)
    a = np.asarray(img).astype(np.int64)
    H, W = a.shape
    p = np.pad(a, ((0, 0), (2, 2)), mode="reflect")
    r = sum(k[i] * p[:, i:i + W] for i in range(5))
    p = np.pad(r, ((2, 2), (0, 0)), mode="reflect")
    return (sum(k[j] * p[j:j + H, :] for j in range(5)) + 128) >> 8


def gradient(img):
    """gx, gy, M [H, W] int64 of the blurred image: k_lt_gradient's Sobel, M = |gx| + |gy|."""
    gx, gy = fd_ref.sobel(blur(img))
    return gx, gy, np.abs(gx) + np.abs(gy)


def sector_of(gx, gy, variant=None):
    """(A, B) of ONE non-zero gradient, the header's integer rule word by word."""
    gx = int(gx); gy = int(gy)
    if gx > 0 and gy >= 0:
        q, px, py = 0, gx, gy
    elif gx <= 0 and gy > 0:
        q, px, py = 1, gy, -gx
    elif gx < 0 and gy <= 0:
        q, px, py = 2, -gx, -gy
    else:
        q, px, py = 3, -gy, gx
    if variant == "gt_boundary":
        return 2 * q + int(py > px), (2 * q + int(985 * py > 408 * px) + int(408 * py > 985 * px)) % 8
    return 2 * q + int(py >= px), (2 * q + int(985 * py >= 408 * px) + int(408 * py >= 985 * px)) % 8


def sectors(gx, gy, M, T, variant=None):
    """secA, secB [H, W] uint8 (255 = no support), vectorized."""
    q = np.select([(gx > 0) & (gy >= 0), (gx <= 0) & (gy > 0), (gx < 0) & (gy <= 0)], [0, 1, 2], 3)
    px = np.choose(q, [gx, gy, -gx, -gy]); py = np.choose(q, [gy, -gx, -gy, gx])
    if variant == "gt_boundary":
        A = 2 * q + (py > px); B = (2 * q + (985 * py > 408 * px).astype(np.int64) + (408 * py > 985 * px)) % 8
    else:
        A = 2 * q + (py >= px); B = (2 * q + (985 * py >= 408 * px).astype(np.int64) + (408 * py >= 985 * px)) % 8
    sup = M >= T
    return np.where(sup, A, NONE).astype(np.uint8), np.where(sup, B, NONE).astype(np.uint8)


def names(sec, variant=None):
    """[H, W] int64: the smallest linear index of the pixel's region, -1 without support.  Minimum propagation over the neighbours of like
    sector, with pointer jumping (the name of my name's pixel is a pixel of my region)."""
    H, W = sec.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    big = np.int64(H * W)
    lab = np.where(sec != NONE, idx, big)
    nb = NB4 if variant == "four_connected" else NB8
    s = np.pad(sec, 1, constant_values=NONE)
    same = [(s[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] == sec) & (sec != NONE) for dy, dx in nb]
    while True:
        p = np.pad(lab, 1, constant_values=big)
        new = lab
        for (dy, dx), sm in zip(nb, same):
            new = np.minimum(new, np.where(sm, p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W], big))
        flat = np.append(new.reshape(-1), big)
        new = flat[new]                                   # pointer jumping
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(sec != NONE, lab, -1)


def names_loops(sec, variant=None):
    """The same by a flood fill in raster order: the first pixel of a region met is its smallest index."""
    H, W = sec.shape
    out = np.full((H, W), -1, np.int64)
    nb = NB4 if variant == "four_connected" else NB8
    for y0 in range(H):
        for x0 in range(W):
            if sec[y0, x0] == NONE or out[y0, x0] >= 0:
                continue
            name = y0 * W + x0
            out[y0, x0] = name
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for dy, dx in nb:
                    v, u = y + dy, x + dx
                    if 0 <= v < H and 0 <= u < W and out[v, u] < 0 and sec[v, u] == sec[y0, x0]:
                        out[v, u] = name
                        stack.append((v, u))
    return out


def _sizes(name):
    """n of the region of every pixel (0 without support)."""
    flat = name.reshape(-1)
    cnt = np.bincount(flat[flat >= 0], minlength=flat.size)
    return np.where(name >= 0, cnt[np.maximum(name, 0)], 0)


def fit_region(W, name, xs, ys, ws, variant=None):
    """Steps 6 and 7 for ONE region in plain Python floats (IEEE doubles, one rounding per operation): pixel coordinates xs, ys and weights ws
    (Python ints).  -> None if rejected by nrm == 0, else (seg[4], width2, length)."""
    x0, y0 = name % W, name // W
    S0 = Sx = Sy = Sxx = Sxy = Syy = 0
    for x, y, w in zip(xs, ys, ws):
        dx, dy = x - x0, y - y0
        S0 += w; Sx += w * dx; Sy += w * dy; Sxx += w * dx * dx; Sxy += w * dx * dy; Syy += w * dy * dy
    S0, Sx, Sy, Sxx, Sxy, Syy = (float(v) for v in (S0, Sx, Sy, Sxx, Sxy, Syy))
    mx = Sx / S0; my = Sy / S0
    a = Sxx / S0 - mx * mx; c = Syy / S0 - my * my; b = Sxy / S0 - mx * my
    h = (a - c) * 0.5
    r = math.sqrt(h * h + b * b)
    ux, uy = (h + r, b) if a >= c else (b, r - h)
    nrm = math.sqrt(ux * ux + uy * uy)
    if nrm == 0.0:
        return None
    ux = ux / nrm; uy = uy / nrm
    width2 = (a + c) * 0.5 - r
    ts = [(float(x - x0) - mx) * ux + (float(y - y0) - my) * uy for x, y in zip(xs, ys)]
    tmin, tmax = min(ts), max(ts)
    return [(x0 + mx) + tmin * ux, (y0 + my) + tmin * uy, (x0 + mx) + tmax * ux, (y0 + my) + tmax * uy], width2, tmax - tmin


def _group(name):
    """Pixels of the regions of `name` grouped: -> (region names ascending, start offsets, the pixel indices sorted by region)."""
    flat = name.reshape(-1)
    pix = np.flatnonzero(flat >= 0)
    order = pix[np.argsort(flat[pix], kind="stable")]
    lab = flat[order]
    first = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]]) if len(lab) else np.zeros(0, np.int64)
    return lab[first] if len(lab) else lab, first, order


def stages(img, T, min_pixels, min_length, variant=None, loops=False):
    """Every per-pixel stage and every kept segment (unranked) -> dict."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    bl = blur(img)
    gx, gy, M = gradient(img)
    if loops:
        secA = np.full((H, W), NONE, np.uint8); secB = secA.copy()
        for y in range(H):
            for x in range(W):
                if M[y, x] >= T:
                    secA[y, x], secB[y, x] = sector_of(gx[y, x], gy[y, x], variant)
    else:
        secA, secB = sectors(gx, gy, M, T, variant)
    nm = names_loops if loops else names
    nameA = nm(secA, variant); nameB = nm(secB, variant)
    nA = _sizes(nameA); nB = _sizes(nameB)
    sup = secA != NONE
    votes_a = (nA > nB) if variant == "tie_to_b" else (nA >= nB)
    vote = np.where(sup, np.where(votes_a, 0, 1), NONE).astype(np.uint8)
    kept = []
    regions = [0, 0]
    xs_all = np.tile(np.arange(W, dtype=np.int64), H); ys_all = np.repeat(np.arange(H, dtype=np.int64), W)
    Mf = M.reshape(-1); votef = vote.reshape(-1)
    for part, name in enumerate((nameA, nameB)):
        reg, first, order = _group(name)
        regions[part] = len(reg)
        if not len(reg):
            continue
        n = np.diff(np.r_[first, len(order)])
        s = np.add.reduceat((votef[order] == part).astype(np.int64), first)
        cand = (n >= min_pixels) & ((2 * s >= n) if variant == "half_support" else (2 * s > n))
        if loops:
            for k in np.flatnonzero(cand):
                px = order[first[k]:first[k] + n[k]]
                use = px[votef[px] == part] if variant == "fit_voters" else px
                w = [1] * len(use) if variant == "unweighted" else [int(v) for v in Mf[use]]
                f = fit_region(W, int(reg[k]), [int(v) for v in xs_all[use]], [int(v) for v in ys_all[use]], w, variant)
                if f is not None and f[2] >= min_length:
                    kept.append(dict(seg=f[0], width2=f[1], length=f[2], info=[int(reg[k]), part, int(n[k]), int(s[k])]))
            continue
        # vectorized: the sums by reduceat over the pixels sorted by region
        if variant == "fit_voters":
            sel = votef[order] == part
            order_f = order[sel]; lab_f = name.reshape(-1)[order_f]
            first_f = np.searchsorted(lab_f, reg)               # a candidate has voters (2 s > n), so its run is not empty
        else:
            order_f, first_f = order, first
        x0 = reg % W; y0 = reg // W
        rid = np.searchsorted(reg, name.reshape(-1)[order_f])
        dx = xs_all[order_f] - x0[rid]; dy = ys_all[order_f] - y0[rid]
        w = np.ones(len(order_f), np.int64) if variant == "unweighted" else Mf[order_f]
        # (one neutral element behind the pixels: a region without pixels here, which `cand` rules out below, may start at the very end)
        red = lambda v: np.add.reduceat(np.append(v, 0), first_f).astype(np.float64)
        with np.errstate(all="ignore"):
            S0, Sx, Sy, Sxx, Sxy, Syy = red(w), red(w * dx), red(w * dy), red(w * dx * dx), red(w * dx * dy), red(w * dy * dy)
            mx = Sx / S0; my = Sy / S0
            a = Sxx / S0 - mx * mx; c = Syy / S0 - my * my; b = Sxy / S0 - mx * my
            h = (a - c) * 0.5
            r = np.sqrt(h * h + b * b)
            ux = np.where(a >= c, h + r, b); uy = np.where(a >= c, b, r - h)
            nrm = np.sqrt(ux * ux + uy * uy)
            ux = ux / nrm; uy = uy / nrm
            width2 = (a + c) * 0.5 - r
            t = (dx.astype(np.float64) - mx[rid]) * ux[rid] + (dy.astype(np.float64) - my[rid]) * uy[rid]
            t = np.where(np.isnan(t), 0.0, t)
            tmin = np.minimum.reduceat(np.append(t, np.inf), first_f); tmax = np.maximum.reduceat(np.append(t, -np.inf), first_f)
            length = tmax - tmin
            bx = x0 + mx; by = y0 + my
            seg = np.stack([bx + tmin * ux, by + tmin * uy, bx + tmax * ux, by + tmax * uy], axis=1)
        keep = cand & (nrm != 0.0) & (length >= min_length)
        for k in np.flatnonzero(keep):
            kept.append(dict(seg=[float(v) for v in seg[k]], width2=float(width2[k]), length=float(length[k]),
                             info=[int(reg[k]), part, int(n[k]), int(s[k])]))
    return dict(blur=bl.astype(np.uint8), gx=gx, gy=gy, M=M, grad=pack_gradient(gx, gy), secA=secA, secB=secB, nameA=nameA.astype(np.int32),
                nameB=nameB.astype(np.int32), vote=vote, kept=kept, n_support=int(sup.sum()), n_regions=regions)


def pack_gradient(gx, gy):
    """gx in the low, gy in the high 16 bits of a uint32, as k_lt_gradient packs them."""
    return ((gx & 0xFFFF) | ((gy & 0xFFFF) << 16)).astype(np.uint32)


def detect(img, T, min_pixels, min_length, max_lines, variant=None, loops=False):
    """-> dict: seg [n_returned, 4], width2 [n_returned], info [n_returned, 4] int32 (name, partition, n, s), length [n_returned],
    n_found, n_returned, n_support, n_regions [2], status."""
    st = stages(img, T, min_pixels, min_length, variant, loops)
    kept = sorted(st["kept"], key=lambda k: (-k["length"], k["info"][0], k["info"][1]))
    n_found = len(kept)
    kept = kept[:max_lines]
    n = len(kept)
    return dict(seg=np.array([k["seg"] for k in kept], np.float64).reshape(n, 4), width2=np.array([k["width2"] for k in kept], np.float64).reshape(n),
                info=np.array([k["info"] for k in kept], np.int32).reshape(n, 4), length=np.array([k["length"] for k in kept], np.float64).reshape(n),
                n_found=n_found, n_returned=n, n_support=st["n_support"], n_regions=list(st["n_regions"]),
                status=OVERFLOW if n_found > max_lines else OK)
