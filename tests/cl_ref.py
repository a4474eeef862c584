"""The numpy restatement of uvs_ft_equalize (include/uvs_solver.h states the rule; csrc/uvs_feature_equalize.hip is held to this file bit for bit):
cv::createCLAHE(clip_limit, cv::Size(tiles_x, tiles_y))->apply(img, out) of the reference's readImage (feature_tracker/src/feature_tracker.cpp:60-66).

TEST INFRASTRUCTURE ONLY.  OpenCV is not a dependency, so this file is the pin (as tests/ft_ref.py is for the tracker).  Integers are int64 arrays
or Python ints; every float32 value is a numpy.float32, and every float32 expression is written in the order the header gives, one rounding per
operation.  Two forms of the one rule: equalize() is vectorized, equalize_loops() walks tiles, bins and pixels in plain Python loops; the tests
hold them to each other.

  padding   none if tiles_x | W and tiles_y | H; otherwise Wp = W + tiles_x - W % tiles_x and Hp = H + tiles_y - H % tiles_y (a dimension that
            did divide gains a full extra tiles_x columns / tiles_y rows: OpenCV's behaviour), ext(x, y) = img(refl(x, W), refl(y, H))
  tile      tw = Wp / tiles_x, th = Hp / tiles_y, N = tw th, lutScale = 255.0f / (float)N, clip = 0 if clip_limit == 0 else
            max((int)(clip_limit N / 256), 1)
  per tile  the histogram of ext; the excess above clip is cut and handed back, clipped / 256 to every bin and the residual one each to bins 0,
            step, 2 step, .. (step = max(256 / residual, 1)); lut[i] = sat_u8(rint((float)(h[0] + .. + h[i]) lutScale))
  per pixel the bilinear blend of the four neighbouring tiles' LUTs at the pixel's value, float32, in the order of the header

DEFECTS names the planted defects of the tests: each is a plausible misreading of the rule, and each must change the output of some case.
"""
import numpy as np

MAX_TILES = 16
DEFECTS = ("residual_first_bins", "no_full_tile_padding", "lut_truncates", "no_half_tile_offset", "clip_not_raised")
F = np.float32


def refl(i, n):
    """reflect-101 of an int array (or int) into 0..n-1; exact for -n < i < 2 n - 1."""
    i = np.abs(np.asarray(i, np.int64))
    return np.where(i >= n, 2 * n - 2 - i, i)


def geometry(W, H, clip_limit, tiles_x, tiles_y, defect=None):
    """-> (Wp, Hp, tw, th, N, clip) as Python ints."""
    assert defect is None or defect in DEFECTS
    if W % tiles_x == 0 and H % tiles_y == 0:
        Wp, Hp = W, H
    elif defect == "no_full_tile_padding":
        Wp, Hp = W + (tiles_x - W % tiles_x) % tiles_x, H + (tiles_y - H % tiles_y) % tiles_y
    else:
        Wp, Hp = W + tiles_x - W % tiles_x, H + tiles_y - H % tiles_y
    tw, th = Wp // tiles_x, Hp // tiles_y
    N = tw * th
    if clip_limit == 0:
        clip = 0
    else:
        clip = int(np.float64(clip_limit) * np.float64(N) / np.float64(256.0))
        if defect != "clip_not_raised":
            clip = max(clip, 1)
    return Wp, Hp, tw, th, N, clip


def _sat_u8(a):
    return np.clip(a, 0, 255).astype(np.uint8)


def _result(out, bins, luts, g):
    Wp, Hp, tw, th, N, clip = g
    return dict(out=out, bins=bins.astype(np.int32), luts=luts, info=np.array([Wp, Hp, N, clip], np.int32))


def equalize(img, clip_limit=3.0, tiles_x=8, tiles_y=8, defect=None):
    """img [H, W] uint8 -> dict(out [H, W] uint8, bins [tiles_y, tiles_x, 256] int32 (after clipping and redistribution), luts [tiles_y, tiles_x,
    256] uint8, info int32 (Wp, Hp, N, clip))."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W = img.shape
    g = geometry(W, H, clip_limit, tiles_x, tiles_y, defect)
    Wp, Hp, tw, th, N, clip = g
    T = tiles_x * tiles_y
    ext = img[np.ix_(refl(np.arange(Hp), H), refl(np.arange(Wp), W))].astype(np.int64)
    tiles = ext.reshape(tiles_y, th, tiles_x, tw).transpose(0, 2, 1, 3).reshape(T, N)
    h = np.bincount((np.arange(T)[:, None] * 256 + tiles).ravel(), minlength=T * 256).reshape(T, 256).astype(np.int64)
    if clip > 0:
        clipped = np.maximum(h - clip, 0).sum(axis=1)
        h = np.minimum(h, clip)
        batch = clipped // 256
        residual = clipped - 256 * batch
        h = h + batch[:, None]
        i = np.arange(256)[None, :]
        if defect == "residual_first_bins":
            h = h + (i < residual[:, None])
        else:
            step = np.maximum(256 // np.maximum(residual, 1), 1)[:, None]
            h = h + ((i % step == 0) & (i // step < residual[:, None]))
    lut_scale = F(255.0) / F(N)
    v = np.cumsum(h, axis=1).astype(F) * lut_scale
    luts = _sat_u8(np.floor(v) if defect == "lut_truncates" else np.rint(v)).reshape(tiles_y, tiles_x, 256)

    def axis(n, t, n_tiles):
        f = np.arange(n).astype(F) * (F(1.0) / F(t))
        if defect != "no_half_tile_offset":
            f = f - F(0.5)
        t1 = np.floor(f).astype(np.int64)
        a = f - t1.astype(F)
        return np.maximum(t1, 0), np.minimum(t1 + 1, n_tiles - 1), a, F(1.0) - a

    tx1, tx2, xa, xa1 = axis(W, tw, tiles_x)
    ty1, ty2, ya, ya1 = axis(H, th, tiles_y)
    if defect == "no_half_tile_offset":        # without the offset a pixel of the last partial tile would look past the grid
        tx1 = np.minimum(tx1, tiles_x - 1); ty1 = np.minimum(ty1, tiles_y - 1)
    L = lambda ty, tx: luts[ty[:, None], tx[None, :], img].astype(F)
    xa, xa1, ya, ya1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    res = (L(ty1, tx1) * xa1 + L(ty1, tx2) * xa) * ya1 + (L(ty2, tx1) * xa1 + L(ty2, tx2) * xa) * ya
    assert res.dtype == F
    return _result(_sat_u8(np.rint(res)), h.reshape(tiles_y, tiles_x, 256), luts, g)


def equalize_loops(img, clip_limit=3.0, tiles_x=8, tiles_y=8):
    """The same rule tile by tile, bin by bin and pixel by pixel."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W = img.shape
    g = geometry(W, H, clip_limit, tiles_x, tiles_y)
    Wp, Hp, tw, th, N, clip = g
    r = lambda i, n: -i if i < 0 else (2 * n - 2 - i if i >= n else i)
    px = img.tolist()
    lut_scale = F(255.0) / F(N)
    bins = np.zeros((tiles_y, tiles_x, 256), np.int64)
    luts = np.zeros((tiles_y, tiles_x, 256), np.uint8)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            h = [0] * 256
            for y in range(ty * th, (ty + 1) * th):
                row = px[r(y, H)]
                for x in range(tx * tw, (tx + 1) * tw):
                    h[row[r(x, W)]] += 1
            if clip > 0:
                clipped = 0
                for i in range(256):
                    if h[i] > clip:
                        clipped += h[i] - clip
                        h[i] = clip
                batch = clipped // 256
                residual = clipped - batch * 256
                for i in range(256):
                    h[i] += batch
                if residual > 0:
                    step = max(256 // residual, 1)
                    i = 0
                    while i < 256 and residual > 0:
                        h[i] += 1
                        i += step; residual -= 1
            s = 0
            for i in range(256):
                s += h[i]
                luts[ty, tx, i] = min(max(int(np.rint(F(s) * lut_scale)), 0), 255)
            bins[ty, tx] = h
    out = np.zeros((H, W), np.uint8)
    lt = luts.tolist()
    inv_tw = F(1.0) / F(tw); inv_th = F(1.0) / F(th)
    half, one = F(0.5), F(1.0)
    for y in range(H):
        tyf = F(y) * inv_th - half
        ty1 = int(np.floor(tyf))
        ya = tyf - F(ty1); ya1 = one - ya
        ty2 = min(ty1 + 1, tiles_y - 1); ty1 = max(ty1, 0)
        for x in range(W):
            txf = F(x) * inv_tw - half
            tx1 = int(np.floor(txf))
            xa = txf - F(tx1); xa1 = one - xa
            tx2 = min(tx1 + 1, tiles_x - 1); tx1 = max(tx1, 0)
            v = px[y][x]
            res = (F(lt[ty1][tx1][v]) * xa1 + F(lt[ty1][tx2][v]) * xa) * ya1 + (F(lt[ty2][tx1][v]) * xa1 + F(lt[ty2][tx2][v]) * xa) * ya
            out[y, x] = min(max(int(np.rint(res)), 0), 255)
    return _result(out, bins, luts, g)


def plain_equalization(img):
    """Histogram equalization of the whole image from Python integers: what clip_limit = 0 with one tile must give, since the four LUTs of
    every pixel are then the one LUT and the blend of four equal float32 values with weights that sum to 1 .. is checked, not assumed."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    N = img.size
    h = [0] * 256
    for v in img.ravel().tolist():
        h[v] += 1
    lut, s = [], 0
    for i in range(256):
        s += h[i]
        lut.append(min(max(int(np.rint(F(s) * (F(255.0) / F(N)))), 0), 255))
    return np.array(lut, np.uint8)[img], np.array(lut, np.uint8)
