"""The numpy restatement of uvs_lt_* (include/uvs_solver.h states the rule; csrc/uvs_line_track.hip is held to this file bit for bit): the LBD
descriptor of a line segment (9 bands of width 7, one octave), the Hamming match with the 30 px endpoint gates, and the slot's frame-to-frame
replay.  Positions, projections and row sums are integers; the FP64 of the bands is written operation by operation, in the header's order.
Every function of the rule comes twice: vectorized (what the tests use) and as plain loops in the kernel's formulation (`*_loops`), held to
each other value by value.  `variant` plants one defect for the tests that the cases tell each from the rule; None is the rule."""
import math

import numpy as np

import fd_ref

OK, SHORT, LONG = 0, 1, 2
N_ROWS, N_BANDS, BAND_W = 63, 9, 7
MAX_LINES, MAX_LENGTH, MAX_COORD = 1024, 2048, 1e6
GATE2 = 900
VARIANTS = ("no_half", "truncate", "swap_neighbours", "edge_21", "clamp_first", "ge_bit")

# byte p of the descriptor compares the bands of the p-th pair of the lexicographic list (0, 1), (0, 2), .., (0, 8), (1, 2), ..
PAIRS = [(a, b) for a in range(N_BANDS) for b in range(a + 1, N_BANDS)][:32]


def gauss_tables():
    """G[63], Lc[21]: the global and the local coefficients (the local sigma is the integer (2 * 7 + 1) / 2 = 7)."""
    G = np.array([math.exp(-float((h - 31) * (h - 31)) / 1922.0) for h in range(N_ROWS)])
    Lc = np.array([math.exp(-float((i - 10) * (i - 10)) / 98.0) for i in range(21)])
    return G, Lc


def gradient(img):
    """gx, gy [H, W] int64: uvs_ft_detect's Sobel."""
    return fd_ref.sobel(img)


def keyline(seg, max_length=MAX_LENGTH):
    """-> (geom[8] int64 = L, cq, sq, MX, MY, halfWidth, status, 0;  ends[4] = the truncated ordered end points)."""
    sx, sy, ex, ey = (float(v) for v in seg)
    if sx > ex:
        sx, sy, ex, ey = ex, ey, sx, sy
    dx = ex - sx; dy = ey - sy
    ln = math.sqrt(dx * dx + dy * dy)
    L = int(ln)
    MX = int(np.rint(512.0 * (sx + ex))); MY = int(np.rint(512.0 * (sy + ey)))
    ends = np.array([int(sx), int(sy), int(ex), int(ey)], np.int32)
    status = SHORT if L < 2 else LONG if L > max_length else OK
    if status != OK:
        return np.array([L, 0, 0, MX, MY, 0, status, 0], np.int64), ends
    cq = int(np.rint(1024.0 * dx / ln)); sq = int(np.rint(1024.0 * dy / ln))
    return np.array([L, cq, sq, MX, MY, (L - 1) // 2, status, 0], np.int64), ends


def projections(grad, geom, variant=None):
    """gDL, gDO [63, L] int64 and the mask of the samples that count (all of them, by the rule)."""
    gx, gy = grad
    H, W = gx.shape
    L, cq, sq, MX, MY, hw = (int(v) for v in geom[:6])
    w = np.arange(L, dtype=np.int64)[None, :]; h = np.arange(N_ROWS, dtype=np.int64)[:, None]
    X = MX + (w - hw) * cq - (h - 31) * sq
    Y = MY + (w - hw) * sq + (h - 31) * cq
    half = 0 if variant == "no_half" else 512
    xr = (X + half) >> 10; yr = (Y + half) >> 10
    x = np.clip(xr, 0, W - 1); y = np.clip(yr, 0, H - 1)
    use = np.ones(x.shape, bool) if variant != "truncate" else (xr == x) & (yr == y)
    a = gx[y, x]; b = gy[y, x]
    return a * cq + b * sq, -a * sq + b * cq, use


def row_sums(grad, geom, variant=None):
    """S[63, 4] int64."""
    if int(geom[6]) != OK:
        return np.zeros((N_ROWS, 4), np.int64)
    dl, do, use = projections(grad, geom, variant)
    z = np.int64(0)
    return np.stack([np.where(use, np.maximum(dl, z), z).sum(1), np.where(use, np.maximum(-dl, z), z).sum(1),
                     np.where(use, np.maximum(do, z), z).sum(1), np.where(use, np.maximum(-do, z), z).sum(1)], axis=1)


def row_sums_loops(grad, geom):
    """The same, sample by sample."""
    gx, gy = grad
    H, W = gx.shape
    S = np.zeros((N_ROWS, 4), np.int64)
    if int(geom[6]) != OK:
        return S
    L, cq, sq, MX, MY, hw = (int(v) for v in geom[:6])
    for h in range(N_ROWS):
        s = [0, 0, 0, 0]
        for w in range(L):
            X = MX + (w - hw) * cq - (h - 31) * sq
            Y = MY + (w - hw) * sq + (h - 31) * cq
            x = min(max((X + 512) >> 10, 0), W - 1); y = min(max((Y + 512) >> 10, 0), H - 1)
            a = int(gx[y, x]); b = int(gy[y, x])
            dl = a * cq + b * sq; do = -a * sq + b * cq
            s[0] += max(dl, 0); s[1] += max(-dl, 0); s[2] += max(do, 0); s[3] += max(-do, 0)
        S[h] = s
    return S


def bands(S, variant=None):
    """d[72] before the normalisation: the header's recurrence, h ascending, the four sums of a row side by side."""
    G, Lc = gauss_tables()
    BS = np.zeros((N_BANDS, 4)); B2 = np.zeros((N_BANDS, 4))
    up, down = (14, 0) if variant != "swap_neighbours" else (0, 14)
    for h in range(N_ROWS):
        r = G[h] * S[h].astype(np.float64); r2 = r * r
        b, j = divmod(h, BAND_W)
        BS[b] += Lc[7 + j] * r; B2[b] += (Lc[7 + j] * Lc[7 + j]) * r2
        if b >= 1:
            BS[b - 1] += Lc[up + j] * r; B2[b - 1] += (Lc[up + j] * Lc[up + j]) * r2
        if b <= 7:
            BS[b + 1] += Lc[down + j] * r; B2[b + 1] += (Lc[down + j] * Lc[down + j]) * r2
    inv = np.full((N_BANDS, 1), 1.0 / 21); inv[0] = inv[8] = 1.0 / 14
    if variant == "edge_21":
        inv[:] = 1.0 / 21
    m = BS * inv
    sd = np.sqrt(np.maximum(B2 * inv - m * m, 0.0))
    d = np.zeros(72)
    d[0::2] = m.reshape(-1); d[1::2] = sd.reshape(-1)          # d[8 b + 2 k] = m, d[8 b + 2 k + 1] = sd
    return d


def bands_loops(S):
    """The same in the kernel's formulation: one accumulator at a time, its rows 7 (b - 1) .. 7 (b + 1) + 6 ascending with the coefficient
    Lc[h - 7 b + 7]."""
    G, Lc = gauss_tables()
    d = np.zeros(72)
    for b in range(N_BANDS):
        for k in range(4):
            bs = 0.0; b2 = 0.0
            for h in range(max(0, 7 * (b - 1)), min(N_ROWS - 1, 7 * (b + 1) + 6) + 1):
                c = float(Lc[h - 7 * b + 7])
                r = float(G[h]) * float(int(S[h][k])); r2 = r * r
                bs = bs + c * r; b2 = b2 + (c * c) * r2
            inv = 1.0 / 14 if b in (0, 8) else 1.0 / 21
            m = bs * inv
            v = b2 * inv - m * m
            d[8 * b + 2 * k] = m; d[8 * b + 2 * k + 1] = math.sqrt(v if v > 0.0 else 0.0)
    return d


def _serial_sum_sq(v):
    t = 0.0
    for x in v:
        t = t + float(x) * float(x)
    return t


def normalise(d, variant=None):
    """-> (the clamped d[72] the bits compare, desc_float[72])."""
    d = np.array(d, np.float64)
    if variant == "clamp_first":
        d = np.minimum(d, 0.4)
    tm = _serial_sum_sq(d[0::2]); ts = _serial_sum_sq(d[1::2])
    if tm > 0.0:
        d[0::2] = d[0::2] * (1.0 / math.sqrt(tm))
    if ts > 0.0:
        d[1::2] = d[1::2] * (1.0 / math.sqrt(ts))
    d = np.where(d > 0.4, 0.4, d)
    tot = _serial_sum_sq(d)
    return d, (d * (1.0 / math.sqrt(tot)) if tot > 0.0 else np.zeros(72))


def bits(d, variant=None):
    """desc[32] uint8: bit 7 - i of byte p is d[8 a + i] > d[8 b + i], (a, b) = PAIRS[p]."""
    a = np.array([np.arange(8 * p[0], 8 * p[0] + 8) for p in PAIRS]); b = np.array([np.arange(8 * p[1], 8 * p[1] + 8) for p in PAIRS])
    cmp = d[a] >= d[b] if variant == "ge_bit" else d[a] > d[b]
    return np.packbits(cmp.astype(np.uint8), axis=1, bitorder="big").reshape(32)


def bits_loops(d):
    out = np.zeros(32, np.uint8)
    for p, (a, b) in enumerate(PAIRS):
        v = 0
        for i in range(8):
            if d[8 * a + i] > d[8 * b + i]:
                v |= 1 << (7 - i)
        out[p] = v
    return out


def describe_line(grad, seg, max_length=MAX_LENGTH, variant=None, loops=False):
    """One segment -> dict(geom[8], ends[4], row_sums[63, 4], desc_float[72], desc[32], clamped[72])."""
    geom, ends = keyline(seg, max_length)
    if int(geom[6]) != OK:
        return dict(geom=geom, ends=ends, row_sums=np.zeros((N_ROWS, 4), np.int64), desc_float=np.zeros(72), desc=np.zeros(32, np.uint8),
                    clamped=np.zeros(72))
    S = row_sums_loops(grad, geom) if loops else row_sums(grad, geom, variant)
    d, df = normalise(bands_loops(S) if loops else bands(S, variant), variant)
    return dict(geom=geom, ends=ends, row_sums=S, desc_float=df, desc=bits_loops(d) if loops else bits(d, variant), clamped=d)


def describe(img, segs, max_length=MAX_LENGTH, variant=None, loops=False):
    """A frame's segments [n, 4] -> dict of stacked arrays: geom [n, 8], ends [n, 4] int32, status [n] int32, row_sums [n, 63, 4],
    desc_float [n, 72], desc [n, 32] uint8."""
    grad = gradient(img)
    segs = np.asarray(segs, np.float64).reshape(-1, 4)
    r = [describe_line(grad, s, max_length, variant, loops) for s in segs]
    n = len(r)
    return dict(geom=np.array([x["geom"] for x in r], np.int64).reshape(n, 8), ends=np.array([x["ends"] for x in r], np.int32).reshape(n, 4),
                status=np.array([x["geom"][6] for x in r], np.int32).reshape(n),
                row_sums=np.array([x["row_sums"] for x in r], np.int64).reshape(n, N_ROWS, 4),
                desc_float=np.array([x["desc_float"] for x in r], np.float64).reshape(n, 72),
                desc=np.array([x["desc"] for x in r], np.uint8).reshape(n, 32))


def hamming(a, b):
    """[len(a), len(b)] int: differing bits of descriptors [., 32] uint8."""
    x = np.asarray(a, np.uint8)[:, None, :] ^ np.asarray(b, np.uint8)[None, :, :]
    return np.unpackbits(x, axis=2).sum(2).astype(np.int64)


def match(prev_desc, prev_ends, cur_desc, cur_ends, prev_status=None, cur_status=None):
    """-> (match_of_prev [n_prev], distance [n_prev], prev_of_cur [n_cur]) int32: for each OK previous line the OK current line of the
    smallest Hamming distance (ties: the lowest index), dropped iff a gate point pair is more than 30 px apart; prev_of_cur is the LARGEST
    accepted previous line that chose a current line."""
    prev_desc = np.asarray(prev_desc, np.uint8).reshape(-1, 32); cur_desc = np.asarray(cur_desc, np.uint8).reshape(-1, 32)
    pe = np.asarray(prev_ends, np.int64).reshape(-1, 4); ce = np.asarray(cur_ends, np.int64).reshape(-1, 4)
    nq, nt = len(prev_desc), len(cur_desc)
    ps = np.zeros(nq, np.int32) if prev_status is None else np.asarray(prev_status)
    cs = np.zeros(nt, np.int32) if cur_status is None else np.asarray(cur_status)
    mop = np.full(nq, -1, np.int32); dist = np.full(nq, -1, np.int32); poc = np.full(nt, -1, np.int32)
    ok_t = np.flatnonzero(cs == OK)
    if nq == 0 or len(ok_t) == 0:
        return mop, dist, poc
    D = hamming(prev_desc, cur_desc[ok_t])
    for q in range(nq):
        if ps[q] != OK:
            continue
        j = int(np.argmin(D[q]))                  # the first minimum: the lowest t
        t = int(ok_t[j])
        dist[q] = D[q, j]
        ds = (pe[q, 0] - ce[t, 0]) ** 2 + (pe[q, 1] - ce[t, 1]) ** 2
        de = (pe[q, 2] - ce[t, 2]) ** 2 + (pe[q, 3] - ce[t, 3]) ** 2
        if ds > GATE2 or de > GATE2:
            continue
        mop[q] = t
        poc[t] = q                                # query order: a later q overwrites
    return mop, dist, poc


def match_loops(prev_desc, prev_ends, cur_desc, cur_ends, prev_status, cur_status):
    """The same with the packed key (distance << 16) | t."""
    nq, nt = len(prev_desc), len(cur_desc)
    mop = np.full(nq, -1, np.int32); dist = np.full(nq, -1, np.int32); poc = np.full(nt, -1, np.int32)
    for q in range(nq):
        if prev_status[q] != OK:
            continue
        best = None
        for t in range(nt):
            if cur_status[t] != OK:
                continue
            dd = sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(prev_desc[q], cur_desc[t]))
            key = (dd << 16) | t
            best = key if best is None or key < best else best
        if best is None:
            continue
        t = best & 0xFFFF; dist[q] = best >> 16
        pe = [int(v) for v in prev_ends[q]]; ce = [int(v) for v in cur_ends[t]]
        if (pe[0] - ce[0]) ** 2 + (pe[1] - ce[1]) ** 2 > GATE2 or (pe[2] - ce[2]) ** 2 + (pe[3] - ce[3]) ** 2 > GATE2:
            continue
        mop[q] = t
        poc[t] = max(int(poc[t]), q)
    return mop, dist, poc


class Slot:
    """A slot of uvs_lt_track: the previous frame's descriptors, gate points and statuses."""

    def __init__(self, max_length=MAX_LENGTH):
        self.max_length = max_length
        self.prev = None

    def reset(self):
        self.prev = None

    def track(self, img, segs, variant=None):
        """-> dict: desc [n, 32], status [n], prev_index [n] (prev_of_cur), distance [n] (of the accepted match, else -1), ends [n, 4],
        n_described, n_matched."""
        cur = describe(img, segs, self.max_length, variant)
        n = len(cur["status"])
        prev_index = np.full(n, -1, np.int32); distance = np.full(n, -1, np.int32); n_matched = 0
        if self.prev is not None and len(self.prev["status"]):
            mop, dist, poc = match(self.prev["desc"], self.prev["ends"], cur["desc"], cur["ends"], self.prev["status"], cur["status"])
            prev_index = poc
            distance = np.where(poc >= 0, dist[np.maximum(poc, 0)], -1).astype(np.int32)
            n_matched = int((mop >= 0).sum())
        self.prev = cur
        return dict(desc=cur["desc"], status=cur["status"], prev_index=prev_index, distance=distance, ends=cur["ends"],
                    n_described=int((cur["status"] == OK).sum()), n_matched=n_matched)
