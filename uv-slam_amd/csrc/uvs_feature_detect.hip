// uvs_feature_detect.hip -- the detection step of the point front end (reference feature_tracker/src/feature_tracker.cpp:9-42 setMask's mask,
// :119-131 cv::goodFeaturesToTrack) behind uvs_ft_detect / uvs_ft_set_mask of include/uvs_solver.h, whose comment is the statement of the numerics.
// gfx950, on the tracker handle's stream (uvs_ft_handle.h).  The image is level 0 of the slot's stored pyramid: nothing is uploaded but the occupied
// points.  Every window sum is an integer sum; the FP64 of a pixel is one conversion, one sqrt and one subtraction, and this unit is compiled with
// -ffp-contract=off, so they round as written, which is what tests/fd_ref.py (the numpy restatement, the pin) does.
//
// Kernels of one call, in stream order, the item on the last grid axis:
//   k_ft_detect_score    a workgroup per 32 x 8 tile.  The tile with a 2-pixel halo is staged in LDS through reflect-101; Sobel gx, gy of the
//                        34 x 10 positions the tile's 3 x 3 blocks reach are computed once each into LDS, a position outside the image taking
//                        the gradient of its reflection (the products are reflected, not the image twice); a thread then sums its 3 x 3 block,
//                        writes the FP64 score, tests its pixel against the resident mask and the occupied points (256 at a time, a thread per
//                        point: the discs that reach the tile are compacted into LDS by a ballot, and only those are tested per pixel), writes
//                        the allowed byte, and the workgroup writes the largest score of its allowed pixels.
//   k_ft_detect_max      a workgroup per item: the maximum of the tiles' maxima (an FP64 max is exact in any order) and the threshold.
//   k_ft_detect_mark     a wave per 64-pixel row segment: threshold, 3 x 3 maximum, allowed; the wave's ballot is the segment's mask.
//   k_ft_detect_scan     a workgroup per item: exclusive scan of the segment counts in row-major order; n_candidates and the status.
//   k_ft_detect_emit     a wave per segment: candidate number = segment base + popcount of the mask below the lane, so the list is in row-major
//                        order and what overflows max_candidates is the same from run to run.
//   k_ft_detect_select   a workgroup of 1024 per item: bitonic sort of the (score, index) keys (2048 keys at a time in LDS; only the strides of
//                        2048 and more go through global memory), then the walk down the ranking 1024 candidates
//                        at a time: every thread tests its candidate against the taken list in LDS, the survivors are compacted in rank order,
//                        and wave 0 resolves the conflicts among them 64 at a time by a ballot loop (the first live lane is taken and kills
//                        the lanes within R of it).  The walk ends as soon as max_new are taken.  Then liftProjective of the taken points.
// No kernel uses scratch (build() checks it), no atomic is used, and one download carries the outputs of a call.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/uvs_solver.h"
#include "uvs_camera_models.h"
#include "uvs_frontend_dev.h"
#include "uvs_ft_handle.h"

namespace uvsfd {

constexpr int kThreads = 256;
constexpr int kTW = 32, kTH = 8;                              // a tile: a thread per pixel
constexpr int kPW = kTW + 4, kPH = kTH + 4;                   // staged pixels: Sobel's ring around the 3 x 3 block's ring
constexpr int kGW = kTW + 2, kGH = kTH + 2;                   // gradient positions
constexpr int kOccChunk = 256;
constexpr int kSeg = 64;
constexpr int kSelThreads = 1024, kSelWaves = kSelThreads / 64;
constexpr int kMaxTaken = UVS_FT_MAX_POINTS;                  // the taken list in LDS, (y << 16 | x) each
constexpr int kSortChunk = 2 * kSelThreads;                   // keys sorted in LDS at a time: a thread per pair
static_assert(kSortChunk * 12 <= (kMaxTaken + 2 * kSelThreads) * 4, "a chunk of keys fits the LDS block of the selection");
static_assert(kOccChunk == kThreads, "a thread per occupied point of a chunk");
static_assert(kTW * kTH == kThreads, "a thread per pixel of a tile");
static_assert(UVS_KF_MAX_WIDTH <= 65535 && UVS_KF_MAX_HEIGHT <= 65535, "a taken point packs into 32 bits");

struct FdItem {                        // device copy of one item
    int W, H, pitch, n_occ, max_new, cap, tiles_x, tiles_y, n_seg, segs_per_row, has_mask, pad;
    long long img_off;                 // bytes, in the pyramid buffer: level 0 of the slot's stored pyramid
    long long mask_off;                // bytes, in the mask buffer
    long long occ_off;                 // occupied points before this item's
    long long part_off;                // tiles before this item's
    long long seg_off;                 // segments before this item's
    long long pix_off;                 // pixels (W x H, dense) before this item's: the score and the allowed map
    long long cand_off;                // candidate keys before this item's (each item has a power of two >= cap of them)
    long long out_off;                 // output entries before this item's: the sum of max_new
};

// ---- score map, allowed map, the tiles' maxima
__global__ void __launch_bounds__(kThreads) k_ft_detect_score(const FdItem* __restrict__ items, const uint8_t* __restrict__ pyr, const uint8_t* __restrict__ mask,
                                                            const int* __restrict__ occ, int R, double* __restrict__ score, uint8_t* __restrict__ allowed,
                                                            double* __restrict__ part) {
    __shared__ int sPix[kPH][kPW];
    __shared__ int sGx[kGH][kGW], sGy[kGH][kGW];
    __shared__ int sOcc[2 * kOccChunk];
    __shared__ int sCnt[kThreads / 64];
    __shared__ double sMax[kThreads / 64];
    const FdItem F = items[blockIdx.z];
    if ((int)blockIdx.x >= F.tiles_x || (int)blockIdx.y >= F.tiles_y) return;      // workgroup-uniform: the grid is sized for the largest item of the batch
    const int tid = threadIdx.x, W = F.W, H = F.H;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const uint8_t* img = pyr + F.img_off;
    for (int i = tid; i < kPH * kPW; i += kThreads) {         // sPix[r][c] = p(refl(x0 + c - 2), refl(y0 + r - 2))
        const int r = i / kPW, c = i - r * kPW;
        sPix[r][c] = (int)img[(size_t)reflect101(y0 + r - 2, H) * F.pitch + reflect101(x0 + c - 2, W)];
    }
    __syncthreads();
    for (int i = tid; i < kGH * kGW; i += kThreads) {         // sG[r][c] = g(refl(x0 + c - 1), refl(y0 + r - 1))
        const int r = i / kGW, c = i - r * kGW;
        const int px = x0 + c - 1, py = y0 + r - 1;
        int gx = 0, gy = 0;
        if (px >= -1 && px <= W && py >= -1 && py <= H) {     // what a 3 x 3 block of an image pixel reaches; a reflected position lies in the tile's stage
            const int sc = reflect101(px, W) - x0 + 2, sr = reflect101(py, H) - y0 + 2;
            const int a = sPix[sr - 1][sc - 1], b = sPix[sr - 1][sc], cc = sPix[sr - 1][sc + 1];
            const int d = sPix[sr][sc - 1], f = sPix[sr][sc + 1];
            const int g = sPix[sr + 1][sc - 1], hh = sPix[sr + 1][sc], k = sPix[sr + 1][sc + 1];
            gx = (cc - a) + 2 * (f - d) + (k - g);
            gy = (g - a) + 2 * (hh - b) + (k - cc);
        }
        sGx[r][c] = gx; sGy[r][c] = gy;
    }
    __syncthreads();
    const int tx = tid & (kTW - 1), ty = tid / kTW;
    const int x = x0 + tx, y = y0 + ty;
    const bool in = x < W && y < H;
    int A = 0, B = 0, C = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int gx = sGx[ty + j][tx + i], gy = sGy[ty + j][tx + i];
            A += gx * gx; B += gx * gy; C += gy * gy;
        }
    const long long dAC = (long long)A - (long long)C;
    const long long S = dAC * dAC + 4ll * (long long)B * (long long)B;
    const double s = (double)(A + C) - sqrt((double)S);
    bool al = in;
    if (in && F.has_mask) al = mask[F.mask_off + (size_t)y * F.pitch + x] != 0;
    const int* o = occ + 2 * F.occ_off;
    const int lane = tid & 63, wave = tid >> 6;
    for (int base = 0; base < F.n_occ; base += kOccChunk) {   // workgroup-uniform loop
        // a thread per occupied point of the chunk: the discs that reach the tile are compacted into LDS (an OR over them: their order is free)
        int ox = 0, oy = 0;
        bool hit = false;
        if (base + tid < F.n_occ) {
            ox = o[2 * (base + tid)]; oy = o[2 * (base + tid) + 1];
            hit = !(ox + R < x0 || ox - R > x0 + kTW - 1 || oy + R < y0 || oy - R > y0 + kTH - 1);
        }
        const unsigned long long hm = __ballot(hit);
        __syncthreads();                                      // the reads of the chunk before are done
        if (lane == 0) sCnt[wave] = __popcll(hm);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) { const int v = sCnt[w]; before += w < wave ? v : 0; total += v; }
        if (hit) { const int k = before + uvs_rank_below(hm, lane); sOcc[2 * k] = ox; sOcc[2 * k + 1] = oy; }
        __syncthreads();
        for (int k = 0; k < total; ++k) {
            const int dx = x - sOcc[2 * k], dy = y - sOcc[2 * k + 1];      // |dx| <= R + 31, |dy| <= R + 7
            if (dx * dx + dy * dy <= R * R) al = false;
        }
    }
    if (in) {
        score[F.pix_off + (size_t)y * W + x] = s;
        allowed[F.pix_off + (size_t)y * W + x] = al ? 1 : 0;
    }
    double m = al ? s : 0.0;                                  // scores are >= 0: 0 is the maximum of nothing
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    if ((tid & 63) == 0) sMax[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) part[F.part_off + (size_t)blockIdx.y * F.tiles_x + blockIdx.x] = fmax(fmax(sMax[0], sMax[1]), fmax(sMax[2], sMax[3]));
}

// ---- the item's maximum and threshold
__global__ void __launch_bounds__(kThreads) k_ft_detect_max(const FdItem* __restrict__ items, const double* __restrict__ part, double quality,
                                                          uvs_ft_detect_result* __restrict__ results) {
    __shared__ double sM[kThreads];
    const FdItem F = items[blockIdx.x];
    const int tid = threadIdx.x, n = F.tiles_x * F.tiles_y;
    double m = 0.0;
    for (int i = tid; i < n; i += kThreads) m = fmax(m, part[F.part_off + i]);
    sM[tid] = m;
    __syncthreads();
    for (int off = kThreads / 2; off >= 1; off >>= 1) {
        if (tid < off) sM[tid] = fmax(sM[tid], sM[tid + off]);
        __syncthreads();
    }
    if (tid == 0) {
        uvs_ft_detect_result* r = results + blockIdx.x;
        r->max_score = sM[0]; r->threshold = quality * sM[0];
        r->n_new = 0; r->reserved = 0;
    }
}

// ---- candidates: mask and count of every 64-pixel row segment
__global__ void __launch_bounds__(kThreads) k_ft_detect_mark(const FdItem* __restrict__ items, const double* __restrict__ score, const uint8_t* __restrict__ allowed,
                                                           const uvs_ft_detect_result* __restrict__ results, unsigned long long* __restrict__ seg_mask,
                                                           int* __restrict__ seg_cnt) {
    const FdItem F = items[blockIdx.y];
    const int seg = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (seg >= F.n_seg) return;                               // wave-uniform
    const int W = F.W, H = F.H;
    const int y = seg / F.segs_per_row, x = (seg - y * F.segs_per_row) * kSeg + lane;
    const double mx = results[blockIdx.y].max_score, thr = results[blockIdx.y].threshold;
    bool keep = false;
    if (mx > 0.0 && x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2) {      // the eight neighbours are in the map
        const double* p = score + F.pix_off + (size_t)y * W + x;
        const double s = *p;
        keep = allowed[F.pix_off + (size_t)y * W + x] != 0 && s > thr && s >= p[-W - 1] && s >= p[-W] && s >= p[-W + 1] && s >= p[-1] && s >= p[1] &&
               s >= p[W - 1] && s >= p[W] && s >= p[W + 1];
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) { seg_mask[F.seg_off + seg] = m; seg_cnt[F.seg_off + seg] = __popcll(m); }
}

// ---- exclusive scan of the segment counts of one item; n_candidates and the status
__global__ void __launch_bounds__(kThreads) k_ft_detect_scan(const FdItem* __restrict__ items, const int* __restrict__ seg_cnt, int* __restrict__ seg_base,
                                                           uvs_ft_detect_result* __restrict__ results) {
    __shared__ int sPart[kThreads];
    const FdItem F = items[blockIdx.x];
    const int total = uvs_segment_scan<kThreads>(seg_cnt + F.seg_off, seg_base + F.seg_off, F.n_seg, sPart);
    if (threadIdx.x == kThreads - 1) {
        results[blockIdx.x].status = total > F.cap ? UVS_FT_DETECT_OVERFLOW : UVS_FT_DETECT_OK;
        results[blockIdx.x].n_candidates = total;
    }
}

// ---- ordered scatter of the keys (score, y W + x)
__global__ void __launch_bounds__(kThreads) k_ft_detect_emit(const FdItem* __restrict__ items, const double* __restrict__ score,
                                                           const unsigned long long* __restrict__ seg_mask, const int* __restrict__ seg_base,
                                                           double* __restrict__ cand_score, int* __restrict__ cand_index) {
    const FdItem F = items[blockIdx.y];
    const int seg = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (seg >= F.n_seg) return;
    const unsigned long long m = seg_mask[F.seg_off + seg];
    if (!((m >> lane) & 1ull)) return;
    const int idx = seg_base[F.seg_off + seg] + uvs_rank_below(m, lane);
    if (idx >= F.cap) return;
    const int y = seg / F.segs_per_row, x = (seg - y * F.segs_per_row) * kSeg + lane;
    cand_score[F.cand_off + idx] = score[F.pix_off + (size_t)y * F.W + x];
    cand_index[F.cand_off + idx] = y * F.W + x;
}

// ---- ranking and selection of one item
// key a ranks before key b: the score descending, equal scores by the pixel index descending (padding: score 0, index -1, after every candidate)
__device__ __forceinline__ bool ranks_before(double sa, int ia, double sb, int ib) { return sa > sb || (sa == sb && ia > ib); }

__global__ void __launch_bounds__(kSelThreads) k_ft_detect_select(const FdItem* __restrict__ items, UvsCamDev cam, int R, double* __restrict__ cand_score,
                                                                int* __restrict__ cand_index, uvs_ft_detect_result* __restrict__ results,
                                                                int32_t* __restrict__ new_xy, double* __restrict__ new_score, double* __restrict__ new_norm) {
    // one LDS block, used twice: a chunk of keys while the ranking is sorted, then the taken list (y << 16 | x) and the round's survivors
    __shared__ __align__(8) char sRaw[(kMaxTaken + 2 * kSelThreads) * 4];
    __shared__ int sWaveCnt[kSelWaves];
    __shared__ int sT;                                        // points taken
    double* sKs = reinterpret_cast<double*>(sRaw);
    int* sKi = reinterpret_cast<int*>(sRaw + kSortChunk * 8);
    int* sTaken = reinterpret_cast<int*>(sRaw);
    int* sSurvXY = sTaken + kMaxTaken;
    int* sSurvRank = sSurvXY + kSelThreads;
    const FdItem F = items[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(results[blockIdx.x].n_candidates, F.cap);
    double* ks = cand_score + F.cand_off;
    int* ki = cand_index + F.cand_off;
    int np = 1;
    while (np < n) np <<= 1;                                  // <= the item's key capacity, a power of two >= cap
    for (int i = n + tid; i < np; i += kSelThreads) { ks[i] = 0.0; ki[i] = -1; }
    if (tid == 0) sT = 0;
    __syncthreads();
    // bitonic sort into ranking order.  Pair t of a pass of stride j is (i, i + j), i = t with a zero inserted at bit j; in stage k the run that
    // holds i ends up in ranking order where (i & k) == 0 and reversed elsewhere.  Strides below the chunk stay inside a chunk of 2048 keys and
    // run in LDS, a thread per pair; only the strides of 2048 and more go through global memory.
    const int chunk = min(np, kSortChunk);
    auto in_chunks = [&](int k_lo, int k_hi) {                // the strides below the chunk's size of the stages k_lo .. k_hi, chunk by chunk
        for (int c0 = 0; c0 < np; c0 += chunk) {
            for (int i = tid; i < chunk; i += kSelThreads) { sKs[i] = ks[c0 + i]; sKi[i] = ki[c0 + i]; }
            __syncthreads();
            for (int k = k_lo; k <= k_hi; k <<= 1)
                for (int j = min(k, chunk) >> 1; j > 0; j >>= 1) {
                    if (tid < (chunk >> 1)) {
                        const int i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), p = i + j;
                        const double si = sKs[i], sp = sKs[p];
                        const int ii = sKi[i], ip = sKi[p];
                        if (((c0 + i) & k) == 0 ? ranks_before(sp, ip, si, ii) : ranks_before(si, ii, sp, ip)) { sKs[i] = sp; sKi[i] = ip; sKs[p] = si; sKi[p] = ii; }
                    }
                    __syncthreads();
                }
            for (int i = tid; i < chunk; i += kSelThreads) { ks[c0 + i] = sKs[i]; ki[c0 + i] = sKi[i]; }
            __syncthreads();
        }
    };
    in_chunks(2, chunk);                                      // every chunk sorted, alternately in ranking order and reversed
    for (int k = chunk << 1; k <= np; k <<= 1) {              // the stages that merge chunks
        for (int j = k >> 1; j >= chunk; j >>= 1) {
            for (int t = tid; t < (np >> 1); t += kSelThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i + j;
                const double si = ks[i], sp = ks[p];
                const int ii = ki[i], ip = ki[p];
                if ((i & k) == 0 ? ranks_before(sp, ip, si, ii) : ranks_before(si, ii, sp, ip)) { ks[i] = sp; ki[i] = ip; ks[p] = si; ki[p] = ii; }
            }
            __syncthreads();
        }
        in_chunks(k, k);
    }
    const int W = F.W, max_new = F.max_new, R2 = R * R;
    int32_t* oxy = new_xy + 2 * F.out_off;
    double* osc = new_score + F.out_off;
    for (int base = 0; base < n && max_new > 0; base += kSelThreads) {      // workgroup-uniform loop
        const int T0 = sT;
        if (T0 >= max_new) break;
        const int c = base + tid;
        int xy = 0;
        bool ok = c < n;
        if (ok) {
            const int idx = ki[c], y = idx / W, x = idx - y * W;
            xy = (y << 16) | x;
            for (int t = 0; t < T0; ++t) {
                const int q = sTaken[t], dx = x - (q & 0xffff), dy = y - (q >> 16);
                if (dx * dx + dy * dy < R2) { ok = false; break; }
            }
        }
        const unsigned long long m = __ballot(ok);
        if (lane == 0) sWaveCnt[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kSelWaves; ++w) { const int v = sWaveCnt[w]; before += w < wave ? v : 0; total += v; }
        if (ok) { const int k = before + uvs_rank_below(m, lane); sSurvXY[k] = xy; sSurvRank[k] = c; }
        __syncthreads();
        if (wave == 0) {                                      // the survivors in rank order, 64 at a time
            int T = T0;
            for (int g = 0; g < total && T < max_new; g += 64) {
                const int k = g + lane;
                bool live = k < total;
                const int me = live ? sSurvXY[k] : 0, x = me & 0xffff, y = me >> 16;
                for (int t = T0; t < T && live; ++t) {        // against what the groups before took in this round
                    const int q = sTaken[t], dx = x - (q & 0xffff), dy = y - (q >> 16);
                    if (dx * dx + dy * dy < R2) live = false;
                }
                unsigned long long a = __ballot(live);
                while (a != 0ull && T < max_new) {
                    const int f = __ffsll((long long)a) - 1;  // the best ranked live lane is taken
                    const int q = __shfl(me, f, 64);
                    if (lane == f) {
                        const int rank = sSurvRank[k];
                        sTaken[T] = me;
                        oxy[2 * T] = x; oxy[2 * T + 1] = y;
                        osc[T] = ks[rank];
                        live = false;
                    }
                    const int dx = x - (q & 0xffff), dy = y - (q >> 16);
                    if (dx * dx + dy * dy < R2) live = false;
                    ++T;
                    a = __ballot(live);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");      // sTaken before the next group's reads of it
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            }
            if (lane == 0) sT = T;
        }
        __syncthreads();
    }
    __syncthreads();
    const int T = sT;
    double* onm = new_norm + 2 * F.out_off;
    for (int t = tid; t < T; t += kSelThreads) {
        const int q = sTaken[t];
        double ray[3], mx, my;
        uvs_cam_lift(cam, (double)(q & 0xffff), (double)(q >> 16), ray, mx, my);
        onm[2 * t] = mx; onm[2 * t + 1] = my;
    }
    if (tid == 0) results[blockIdx.x].n_new = T;
}

}  // namespace uvsfd

using namespace uvsfd;

namespace {

inline int pow2_at_least(int n) { int p = 1; while (p < n) p <<= 1; return p; }

struct FdLayout {                      // byte offsets in d_det; res .. norm are one block, downloaded in one copy
    size_t items, occ, part, seg_mask, seg_cnt, seg_base, score, allowed, cscore, cindex, res, xy, sc, norm, end;
};

// what uvs_ft_detect and uvs_ft_debug_detect share; dbg_*: the maps and the ranked candidates of the ONE item
int fd_run(uvs_ft_tracker* h, const char* who_, int n_items, const uvs_ft_detect_item* items, double quality, int min_distance, const uvs_kf_camera* camera,
           int32_t* new_xy, double* new_score, double* new_norm, uvs_ft_detect_result* results, double* dbg_score, uint8_t* dbg_allowed,
           int32_t* dbg_cindex, double* dbg_cscore) {
    const std::string fn = who_;
    h->err.clear();
    if (n_items < 1 || !items || (!camera && h->model.model < 0) || !new_xy || !new_score || !new_norm || !results) { h->err = fn + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG; }
    if (n_items > h->max_streams) { h->err = fn + ": more items than the slots given to uvs_ft_create"; return UVS_ERR_CAPACITY; }
    if (!(quality > 0.0 && quality <= 1.0)) { h->err = fn + ": quality_level must be in (0, 1]"; return UVS_ERR_INVALID_ARG; }
    if (min_distance < 1 || min_distance > UVS_FT_MAX_MIN_DISTANCE) { h->err = fn + ": min_distance must be 1 .. UVS_FT_MAX_MIN_DISTANCE"; return UVS_ERR_INVALID_ARG; }
    UvsCamDev cam;
    if (const int rc = uvs_cam_of_call(h->model, camera, fn, h->err, &cam)) return rc;
    std::vector<char> seen(h->max_streams, 0);
    for (int i = 0; i < n_items; ++i) {
        const uvs_ft_detect_item& it = items[i];
        const std::string who = fn + ": item " + std::to_string(i);
        if (it.n_occupied < 0 || it.max_new < 0 || (it.n_occupied > 0 && !it.occupied_xy)) { h->err = who + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG; }
        if (it.stream < 0 || it.stream >= h->max_streams) { h->err = who + ": the stream is not a slot of the handle"; return UVS_ERR_INVALID_ARG; }
        if (seen[it.stream]) { h->err = who + ": the stream appears twice in the call"; return UVS_ERR_INVALID_ARG; }
        seen[it.stream] = 1;
        if (!h->slots[it.stream].holds) { h->err = who + ": the slot holds no image"; return UVS_ERR_INVALID_ARG; }
        if (it.n_occupied > h->max_points || it.max_new > h->max_points) { h->err = who + " exceeds the capacity given to uvs_ft_create"; return UVS_ERR_CAPACITY; }
        for (int k = 0; k < 2 * it.n_occupied; ++k)
            if (!std::isfinite(it.occupied_xy[k]) || std::fabs(it.occupied_xy[k]) > UVS_KF_MAX_COORD) {
                h->err = who + ": an occupied point is not finite or beyond UVS_KF_MAX_COORD"; return UVS_ERR_INVALID_ARG;
            }
    }
    // the layout of the call
    std::vector<FdItem> F(n_items);
    size_t n_occ = 0, n_part = 0, n_seg = 0, n_pix = 0, n_key = 0, n_out = 0;
    int top_tx = 0, top_ty = 0, top_seg = 0;
    for (int i = 0; i < n_items; ++i) {
        const uvs_ft_detect_item& it = items[i];
        const uvs_ft_tracker::Slot& s = h->slots[it.stream];
        FdItem& d = F[i];
        d.W = s.W; d.H = s.H; d.pitch = pitch_of(s.W); d.n_occ = it.n_occupied; d.max_new = it.max_new;
        d.cap = (int)std::min<long long>(h->max_candidates, (long long)s.W * s.H);
        d.tiles_x = (s.W + kTW - 1) / kTW; d.tiles_y = (s.H + kTH - 1) / kTH;
        d.segs_per_row = (s.W + kSeg - 1) / kSeg; d.n_seg = d.segs_per_row * s.H;
        d.has_mask = s.has_mask ? 1 : 0; d.pad = 0;
        d.img_off = (long long)((size_t)(2 * it.stream + s.cur) * h->pyr_bytes);      // level 0 is the first of a pyramid
        d.mask_off = (long long)((size_t)it.stream * h->img_slot);
        d.occ_off = (long long)n_occ; d.part_off = (long long)n_part; d.seg_off = (long long)n_seg; d.pix_off = (long long)n_pix;
        d.cand_off = (long long)n_key; d.out_off = (long long)n_out;
        n_occ += it.n_occupied; n_part += (size_t)d.tiles_x * d.tiles_y; n_seg += d.n_seg; n_pix += (size_t)s.W * s.H;
        n_key += pow2_at_least(d.cap); n_out += it.max_new;
        top_tx = std::max(top_tx, d.tiles_x); top_ty = std::max(top_ty, d.tiles_y); top_seg = std::max(top_seg, d.n_seg);
    }
    FdLayout L;
    UvsArena A;
    L.items = A.take(n_items * sizeof(FdItem)); L.occ = A.take(n_occ * 8);
    L.part = A.take(n_part * 8); L.seg_mask = A.take(n_seg * 8); L.seg_cnt = A.take(n_seg * 4); L.seg_base = A.take(n_seg * 4);
    L.score = A.take(n_pix * 8); L.allowed = A.take(n_pix); L.cscore = A.take(n_key * 8); L.cindex = A.take(n_key * 4);
    L.res = A.take(n_items * sizeof(uvs_ft_detect_result));
    L.xy = A.take(n_out * 8); L.sc = A.take(n_out * 8); L.norm = A.take(n_out * 16);
    L.end = A.o;
    const size_t in_bytes = L.part, out_bytes = L.end - L.res;      // items | occupied points;  results | new_xy | new_score | new_norm
    UVS_HIP(h->err, hipSetDevice(h->device));
    int rc;
    if ((rc = h->d_det.ensure(L.end, h->err)) != UVS_OK || (rc = h->h_det_in.ensure(in_bytes, h->err, grow_pinned)) != UVS_OK ||
        (rc = h->h_det_out.ensure(out_bytes, h->err, grow_pinned)) != UVS_OK) return rc;
    std::memcpy(h->h_det_in + L.items, F.data(), n_items * sizeof(FdItem));
    int* h_occ = reinterpret_cast<int*>(h->h_det_in + L.occ);
    for (int i = 0, k = 0; i < n_items; ++i)
        for (int j = 0; j < 2 * items[i].n_occupied; ++j) h_occ[k++] = (int)std::nearbyint(items[i].occupied_xy[j]);      // half to even
    char* D = h->d_det;
    const FdItem* dF = reinterpret_cast<const FdItem*>(D + L.items);
    const int* dOcc = reinterpret_cast<const int*>(D + L.occ);
    double* dPart = reinterpret_cast<double*>(D + L.part);
    unsigned long long* dMask = reinterpret_cast<unsigned long long*>(D + L.seg_mask);
    int* dCnt = reinterpret_cast<int*>(D + L.seg_cnt);
    int* dBase = reinterpret_cast<int*>(D + L.seg_base);
    double* dScore = reinterpret_cast<double*>(D + L.score);
    uint8_t* dAllowed = reinterpret_cast<uint8_t*>(D + L.allowed);
    double* dCs = reinterpret_cast<double*>(D + L.cscore);
    int* dCi = reinterpret_cast<int*>(D + L.cindex);
    uvs_ft_detect_result* dRes = reinterpret_cast<uvs_ft_detect_result*>(D + L.res);
    int32_t* dXy = reinterpret_cast<int32_t*>(D + L.xy);
    double* dSc = reinterpret_cast<double*>(D + L.sc);
    double* dNorm = reinterpret_cast<double*>(D + L.norm);
    const unsigned seg_blocks = (unsigned)((top_seg + kThreads / 64 - 1) / (kThreads / 64));
    hipStream_t st = h->st;
    UVS_HIP(h->err, hipEventRecord(h->ev0, st));
    UVS_HIP(h->err, hipMemcpyAsync(D, h->h_det_in, in_bytes, hipMemcpyHostToDevice, st));
    k_ft_detect_score<<<dim3(top_tx, top_ty, n_items), kThreads, 0, st>>>(dF, h->d_pyr, h->d_mask, dOcc, min_distance, dScore, dAllowed, dPart);
    k_ft_detect_max<<<n_items, kThreads, 0, st>>>(dF, dPart, quality, dRes);
    k_ft_detect_mark<<<dim3(seg_blocks, n_items), kThreads, 0, st>>>(dF, dScore, dAllowed, dRes, dMask, dCnt);
    k_ft_detect_scan<<<n_items, kThreads, 0, st>>>(dF, dCnt, dBase, dRes);
    k_ft_detect_emit<<<dim3(seg_blocks, n_items), kThreads, 0, st>>>(dF, dScore, dMask, dBase, dCs, dCi);
    k_ft_detect_select<<<n_items, kSelThreads, 0, st>>>(dF, cam, min_distance, dCs, dCi, dRes, dXy, dSc, dNorm);
    UVS_HIP(h->err, hipGetLastError());
    UVS_HIP(h->err, hipMemcpyAsync(h->h_det_out, D + L.res, out_bytes, hipMemcpyDeviceToHost, st));
    UVS_HIP(h->err, hipEventRecord(h->ev1, st));
    UVS_HIP(h->err, hipStreamSynchronize(st));
    UVS_HIP(h->err, hipEventElapsedTime(&h->detect_ms, h->ev0, h->ev1));
    const char* out = h->h_det_out;
    std::memcpy(results, out, n_items * sizeof(uvs_ft_detect_result));
    for (int i = 0; i < n_items; ++i) {
        const size_t off = (size_t)F[i].out_off, n = (size_t)results[i].n_new;
        std::memcpy(new_xy + 2 * off, out + (L.xy - L.res) + off * 8, n * 8);
        std::memcpy(new_score + off, out + (L.sc - L.res) + off * 8, n * 8);
        std::memcpy(new_norm + 2 * off, out + (L.norm - L.res) + off * 16, n * 16);
    }
    if (dbg_score) {                                          // one item: its maps and keys start at their arrays' heads
        const size_t px = (size_t)F[0].W * F[0].H, nk = (size_t)std::min(results[0].n_candidates, F[0].cap);
        UVS_HIP(h->err, hipMemcpy(dbg_score, dScore, px * 8, hipMemcpyDeviceToHost));
        UVS_HIP(h->err, hipMemcpy(dbg_allowed, dAllowed, px, hipMemcpyDeviceToHost));
        if (nk) {
            UVS_HIP(h->err, hipMemcpy(dbg_cscore, dCs, nk * 8, hipMemcpyDeviceToHost));
            UVS_HIP(h->err, hipMemcpy(dbg_cindex, dCi, nk * 4, hipMemcpyDeviceToHost));
        }
    }
    return UVS_OK;
}

}  // namespace

extern "C" {

int uvs_ft_set_max_candidates(uvs_ft_tracker* h, int max_candidates) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    if (max_candidates < 1 || max_candidates > UVS_FT_MAX_CANDIDATES) { h->err = "uvs_ft_set_max_candidates: 1 .. UVS_FT_MAX_CANDIDATES"; return UVS_ERR_INVALID_ARG; }
    h->max_candidates = max_candidates;
    return UVS_OK;
}

int uvs_ft_set_mask(uvs_ft_tracker* h, int stream, const uint8_t* mask, int width, int height) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    if (stream < 0 || stream >= h->max_streams) { h->err = "uvs_ft_set_mask: the stream is not a slot of the handle"; return UVS_ERR_INVALID_ARG; }
    uvs_ft_tracker::Slot& s = h->slots[stream];
    if (!mask) { s.has_mask = false; return UVS_OK; }
    if (!s.holds) { h->err = "uvs_ft_set_mask: the slot holds no image"; return UVS_ERR_INVALID_ARG; }
    if (width != s.W || height != s.H) { h->err = "uvs_ft_set_mask: the mask's size is not the slot's"; return UVS_ERR_INVALID_ARG; }
    UVS_HIP(h->err, hipSetDevice(h->device));
    const int rc = h->d_mask.ensure((size_t)h->max_streams * h->img_slot, h->err);
    if (rc != UVS_OK) return rc;
    UVS_HIP(h->err, hipMemcpy2DAsync(h->d_mask + (size_t)stream * h->img_slot, pitch_of(width), mask, width, width, height, hipMemcpyHostToDevice, h->st));
    UVS_HIP(h->err, hipStreamSynchronize(h->st));
    s.has_mask = true;
    return UVS_OK;
}

int uvs_ft_detect(uvs_ft_tracker* h, int n_items, const uvs_ft_detect_item* items, double quality_level, int min_distance, const uvs_kf_camera* camera,
                  int32_t* new_xy, double* new_score, double* new_norm, uvs_ft_detect_result* results) {
    if (!h) return UVS_ERR_INVALID_ARG;
    return fd_run(h, "uvs_ft_detect", n_items, items, quality_level, min_distance, camera, new_xy, new_score, new_norm, results, nullptr, nullptr, nullptr, nullptr);
}

double uvs_ft_last_detect_device_ms(const uvs_ft_tracker* h) { return h ? (double)h->detect_ms : 0.0; }

int uvs_ft_debug_detect(uvs_ft_tracker* h, const uvs_ft_detect_item* item, double quality_level, int min_distance, const uvs_kf_camera* camera, double* score,
                        uint8_t* allowed, int32_t* cand_index, double* cand_score, int32_t* new_xy, double* new_score, double* new_norm,
                        uvs_ft_detect_result* result) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    if (!item || !score || !allowed || !cand_index || !cand_score) { h->err = "uvs_ft_debug_detect: null pointer"; return UVS_ERR_INVALID_ARG; }
    return fd_run(h, "uvs_ft_debug_detect", 1, item, quality_level, min_distance, camera, new_xy, new_score, new_norm, result, score, allowed, cand_index, cand_score);
}

}  // extern "C"
