// uvs_ft_reject_kernel.h -- the fundamental-matrix RANSAC kernel k_ft_reject_run with the item type and the device functions it needs, the one
// statement of it for the two units that launch it: csrc/uvs_feature_reject.hip (uvs_ft_reject, on the tracker handle) and
// csrc/uvs_relative_pose.hip (uvs_rp_relative_pose, between its gate and its recover kernel).  The comment of uvs_ft_reject in
// include/uvs_solver.h is the statement of the numerics, tests/fr_ref.py the pin.  Every FP64 operation is one of + - * / sqrt in the order the
// header gives, and an including unit must compile this file without contraction (-ffp-contract=off, or #pragma clang fp contract(off) in front
// of the include), so that they round as written; the one log is in the stopping rule.
//
// k_ft_reject_run<kGated>: a workgroup of 256 per item, a thread per hypothesis, in rounds of 256 hypotheses.
//   solve      the thread draws its 7 tracks and writes the 7 x 9 matrix into LDS, laid out [entry][thread] (63 x 256 doubles = 126 KiB of the
//              CU's 160; a lane's entries are a fixed bank apart from its neighbours' whatever entry each lane picks, so the run-time indexed
//              pivot search costs no conflict and nothing lands in scratch).  Gauss-Jordan with complete pivoting moves no row or column:
//              two bit masks say which hold a pivot.  The two null vectors are scattered through the same LDS column into F1, F2, read back
//              into registers; cubic, bisection and Newton run out of registers.
//   score      each thread scores its up to three models against all n tracks; the track index is the same in every lane, so the
//              coordinates are wave-uniform loads.
//   replay     thread 0 replays OpenCV's sequential selection over the round's counts; the owner of a new best model publishes its F in LDS.
//              The loop over the rounds ends as soon as niters <= the hypotheses done (uvs_ft_debug_reject evaluates every round; the replay
//              has ended all the same, so the result is the same).
//   mask       a thread per track tests the chosen F with the instructions that counted it: popcount(keep) == n_inliers.
// kGated (uvs_relative_pose only): an item whose `gated` word is set leaves at once, before it touches LDS or writes anything; with kGated =
// false the word is not read and the kernel is the one uvs_feature_reject.hip held before this header existed.
// No scratch (build() checks it), no atomic; an item gives the same bits alone or in a batch.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/uvs_solver.h"
#include "uvs_frontend_dev.h"

namespace uvsfr {

constexpr int kThreads = 256;                                 // hypotheses of a round
constexpr int kHyp = UVS_FT_REJECT_HYPOTHESES;
constexpr int kModel = 7;
constexpr int kAttempts = 64;
constexpr int kBisections = 60, kNewton = 4;
constexpr double kPivotRel = 1e-10;
static_assert(63 * kThreads * 8 + 4096 <= 160 * 1024, "the matrices of a round fit the LDS of a CU");

struct FrItem {                        // device copy of one item
    int n, gated;                      // gated: read by k_ft_reject_run<true> only (written by k_rp_gate)
    unsigned long long seed;
    long long pts_off;                 // doubles before this item's prev[n][2] | next[n][2]
    long long keep_off;                // tracks before this item's
};

__device__ __forceinline__ double det3(double u0, double u1, double u2, double v0, double v1, double v2, double w0, double w1, double w2) {
    return (u0 * (v1 * w2 - v2 * w1) - u1 * (v0 * w2 - v2 * w0)) + u2 * (v0 * w1 - v1 * w0);
}

__device__ __forceinline__ double poly(double c0, double c1, double c2, double c3, double x) { return ((c3 * x + c2) * x + c1) * x + c0; }

// OpenCV's computeError on one track; a NaN is an outlier
__device__ __forceinline__ bool inlier(const double* F, double x1, double y1, double x2, double y2, double t2) {
    double a = (F[0] * x1 + F[1] * y1) + F[2];
    double b = (F[3] * x1 + F[4] * y1) + F[5];
    double c = (F[6] * x1 + F[7] * y1) + F[8];
    const double s2 = (x2 * a + y2 * b) + c;
    const double d2 = s2 * s2 / (a * a + b * b);
    a = (F[0] * x2 + F[3] * y2) + F[6];
    b = (F[1] * x2 + F[4] * y2) + F[7];
    c = (F[2] * x2 + F[5] * y2) + F[8];
    const double s1 = (x1 * a + y1 * b) + c;
    const double d1 = s1 * s1 / (a * a + b * b);
    return d1 <= t2 && d2 <= t2;
}

// OpenCV RANSACUpdateNumIters with model_points = 7, (1 - ep)^7 by six multiplications; cvRound = round half to even (rint)
__device__ inline int update_num_iters(double p, double ep, int max_iters) {
    p = fmin(fmax(p, 0.0), 1.0); ep = fmin(fmax(ep, 0.0), 1.0);
    double num = fmax(1.0 - p, DBL_MIN);
    const double w = 1.0 - ep;
    double q = w;
#pragma unroll
    for (int i = 0; i < kModel - 1; ++i) q = q * w;
    double denom = 1.0 - q;
    if (denom < DBL_MIN) return 0;
    num = log(num); denom = log(denom);
    return (denom >= 0 || -num >= max_iters * (-denom)) ? max_iters : (int)rint(num / denom);
}

enum { kSelH = 0, kSelR, kSelBest, kSelNiters, kSelPos, kSelDone, kSelWords };

template <bool kGated>
__global__ void __launch_bounds__(kThreads) k_ft_reject_run(const FrItem* __restrict__ items, const double* __restrict__ pts, double threshold, double confidence,
                                                          int full, uint8_t* __restrict__ keep, uvs_ft_reject_result* __restrict__ results,
                                                          int32_t* __restrict__ dbg_samples, double* __restrict__ dbg_models, int32_t* __restrict__ dbg_counts) {
    __shared__ double sA[63 * kThreads];                      // [entry][thread]
    __shared__ int sCnt[3 * kThreads];
    __shared__ double sF[9];
    __shared__ int sSel[kSelWords];
    const FrItem it = items[blockIdx.x];
    if (kGated && it.gated) return;                           // workgroup-uniform, in front of every barrier
    const int tid = threadIdx.x, n = it.n;
    const double* prev = pts + it.pts_off;
    const double* next = prev + 2 * (size_t)n;
    const double t2 = threshold * threshold;
    double* A = sA + tid;
#define FR_A(r, c) A[((r) * 9 + (c)) * kThreads]
    if (tid == 0) {
        sSel[kSelH] = -1; sSel[kSelR] = -1; sSel[kSelBest] = 0; sSel[kSelNiters] = kHyp; sSel[kSelPos] = 0; sSel[kSelDone] = n < 8 ? 1 : 0;
    }
    if (tid < 9) sF[tid] = 0.0;
    __syncthreads();
    if (n < 8) {
        if (full)                                             // nothing is drawn: no sample, no model, no count
            for (int h = tid; h < kHyp; h += kThreads) {
                for (int j = 0; j < kModel; ++j) dbg_samples[h * kModel + j] = -1;
                for (int j = 0; j < 27; ++j) dbg_models[h * 27 + j] = 0.0;
                for (int j = 0; j < 3; ++j) dbg_counts[h * 3 + j] = -1;
            }
    } else {
        for (int base = 0; base < kHyp; base += kThreads) {   // workgroup-uniform loop
            const int h = base + tid;
            bool valid = h < kHyp;
            // ---- sample: 7 distinct tracks within 64 draws; each taken track's row goes straight into the matrix
            int i0 = -1, i1 = -1, i2 = -1, i3 = -1, i4 = -1, i5 = -1, i6 = -1, cnt = 0;
            if (valid) {
                for (int a = 0; a < kAttempts && cnt < kModel; ++a) {
                    const unsigned long long z = uvs_draw(it.seed, h, a);
                    const int v = (int)(z % (unsigned long long)n);
                    if (v == i0 || v == i1 || v == i2 || v == i3 || v == i4 || v == i5 || v == i6) continue;
                    i0 = cnt == 0 ? v : i0; i1 = cnt == 1 ? v : i1; i2 = cnt == 2 ? v : i2; i3 = cnt == 3 ? v : i3;
                    i4 = cnt == 4 ? v : i4; i5 = cnt == 5 ? v : i5; i6 = cnt == 6 ? v : i6;
                    const double x1 = prev[2 * v], y1 = prev[2 * v + 1], x2 = next[2 * v], y2 = next[2 * v + 1];
                    FR_A(cnt, 0) = x2 * x1; FR_A(cnt, 1) = x2 * y1; FR_A(cnt, 2) = x2;
                    FR_A(cnt, 3) = y2 * x1; FR_A(cnt, 4) = y2 * y1; FR_A(cnt, 5) = y2;
                    FR_A(cnt, 6) = x1; FR_A(cnt, 7) = y1; FR_A(cnt, 8) = 1.0;
                    ++cnt;
                }
                if (cnt < kModel) { valid = false; i0 = i1 = i2 = i3 = i4 = i5 = i6 = -1; }
                if (full) {
                    int32_t* s = dbg_samples + h * kModel;
                    s[0] = i0; s[1] = i1; s[2] = i2; s[3] = i3; s[4] = i4; s[5] = i5; s[6] = i6;
                }
            }
            // ---- null space: Gauss-Jordan with complete pivoting; rf, cf: the rows and columns that hold no pivot yet
            unsigned rf = 0x7fu, cf = 0x1ffu, prow = 0u, pcol = 0u;
            double first = 0.0;
#pragma unroll 1
            for (int k = 0; k < kModel; ++k) {
                if (!valid) continue;
                double best = -1.0;
                int pr = 0, pc = 0;
#pragma unroll
                for (int r = 0; r < 7; ++r)
#pragma unroll
                    for (int c = 0; c < 9; ++c)
                        if (((rf >> r) & 1u) && ((cf >> c) & 1u)) {
                            const double v = fabs(FR_A(r, c));
                            if (v > best) { best = v; pr = r; pc = c; }
                        }
                const double p = FR_A(pr, pc);
                if (k == 0) first = fabs(p);
                if (!(fabs(p) > kPivotRel * first)) { valid = false; continue; }
                rf &= ~(1u << pr); cf &= ~(1u << pc);
                prow |= (unsigned)pr << (4 * k); pcol |= (unsigned)pc << (4 * k);
                double piv[9];
#pragma unroll
                for (int c = 0; c < 9; ++c) {
                    piv[c] = 0.0;
                    if ((cf >> c) & 1u) { piv[c] = FR_A(pr, c) / p; FR_A(pr, c) = piv[c]; }
                }
#pragma unroll
                for (int r = 0; r < 7; ++r) {
                    if (r == pr) continue;
                    const double f = FR_A(r, pc);
#pragma unroll
                    for (int c = 0; c < 9; ++c)
                        if ((cf >> c) & 1u) FR_A(r, c) = FR_A(r, c) - f * piv[c];
                }
            }
            double f1[9], f2[9];
            double lam0 = 0.0, lam1 = 0.0, lam2 = 0.0;
            int nroots = 0;
            if (valid) {
                // the two columns left, c1 < c2; the null vectors are scattered by pivot column through this thread's LDS column
                const int c1 = __ffs((int)cf) - 1, c2 = __ffs((int)(cf & (cf - 1u))) - 1;
                double v1[7], v2[7];
#pragma unroll
                for (int k = 0; k < 7; ++k) { const int r = (prow >> (4 * k)) & 15; v1[k] = -FR_A(r, c1); v2[k] = -FR_A(r, c2); }
#pragma unroll
                for (int k = 0; k < 7; ++k) { const int c = (pcol >> (4 * k)) & 15; A[c * kThreads] = v1[k]; A[(9 + c) * kThreads] = v2[k]; }
                A[c1 * kThreads] = 1.0; A[c2 * kThreads] = 0.0; A[(9 + c1) * kThreads] = 0.0; A[(9 + c2) * kThreads] = 1.0;
#pragma unroll
                for (int j = 0; j < 9; ++j) { f1[j] = A[j * kThreads]; f2[j] = A[(9 + j) * kThreads]; }
                // ---- the cubic det(F1 + l F2): columns taken from F1 (a) or F2 (b)
#define FR_COL(f, j) f[j], f[3 + j], f[6 + j]
                const double c0 = det3(FR_COL(f1, 0), FR_COL(f1, 1), FR_COL(f1, 2));
                const double cc1 = (det3(FR_COL(f2, 0), FR_COL(f1, 1), FR_COL(f1, 2)) + det3(FR_COL(f1, 0), FR_COL(f2, 1), FR_COL(f1, 2))) +
                                   det3(FR_COL(f1, 0), FR_COL(f1, 1), FR_COL(f2, 2));
                const double cc2 = (det3(FR_COL(f2, 0), FR_COL(f2, 1), FR_COL(f1, 2)) + det3(FR_COL(f2, 0), FR_COL(f1, 1), FR_COL(f2, 2))) +
                                   det3(FR_COL(f1, 0), FR_COL(f2, 1), FR_COL(f2, 2));
                const double c3 = det3(FR_COL(f2, 0), FR_COL(f2, 1), FR_COL(f2, 2));
#undef FR_COL
                double m = fabs(c0);
                m = fabs(cc1) > m ? fabs(cc1) : m;
                m = fabs(cc2) > m ? fabs(cc2) : m;
                const double R = 1.0 + m / fabs(c3);
                if (!(isfinite(c0) && isfinite(cc1) && isfinite(cc2) && isfinite(c3) && c3 != 0.0 && isfinite(R))) valid = false;
                if (valid) {
                    const double D = cc2 * cc2 - (3.0 * c3) * cc1;
                    const bool three = D > 0.0;
                    double lo = -R, hi = -R;
                    if (three) {
                        const double s = sqrt(D);
                        double e1 = (-cc2 - s) / (3.0 * c3), e2 = (-cc2 + s) / (3.0 * c3);
                        e1 = e1 < -R ? -R : e1; e1 = e1 > R ? R : e1;
                        e2 = e2 < -R ? -R : e2; e2 = e2 > R ? R : e2;
                        lo = e2 < e1 ? e2 : e1; hi = e2 < e1 ? e1 : e2;
                    }
#pragma unroll 1
                    for (int iv = 0; iv < 3; ++iv) {          // the monotone intervals in ascending order
                        if (iv > 0 && !three) continue;
                        double a = iv == 0 ? -R : (iv == 1 ? lo : hi);
                        double b = three ? (iv == 0 ? lo : (iv == 1 ? hi : R)) : R;
                        const double fa = poly(c0, cc1, cc2, c3, a), fb = poly(c0, cc1, cc2, c3, b);
                        const bool up = fa <= 0.0 && fb > 0.0, down = fa >= 0.0 && fb < 0.0;
                        if (!(up || down)) continue;
#pragma unroll 1
                        for (int i = 0; i < kBisections; ++i) {
                            const double mid = 0.5 * a + 0.5 * b;
                            const double fm = poly(c0, cc1, cc2, c3, mid);
                            const bool to_b = up ? fm > 0.0 : fm < 0.0;
                            b = to_b ? mid : b; a = to_b ? a : mid;
                        }
                        double x = 0.5 * a + 0.5 * b;
#pragma unroll 1
                        for (int i = 0; i < kNewton; ++i) {
                            const double d = ((3.0 * c3) * x + 2.0 * cc2) * x + cc1;
                            const double xn = x - poly(c0, cc1, cc2, c3, x) / d;
                            x = (xn >= a && xn <= b) ? xn : x;
                        }
                        lam0 = nroots == 0 ? x : lam0; lam1 = nroots == 1 ? x : lam1; lam2 = nroots == 2 ? x : lam2;
                        ++nroots;
                    }
                }
            }
            // ---- score: the count of every model over all the tracks
#pragma unroll 1
            for (int r = 0; r < 3; ++r) {
                int count = -1;
                double F[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) F[j] = 0.0;
                if (valid && r < nroots) {
                    const double lam = r == 0 ? lam0 : (r == 1 ? lam1 : lam2);
#pragma unroll
                    for (int j = 0; j < 9; ++j) F[j] = f1[j] + lam * f2[j];
                    count = 0;
                    for (int i = 0; i < n; ++i) count += inlier(F, prev[2 * i], prev[2 * i + 1], next[2 * i], next[2 * i + 1], t2) ? 1 : 0;
                }
                sCnt[3 * tid + r] = count;
                if (full && h < kHyp) {
#pragma unroll
                    for (int j = 0; j < 9; ++j) dbg_models[(h * 3 + r) * 9 + j] = F[j];
                    dbg_counts[h * 3 + r] = count;
                }
            }
            __syncthreads();
            // ---- replay of the sequential selection over the round's counts
            if (tid == 0 && !sSel[kSelDone]) {
                int bh = sSel[kSelH], br = sSel[kSelR], best = sSel[kSelBest], niters = sSel[kSelNiters], hh = sSel[kSelPos];
                const int lim = min(base + kThreads, kHyp);
                while (hh < niters && hh < lim) {
                    for (int r = 0; r < 3; ++r) {
                        const int c = sCnt[3 * (hh - base) + r];
                        if (c > max(best, kModel - 1)) {
                            bh = hh; br = r; best = c;
                            niters = update_num_iters(confidence, (double)(n - c) / (double)n, niters);
                        }
                    }
                    ++hh;
                }
                sSel[kSelH] = bh; sSel[kSelR] = br; sSel[kSelBest] = best; sSel[kSelNiters] = niters; sSel[kSelPos] = hh;
                sSel[kSelDone] = hh >= niters ? 1 : 0;
            }
            __syncthreads();
            if (sSel[kSelH] == h) {                           // the owner of the best model so far publishes it (again, if it was this round's already)
                const int r = sSel[kSelR];
                const double lam = r == 0 ? lam0 : (r == 1 ? lam1 : lam2);
#pragma unroll
                for (int j = 0; j < 9; ++j) sF[j] = f1[j] + lam * f2[j];
            }
            __syncthreads();                                  // sF; and the round's reads of sCnt and sA before the next round's writes
            if (sSel[kSelDone] && !full) break;
        }
    }
#undef FR_A
    // ---- the chosen model's mask, by the instructions that counted it; the result block
    const int bh = sSel[kSelH];
    uint8_t* kp = keep + it.keep_off;
    double F[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) F[j] = sF[j];
    for (int i = tid; i < n; i += kThreads)
        kp[i] = bh < 0 ? 1 : (inlier(F, prev[2 * i], prev[2 * i + 1], next[2 * i], next[2 * i + 1], t2) ? 1 : 0);
    if (tid == 0) {
        uvs_ft_reject_result* res = results + blockIdx.x;
        res->status = n < 8 ? UVS_FT_REJECT_SKIPPED : (bh < 0 ? UVS_FT_REJECT_NO_MODEL : UVS_FT_REJECT_OK);
        res->n_inliers = bh < 0 ? n : sSel[kSelBest];
        res->hypothesis = bh; res->root = sSel[kSelR]; res->iterations = sSel[kSelPos]; res->reserved = 0;
        int k = 0;
        double big = -1.0;
        for (int j = 0; j < 9; ++j) { const double v = fabs(sF[j]); if (v > big) { big = v; k = j; } }
        const double s = sF[k];
        for (int j = 0; j < 9; ++j) res->F[j] = bh < 0 ? 0.0 : sF[j] / s;
    }
}

}  // namespace uvsfr
