// uvs_vanishing_points.hip -- vanishing-point estimation of the line front end (reference feature_tracker/src/line_feature_tracker.cpp:1977-2299:
// getVPHypVia2Lines, getSphereGrids, getBestVpsHyp, lines2Vps; called at :86-91, consumed at :379-385) behind the uvs_vp_* calls of
// include/uvs_solver.h.  FP64, gfx950, one stream per handle.  Pure geometry on line segments: no image is involved.
//
// One call estimates a batch of frames; every kernel's grid has the frame on blockIdx.x and no kernel reads another frame's data, so a frame
// gives the same bits alone or in a batch.  This unit is compiled with -ffp-contract=off: products and sums round as written, which is what
// tests/vp_ref.py (the numpy restatement, the pin) does.  Kernels of one call, in stream order:
//   k_vp_prepare   one workgroup per frame.  Line parameters (para = p1 x p2, length, orientation folded into [0, pi)), the power-of-two scale
//                  of the frame's voting grid, and the UVS_VP_N_SAMPLES line pairs of the hypotheses:
//                  UVS_VP_N_SAMPLES = int(log(1 - 0.9999) / log(1 - (1/3) * 0.5^2)) = 105  (:1981-1985).
//                  Sample s, attempt t draws a = z(2t) % n, b = z(2t + 1) % n with z(c) = mix64(seed + 0x9E3779B97F4A7C15 * (1 + (s << 20) + c))
//                  (uvs_draw of uvs_frontend_dev.h, the generator of uvs_loop_verify.hip); the attempt is redrawn when a == b or
//                  (para_a x para_b).z == 0 (:2016-2029).
//                  The reference redraws forever; here a sample that finds no pair in kMaxAttempts attempts makes the frame UVS_VP_NO_HYPOTHESIS.
//   k_vp_vote      thread per line pair i < j (:2104-2148).  The weight sqrt(len_i len_j) (sin(2 dev) + 0.2) goes into the pair's cell of the
//                  90 x 360 grid.  Deterministic sum: the grid lives in global memory (259 200 B of doubles per frame do not fit the 160 KiB of
//                  LDS) as TWO 64-bit integers per cell (518 400 B per frame), and a weight is added as
//                  hi = rint(w 2^e), lo = rint((w 2^e - hi) 2^40) with integer atomics.  Integer addition is associative, so the cell does
//                  not depend on the order in which the atomics land; 2^e is chosen per frame so that 1.2 max(len) 2^e <= 2^40 (hi of
//                  2^19 pairs cannot overflow), and what is dropped is below 2^-81 of the largest possible weight: the cell is the exact sum
//                  of its weights to well inside one double rounding.
//   k_vp_smooth    thread per cell: limbs -> double, the 3 x 3 window of :2151-2173, border rows and columns zero.
//   k_vp_score     workgroup per (frame, sample): thread j builds hypothesis 360 s + j exactly as :2031-2071 (the 0.0011 substitutions, the
//                  flip to z >= 0), its three cells and score = ((0 + g[c0]) + g[c1]) + g[c2]; the workgroup keeps its best (largest score,
//                  lowest index).
//   k_vp_select    workgroup per frame: the best of the 105 (lowest index of the maximum; 0 when every score is 0), then lines2Vps (:2232-2299)
//                  and the per-line vector vps[tag] / vps[tag].z (:379-385).
//
// The cell rule (all four indices: pair latitude / longitude, hypothesis latitude / longitude): q = angle / (pi / 180); when |q - rint(q)| <= 1e-9
// the cell is rint(q), otherwise q truncated; then clamped to the grid as the reference does.  vp2's longitude is lambda (+ pi) by construction --
// exactly a cell boundary -- so the reference's int(longitude / oneDegree) is decided by the rounding of libm there; the snap differs from it only
// where its own answer is arbitrary.  acos is taken of min(z, 1) (the reference prints a warning and goes on for z > 1).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/uvs_solver.h"
#include "uvs_frontend_dev.h"
#include "uvs_handle.h"

namespace uvsvp {

constexpr int kSamples = UVS_VP_N_SAMPLES;
constexpr int kRot = UVS_VP_N_ROTATIONS;
constexpr int kHyp = UVS_VP_N_HYPOTHESES;
constexpr int kLA = UVS_VP_GRID_LA, kLO = UVS_VP_GRID_LO, kCells = kLA * kLO;
constexpr int kMaxLines = UVS_VP_MAX_LINES;
constexpr int kMaxAttempts = 64;
constexpr int kPrepThreads = 256, kVoteThreads = 128, kSmoothThreads = 256, kScoreThreads = 384, kSelThreads = 256;
constexpr double kPi = 3.1415926535897932384626433832795;      // CV_PI
constexpr double kDeg = 1.0 / 180.0 * kPi;                     // angelAccuracy / oneDegree
constexpr double kTol60 = 60.0 / 180.0 * kPi;                  // angelTolerance
constexpr double kSnap = 1e-9;
constexpr double kTwo40 = 1099511627776.0;
static_assert(kSamples * kRot == kHyp, "hypotheses");
static_assert(kRot <= kScoreThreads, "one thread per rotation");
static_assert((long long)kMaxLines * (kMaxLines - 1) / 2 < (1ll << 19), "the hi limb holds 2^19 weights of 2^40");

struct VpFrame {                   // device copy of one uvs_vp_frame
    int n_lines, l_off;            // lines, offset of the first one in the concatenated arrays
    long long p_off;               // offset of the first pair in the debug pair-cell array
    unsigned long long seed;
};
struct VpCtl {                     // per frame, written by k_vp_prepare
    int status, pad;
    double scale, inv_scale;       // 2^e, 2^-e of the voting grid
};
struct VpBlockBest { double score; int idx, pad; double hyp[9]; };
struct VpCam { double fx, fy, cx, cy, th; };

// the cell rule of the header comment; q >= 0 for every caller, anything else (a NaN) goes to cell 0 so that no index leaves the grid
__device__ __forceinline__ int snap_cell(double angle, int n) {
    const double q = angle / kDeg;
    if (!(q >= 0.0)) return 0;
    const double r = rint(q);
    int c = fabs(q - r) <= kSnap ? (int)r : (int)q;
    return c >= n ? n - 1 : c;
}

__device__ __forceinline__ double limbs_to_double(const unsigned long long* g, int cell, double inv) {
    const long long hi = (long long)g[2 * cell], lo = (long long)g[2 * cell + 1];
    return (double)hi * inv + (double)lo * (inv * (1.0 / kTwo40));
}

// ---- line parameters, grid scale, sample pairs
__global__ void __launch_bounds__(kPrepThreads) k_vp_prepare(const VpFrame* __restrict__ frames, const double* __restrict__ seg,
                                                            double* __restrict__ lp, VpCtl* __restrict__ ctl, int* __restrict__ samples) {
    __shared__ double sPara[kMaxLines * 3];
    __shared__ double sMax[kPrepThreads];
    __shared__ int sFail;
    const int tid = threadIdx.x, f = blockIdx.x;
    const VpFrame F = frames[f];
    const int n = F.n_lines;
    if (tid == 0) sFail = 0;
    double mx = 0.0;
    for (int l = tid; l < n; l += kPrepThreads) {
        const double* s = seg + 4 * (size_t)(F.l_off + l);
        const double x1 = s[0], y1 = s[1], x2 = s[2], y2 = s[3];
        const double p0 = y1 - y2, p1 = x2 - x1, p2 = x1 * y2 - y1 * x2;      // (x1, y1, 1) x (x2, y2, 1)
        const double dx = x2 - x1, dy = y2 - y1;
        const double len = sqrt(dx * dx + dy * dy);
        double ori = atan2(dy, dx);
        if (ori < 0) ori += kPi;
        double* o = lp + 5 * (size_t)(F.l_off + l);
        o[0] = p0; o[1] = p1; o[2] = p2; o[3] = len; o[4] = ori;
        sPara[3 * l] = p0; sPara[3 * l + 1] = p1; sPara[3 * l + 2] = p2;
        mx = fmax(mx, len);
    }
    sMax[tid] = mx;
    __syncthreads();
    for (int off = kPrepThreads / 2; off > 0; off >>= 1) {
        if (tid < off) sMax[tid] = fmax(sMax[tid], sMax[tid + off]);
        __syncthreads();
    }
    if (n < 2) {
        if (tid == 0) { ctl[f].status = UVS_VP_TOO_FEW_LINES; ctl[f].scale = 1.0; ctl[f].inv_scale = 1.0; }
        return;
    }
    if (tid < kSamples) {
        const int s = tid;
        int a = -1, b = -1;
        for (int t = 0; t < kMaxAttempts; ++t) {
            const int ia = (int)(uvs_draw(F.seed, s, 2 * t) % (unsigned long long)n);
            const int ib = (int)(uvs_draw(F.seed, s, 2 * t + 1) % (unsigned long long)n);
            if (ia == ib) continue;
            const double z = sPara[3 * ia] * sPara[3 * ib + 1] - sPara[3 * ia + 1] * sPara[3 * ib];
            if (z == 0) continue;
            a = ia; b = ib;
            break;
        }
        if (a < 0) atomicOr(&sFail, 1);
        samples[2 * ((size_t)f * kSamples + s)] = a;
        samples[2 * ((size_t)f * kSamples + s) + 1] = b;
    }
    __syncthreads();
    if (tid == 0) {
        // 1.2 max(len) < 2^x  =>  every weight times 2^(40 - x) is below 2^40
        int x;
        (void)frexp(1.2 * sMax[0], &x);
        ctl[f].status = sFail ? UVS_VP_NO_HYPOTHESIS : UVS_VP_OK;
        ctl[f].scale = ldexp(1.0, 40 - x);
        ctl[f].inv_scale = ldexp(1.0, x - 40);
    }
}

// ---- voting: thread per pair, two integer atomics per kept pair
__global__ void __launch_bounds__(kVoteThreads) k_vp_vote(const VpFrame* __restrict__ frames, const VpCtl* __restrict__ ctl,
                                                         const double* __restrict__ lp, VpCam cam, unsigned long long* __restrict__ limbs,
                                                         int32_t* __restrict__ dbg_pair_cell) {
    const int f = blockIdx.x;
    if (ctl[f].status != UVS_VP_OK) return;
    const VpFrame F = frames[f];
    const int n = F.n_lines;
    const double scale = ctl[f].scale;
    unsigned long long* g = limbs + 2 * (size_t)kCells * f;
    const double* L = lp + 5 * (size_t)F.l_off;
    for (int i = blockIdx.y; i < n - 1; i += gridDim.y) {
        const double a0 = L[5 * i], a1 = L[5 * i + 1], a2 = L[5 * i + 2], alen = L[5 * i + 3], aori = L[5 * i + 4];
        for (int j = i + 1 + threadIdx.x; j < n; j += kVoteThreads) {
            const double b0 = L[5 * j], b1 = L[5 * j + 1], b2 = L[5 * j + 2], blen = L[5 * j + 3], bori = L[5 * j + 4];
            const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
            int cell = -1;
            if (c2 != 0) {
                const double X = c0 / c2 - cam.cx, Y = c1 / c2 - cam.cy, Z = cam.fx;
                const double N = sqrt(X * X + Y * Y + Z * Z);
                const int la = snap_cell(acos(fmin(Z / N, 1.0)), kLA);
                const int lo = snap_cell(atan2(X, Y) + kPi, kLO);
                double dev = fabs(aori - bori);
                dev = fmin(kPi - dev, dev);
                if (!(dev > kTol60)) {
                    cell = la * kLO + lo;
                    const double w = sqrt(alen * blen) * (sin(2.0 * dev) + 0.2);
                    const double ws = w * scale;
                    const double hi = rint(ws);
                    const double lo40 = rint((ws - hi) * kTwo40);
                    if (hi >= 0.0 && hi <= kTwo40) {      // always, by the choice of the scale (a NaN weight adds nothing)
                        atomicAdd(&g[2 * cell], (unsigned long long)(long long)hi);
                        atomicAdd(&g[2 * cell + 1], (unsigned long long)(long long)lo40);
                    }
                }
            }
            if (dbg_pair_cell) dbg_pair_cell[F.p_off + (long long)i * n - (long long)i * (i + 1) / 2 + (j - i - 1)] = cell;
        }
    }
}

// ---- smoothing (:2151-2173)
__global__ void __launch_bounds__(kSmoothThreads) k_vp_smooth(const VpCtl* __restrict__ ctl, const unsigned long long* __restrict__ limbs,
                                                             double* __restrict__ smooth, double* __restrict__ dbg_raw) {
    const int f = blockIdx.x;
    if (ctl[f].status != UVS_VP_OK) return;
    const int cell = blockIdx.y * kSmoothThreads + threadIdx.x;
    if (cell >= kCells) return;
    const double inv = ctl[f].inv_scale;
    const unsigned long long* g = limbs + 2 * (size_t)kCells * f;
    const int i = cell / kLO, j = cell % kLO;
    const double own = limbs_to_double(g, cell, inv);
    double out = 0.0;
    if (i >= 1 && i < kLA - 1 && j >= 1 && j < kLO - 1) {
        double total = 0.0;
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int k = 0; k < 3; ++k) total += limbs_to_double(g, (i - 1 + m) * kLO + (j - 1 + k), inv);
        out = own + total / 9;
    }
    smooth[(size_t)kCells * f + cell] = out;
    if (dbg_raw) dbg_raw[(size_t)kCells * f + cell] = own;
}

// ---- hypotheses and their scores: workgroup per (frame, sample), thread per rotation
__global__ void __launch_bounds__(kScoreThreads) k_vp_score(const VpFrame* __restrict__ frames, const VpCtl* __restrict__ ctl,
                                                           const double* __restrict__ lp, const int* __restrict__ samples, VpCam cam,
                                                           const double* __restrict__ smooth, VpBlockBest* __restrict__ best,
                                                           double* __restrict__ dbg_hyp, int32_t* __restrict__ dbg_cells,
                                                           double* __restrict__ dbg_score) {
    __shared__ double sScore[kScoreThreads];
    __shared__ int sIdx[kScoreThreads];
    const int f = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    if (ctl[f].status != UVS_VP_OK) return;
    const VpFrame F = frames[f];
    const double* L = lp + 5 * (size_t)F.l_off;
    const int ia = samples[2 * ((size_t)f * kSamples + s)], ib = samples[2 * ((size_t)f * kSamples + s) + 1];
    const double* g = smooth + (size_t)kCells * f;
    double h0 = 0, h1 = 0, h2 = 0, h3 = 0, h4 = 0, h5 = 0, h6 = 0, h7 = 0, h8 = 0, score = -1.0;
    if (tid < kRot) {
        // vp1 (:2024-2036)
        const double a0 = L[5 * ia], a1 = L[5 * ia + 1], a2 = L[5 * ia + 2], b0 = L[5 * ib], b1 = L[5 * ib + 1], b2 = L[5 * ib + 2];
        const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
        h0 = c0 / c2 - cam.cx; h1 = c1 / c2 - cam.cy; h2 = cam.fx;
        if (h2 == 0) h2 = 0.0011;
        double N = sqrt(h0 * h0 + h1 * h1 + h2 * h2);
        double rN = 1.0 / N;
        h0 *= rN; h1 *= rN; h2 *= rN;
        // vp2 (:2046-2060)
        const double lambda = tid * (2.0 * kPi / kRot);
        const double sl = sin(lambda), cl = cos(lambda);
        const double k1 = h0 * sl + h1 * cl, k2 = h2;
        const double phi = atan(-k2 / k1);
        const double sp = sin(phi);
        h5 = cos(phi); h3 = sp * sl; h4 = sp * cl;
        if (h5 == 0.0) h5 = 0.0011;
        N = sqrt(h3 * h3 + h4 * h4 + h5 * h5); rN = 1.0 / N;
        h3 *= rN; h4 *= rN; h5 *= rN;
        if (h5 < 0) { h3 *= -1.0; h4 *= -1.0; h5 *= -1.0; }
        // vp3 = vp1 x vp2 (:2063-2067)
        h6 = h1 * h5 - h2 * h4; h7 = h2 * h3 - h0 * h5; h8 = h0 * h4 - h1 * h3;
        if (h8 == 0.0) h8 = 0.0011;
        N = sqrt(h6 * h6 + h7 * h7 + h8 * h8); rN = 1.0 / N;
        h6 *= rN; h7 *= rN; h8 *= rN;
        if (h8 < 0) { h6 *= -1.0; h7 *= -1.0; h8 *= -1.0; }
        // cells and score (:2183-2214); a vanishing point with z == 0 is skipped there
        int c_0 = -1, c_1 = -1, c_2 = -1;
        score = 0.0;
        if (h2 != 0.0) { c_0 = snap_cell(acos(fmin(h2, 1.0)), kLA) * kLO + snap_cell(atan2(h0, h1) + kPi, kLO); score += g[c_0]; }
        if (h5 != 0.0) { c_1 = snap_cell(acos(fmin(h5, 1.0)), kLA) * kLO + snap_cell(atan2(h3, h4) + kPi, kLO); score += g[c_1]; }
        if (h8 != 0.0) { c_2 = snap_cell(acos(fmin(h8, 1.0)), kLA) * kLO + snap_cell(atan2(h6, h7) + kPi, kLO); score += g[c_2]; }
        if (dbg_hyp) {
            const size_t h = (size_t)s * kRot + tid;
            double* o = dbg_hyp + 9 * h;
            o[0] = h0; o[1] = h1; o[2] = h2; o[3] = h3; o[4] = h4; o[5] = h5; o[6] = h6; o[7] = h7; o[8] = h8;
            dbg_cells[3 * h] = c_0; dbg_cells[3 * h + 1] = c_1; dbg_cells[3 * h + 2] = c_2;
            dbg_score[h] = score;
        }
    }
    // a NaN score (it cannot come from a finite grid) never wins
    sScore[tid] = score == score ? score : -1.0; sIdx[tid] = tid;
    __syncthreads();
    for (int off = 256; off > 0; off >>= 1) {
        if (tid < off && tid + off < kScoreThreads) {
            const double o = sScore[tid + off]; const int oi = sIdx[tid + off];
            if (o > sScore[tid] || (o == sScore[tid] && oi < sIdx[tid])) { sScore[tid] = o; sIdx[tid] = oi; }
        }
        __syncthreads();
    }
    if (tid == sIdx[0]) {
        VpBlockBest* b = best + (size_t)f * kSamples + s;
        b->score = sScore[0]; b->idx = s * kRot + tid; b->pad = 0;
        b->hyp[0] = h0; b->hyp[1] = h1; b->hyp[2] = h2; b->hyp[3] = h3; b->hyp[4] = h4; b->hyp[5] = h5; b->hyp[6] = h6; b->hyp[7] = h7; b->hyp[8] = h8;
    }
}

// ---- selection (:2216-2228), lines2Vps (:2232-2299), the per-line vector (:379-385)
__global__ void __launch_bounds__(kSelThreads) k_vp_select(const VpFrame* __restrict__ frames, const VpCtl* __restrict__ ctl,
                                                          const double* __restrict__ seg, const VpBlockBest* __restrict__ best, VpCam cam,
                                                          uvs_vp_result* __restrict__ results, int32_t* __restrict__ tag,
                                                          double* __restrict__ line_vp) {
    __shared__ double sV[9];
    __shared__ int sCount[3];
    const int f = blockIdx.x, tid = threadIdx.x;
    const VpFrame F = frames[f];
    const int n = F.n_lines, status = ctl[f].status;
    uvs_vp_result* res = results + f;
    if (status != UVS_VP_OK) {
        for (int l = tid; l < n; l += kSelThreads) {
            tag[F.l_off + l] = 3;
            for (int k = 0; k < 3; ++k) line_vp[3 * (size_t)(F.l_off + l) + k] = 0.0;
        }
        if (tid == 0) {
            res->status = status; res->best_hypothesis = -1; res->score = 0.0; res->reserved = 0;
            for (int k = 0; k < 9; ++k) res->vps[k / 3][k % 3] = 0.0;
            for (int k = 0; k < 3; ++k) res->n_tagged[k] = 0;
        }
        return;
    }
    if (tid == 0) {
        const VpBlockBest* b = best + (size_t)f * kSamples;
        int bs = 0; double mx = b[0].score;       // block 0's best is hypothesis 0 when every score is 0
        for (int s = 1; s < kSamples; ++s) if (b[s].score > mx) { mx = b[s].score; bs = s; }
        for (int k = 0; k < 9; ++k) { sV[k] = b[bs].hyp[k]; res->vps[k / 3][k % 3] = b[bs].hyp[k]; }
        res->status = UVS_VP_OK; res->best_hypothesis = b[bs].idx; res->score = mx; res->reserved = 0;
        sCount[0] = sCount[1] = sCount[2] = 0;
    }
    __syncthreads();
    const double v0x = sV[0], v0y = sV[1], v0z = sV[2], v1x = sV[3], v1y = sV[4], v1z = sV[5], v2x = sV[6], v2y = sV[7], v2z = sV[8];
    const double px[3] = {v0x * cam.fx / v0z + cam.cx, v1x * cam.fx / v1z + cam.cx, v2x * cam.fx / v2z + cam.cx};
    const double py[3] = {v0y * cam.fy / v0z + cam.cy, v1y * cam.fy / v1z + cam.cy, v2y * cam.fy / v2z + cam.cy};
    for (int l = tid; l < n; l += kSelThreads) {
        const double* s = seg + 4 * (size_t)(F.l_off + l);
        const double x1 = s[0], y1 = s[1], x2 = s[2], y2 = s[3];
        const double xm = (x1 + x2) / 2.0, ym = (y1 + y2) / 2.0;
        double ax = x1 - x2, ay = y1 - y2;
        const double N1 = sqrt(ax * ax + ay * ay);
        ax /= N1; ay /= N1;
        double minAngle = 1000.0;
        int bi = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double bx = px[j] - xm, by = py[j] - ym;
            const double N2 = sqrt(bx * bx + by * by);
            bx /= N2; by /= N2;
            double cv = ax * bx + ay * by;
            if (cv > 1.0) cv = 1.0;
            if (cv < -1.0) cv = -1.0;
            double angle = acos(cv);
            angle = (angle < kPi - angle) ? angle : kPi - angle;      // std::min(CV_PI - angle, angle)
            if (angle < minAngle) { minAngle = angle; bi = j; }
        }
        const int t = minAngle < cam.th ? bi : 3;
        tag[F.l_off + l] = t;
        double ox = 0.0, oy = 0.0, oz = 0.0;
        if (t == 0) { ox = v0x / v0z; oy = v0y / v0z; oz = v0z / v0z; }
        else if (t == 1) { ox = v1x / v1z; oy = v1y / v1z; oz = v1z / v1z; }
        else if (t == 2) { ox = v2x / v2z; oy = v2y / v2z; oz = v2z / v2z; }
        double* o = line_vp + 3 * (size_t)(F.l_off + l);
        o[0] = ox; o[1] = oy; o[2] = oz;
        if (t < 3) atomicAdd(&sCount[t], 1);
    }
    __syncthreads();
    if (tid < 3) res->n_tagged[tid] = sCount[tid];
}

}  // namespace uvsvp

using namespace uvsvp;

struct uvs_vp_estimator : UvsHandle {
    int max_frames = 0, max_lines = 0;
    float device_ms = 0.f;                      // uvs_vp_last_device_ms
    size_t in_bytes = 0, out_bytes = 0;
    DevBuf<char> d_in, d_out;                   // packed inputs (frames | segments) / outputs (results | tags | line_vp) of one call
    PinnedBuf<char> h_in, h_out;                // pinned staging
    DevBuf<double> d_lp, d_smooth;              // line parameters [lines][5]; smoothed grids [frames][90 x 360]
    DevBuf<VpCtl> d_ctl;
    DevBuf<int> d_samples;                      // [frames][105][2]
    DevBuf<unsigned long long> d_limbs;         // voting grids, two integers per cell
    DevBuf<VpBlockBest> d_best;                 // [frames][105]
    DevBuf<char> d_dbg;                         // uvs_vp_debug_frame only (allocated by its first call)
};

namespace {

inline size_t align8(size_t b) { return (b + 7) & ~size_t(7); }

struct VpDebug { double* hyp; int32_t* cells; double* score; double* raw; double* smooth; int32_t* pair_cell; };

int vp_run(uvs_vp_estimator* h, const char* who_, int n_frames, const uvs_vp_frame* frames, const uvs_vp_camera* camera, double th_angle,
           int32_t* tag, double* line_vp, uvs_vp_result* results, const VpDebug* dbg) {
    const std::string fn = who_;
    h->err.clear();
    if (n_frames < 1 || !frames || !camera || !tag || !line_vp || !results) { h->err = fn + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG; }
    if (n_frames > h->max_frames) { h->err = fn + ": more frames than the capacity given to uvs_vp_create"; return UVS_ERR_CAPACITY; }
    if (!(camera->fx > 0.0) || !(camera->fy > 0.0) || !std::isfinite(camera->fx) || !std::isfinite(camera->fy) || !std::isfinite(camera->cx) ||
        !std::isfinite(camera->cy)) { h->err = fn + ": fx and fy must be positive, the camera finite"; return UVS_ERR_INVALID_ARG; }
    if (!(th_angle > 0.0) || !std::isfinite(th_angle)) { h->err = fn + ": th_angle must be positive"; return UVS_ERR_INVALID_ARG; }
    size_t tl = 0; int max_n = 0;
    for (int f = 0; f < n_frames; ++f) {
        const uvs_vp_frame& fr = frames[f];
        const std::string who = fn + ": frame " + std::to_string(f);
        if (fr.n_lines < 0 || (fr.n_lines > 0 && !fr.segments)) { h->err = who + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG; }
        if (fr.n_lines > h->max_lines) { h->err = who + " exceeds the capacity given to uvs_vp_create"; return UVS_ERR_CAPACITY; }
        for (int l = 0; l < fr.n_lines; ++l) {
            const double* s = fr.segments + 4 * (size_t)l;
            for (int k = 0; k < 4; ++k)
                if (!std::isfinite(s[k]) || std::fabs(s[k]) > UVS_VP_MAX_COORD) { h->err = who + ": a coordinate is not finite or beyond UVS_VP_MAX_COORD"; return UVS_ERR_INVALID_ARG; }
            if (s[0] == s[2] && s[1] == s[3]) { h->err = who + ": zero-length segment"; return UVS_ERR_INVALID_ARG; }
        }
        tl += fr.n_lines; max_n = std::max(max_n, fr.n_lines);
    }
    // packed input: frames | segments
    const size_t o_seg = align8(n_frames * sizeof(VpFrame)), in_used = o_seg + tl * 32;
    VpFrame* hf = reinterpret_cast<VpFrame*>(h->h_in.get());
    size_t lo = 0; long long po = 0;
    for (int f = 0; f < n_frames; ++f) {
        VpFrame d;
        d.n_lines = frames[f].n_lines; d.l_off = (int)lo; d.p_off = po; d.seed = frames[f].seed;
        hf[f] = d;
        if (d.n_lines) std::memcpy(h->h_in + o_seg + lo * 32, frames[f].segments, (size_t)d.n_lines * 32);
        lo += d.n_lines; po += (long long)d.n_lines * (d.n_lines - 1) / 2;
    }
    const size_t o_tag = align8(n_frames * sizeof(uvs_vp_result)), o_lvp = o_tag + align8(tl * 4), out_used = o_lvp + tl * 24;
    const VpFrame* dF = reinterpret_cast<const VpFrame*>(h->d_in.get());
    const double* dSeg = reinterpret_cast<const double*>(h->d_in + o_seg);
    uvs_vp_result* dRes = reinterpret_cast<uvs_vp_result*>(h->d_out.get());
    int32_t* dTag = reinterpret_cast<int32_t*>(h->d_out + o_tag);
    double* dLvp = reinterpret_cast<double*>(h->d_out + o_lvp);
    const VpCam cam{camera->fx, camera->fy, camera->cx, camera->cy, th_angle};
    const VpDebug none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const VpDebug& D = dbg ? *dbg : none;
    hipStream_t st = h->st;
    UVS_HIP(h->err, hipSetDevice(h->device));
    UVS_HIP(h->err, hipEventRecord(h->ev0, st));
    UVS_HIP(h->err, hipMemcpyAsync(h->d_in, h->h_in, in_used, hipMemcpyHostToDevice, st));
    UVS_HIP(h->err, hipMemsetAsync(h->d_limbs, 0, (size_t)n_frames * kCells * 16, st));
    k_vp_prepare<<<n_frames, kPrepThreads, 0, st>>>(dF, dSeg, h->d_lp, h->d_ctl, h->d_samples);
    k_vp_vote<<<dim3(n_frames, std::max(1, max_n - 1)), kVoteThreads, 0, st>>>(dF, h->d_ctl, h->d_lp, cam, h->d_limbs, D.pair_cell);
    k_vp_smooth<<<dim3(n_frames, (kCells + kSmoothThreads - 1) / kSmoothThreads), kSmoothThreads, 0, st>>>(h->d_ctl, h->d_limbs, h->d_smooth, D.raw);
    k_vp_score<<<dim3(n_frames, kSamples), kScoreThreads, 0, st>>>(dF, h->d_ctl, h->d_lp, h->d_samples, cam, h->d_smooth, h->d_best, D.hyp, D.cells, D.score);
    k_vp_select<<<n_frames, kSelThreads, 0, st>>>(dF, h->d_ctl, dSeg, h->d_best, cam, dRes, dTag, dLvp);
    UVS_HIP(h->err, hipGetLastError());
    UVS_HIP(h->err, hipMemcpyAsync(h->h_out, h->d_out, out_used, hipMemcpyDeviceToHost, st));
    UVS_HIP(h->err, hipEventRecord(h->ev1, st));
    UVS_HIP(h->err, hipStreamSynchronize(st));
    UVS_HIP(h->err, hipEventElapsedTime(&h->device_ms, h->ev0, h->ev1));
    std::memcpy(results, h->h_out, n_frames * sizeof(uvs_vp_result));
    if (tl) {
        std::memcpy(tag, h->h_out + o_tag, tl * 4);
        std::memcpy(line_vp, h->h_out + o_lvp, tl * 24);
    }
    return UVS_OK;
}

}  // namespace

extern "C" {

int uvs_vp_create(int device, int max_frames, int max_lines, uvs_vp_estimator** out) {
    if (!out || max_frames < 1 || max_lines < 1) return UVS_ERR_INVALID_ARG;
    *out = nullptr;
    if (max_frames > UVS_VP_MAX_FRAMES || max_lines > UVS_VP_MAX_LINES) return UVS_ERR_CAPACITY;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return UVS_ERR_NO_DEVICE;
    uvs_vp_estimator* h = new uvs_vp_estimator();
    h->max_frames = max_frames; h->max_lines = max_lines;
    const size_t B = max_frames, Lt = B * max_lines;
    h->in_bytes = align8(B * sizeof(VpFrame)) + Lt * 32;
    h->out_bytes = align8(B * sizeof(uvs_vp_result)) + align8(Lt * 4) + Lt * 24;
    int rc = h->open(device);
    if (rc == UVS_OK && (rc = h->d_in.ensure(h->in_bytes, h->err)) == UVS_OK && (rc = h->d_out.ensure(h->out_bytes, h->err)) == UVS_OK &&
        (rc = h->h_in.ensure(h->in_bytes, h->err)) == UVS_OK && (rc = h->h_out.ensure(h->out_bytes, h->err)) == UVS_OK &&
        (rc = h->d_lp.ensure(Lt * 40, h->err)) == UVS_OK && (rc = h->d_smooth.ensure(B * kCells * 8, h->err)) == UVS_OK &&
        (rc = h->d_ctl.ensure(B * sizeof(VpCtl), h->err)) == UVS_OK && (rc = h->d_samples.ensure(B * kSamples * 8, h->err)) == UVS_OK &&
        (rc = h->d_limbs.ensure(B * kCells * 16, h->err)) == UVS_OK) rc = h->d_best.ensure(B * kSamples * sizeof(VpBlockBest), h->err);
    if (rc != UVS_OK) { uvs_vp_destroy(h); return rc; }
    *out = h;
    return UVS_OK;
}

void uvs_vp_destroy(uvs_vp_estimator* h) { if (h) { h->close(); delete h; } }

const char* uvs_vp_last_error(const uvs_vp_estimator* h) { return h ? h->err.c_str() : "null vanishing-point estimator"; }

double uvs_vp_last_device_ms(const uvs_vp_estimator* h) { return h ? (double)h->device_ms : 0.0; }

int uvs_vp_estimate(uvs_vp_estimator* h, int n_frames, const uvs_vp_frame* frames, const uvs_vp_camera* camera, double th_angle,
                    int32_t* tag, double* line_vp, uvs_vp_result* results) {
    if (!h) return UVS_ERR_INVALID_ARG;
    return vp_run(h, "uvs_vp_estimate", n_frames, frames, camera, th_angle, tag, line_vp, results, nullptr);
}

int uvs_vp_debug_frame(uvs_vp_estimator* h, const uvs_vp_frame* frame, const uvs_vp_camera* camera, double th_angle, double* hyp,
                       int32_t* cells, double* scores, double* grid_raw, double* grid_smooth, int32_t* pair_cell, uvs_vp_result* result) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    if (!frame || !hyp || !cells || !scores || !grid_raw || !grid_smooth || !pair_cell || !result) {
        h->err = "uvs_vp_debug_frame: null pointer"; return UVS_ERR_INVALID_ARG;
    }
    if (frame->n_lines > h->max_lines) { h->err = "uvs_vp_debug_frame: the frame exceeds the capacity given to uvs_vp_create"; return UVS_ERR_CAPACITY; }
    const size_t n = frame->n_lines > 0 ? (size_t)frame->n_lines : 0, np = n * (n > 0 ? n - 1 : 0) / 2;
    // debug block: hyp | scores | raw | cells | pair cells
    const size_t o_sc = (size_t)kHyp * 72, o_raw = o_sc + (size_t)kHyp * 8, o_cells = o_raw + (size_t)kCells * 8, o_pc = o_cells + align8((size_t)kHyp * 12),
                 total = o_pc + align8(np * 4);
    int rc = h->d_dbg.ensure(total, h->err, grow_half);
    if (rc != UVS_OK) return rc;
    UVS_HIP(h->err, hipSetDevice(h->device));
    UVS_HIP(h->err, hipMemsetAsync(h->d_dbg, 0, total, h->st));
    UVS_HIP(h->err, hipMemsetAsync(h->d_smooth, 0, (size_t)kCells * 8, h->st));
    const VpDebug D{reinterpret_cast<double*>(h->d_dbg.get()), reinterpret_cast<int32_t*>(h->d_dbg + o_cells), reinterpret_cast<double*>(h->d_dbg + o_sc),
                    reinterpret_cast<double*>(h->d_dbg + o_raw), nullptr, reinterpret_cast<int32_t*>(h->d_dbg + o_pc)};
    std::vector<int32_t> tag(n + 1); std::vector<double> lvp(3 * n + 3);
    rc = vp_run(h, "uvs_vp_debug_frame", 1, frame, camera, th_angle, tag.data(), lvp.data(), result, &D);
    if (rc != UVS_OK) return rc;
    UVS_HIP(h->err, hipMemcpy(hyp, h->d_dbg, (size_t)kHyp * 72, hipMemcpyDeviceToHost));
    UVS_HIP(h->err, hipMemcpy(scores, h->d_dbg + o_sc, (size_t)kHyp * 8, hipMemcpyDeviceToHost));
    UVS_HIP(h->err, hipMemcpy(grid_raw, h->d_dbg + o_raw, (size_t)kCells * 8, hipMemcpyDeviceToHost));
    UVS_HIP(h->err, hipMemcpy(cells, h->d_dbg + o_cells, (size_t)kHyp * 12, hipMemcpyDeviceToHost));
    if (np) UVS_HIP(h->err, hipMemcpy(pair_cell, h->d_dbg + o_pc, np * 4, hipMemcpyDeviceToHost));
    UVS_HIP(h->err, hipMemcpy(grid_smooth, h->d_smooth, (size_t)kCells * 8, hipMemcpyDeviceToHost));
    return UVS_OK;
}

}  // extern "C"
