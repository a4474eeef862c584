// uvs_loop_verify.hip -- loop verification of loop closure (reference pose_graph/src/keyframe.cpp:259-521, KeyFrame::findConnection with the
// F-matrix RANSAC commented out) behind the uvs_lc_* calls of include/uvs_solver.h.  FP64 geometry, gfx950, one stream per handle.
//
// One call verifies a batch of B candidate pairs (current keyframe, old keyframe); k_lc_verify runs one 256-thread workgroup per pair, so a
// pair gives the same bits alone or in a batch.  Phases of the workgroup (barriers between them):
//   match    thread per query (up to 4 each): the old descriptors pass through LDS in tiles of kTile keypoints; XOR + popcount over the
//            four 64-bit words, bestDist from 128 on a strict <, so ties keep the first index (searchInAera, keyframe.cpp:121-151);
//            kept when bestDist < 80.
//   compact  ordered prefix sum over the match flags (4 contiguous queries per thread): match m is the m-th matched query in query order;
//            its 3-D point and the old keypoint's normalized uv are staged in LDS.
//   gate 1   matches > MIN_LOOP_NUM (25).
//   hyps     thread h < 100: 5 distinct match indices from the counter-based generator, a 6-DoF LM on them from the VIO prior (the
//            camera pose of origin_vio through the extrinsic, PnPRANSAC :213-219), then the inlier count over every match.
//   select   thread 0 replays OpenCV's sequential adaptive rule over the 100 counts (RANSACPointSetRegistrator::run).
//   mask     the chosen hypothesis's inlier mask; the refinement LM on those inliers from its pose, normal equations reduced in a fixed
//            order (lane-ordered partials, a shuffle tree per wave, the 4 wave sums in wave order).
//   finish   thread 0: body pose PnP_R_old / PnP_T_old (:244-255), loop_info (:472-487), gates 2 and 3.
//
// Numerics (restated in tests/lc_ref.py, which is the pin: OpenCV is not a dependency):
//   generator  z = mix64(seed + 0x9E3779B97F4A7C15 * (1 + (h << 20) + a)) mod 2^64, mix64 = the splitmix64 finalizer; draw a = 0, 1, ..
//              gives the match index z % n; a duplicate of an earlier draw of the same hypothesis is skipped; 5 distinct within 64 draws
//              or the hypothesis is invalid (count -1).
//   LM         residual (x / z, y / z) - uv of p = R X + t; analytic Jacobian; left perturbation R <- Exp(dtheta) R, t <- t + dt;
//              (J^T J + lambda diag(J^T J)) delta = -J^T r by a 6 x 6 Cholesky; lambda0 = 1e-3, / 10 when the step lowers the cost
//              (strict <, the step is taken), x 10 otherwise; at most 20 iterations (CvLevMarq's count in solvePnP); stops after a step with
//              |delta| < FLT_EPSILON max(1, |t|).  A pivot that is not > 0 and finite makes a hypothesis invalid (the refinement stops and
//              keeps its pose); so does a non-finite initial cost.
//   inlier     z > 0 and dx^2 + dy^2 <= (10 / 460)^2, evaluated without FMA contraction so the count and the mask agree bit for bit.
//   selection  h >= niters ends the loop; count > max(best, 4) makes h the best and niters = RANSACUpdateNumIters(0.99, (n - count) / n,
//              5, niters).  The reported inlier set is the chosen hypothesis's mask, not recomputed after the refinement (as OpenCV).
//
// uvs_lc_debug_pair (tests only) runs one pair through k_lc_verify<true>, the same body with stores of every intermediate value of the PnP
// (samples, the normal equations, steps, candidates, costs and decisions of every LM iteration, the staged matches) into a trace buffer;
// tests/lc_hp.py checks that trace against a 60-digit reference stage by stage.  k_lc_verify<false> is what uvs_lc_verify launches.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/uvs_solver.h"
#include "uvs_frontend_dev.h"
#include "uvs_handle.h"

namespace uvslc {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 256;                  // old descriptors per LDS tile (8 KiB)
constexpr int kMaxQ = UVS_LC_MAX_QUERY;     // LDS staging is sized for the largest handle
constexpr int kQPerThread = kMaxQ / kThreads;
constexpr int kHyp = UVS_LC_N_HYPOTHESES;
constexpr int kModel = 5;                   // OpenCV's model_points for SOLVEPNP_ITERATIVE
constexpr int kMaxAttempts = 64;
constexpr int kLmIters = 20;
constexpr int kMinLoop = 25;                // MIN_LOOP_NUM, keyframe.h:16
constexpr double kThresh = 10.0 / 460.0;
constexpr double kThresh2 = kThresh * kThresh;
constexpr double kLambda0 = 1e-3;
constexpr double kConfidence = 0.99;
constexpr int kRed = 28;                    // packed upper J^T J (21), J^T r (6), cost
static_assert(kMaxQ % kThreads == 0, "queries per thread");

struct LcPair {                             // device copy of one uvs_lc_pair
    int n_query, n_old, q_off, o_off;
    unsigned long long seed;
    double vio_t[3], vio_q[4];
};

// Eigen's Quaternion::toRotationMatrix, q = (x, y, z, w), row-major
__device__ inline void quat_to_R(const double* q, double* R) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}

// Eigen's Quaternion(Matrix3d) (no sign normalization) -> (w, x, y, z); the three branches of its largest-diagonal case written out, so the
// matrix stays in registers (a run-time index would put it in scratch)
__device__ inline void R_to_quat_wxyz(const double* m, double* q) {
    double t = m[0] + m[4] + m[8], w, x, y, z;
    if (t > 0) {
        t = sqrt(t + 1.0); w = 0.5 * t; t = 0.5 / t;
        x = (m[7] - m[5]) * t; y = (m[2] - m[6]) * t; z = (m[3] - m[1]) * t;
    } else if (m[8] > fmax(m[0], m[4])) {     // i = 2 (j = 0, k = 1)
        t = sqrt(m[8] - m[0] - m[4] + 1.0); z = 0.5 * t; t = 0.5 / t;
        w = (m[3] - m[1]) * t; x = (m[2] + m[6]) * t; y = (m[5] + m[7]) * t;
    } else if (m[4] > m[0]) {                 // i = 1 (j = 2, k = 0)
        t = sqrt(m[4] - m[8] - m[0] + 1.0); y = 0.5 * t; t = 0.5 / t;
        w = (m[2] - m[6]) * t; z = (m[7] + m[5]) * t; x = (m[1] + m[3]) * t;
    } else {                                  // i = 0 (j = 1, k = 2)
        t = sqrt(m[0] - m[4] - m[8] + 1.0); x = 0.5 * t; t = 0.5 / t;
        w = (m[7] - m[5]) * t; y = (m[3] + m[1]) * t; z = (m[6] + m[2]) * t;
    }
    q[0] = w; q[1] = x; q[2] = y; q[3] = z;
}

__device__ inline double yaw_deg(const double* R) { return atan2(R[3], R[0]) / M_PI * 180.0; }   // Utility::R2ypr().x()

__device__ inline double normalize_angle(double a) {     // Utility::normalizeAngle of the pose_graph package (floor form)
    return a > 0 ? a - 360.0 * floor((a + 180.0) / 360.0) : a + 360.0 * floor((-a + 180.0) / 360.0);
}

__device__ inline void matmul3(const double* A, const double* B, double* C) {         // C = A B
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
__device__ inline void matmul3_tn(const double* A, const double* B, double* C) {      // C = A^T B
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
__device__ inline void matmul3_nt(const double* A, const double* B, double* C) {      // C = A B^T
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1] + A[3 * i + 2] * B[3 * j + 2];
}

// Adds one point's residual, J^T J (packed upper, row by row), J^T r and r^T r at (R, t).
__device__ __forceinline__ void accum_point(const double* R, const double* t, const double* X, const double* uv, double* acc) {
    const double a0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2];
    const double a1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2];
    const double a2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2];
    const double x = a0 + t[0], y = a1 + t[1], z = a2 + t[2];
    const double iz = 1.0 / z;
    const double r0 = x * iz - uv[0], r1 = y * iz - uv[1];
    const double dxz = -x * iz * iz, dyz = -y * iz * iz;
    // d p / d dtheta = -[R X]x; rows of d(u, v)/dp = (iz, 0, dxz), (0, iz, dyz)
    double J0[6], J1[6];
    J0[0] = dxz * a1;              J0[1] = iz * a2 - dxz * a0;    J0[2] = -iz * a1;
    J1[0] = dyz * a1 - iz * a2;    J1[1] = -dyz * a0;             J1[2] = iz * a0;
    J0[3] = iz; J0[4] = 0.0; J0[5] = dxz;
    J1[3] = 0.0; J1[4] = iz; J1[5] = dyz;
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) acc[k++] += J0[i] * J0[j] + J1[i] * J1[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += J0[i] * r0 + J1[i] * r1;
    acc[27] += r0 * r0 + r1 * r1;
}

__device__ __forceinline__ double point_cost(const double* R, const double* t, const double* X, const double* uv) {
    const double x = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
    const double y = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
    const double z = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
    const double r0 = x / z - uv[0], r1 = y / z - uv[1];
    return r0 * r0 + r1 * r1;
}

__device__ __forceinline__ bool is_inlier(const double* R, const double* t, const double* X, const double* uv) {
#pragma clang fp contract(off)
    const double x = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
    const double y = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
    const double z = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
    const double dx = x / z - uv[0], dy = y / z - uv[1];
    return z > 0.0 && dx * dx + dy * dy <= kThresh2;
}

// (A + lambda diag(A)) d = -g, A packed upper (row by row).  false: a pivot not > 0 or not finite.
__device__ __forceinline__ bool chol_solve6(const double* acc, double lam, double* d) {
    double L[21];                     // packed lower, row by row: L(i, j) at i (i + 1) / 2 + j
    auto up = [](int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); };    // packed upper index of (i <= j)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = acc[up(j, j)] * (1.0 + lam);
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
        if (!(s > 0.0) || !isfinite(s)) return false;
        const double dj = sqrt(s);
        L[j * (j + 1) / 2 + j] = dj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = acc[up(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            L[i * (i + 1) / 2 + j] = v / dj;
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = -acc[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[i * (i + 1) / 2 + k] * y[k];
        y[i] = v / L[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v -= L[k * (k + 1) / 2 + i] * d[k];
        d[i] = v / L[i * (i + 1) / 2 + i];
    }
    return true;
}

// Rc = Exp(d[0..2]) R, tc = t + d[3..5]
__device__ __forceinline__ void apply_step(const double* R, const double* t, const double* d, double* Rc, double* tc) {
    const double w0 = d[0], w1 = d[1], w2 = d[2];
    const double th2 = w0 * w0 + w1 * w1 + w2 * w2;
    double A, B;
    if (th2 < 1e-20) { A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; }
    else { const double th = sqrt(th2); A = sin(th) / th; B = (1.0 - cos(th)) / th2; }
    const double K[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
    double K2[9], E[9];
    matmul3(K, K, K2);
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = (i % 4 == 0 ? 1.0 : 0.0) + A * K[i] + B * K2[i];
    matmul3(E, R, Rc);
    tc[0] = t[0] + d[3]; tc[1] = t[1] + d[4]; tc[2] = t[2] + d[5];
}

__device__ __forceinline__ bool step_small(const double* d, const double* t) {
    const double dn = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
    const double tn = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    return dn < (double)FLT_EPSILON * fmax(1.0, tn);
}

// OpenCV RANSACUpdateNumIters; cvRound = round half to even (rint)
__device__ inline int update_num_iters(double p, double ep, int model_points, int max_iters) {
    p = fmin(fmax(p, 0.0), 1.0); ep = fmin(fmax(ep, 0.0), 1.0);
    double num = fmax(1.0 - p, DBL_MIN);
    double denom = 1.0 - pow(1.0 - ep, (double)model_points);
    if (denom < DBL_MIN) return 0;
    num = log(num); denom = log(denom);
    return (denom >= 0 || -num >= max_iters * (-denom)) ? max_iters : (int)rint(num / denom);
}

// Fixed-order block sum of kRed values: every thread passes its partials; thread 0 gets the sums in `out` (LDS, kRed doubles).
__device__ __forceinline__ void block_sum(double* v, double (*wred)[kRed], double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kRed; ++k) {
        double s = v[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        v[k] = s;
    }
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < kRed; ++k) wred[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x < kRed) {
        double s = wred[0][threadIdx.x];
        for (int w = 1; w < kWaves; ++w) s += wred[w][threadIdx.x];
        out[threadIdx.x] = s;
    }
    __syncthreads();
}

struct HypSlot { double pose[12]; };

// The trace of uvs_lc_debug_pair (layout: include/uvs_solver.h).  Every store goes from registers to global memory at an offset made of the
// hypothesis, the iteration counter and these constants; the shipped instantiation (kTrace = false) has none of them.
constexpr int kTrHead = UVS_LC_TRACE_HEAD_LEN, kTrIter = UVS_LC_TRACE_ITER_LEN, kTrRec = UVS_LC_TRACE_REC_LEN;
constexpr int kTrStage = UVS_LC_TRACE_STAGE_OFF;
static_assert(kTrRec == kTrHead + kLmIters * kTrIter && kTrStage == (kHyp + 1) * kTrRec, "trace layout");
static_assert(UVS_LC_TRACE_LEN == kTrStage + 1 + 6 * kMaxQ, "trace layout");

// k_lc_verify<false> is the shipped kernel (`trace` unused); k_lc_verify<true> is uvs_lc_debug_pair's instantiation of the same body (tests
// only: one pair, `trace` zeroed before the launch).
template <bool kTrace>
__global__ void __launch_bounds__(kThreads) k_lc_verify(const LcPair* __restrict__ pairs, const double* __restrict__ ex,
                                                      const double* __restrict__ p3d, const unsigned long long* __restrict__ qdesc,
                                                      const double* __restrict__ ouv, const unsigned long long* __restrict__ odesc,
                                                      uvs_lc_result* __restrict__ results, int32_t* __restrict__ match_old,
                                                      uint8_t* __restrict__ inlier, double* __restrict__ trace) {
    __shared__ double sX[kMaxQ * 3];
    __shared__ double sUV[kMaxQ * 2];
    __shared__ short sMq[kMaxQ];                 // query index of match m
    __shared__ unsigned char sFlag[kMaxQ];       // per query: matched; later per match: inlier of the chosen hypothesis
    __shared__ union {
        unsigned long long tile[kTile * 4];
        struct { HypSlot hyp[kHyp]; int cnt[kHyp]; } h;
    } sU;
    __shared__ int sScan[2][kThreads];
    __shared__ double sWred[kWaves][kRed];
    __shared__ double sSum[kRed];
    __shared__ double sPose[12], sCand[12];
    __shared__ int sCtl[4];                      // best hypothesis, hypotheses examined, stop flag

    const int tid = threadIdx.x;
    const LcPair P = pairs[blockIdx.x];
    const int nq = P.n_query, no = P.n_old;
    uvs_lc_result* res = results + blockIdx.x;
    int32_t* mo = match_old + P.q_off;
    uint8_t* inl = inlier + P.q_off;

    // ---- match (searchInAera): thread tid owns queries tid + kThreads k
    int best[kQPerThread], bidx[kQPerThread];
    unsigned long long qd[kQPerThread][4];
#pragma unroll
    for (int k = 0; k < kQPerThread; ++k) {
        const int i = tid + kThreads * k;
        best[k] = 128; bidx[k] = -1;
#pragma unroll
        for (int w = 0; w < 4; ++w) qd[k][w] = i < nq ? qdesc[4 * (size_t)(P.q_off + i) + w] : 0ull;
    }
    for (int base = 0; base < no; base += kTile) {
        const int m = min(kTile, no - base);
        for (int e = tid; e < 4 * m; e += kThreads) sU.tile[e] = odesc[4 * (size_t)(P.o_off + base) + e];
        __syncthreads();
        for (int j = 0; j < m; ++j) {
            const unsigned long long o0 = sU.tile[4 * j], o1 = sU.tile[4 * j + 1], o2 = sU.tile[4 * j + 2], o3 = sU.tile[4 * j + 3];
#pragma unroll
            for (int k = 0; k < kQPerThread; ++k) {
                if (tid + kThreads * k >= nq) continue;
                const int dist = __builtin_popcountll(qd[k][0] ^ o0) + __builtin_popcountll(qd[k][1] ^ o1) +
                                 __builtin_popcountll(qd[k][2] ^ o2) + __builtin_popcountll(qd[k][3] ^ o3);
                if (dist < best[k]) { best[k] = dist; bidx[k] = base + j; }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kQPerThread; ++k) {
        const int i = tid + kThreads * k;
        if (i < nq) {
            const bool ok = bidx[k] != -1 && best[k] < 80;
            mo[i] = ok ? bidx[k] : -1;
            inl[i] = 0;
            sFlag[i] = ok;
        }
    }
    __syncthreads();

    // ---- compact: ordered prefix sum, 4 contiguous queries per thread
    int cnt = 0;
    for (int c = 0; c < kQPerThread; ++c) { const int i = kQPerThread * tid + c; cnt += (i < nq) ? sFlag[i] : 0; }
    sScan[0][tid] = cnt;
    __syncthreads();
    int src = 0;
    for (int off = 1; off < kThreads; off <<= 1) {
        const int v = sScan[src][tid] + (tid >= off ? sScan[src][tid - off] : 0);
        sScan[src ^ 1][tid] = v;
        src ^= 1;
        __syncthreads();
    }
    const int n = sScan[src][kThreads - 1];
    int m = sScan[src][tid] - cnt;
    for (int c = 0; c < kQPerThread; ++c) {
        const int i = kQPerThread * tid + c;
        if (i < nq && sFlag[i]) {
            const int j = mo[i];
            sMq[m] = (short)i;
            for (int a = 0; a < 3; ++a) sX[3 * m + a] = p3d[3 * (size_t)(P.q_off + i) + a];
            for (int a = 0; a < 2; ++a) sUV[2 * m + a] = ouv[2 * (size_t)(P.o_off + j) + a];
            ++m;
        }
    }
    __syncthreads();

    if (tid == 0) {
        res->accepted = 0; res->n_matches = n; res->n_inliers = 0; res->best_hypothesis = -1; res->ransac_iters = 0;
        res->reason = n == 0 ? UVS_LC_NO_MATCHES : UVS_LC_FEW_MATCHES;
        for (int k = 0; k < 8; ++k) res->loop_info[k] = 0.0;
        for (int k = 0; k < 3; ++k) res->PnP_T_old[k] = 0.0;
        res->PnP_q_old[0] = res->PnP_q_old[1] = res->PnP_q_old[2] = 0.0; res->PnP_q_old[3] = 1.0;
    }
    if (tid < kHyp) res->hyp_inliers[tid] = -1;
    if constexpr (kTrace) {                                     // what the kernel staged: n, sX, sUV, sMq
        double* ts = trace + kTrStage;
        if (tid == 0) ts[0] = n;
        for (int j = tid; j < n; j += kThreads) {
            for (int a = 0; a < 3; ++a) ts[1 + 3 * j + a] = sX[3 * j + a];
            for (int a = 0; a < 2; ++a) ts[1 + 3 * kMaxQ + 2 * j + a] = sUV[2 * j + a];
            ts[1 + 5 * kMaxQ + j] = sMq[j];
        }
    }
    if (n <= kMinLoop) return;                                  // gate 1 (uniform across the workgroup)

    // ---- the VIO prior: camera pose of origin_vio through the extrinsic (PnPRANSAC :213-219)
    const double tic[3] = {ex[0], ex[1], ex[2]};
    double ric[9], vR[9], Rwc[9], R0[9], t0[3];
    for (int k = 0; k < 9; ++k) ric[k] = ex[3 + k];
    quat_to_R(P.vio_q, vR);
    matmul3(vR, ric, Rwc);
    double Twc[3];
    for (int i = 0; i < 3; ++i) Twc[i] = P.vio_t[i] + vR[3 * i] * tic[0] + vR[3 * i + 1] * tic[1] + vR[3 * i + 2] * tic[2];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R0[3 * i + j] = Rwc[3 * j + i];
    for (int i = 0; i < 3; ++i) t0[i] = -(R0[3 * i] * Twc[0] + R0[3 * i + 1] * Twc[1] + R0[3 * i + 2] * Twc[2]);

    // ---- hypotheses: thread h
    if (tid < kHyp) {
        const int h = tid;
        int s[kModel], got = 0;
        for (int a = 0; a < kMaxAttempts && got < kModel; ++a) {
            const unsigned long long z = uvs_draw(P.seed, h, a);
            const int v = (int)(z % (unsigned long long)n);
            bool dup = false;
#pragma unroll
            for (int k = 0; k < kModel; ++k) dup |= (k < got && s[k] == v);
            if (!dup) {
#pragma unroll
                for (int k = 0; k < kModel; ++k) if (k == got) s[k] = v;
                ++got;
            }
        }
        bool valid = got == kModel;
        double* th = nullptr;                                   // this hypothesis's trace record
        int nrec = 0;
        if constexpr (kTrace) {
            th = trace + h * kTrRec;
#pragma unroll
            for (int k = 0; k < kModel; ++k) th[k] = valid ? s[k] : -1;
            th[20] = valid;
        }
        double R[9], t[3];
        for (int k = 0; k < 9; ++k) R[k] = R0[k];
        for (int k = 0; k < 3; ++k) t[k] = t0[k];
        if (valid) {
            double cost = 0.0;
#pragma unroll
            for (int k = 0; k < kModel; ++k) cost += point_cost(R, t, sX + 3 * s[k], sUV + 2 * s[k]);
            valid = isfinite(cost);
            if constexpr (kTrace) th[7] = cost;
            double lam = kLambda0;
            for (int it = 0; it < kLmIters && valid; ++it) {
                double* ti = nullptr;
                if constexpr (kTrace) {
                    ti = th + kTrHead + it * kTrIter; nrec = it + 1;
                    for (int k = 0; k < 9; ++k) ti[k] = R[k];
                    for (int k = 0; k < 3; ++k) ti[9 + k] = t[k];
                    ti[12] = lam;
                }
                double acc[kRed];
#pragma unroll
                for (int k = 0; k < kRed; ++k) acc[k] = 0.0;
#pragma unroll
                for (int k = 0; k < kModel; ++k) accum_point(R, t, sX + 3 * s[k], sUV + 2 * s[k], acc);
                if constexpr (kTrace) {
#pragma unroll
                    for (int k = 0; k < kRed; ++k) ti[13 + k] = acc[k];
                }
                double d[6];
                if (!chol_solve6(acc, lam, d)) { valid = false; break; }
                double Rc[9], tc[3];
                apply_step(R, t, d, Rc, tc);
                double cc = 0.0;
#pragma unroll
                for (int k = 0; k < kModel; ++k) cc += point_cost(Rc, tc, sX + 3 * s[k], sUV + 2 * s[k]);
                if constexpr (kTrace) {
                    ti[41] = 1.0;
                    for (int k = 0; k < 6; ++k) ti[42 + k] = d[k];
                    for (int k = 0; k < 9; ++k) ti[48 + k] = Rc[k];
                    for (int k = 0; k < 3; ++k) ti[57 + k] = tc[k];
                    ti[60] = cc; ti[61] = cost; ti[62] = cc < cost;
                }
                if (cc < cost) {
                    for (int k = 0; k < 9; ++k) R[k] = Rc[k];
                    for (int k = 0; k < 3; ++k) t[k] = tc[k];
                    cost = cc; lam /= 10.0;
                } else {
                    lam *= 10.0;
                }
                if constexpr (kTrace) {
                    const bool stop = step_small(d, t);
                    ti[63] = stop;
                    if (stop) break;
                } else {
                    if (step_small(d, t)) break;
                }
            }
        }
        if constexpr (kTrace) {
            th[5] = valid; th[6] = nrec;
            for (int k = 0; k < 9; ++k) th[8 + k] = R[k];
            for (int k = 0; k < 3; ++k) th[17 + k] = t[k];
        }
        int c = -1;
        if (valid) {
            c = 0;
            for (int j = 0; j < n; ++j) c += is_inlier(R, t, sX + 3 * j, sUV + 2 * j);
        }
        for (int k = 0; k < 9; ++k) sU.h.hyp[h].pose[k] = R[k];
        for (int k = 0; k < 3; ++k) sU.h.hyp[h].pose[9 + k] = t[k];
        sU.h.cnt[h] = c;
        res->hyp_inliers[h] = c;
    }
    __syncthreads();

    // ---- select: OpenCV's sequential rule over the counts
    if (tid == 0) {
        int bh = -1, bc = 0, niters = kHyp, h = 0;
        for (; h < niters; ++h) {
            const int c = sU.h.cnt[h];
            if (c > max(bc, kModel - 1)) {
                bh = h; bc = c;
                niters = update_num_iters(kConfidence, (double)(n - c) / n, kModel, niters);
            }
        }
        sCtl[0] = bh; sCtl[1] = h; sCtl[2] = 0;
        res->best_hypothesis = bh; res->ransac_iters = h;
        if (bh < 0) res->reason = UVS_LC_RANSAC_FAILED;
        else for (int k = 0; k < 12; ++k) sPose[k] = sU.h.hyp[bh].pose[k];
        if constexpr (kTrace) {
            if (bh >= 0) for (int k = 0; k < 12; ++k) trace[kHyp * kTrRec + 20 + k] = sPose[k];       // the refinement's start pose
        }
    }
    __syncthreads();
    const int bh = sCtl[0];
    if (bh < 0) return;

    // ---- the chosen hypothesis's inlier mask
    int my_inl = 0;
    {
        double R[9], t[3];
        for (int k = 0; k < 9; ++k) R[k] = sPose[k];
        for (int k = 0; k < 3; ++k) t[k] = sPose[9 + k];
        for (int j = tid; j < n; j += kThreads) {
            const bool in = is_inlier(R, t, sX + 3 * j, sUV + 2 * j);
            sFlag[j] = in;
            inl[sMq[j]] = in;
            my_inl += in;
        }
    }
    __syncthreads();

    // ---- refinement LM on the inliers from the hypothesis's pose (fixed-order reductions)
    double cost = 0.0, lam = kLambda0;
    double* tr = nullptr;                                       // the refinement's trace record (thread 0 writes it)
    int nrec = 0;
    if constexpr (kTrace) tr = trace + kHyp * kTrRec;
    for (int it = 0; it < kLmIters; ++it) {
        double acc[kRed];
#pragma unroll
        for (int k = 0; k < kRed; ++k) acc[k] = 0.0;
        {
            double R[9], t[3];
            for (int k = 0; k < 9; ++k) R[k] = sPose[k];
            for (int k = 0; k < 3; ++k) t[k] = sPose[9 + k];
            for (int j = tid; j < n; j += kThreads) if (sFlag[j]) accum_point(R, t, sX + 3 * j, sUV + 2 * j, acc);
        }
        block_sum(acc, sWred, sSum);
        if (tid == 0) {
            if (it == 0) cost = sSum[27];
            double* ti = nullptr;
            if constexpr (kTrace) {
                ti = tr + kTrHead + it * kTrIter; nrec = it + 1;
                if (it == 0) tr[7] = cost;
                for (int k = 0; k < 12; ++k) ti[k] = sPose[k];
                ti[12] = lam;
                for (int k = 0; k < kRed; ++k) ti[13 + k] = sSum[k];
            }
            double d[6];
            if (!chol_solve6(sSum, lam, d)) sCtl[2] = 1;
            else {
                apply_step(sPose, sPose + 9, d, sCand, sCand + 9);
                for (int k = 0; k < 6; ++k) sSum[k] = d[k];        // keep the step for the stop test
                if constexpr (kTrace) {
                    ti[41] = 1.0;
                    for (int k = 0; k < 6; ++k) ti[42 + k] = d[k];
                    for (int k = 0; k < 12; ++k) ti[48 + k] = sCand[k];
                }
            }
        }
        __syncthreads();
        if (sCtl[2]) break;
        double pc[kRed];
#pragma unroll
        for (int k = 0; k < kRed; ++k) pc[k] = 0.0;
        {
            double R[9], t[3];
            for (int k = 0; k < 9; ++k) R[k] = sCand[k];
            for (int k = 0; k < 3; ++k) t[k] = sCand[9 + k];
            for (int j = tid; j < n; j += kThreads) if (sFlag[j]) pc[27] += point_cost(R, t, sX + 3 * j, sUV + 2 * j);
        }
        double d[6];
        if (tid == 0) for (int k = 0; k < 6; ++k) d[k] = sSum[k];
        block_sum(pc, sWred, sSum);
        if (tid == 0) {
            const double cc = sSum[27];
            double* ti = nullptr;
            if constexpr (kTrace) {
                ti = tr + kTrHead + it * kTrIter;
                ti[60] = cc; ti[61] = cost; ti[62] = cc < cost;
            }
            if (cc < cost) {
                for (int k = 0; k < 12; ++k) sPose[k] = sCand[k];
                cost = cc; lam /= 10.0;
            } else {
                lam *= 10.0;
            }
            if constexpr (kTrace) {
                const bool stop = step_small(d, sPose + 9);
                ti[63] = stop;
                if (stop) sCtl[2] = 1;
            } else {
                if (step_small(d, sPose + 9)) sCtl[2] = 1;
            }
        }
        __syncthreads();
        if (sCtl[2]) break;
    }

    // ---- n_inliers (fixed order), finish on thread 0
    {
        int v = my_inl;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((tid & 63) == 0) sScan[0][tid >> 6] = v;
    }
    __syncthreads();
    if (tid == 0) {
        int ni = 0;
        for (int w = 0; w < kWaves; ++w) ni += sScan[0][w];
        res->n_inliers = ni;
        if constexpr (kTrace) {
            tr[5] = 1.0; tr[6] = nrec;
            for (int k = 0; k < 12; ++k) tr[8 + k] = sPose[k];
        }
        double Rwco[9], PR[9], Two[3], PT[3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Rwco[3 * i + j] = sPose[3 * j + i];             // R_w_c_old = R_pnp^T
        for (int i = 0; i < 3; ++i) Two[i] = -(Rwco[3 * i] * sPose[9] + Rwco[3 * i + 1] * sPose[10] + Rwco[3 * i + 2] * sPose[11]);
        matmul3_nt(Rwco, ric, PR);                                                      // PnP_R_old = R_w_c_old qic^T
        for (int i = 0; i < 3; ++i) PT[i] = Two[i] - (PR[3 * i] * tic[0] + PR[3 * i + 1] * tic[1] + PR[3 * i + 2] * tic[2]);
        double q[4];
        R_to_quat_wxyz(PR, q);
        for (int k = 0; k < 3; ++k) res->PnP_T_old[k] = PT[k];
        res->PnP_q_old[0] = q[1]; res->PnP_q_old[1] = q[2]; res->PnP_q_old[2] = q[3]; res->PnP_q_old[3] = q[0];
        if (ni <= kMinLoop) {
            res->reason = UVS_LC_FEW_INLIERS;
        } else {
            double rt[3], d[3], RQ[9], rq[4];
            for (int i = 0; i < 3; ++i) d[i] = P.vio_t[i] - PT[i];
            for (int i = 0; i < 3; ++i) rt[i] = PR[i] * d[0] + PR[3 + i] * d[1] + PR[6 + i] * d[2];
            matmul3_tn(PR, vR, RQ);
            R_to_quat_wxyz(RQ, rq);
            const double ryaw = normalize_angle(yaw_deg(vR) - yaw_deg(PR));
            for (int k = 0; k < 3; ++k) res->loop_info[k] = rt[k];
            for (int k = 0; k < 4; ++k) res->loop_info[3 + k] = rq[k];
            res->loop_info[7] = ryaw;
            const double tn = sqrt(rt[0] * rt[0] + rt[1] * rt[1] + rt[2] * rt[2]);
            if (!(fabs(ryaw) < 30.0)) res->reason = UVS_LC_YAW_GATE;
            else if (!(tn < 20.0)) res->reason = UVS_LC_T_GATE;
            else { res->reason = UVS_LC_ACCEPTED; res->accepted = 1; }
        }
    }
}

}  // namespace uvslc

using namespace uvslc;

struct uvs_loop_verifier : UvsHandle {       // no call is timed: opened without events
    int max_pairs = 0, max_query = 0, max_old = 0;
    size_t in_bytes = 0, out_bytes = 0;
    DevBuf<char> d_in, d_out;                   // packed inputs / outputs of one call
    DevBuf<double> d_trace;                     // uvs_lc_debug_pair's trace, allocated by its first call
    PinnedBuf<char> h_in, h_out;                // pinned staging
};

namespace {

inline size_t align8(size_t b) { return (b + 7) & ~size_t(7); }

bool unit_quat(const double* q) {
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    return std::isfinite(n) && std::fabs(n - 1.0) <= 1e-6;
}

}  // namespace

extern "C" {

int uvs_lc_create(int device, int max_pairs, int max_query, int max_old, uvs_loop_verifier** out) {
    if (!out || max_pairs < 1 || max_query < 1 || max_old < 1) return UVS_ERR_INVALID_ARG;
    *out = nullptr;
    if (max_pairs > UVS_LC_MAX_PAIRS || max_query > UVS_LC_MAX_QUERY || max_old > UVS_LC_MAX_OLD) return UVS_ERR_CAPACITY;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return UVS_ERR_NO_DEVICE;
    uvs_loop_verifier* lc = new uvs_loop_verifier();
    lc->max_pairs = max_pairs; lc->max_query = max_query; lc->max_old = max_old;
    const size_t B = max_pairs, Q = B * max_query, O = B * max_old;
    lc->in_bytes = align8(B * sizeof(LcPair)) + 12 * 8 + Q * (3 * 8 + 4 * 8) + O * (2 * 8 + 4 * 8);
    lc->out_bytes = align8(B * sizeof(uvs_lc_result)) + align8(Q * 4) + align8(Q);
    int rc = lc->open(device, false);
    if (rc == UVS_OK && (rc = lc->d_in.ensure(lc->in_bytes, lc->err)) == UVS_OK && (rc = lc->d_out.ensure(lc->out_bytes, lc->err)) == UVS_OK &&
        (rc = lc->h_in.ensure(lc->in_bytes, lc->err)) == UVS_OK) rc = lc->h_out.ensure(lc->out_bytes, lc->err);
    if (rc != UVS_OK) { uvs_lc_destroy(lc); return rc; }
    *out = lc;
    return UVS_OK;
}

void uvs_lc_destroy(uvs_loop_verifier* lc) { if (lc) { lc->close(); delete lc; } }

const char* uvs_lc_last_error(const uvs_loop_verifier* lc) { return lc ? lc->err.c_str() : "null loop verifier"; }

}  // extern "C"

namespace {

// uvs_lc_verify (trace = nullptr) and uvs_lc_debug_pair (one pair, trace[UVS_LC_TRACE_LEN]): the same checks, packing and copies
int lc_run(uvs_loop_verifier* lc, int n_pairs, const uvs_lc_pair* pairs, const double tic[3], const double qic_xyzw[4],
           int32_t* match_old, uint8_t* inlier, uvs_lc_result* results, double* trace) {
    if (n_pairs < 1 || !pairs || !tic || !qic_xyzw || !match_old || !inlier || !results) {
        lc->err = "uvs_lc_verify: null pointer or bad count"; return UVS_ERR_INVALID_ARG;
    }
    if (n_pairs > lc->max_pairs) { lc->err = "uvs_lc_verify: more pairs than the capacity given to uvs_lc_create"; return UVS_ERR_CAPACITY; }
    if (!unit_quat(qic_xyzw)) { lc->err = "uvs_lc_verify: qic is not a unit quaternion"; return UVS_ERR_INVALID_ARG; }
    size_t tq = 0, to = 0;
    for (int b = 0; b < n_pairs; ++b) {
        const uvs_lc_pair& p = pairs[b];
        const std::string who = "uvs_lc_verify: pair " + std::to_string(b);
        if (p.n_query < 0 || p.n_old < 0 || (p.n_query > 0 && (!p.p3d || !p.desc)) || (p.n_old > 0 && (!p.old_uv_norm || !p.old_desc))) {
            lc->err = who + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG;
        }
        if (p.n_query > lc->max_query || p.n_old > lc->max_old) { lc->err = who + " exceeds the capacity given to uvs_lc_create"; return UVS_ERR_CAPACITY; }
        if (!unit_quat(p.vio_q)) { lc->err = who + ": vio_q is not a unit quaternion"; return UVS_ERR_INVALID_ARG; }
        tq += p.n_query; to += p.n_old;
    }
    // packed input: pairs | tic, R(qic) | p3d | query desc | old uv | old desc
    const size_t o_ex = align8(n_pairs * sizeof(LcPair)), o_p3d = o_ex + 12 * 8, o_qd = o_p3d + tq * 24, o_uv = o_qd + tq * 32, o_od = o_uv + to * 16;
    const size_t in_used = o_od + to * 32;
    LcPair* hp = reinterpret_cast<LcPair*>(lc->h_in.get());
    double* hex = reinterpret_cast<double*>(lc->h_in + o_ex);
    size_t qo = 0, oo = 0;
    for (int b = 0; b < n_pairs; ++b) {
        const uvs_lc_pair& p = pairs[b];
        LcPair d;
        d.n_query = p.n_query; d.n_old = p.n_old; d.q_off = (int)qo; d.o_off = (int)oo; d.seed = p.seed;
        for (int k = 0; k < 3; ++k) d.vio_t[k] = p.vio_t[k];
        for (int k = 0; k < 4; ++k) d.vio_q[k] = p.vio_q[k];
        hp[b] = d;
        if (p.n_query) {
            std::memcpy(lc->h_in + o_p3d + qo * 24, p.p3d, (size_t)p.n_query * 24);
            std::memcpy(lc->h_in + o_qd + qo * 32, p.desc, (size_t)p.n_query * 32);
        }
        if (p.n_old) {
            std::memcpy(lc->h_in + o_uv + oo * 16, p.old_uv_norm, (size_t)p.n_old * 16);
            std::memcpy(lc->h_in + o_od + oo * 32, p.old_desc, (size_t)p.n_old * 32);
        }
        qo += p.n_query; oo += p.n_old;
    }
    {   // the extrinsic: tic, then Eigen's toRotationMatrix of qic
        const double x = qic_xyzw[0], y = qic_xyzw[1], z = qic_xyzw[2], w = qic_xyzw[3];
        const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                             2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                             2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
        for (int k = 0; k < 3; ++k) hex[k] = tic[k];
        for (int k = 0; k < 9; ++k) hex[3 + k] = R[k];
    }
    const size_t r_bytes = align8(n_pairs * sizeof(uvs_lc_result)), o_mo = r_bytes, o_in = o_mo + align8(tq * 4), out_used = o_in + tq;
    hipStream_t st = lc->st;
    UVS_HIP(lc->err, hipSetDevice(lc->device));
    UVS_HIP(lc->err, hipMemcpyAsync(lc->d_in, lc->h_in, in_used, hipMemcpyHostToDevice, st));
    if (trace) {
        const size_t t_bytes = sizeof(double) * UVS_LC_TRACE_LEN;
        if (const int rc = lc->d_trace.ensure(t_bytes, lc->err)) return rc;
        UVS_HIP(lc->err, hipMemsetAsync(lc->d_trace, 0, t_bytes, st));
        k_lc_verify<true><<<1, kThreads, 0, st>>>(reinterpret_cast<const LcPair*>(lc->d_in.get()), reinterpret_cast<const double*>(lc->d_in + o_ex),
                                                 reinterpret_cast<const double*>(lc->d_in + o_p3d), reinterpret_cast<const unsigned long long*>(lc->d_in + o_qd),
                                                 reinterpret_cast<const double*>(lc->d_in + o_uv), reinterpret_cast<const unsigned long long*>(lc->d_in + o_od),
                                                 reinterpret_cast<uvs_lc_result*>(lc->d_out.get()), reinterpret_cast<int32_t*>(lc->d_out + o_mo),
                                                 reinterpret_cast<uint8_t*>(lc->d_out + o_in), lc->d_trace.get());
        UVS_HIP(lc->err, hipGetLastError());
        UVS_HIP(lc->err, hipMemcpyAsync(trace, lc->d_trace, t_bytes, hipMemcpyDeviceToHost, st));
    } else {
        k_lc_verify<false><<<n_pairs, kThreads, 0, st>>>(reinterpret_cast<const LcPair*>(lc->d_in.get()), reinterpret_cast<const double*>(lc->d_in + o_ex),
                                                 reinterpret_cast<const double*>(lc->d_in + o_p3d), reinterpret_cast<const unsigned long long*>(lc->d_in + o_qd),
                                                 reinterpret_cast<const double*>(lc->d_in + o_uv), reinterpret_cast<const unsigned long long*>(lc->d_in + o_od),
                                                 reinterpret_cast<uvs_lc_result*>(lc->d_out.get()), reinterpret_cast<int32_t*>(lc->d_out + o_mo),
                                                 reinterpret_cast<uint8_t*>(lc->d_out + o_in), nullptr);
        UVS_HIP(lc->err, hipGetLastError());
    }
    UVS_HIP(lc->err, hipMemcpyAsync(lc->h_out, lc->d_out, out_used, hipMemcpyDeviceToHost, st));
    UVS_HIP(lc->err, hipStreamSynchronize(st));
    std::memcpy(results, lc->h_out, n_pairs * sizeof(uvs_lc_result));
    if (tq) {
        std::memcpy(match_old, lc->h_out + o_mo, tq * 4);
        std::memcpy(inlier, lc->h_out + o_in, tq);
    }
    return UVS_OK;
}

}  // namespace

extern "C" {

int uvs_lc_verify(uvs_loop_verifier* lc, int n_pairs, const uvs_lc_pair* pairs, const double tic[3], const double qic_xyzw[4],
                  int32_t* match_old, uint8_t* inlier, uvs_lc_result* results) {
    if (!lc) return UVS_ERR_INVALID_ARG;
    lc->err.clear();
    return lc_run(lc, n_pairs, pairs, tic, qic_xyzw, match_old, inlier, results, nullptr);
}

int uvs_lc_debug_pair(uvs_loop_verifier* lc, const uvs_lc_pair* pair, const double tic[3], const double qic_xyzw[4],
                      int32_t* match_old, uint8_t* inlier, uvs_lc_result* result, double* trace) {
    if (!lc) return UVS_ERR_INVALID_ARG;
    lc->err.clear();
    if (!trace) { lc->err = "uvs_lc_debug_pair: null pointer"; return UVS_ERR_INVALID_ARG; }
    return lc_run(lc, 1, pair, tic, qic_xyzw, match_old, inlier, result, trace);
}

}  // extern "C"
