// uvs_svd_dev.h -- the small dense SVD pieces that a lane runs out of registers, one statement of each for the units that use them:
// csrc/uvs_triangulate.hip (k_tri_points: the DLT of a point track) and csrc/uvs_relative_pose.hip (k_rp_recover: the 3 x 3 SVD of F and the
// 4 x 4 null vector of every two-view triangulation).  Every matrix is a fixed-size array that only fully unrolled loops index, so nothing lands
// in scratch.  FP64; the including unit's contraction setting applies (neither unit claims bit equality for what comes out of here).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace uvssvd {

constexpr int kMaxSweeps = 30;             // a 4 x 4 triangle converges in 4 .. 7 sweeps; the cap only bounds a lane that holds NaNs
constexpr double kEps = 2.220446049250313e-16;

// one row x of a matrix A into the upper triangle T of A = Q T by Givens rotations (x is destroyed)
__device__ __forceinline__ void givens_row(double T[4][4], double x[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (x[j] != 0.0) {
            const double a = T[j][j], b = x[j], h = sqrt(a * a + b * b), c = a / h, s = b / h;
            T[j][j] = h;
#pragma unroll
            for (int m = j + 1; m < 4; ++m) {
                const double tm = T[j][m], xm = x[m];
                T[j][m] = c * tm + s * xm;
                x[m] = c * xm - s * tm;
            }
        }
    }
}

// one-sided Jacobi on the columns of T (Hestenes): T V = U Sigma on return, V the identity on entry.  Columns are rotated in the fixed order
// (0,1) (0,2) .. (N-2,N-1) until a sweep rotates nothing, at most kMaxSweeps sweeps.
// The one statement of the sweep is a macro, expanded in the body of the kernel that uses it.  As a function taking the two arrays -- inlined
// all the same -- it cost k_tri_points 138 VGPRs and 3 waves per SIMD; the text in place costs 118 VGPRs and 4 waves per SIMD (106 and 4
// before the move: the occupancy is what it was).  The difference is the compiler's allocation, not the arithmetic.  jacobi_columns<N> below
// is the same text as a function, for a caller without that history (k_rp_recover).
#define UVS_JACOBI_COLUMNS(N, T, V)                                                                                                     \
    do {                                                                                                                                \
        _Pragma("unroll") for (int r_ = 0; r_ < (N); ++r_)                                                                              \
            _Pragma("unroll") for (int c_ = 0; c_ < (N); ++c_) V[r_][c_] = r_ == c_ ? 1.0 : 0.0;                                        \
        for (int sweep_ = 0; sweep_ < uvssvd::kMaxSweeps; ++sweep_) {                                                                   \
            bool rotated_ = false;                                                                                                      \
            _Pragma("unroll") for (int p_ = 0; p_ < (N) - 1; ++p_) {                                                                    \
                _Pragma("unroll") for (int q_ = p_ + 1; q_ < (N); ++q_) {                                                               \
                    double alpha_ = 0.0, beta_ = 0.0, gamma_ = 0.0;                                                                     \
                    _Pragma("unroll") for (int k_ = 0; k_ < (N); ++k_) {                                                                \
                        alpha_ += T[k_][p_] * T[k_][p_]; beta_ += T[k_][q_] * T[k_][q_]; gamma_ += T[k_][p_] * T[k_][q_];               \
                    }                                                                                                                   \
                    if (fabs(gamma_) > uvssvd::kEps * sqrt(alpha_ * beta_)) {      /* false for a zero column and for NaN */            \
                        rotated_ = true;                                                                                                \
                        const double zeta_ = (beta_ - alpha_) / (2.0 * gamma_);                                                         \
                        const double tt_ = copysign(1.0, zeta_) / (fabs(zeta_) + sqrt(1.0 + zeta_ * zeta_));                            \
                        const double cs_ = 1.0 / sqrt(1.0 + tt_ * tt_), sn_ = cs_ * tt_;                                                \
                        _Pragma("unroll") for (int k_ = 0; k_ < (N); ++k_) {                                                            \
                            const double gp_ = T[k_][p_], gq_ = T[k_][q_];                                                              \
                            T[k_][p_] = cs_ * gp_ - sn_ * gq_; T[k_][q_] = sn_ * gp_ + cs_ * gq_;                                       \
                            const double vp_ = V[k_][p_], vq_ = V[k_][q_];                                                              \
                            V[k_][p_] = cs_ * vp_ - sn_ * vq_; V[k_][q_] = sn_ * vp_ + cs_ * vq_;                                       \
                        }                                                                                                               \
                    }                                                                                                                   \
                }                                                                                                                       \
            }                                                                                                                           \
            if (!rotated_) break;                                                                                                       \
        }                                                                                                                               \
    } while (0)

template <int N>
__device__ __forceinline__ void jacobi_columns(double T[N][N], double V[N][N]) { UVS_JACOBI_COLUMNS(N, T, V); }

// after the sweeps of a 4 x 4: the column of V whose column of T has the smallest norm (the first such; a NaN norm takes it)
__device__ __forceinline__ void smallest_column(const double T[4][4], const double V[4][4], double q[4]) {
    double best = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double nn = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) nn += T[k][c] * T[k][c];
        if (c == 0 || nn < best || nn != nn) {
            best = nn;
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = V[k][c];
        }
    }
}

}  // namespace uvssvd
