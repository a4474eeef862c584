// uvs_pose_graph.hip -- the 4-DoF pose-graph optimizer of loop closure (reference pose_graph/src/pose_graph.cpp:403-579, the
// ceres::Solve of PoseGraph::optimize4DoF) behind the uvs_pg_* calls of include/uvs_solver.h.  FP64 end to end, gfx950.
//
// Problem (pose_graph.h:90-248): per keyframe a yaw in DEGREES (AngleLocalParameterization: yaw + d, then the single wrap of the file-local
// NormalizeAngle) and a translation; pitch / roll are never variables.  Sequential edges FourDOFError (i-j, i), j = 1..4, same sequence, no loss,
// measured from the initial poses; loop edges FourDOFWeightError (old, cur), HuberLoss(0.1), yaw residual / 10.
//
// Device path of one call (one stream; the host runs the LM controller on the scalars that come back once per iteration):
//   k_pg_prep      per keyframe    ypr of the initial rotation, x = (yaw, t)
//   k_pg_meas      per edge slot   topology (slot 4 i + j - 1 = sequential edge (i - j, i); slot 4 n + l = loop edge l) + measurement
//   k_pg_lin<0>    per edge        residual, analytic 4 x 8 Jacobian, Huber corrector, cost
//   k_pg_assemble  per free kf     GATHER of the block band (4 sub-diagonal blocks), gradient, diag(J^T J) -- no atomics: fixed summation order
//   k_pg_jacobi / k_pg_scale       Jacobi scaling (computed once, from the first Jacobian) and the Marquardt diagonal
//   k_pg_factor    1 wave          banded Cholesky of A = band + D^T D / radius (the loop edges with two free ends are left out of A: H = A + U U^T)
//   k_pg_forward   lane per column W = L^-1 [U | -g]   (U: corrected, scaled loop-edge Jacobians, 4 columns per edge)
//   k_pg_gram + k_pg_potrf/trsm/syrk   G = I + W^T W and its blocked Cholesky; the z column last, so the factor's last row is l = Lc^-1 (U^T A^-1 g)
//   k_pg_capsolve  1 workgroup     v = Lc^-T l = C^-1 U^T A^-1 (-g)
//   k_pg_wv        wave per row    u = z - W v      (Woodbury: (A + U U^T)^-1 = L^-T (I - W C^-1 W^T) L^-1)
//   k_pg_back      1 wave          y = L^-T u
//   (nu > 0: one step of iterative refinement with the same factors)
//   k_pg_resid     per free kf     r = b - (A + U U^T) y in FP64, fixed order
//   k_pg_forward   1 wave          w = L^-1 r into the z column of W
//   k_pg_wtz + k_pg_capsolve       v = C^-1 W_U^T w
//   k_pg_wv + k_pg_back            y += L^-T (w - W_U v)
//   k_pg_step      per free kf     delta = s y, candidate plus with the yaw wrap, |step|^2, |x|^2
//   k_pg_lin<1>    per edge        candidate cost and the model cost change -(J delta).(r + J delta / 2)
//   k_pg_reduce    1 workgroup     fixed-order sums / maxima of the per-edge and per-keyframe partials
// Every reduction has a fixed order, so two calls on the same input give the same bits.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/uvs_solver.h"
#include "uvs_handle.h"

namespace uvspg {

constexpr int kWave = 64;
constexpr int kChunk = 32;          // band rows staged in LDS per pass of the sequential kernels
constexpr int kBand = 5;            // blocks per band row: (a, a), (a, a-1) .. (a, a-4)
constexpr int kRow = kBand * 16;    // doubles per band row
constexpr int kTile = 64;           // Gram / capacitance block size
constexpr double kHuberA = 0.1;     // HuberLoss(0.1), pose_graph.cpp:437
constexpr double kD2R = M_PI / 180.0;
constexpr double kMinDiag = 1e-6, kMaxDiag = 1e32;   // Ceres' min / max_lm_diagonal

// One step of iterative refinement after the Woodbury solve when the problem has loop edges with two free ends (nu > 0): A alone can be
// near singular (a sequence anchored only through U has a gauge null space that only the damping closes), and the Woodbury formula then
// loses accuracy in proportion to cond(A).  0 leaves the plain Woodbury solve (A/B builds only).
#ifndef UVS_PG_REFINE
#define UVS_PG_REFINE 1
#endif

__device__ __host__ inline double normalize_angle(double a) {     // pose_graph.h NormalizeAngle: ONE wrap
    return a > 180.0 ? a - 360.0 : (a < -180.0 ? a + 360.0 : a);
}

// Eigen's Quaternion::toRotationMatrix for q = (x, y, z, w)
__device__ inline void quat_to_R(const double* q, double* R) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

// Utility::R2ypr (utility.h:66-81), degrees
__device__ inline void R_to_ypr(const double* R, double* ypr) {
    const double yaw = atan2(R[3], R[0]), cy = cos(yaw), sy = sin(yaw);
    const double pitch = atan2(-R[6], R[0] * cy + R[3] * sy);
    const double roll = atan2(R[2] * sy - R[5] * cy, R[4] * cy - R[1] * sy);
    ypr[0] = yaw / M_PI * 180.0; ypr[1] = pitch / M_PI * 180.0; ypr[2] = roll / M_PI * 180.0;
}

// YawPitchRollToRotationMatrix (pose_graph.h), degrees in, row-major R
__device__ inline void ypr_to_R(double yaw, double pitch, double roll, double* R) {
    const double y = yaw / 180.0 * M_PI, p = pitch / 180.0 * M_PI, r = roll / 180.0 * M_PI;
    const double cy = cos(y), sy = sin(y), cp = cos(p), sp = sin(p), cr = cos(r), sr = sin(r);
    R[0] = cy * cp; R[1] = -sy * cr + cy * sp * sr; R[2] = sy * sr + cy * sp * cr;
    R[3] = sy * cp; R[4] = cy * cr + sy * sp * sr; R[5] = -cy * sr + sy * sp * cr;
    R[6] = -sp; R[7] = cp * sr; R[8] = cp * cr;
}

struct Edge {          // device edge record, written by k_pg_meas
    int a, b;          // keyframe indices (a = the end whose yaw rotates the residual); a < 0: no edge in this slot
    int fa, fb;        // free indices, -1 for a constant keyframe
    double rel_t[3], rel_yaw, pitch, roll;
};

__global__ void k_pg_prep(int n, const double* __restrict__ t, const double* __restrict__ q, double* __restrict__ x, double* __restrict__ pr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double R[9], ypr[3];
    quat_to_R(q + 4 * i, R);
    R_to_ypr(R, ypr);
    x[4 * i] = ypr[0]; x[4 * i + 1] = t[3 * i]; x[4 * i + 2] = t[3 * i + 1]; x[4 * i + 3] = t[3 * i + 2];
    pr[2 * i] = ypr[1]; pr[2 * i + 1] = ypr[2];
}

__global__ void k_pg_meas(int n, int n_loops, const double* __restrict__ t, const double* __restrict__ q, const int* __restrict__ seq,
                          const int* __restrict__ fidx, const double* __restrict__ x0, const double* __restrict__ pr, const uvs_pg_loop* __restrict__ loops,
                          Edge* __restrict__ E) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 4 * n + n_loops) return;
    Edge ed; ed.a = -1; ed.b = -1; ed.fa = -1; ed.fb = -1;
    ed.rel_t[0] = ed.rel_t[1] = ed.rel_t[2] = 0; ed.rel_yaw = ed.pitch = ed.roll = 0;
    if (e < 4 * n) {                                   // pose_graph.cpp:497-512
        const int b = e >> 2, a = b - ((e & 3) + 1);
        if (a >= 0 && seq[a] == seq[b] && (fidx[a] >= 0 || fidx[b] >= 0)) {
            double R[9];
            quat_to_R(q + 4 * a, R);
            const double d0 = t[3 * b] - t[3 * a], d1 = t[3 * b + 1] - t[3 * a + 1], d2 = t[3 * b + 2] - t[3 * a + 2];
            ed.a = a; ed.b = b; ed.fa = fidx[a]; ed.fb = fidx[b];
            ed.rel_t[0] = R[0] * d0 + R[3] * d1 + R[6] * d2;      // q_{i-j}^-1 (t_i - t_{i-j})
            ed.rel_t[1] = R[1] * d0 + R[4] * d1 + R[7] * d2;
            ed.rel_t[2] = R[2] * d0 + R[5] * d1 + R[8] * d2;
            ed.rel_yaw = x0[4 * b] - x0[4 * a];                      // not normalized
            ed.pitch = pr[2 * a]; ed.roll = pr[2 * a + 1];
        }
    } else {                                           // pose_graph.cpp:516-530
        const uvs_pg_loop L = loops[e - 4 * n];
        if (fidx[L.old] >= 0 || fidx[L.cur] >= 0) {
            ed.a = L.old; ed.b = L.cur; ed.fa = fidx[L.old]; ed.fb = fidx[L.cur];
            ed.rel_t[0] = L.rel_t[0]; ed.rel_t[1] = L.rel_t[1]; ed.rel_t[2] = L.rel_t[2]; ed.rel_yaw = L.rel_yaw;
            ed.pitch = pr[2 * L.old]; ed.roll = pr[2 * L.old + 1];     // of the CONNECTED keyframe
        }
    }
    E[e] = ed;
}

// Residual and Jacobian of one edge at x.  J row-major 4 x 8, columns (yaw_a, t_a, yaw_b, t_b).  Loop edges: yaw row / 10, Huber corrector
// (rho'' <= 0 on both branches of Huber, so Ceres' corrector is the plain sqrt(rho') scaling -- the Cauchy path of uvs_factors.h takes the
// same branch).  Returns 0.5 rho(|r|^2).
__device__ __forceinline__ double edge_eval(const Edge& ed, bool loop, const double* __restrict__ x, double* r, double* J) {
    const double ya = x[4 * ed.a], yb = x[4 * ed.b];
    double R[9];
    ypr_to_R(ya, ed.pitch, ed.roll, R);
    const double d0 = x[4 * ed.b + 1] - x[4 * ed.a + 1], d1 = x[4 * ed.b + 2] - x[4 * ed.a + 2], d2 = x[4 * ed.b + 3] - x[4 * ed.a + 3];
    const double w = loop ? 0.1 : 1.0;
    r[0] = R[0] * d0 + R[3] * d1 + R[6] * d2 - ed.rel_t[0];
    r[1] = R[1] * d0 + R[4] * d1 + R[7] * d2 - ed.rel_t[1];
    r[2] = R[2] * d0 + R[5] * d1 + R[8] * d2 - ed.rel_t[2];
    r[3] = normalize_angle(yb - ya - ed.rel_yaw) * w;
    if (J) {
        // d(R^T d)/d yaw = R^T (K^T d), K = [e_z]x:  K^T d = (d1, -d0, 0); yaw in degrees => * pi / 180
        const double k0 = d1 * kD2R, k1 = -d0 * kD2R;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            J[8 * i + 0] = R[i] * k0 + R[3 + i] * k1;
            J[8 * i + 4] = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) { J[8 * i + 1 + c] = -R[3 * c + i]; J[8 * i + 5 + c] = R[3 * c + i]; }
        }
        J[24] = -w; J[25] = J[26] = J[27] = 0.0; J[28] = w; J[29] = J[30] = J[31] = 0.0;
    }
    const double s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3];
    const double b = kHuberA * kHuberA;
    const bool outer = loop && s > b;
    const double sr = sqrt(s);
    const double sc = outer ? sqrt(fmax(2.2250738585072014e-308, kHuberA / sr)) : 1.0;    // HuberLoss::Evaluate: rho' = max(DBL_MIN, a / sqrt(s))
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] *= sc;
    if (J) {
#pragma unroll
        for (int i = 0; i < 32; ++i) J[i] *= sc;
    }
    return outer ? 0.5 * (2.0 * kHuberA * sr - b) : 0.5 * s;
}

// MODE 0: linearize at x -> er, eJ, per-edge cost.  MODE 1: candidate cost at xc -> ecost, model cost change with the stored (er, eJ) and delta.
template <int MODE>
__global__ void k_pg_lin(int n_slots, int n_seq, const Edge* __restrict__ E, const double* __restrict__ x, const double* __restrict__ delta,
                         double* __restrict__ er, double* __restrict__ eJ, double* __restrict__ ecost, double* __restrict__ emcc) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_slots) return;
    const Edge ed = E[e];
    if (ed.a < 0) { ecost[e] = 0.0; if (MODE == 1) emcc[e] = 0.0; return; }
    double r[4];
    if (MODE == 0) {
        ecost[e] = edge_eval(ed, e >= n_seq, x, r, eJ + 32 * e);
#pragma unroll
        for (int i = 0; i < 4; ++i) er[4 * e + i] = r[i];
    } else {
        ecost[e] = edge_eval(ed, e >= n_seq, x, r, nullptr);
        double d[8];
        for (int c = 0; c < 4; ++c) {
            d[c] = ed.fa >= 0 ? delta[4 * ed.fa + c] : 0.0;
            d[4 + c] = ed.fb >= 0 ? delta[4 * ed.fb + c] : 0.0;
        }
        double m = 0.0;
        for (int i = 0; i < 4; ++i) {
            double jd = 0.0;
            for (int c = 0; c < 8; ++c) jd += eJ[32 * e + 8 * i + c] * d[c];
            m += jd * (er[4 * e + i] + 0.5 * jd);
        }
        emcc[e] = -m;
    }
}

// One free keyframe's share of J^T J and J^T r (edge ends: side 0 = a, side 1 = b).
__device__ inline void add_diag(const double* __restrict__ J, const double* __restrict__ r, int side, double* H, double* g, double* hd) {
    const int o = 4 * side;
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) {
            g[k] += J[8 * i + o + k] * r[i];
            for (int c = 0; c < 4; ++c) H[4 * k + c] += J[8 * i + o + k] * J[8 * i + o + c];
        }
    (void)hd;
}

// Gather per free keyframe a (keyframe i): band row a of A (blocks (a, a-d), d = 0..4, A = edges with at most one free end off the U set), the
// gradient, diag(H) of the FULL H (A + U U^T), and the projected-gradient max |x - Plus(x, -g)| of its four variables.
__global__ void k_pg_assemble(int n, int nf, int n_loops, const int* __restrict__ kf_of_free, const int* __restrict__ fidx, const Edge* __restrict__ E,
                              const double* __restrict__ er, const double* __restrict__ eJ, const double* __restrict__ x,
                              double* __restrict__ band, double* __restrict__ g, double* __restrict__ hdiag, double* __restrict__ gproj) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= nf) return;
    const int i = kf_of_free[a];
    double H[16] = {}, gg[4] = {}, HU[4] = {};
    // sequential edges, i as the b end (slots 4 i + j - 1), then as the a end (slots 4 (i + j) + j - 1)
    for (int j = 1; j <= 4; ++j) {
        const int e = 4 * i + j - 1;
        if (E[e].a >= 0) add_diag(eJ + 32 * e, er + 4 * e, 1, H, gg, nullptr);
    }
    for (int j = 1; j <= 4 && i + j < n; ++j) {
        const int e = 4 * (i + j) + j - 1;
        if (E[e].a >= 0) add_diag(eJ + 32 * e, er + 4 * e, 0, H, gg, nullptr);
    }
    // loop edges in loop order: one free end -> A; two free ends -> U (diag only into HU for diag(H))
    for (int l = 0; l < n_loops; ++l) {
        const int e = 4 * n + l;
        const Edge ed = E[e];
        if (ed.a < 0 || (ed.a != i && ed.b != i)) continue;
        const bool two_free = ed.fa >= 0 && ed.fb >= 0;
        const int side = ed.b == i ? 1 : 0;
        if (!two_free) { add_diag(eJ + 32 * e, er + 4 * e, side, H, gg, nullptr); continue; }
        double Hu[16] = {};
        add_diag(eJ + 32 * e, er + 4 * e, side, Hu, gg, nullptr);
        for (int k = 0; k < 4; ++k) HU[k] += Hu[5 * k];
    }
    double* row = band + (size_t)a * kRow;
    for (int k = 0; k < 16; ++k) row[k] = H[k];
    for (int k = 0; k < 4; ++k) { g[4 * a + k] = gg[k]; hdiag[4 * a + k] = H[5 * k] + HU[k]; }
    // off-diagonal band blocks (a, a-d): the sequential edge (c, i) with c = kf_of_free[a - d], if any -> J_b^T J_a
    for (int d = 1; d < kBand; ++d) {
        double B[16] = {};
        if (a - d >= 0) {
            const int c = kf_of_free[a - d], j = i - c;
            if (j >= 1 && j <= 4) {
                const int e = 4 * i + j - 1;
                if (E[e].a >= 0) {
                    const double* J = eJ + 32 * e;
                    for (int rr = 0; rr < 4; ++rr)
                        for (int k = 0; k < 4; ++k)
                            for (int c2 = 0; c2 < 4; ++c2) B[4 * k + c2] += J[8 * rr + 4 + k] * J[8 * rr + c2];
                }
            }
        }
        for (int k = 0; k < 16; ++k) row[16 * d + k] = B[k];
    }
    // Ceres' projected gradient: yaw through the wrap, t Euclidean
    const double y = x[4 * i];
    double m = fabs(y - normalize_angle(y - gg[0]));
    for (int k = 1; k < 4; ++k) m = fmax(m, fabs(gg[k]));
    gproj[a] = m;
}

__global__ void k_pg_jacobi(int m, const double* __restrict__ hdiag, double* __restrict__ s) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < m) s[k] = 1.0 / (1.0 + sqrt(hdiag[k]));
}

// scaled band S A S (in place), scaled gradient, Marquardt diagonal clip(diag(S H S)) (refreshed after every accepted step)
__global__ void k_pg_scale(int nf, const double* __restrict__ s, double* __restrict__ band, double* __restrict__ g,
                           const double* __restrict__ hdiag, double* __restrict__ lmdiag, double min_d, double max_d) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= nf) return;
    double* row = band + (size_t)a * kRow;
    for (int d = 0; d < kBand; ++d) {
        if (a - d < 0) continue;
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) row[16 * d + 4 * r + c] *= s[4 * a + r] * s[4 * (a - d) + c];
    }
    for (int k = 0; k < 4; ++k) {
        const double sk = s[4 * a + k];
        g[4 * a + k] *= sk;
        lmdiag[4 * a + k] = fmin(fmax(hdiag[4 * a + k] * sk * sk, min_d), max_d);
    }
}

// Banded block Cholesky of A + diag(lmdiag) / radius, one wave: the wave stages kChunk band rows in LDS, lane 0 runs the dependency chain.
// L row a: blocks L(a, a-d) at band index d.  fail[0] = 1 on a non-positive or non-finite pivot.
__global__ void __launch_bounds__(kWave) k_pg_factor(int nf, const double* __restrict__ A, const double* __restrict__ lmdiag, double inv_radius,
                                                     double* __restrict__ L, int* __restrict__ fail) {
    __shared__ double rows[(kChunk + 4) * kRow];
    const int lane = threadIdx.x;
    for (int k = lane; k < 4 * kRow; k += kWave) rows[k] = 0.0;
    int bad = 0;
    for (int a0 = 0; a0 < nf; a0 += kChunk) {
        const int cnt = min(kChunk, nf - a0);
        for (int k = lane; k < cnt * kRow; k += kWave) {
            const int rr = k / kRow, o = k % kRow;
            double v = A[(size_t)(a0 + rr) * kRow + o];
            if (o < 16 && (o % 5) == 0) v += lmdiag[4 * (a0 + rr) + o / 5] * inv_radius;
            rows[4 * kRow + k] = v;
        }
        __syncthreads();
        if (lane == 0) {
            for (int rr = 0; rr < cnt; ++rr) {
                const int a = a0 + rr;
                double* Ra = rows + (4 + rr) * kRow;
                for (int d = 4; d >= 1; --d) {
                    if (a - d < 0) continue;
                    const double* Rc = rows + (4 + rr - d) * kRow;      // row c = a - d
                    double X[16];
                    for (int k = 0; k < 16; ++k) X[k] = Ra[16 * d + k];
                    for (int e = 1; e <= 4 - d; ++e) {                     // - L(a, c-e) L(c, c-e)^T
                        const double* P = Ra + 16 * (d + e); const double* Q = Rc + 16 * e;
                        for (int r = 0; r < 4; ++r)
                            for (int c = 0; c < 4; ++c) {
                                double acc = X[4 * r + c];
                                for (int m = 0; m < 4; ++m) acc -= P[4 * r + m] * Q[4 * c + m];
                                X[4 * r + c] = acc;
                            }
                    }
                    const double* Lc = Rc;                                  // L(c, c): X L(c,c)^-T
                    for (int r = 0; r < 4; ++r)
                        for (int k = 0; k < 4; ++k) {
                            double v = X[4 * r + k];
                            for (int m = 0; m < k; ++m) v -= Lc[4 * k + m] * X[4 * r + m];
                            X[4 * r + k] = v / Lc[5 * k];
                        }
                    for (int k = 0; k < 16; ++k) Ra[16 * d + k] = X[k];
                }
                double S[16];
                for (int k = 0; k < 16; ++k) S[k] = Ra[k];
                for (int d = 1; d <= 4; ++d) {
                    if (a - d < 0) continue;
                    const double* P = Ra + 16 * d;
                    for (int r = 0; r < 4; ++r)
                        for (int c = 0; c <= r; ++c) {
                            double acc = S[4 * r + c];
                            for (int m = 0; m < 4; ++m) acc -= P[4 * r + m] * P[4 * c + m];
                            S[4 * r + c] = acc;
                        }
                }
                for (int k = 0; k < 4; ++k) {
                    double p = S[5 * k];
                    for (int m = 0; m < k; ++m) p -= S[4 * k + m] * S[4 * k + m];
                    if (!(p > 0.0) || !isfinite(p)) { bad = 1; p = 1.0; }
                    const double lk = sqrt(p);
                    S[5 * k] = lk;
                    for (int r = k + 1; r < 4; ++r) {
                        double v = S[4 * r + k];
                        for (int m = 0; m < k; ++m) v -= S[4 * r + m] * S[4 * k + m];
                        S[4 * r + k] = v / lk;
                    }
                    for (int c = k + 1; c < 4; ++c) S[4 * k + c] = 0.0;
                }
                for (int k = 0; k < 16; ++k) Ra[k] = S[k];
            }
        }
        __syncthreads();
        for (int k = lane; k < cnt * kRow; k += kWave) L[(size_t)a0 * kRow + k] = rows[4 * kRow + k];
        __syncthreads();
        // the last four rows of a full chunk precede the next one (only the final chunk can be shorter)
        if (a0 + cnt < nf)
            for (int k = lane; k < 4 * kRow; k += kWave) rows[k] = rows[cnt * kRow + k];
        __syncthreads();
    }
    if (lane == 0 && bad) fail[0] = 1;
}

// Forward substitution W = L^-1 B for many right-hand sides, one column per lane.  Column q < 4 nu: scaled U column (loop edge ucol[q / 4], row q % 4
// of its corrected Jacobian); column zc = 4 nu: zsign * z (z = g, zsign = -1 for the step; the residual, +1, in the refinement pass); the rest:
// zero padding.  A wave starts at the smallest first-nonzero row of its columns (the U columns are sorted by their older end), wstart[wave]
// records it; rows of a column before its wave's start are never written.  Block b runs wave wave0 + b; zonly: only column zc is written.
__global__ void __launch_bounds__(kWave) k_pg_forward(int nf, int ncols, int nu, int wave0, int zonly, const double* __restrict__ L,
                                                      const int* __restrict__ ucol, const Edge* __restrict__ E, const double* __restrict__ eJ,
                                                      const double* __restrict__ s, const double* __restrict__ z, double zsign,
                                                      const int* __restrict__ wstart, double* __restrict__ W) {
    __shared__ double rows[kChunk * kRow], gch[kChunk * 4];
    const int lane = threadIdx.x, wave = wave0 + blockIdx.x, q = wave * kWave + lane;
    const int zc = 4 * nu;
    const bool write = q < ncols && (!zonly || q == zc);
    int fa = -1, fb = -1;
    double ja[4] = {}, jb[4] = {};
    if (q < zc) {
        const int e = ucol[q >> 2], rr = q & 3;
        fa = E[e].fa; fb = E[e].fb;
        for (int c = 0; c < 4; ++c) { ja[c] = eJ[32 * e + 8 * rr + c] * s[4 * fa + c]; jb[c] = eJ[32 * e + 8 * rr + 4 + c] * s[4 * fb + c]; }
    }
    double w1[4] = {}, w2[4] = {}, w3[4] = {}, w4[4] = {};
    const int a_begin = wstart[wave];
    for (int a0 = a_begin; a0 < nf; a0 += kChunk) {
        const int cnt = min(kChunk, nf - a0);
        __syncthreads();
        for (int k = lane; k < cnt * kRow; k += kWave) rows[k] = L[(size_t)a0 * kRow + k];
        for (int k = lane; k < cnt * 4; k += kWave) gch[k] = zsign * z[4 * a0 + k];  // off the dependency chain: no global load per row
        __syncthreads();
        for (int rr = 0; rr < cnt; ++rr) {
            const int a = a0 + rr;
            const double* R = rows + rr * kRow;
            double b[4];
            for (int k = 0; k < 4; ++k) b[k] = q == zc ? gch[4 * rr + k] : (a == fa ? ja[k] : (a == fb ? jb[k] : 0.0));
            for (int k = 0; k < 4; ++k) {
                double v = b[k];
                for (int m = 0; m < 4; ++m) v -= R[16 + 4 * k + m] * w1[m] + R[32 + 4 * k + m] * w2[m] + R[48 + 4 * k + m] * w3[m] + R[64 + 4 * k + m] * w4[m];
                b[k] = v;
            }
            for (int k = 0; k < 4; ++k) {
                double v = b[k];
                for (int m = 0; m < k; ++m) v -= R[4 * k + m] * b[m];
                b[k] = v / R[5 * k];
            }
            for (int k = 0; k < 4; ++k) { w4[k] = w3[k]; w3[k] = w2[k]; w2[k] = w1[k]; w1[k] = b[k]; }
            if (write) for (int k = 0; k < 4; ++k) W[(size_t)(4 * a + k) * ncols + q] = b[k];
        }
    }
}

// G(P, Q) = delta_PQ + sum_r W(r, P)^T W(r, Q) for 64 x 64 tiles P >= Q, summed over the rows both waves wrote (r >= 4 max(wstart)); written to both halves.
__global__ void __launch_bounds__(256) k_pg_gram(int nf, int ncols, const double* __restrict__ W, const int* __restrict__ wstart, double* __restrict__ G) {
    int P = 0, rem = blockIdx.x;                      // lower-triangular tile index -> (P, Q)
    while (rem > P) { rem -= P + 1; ++P; }
    const int Q = rem;
    __shared__ double sp[16][kTile], sq[16][kTile];
    const int tid = threadIdx.x, tr = tid / 16, tc = tid % 16;      // 4 x 4 outputs per thread
    double acc[4][4] = {};
    const int r_begin = 4 * max(wstart[P], wstart[Q]), r_end = 4 * nf;
    for (int r0 = r_begin; r0 < r_end; r0 += 16) {
        __syncthreads();
        for (int k = tid; k < 16 * kTile; k += 256) {
            const int rr = k / kTile, c = k % kTile, r = r0 + rr;
            sp[rr][c] = r < r_end ? W[(size_t)r * ncols + P * kTile + c] : 0.0;
            sq[rr][c] = r < r_end ? W[(size_t)r * ncols + Q * kTile + c] : 0.0;
        }
        __syncthreads();
        for (int rr = 0; rr < 16; ++rr)
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) acc[i][j] += sp[rr][4 * tr + i] * sq[rr][4 * tc + j];
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const int gi = P * kTile + 4 * tr + i, gj = Q * kTile + 4 * tc + j;
            const double v = acc[i][j] + (gi == gj ? 1.0 : 0.0);
            G[(size_t)gi * ncols + gj] = v;
            G[(size_t)gj * ncols + gi] = v;
        }
}

// Blocked right-looking Cholesky of G (lower), 64 x 64 blocks: potrf of diagonal block k, trsm of the panel below, syrk/gemm of the trailing matrix.
__global__ void __launch_bounds__(256) k_pg_potrf(int ncols, int k, double* __restrict__ G, int* __restrict__ fail) {
    __shared__ double T[kTile][kTile + 1];
    const int tid = threadIdx.x, base = k * kTile;
    for (int e = tid; e < kTile * kTile; e += 256) T[e / kTile][e % kTile] = G[(size_t)(base + e / kTile) * ncols + base + e % kTile];
    __syncthreads();
    for (int j = 0; j < kTile; ++j) {
        if (tid == 0) {
            double p = T[j][j];
            if (!(p > 0.0) || !isfinite(p)) { fail[0] = 1; p = 1.0; }
            T[j][j] = sqrt(p);
        }
        __syncthreads();
        for (int i = j + 1 + tid; i < kTile; i += 256) T[i][j] /= T[j][j];
        __syncthreads();
        for (int e = tid; e < kTile * kTile; e += 256) {
            const int i = e / kTile, c = e % kTile;
            if (c > j && i >= c) T[i][c] -= T[i][j] * T[c][j];
        }
        __syncthreads();
    }
    for (int e = tid; e < kTile * kTile; e += 256) {
        const int i = e / kTile, c = e % kTile;
        G[(size_t)(base + i) * ncols + base + c] = c <= i ? T[i][c] : 0.0;
    }
}

__global__ void __launch_bounds__(kTile) k_pg_trsm(int ncols, int k, double* __restrict__ G) {
    __shared__ double Lk[kTile][kTile + 1], X[kTile][kTile + 1];
    const int tid = threadIdx.x, base = k * kTile, I = k + 1 + blockIdx.x;
    for (int e = tid; e < kTile * kTile; e += kTile) {
        Lk[e / kTile][e % kTile] = G[(size_t)(base + e / kTile) * ncols + base + e % kTile];
        X[e / kTile][e % kTile] = G[(size_t)(I * kTile + e / kTile) * ncols + base + e % kTile];
    }
    __syncthreads();
    for (int c = 0; c < kTile; ++c) {                                  // row tid of block (I, k): X Lk^T = B
        double v = X[tid][c];
        for (int m = 0; m < c; ++m) v -= X[tid][m] * Lk[c][m];
        X[tid][c] = v / Lk[c][c];
    }
    __syncthreads();
    for (int e = tid; e < kTile * kTile; e += kTile) G[(size_t)(I * kTile + e / kTile) * ncols + base + e % kTile] = X[e / kTile][e % kTile];
}

__global__ void __launch_bounds__(256) k_pg_syrk(int ncols, int k, int nb, double* __restrict__ G) {
    int I = 0, rem = blockIdx.x;                      // tiles k < J <= I < nb
    const int m = nb - k - 1;
    while (rem > I) { rem -= I + 1; ++I; }
    const int Ib = k + 1 + I, Jb = k + 1 + rem;
    (void)m;
    __shared__ double A[kTile][kTile + 1], B[kTile][kTile + 1];
    const int tid = threadIdx.x, tr = tid / 16, tc = tid % 16, base = k * kTile;
    for (int e = tid; e < kTile * kTile; e += 256) {
        A[e / kTile][e % kTile] = G[(size_t)(Ib * kTile + e / kTile) * ncols + base + e % kTile];
        B[e / kTile][e % kTile] = G[(size_t)(Jb * kTile + e / kTile) * ncols + base + e % kTile];
    }
    __syncthreads();
    double acc[4][4] = {};
#pragma unroll 2
    for (int mm = 0; mm < kTile; ++mm) {
        double av[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { av[i] = A[4 * tr + i][mm]; bv[i] = B[4 * tc + i][mm]; }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += av[i] * bv[j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) G[(size_t)(Ib * kTile + 4 * tr + i) * ncols + Jb * kTile + 4 * tc + j] -= acc[i][j];
}

// v = Lc^-T l, l = row zc of the factor (columns 0 .. zc-1); v padded with zeros to ncols.  rhs != nullptr (refinement pass): l = Lc^-1 rhs.
__global__ void __launch_bounds__(1024) k_pg_capsolve(int ncols, int zc, const double* __restrict__ G, const double* __restrict__ rhs,
                                                      double* __restrict__ v) {
    __shared__ double l[1088];
    const int tid = threadIdx.x;
    for (int k = tid; k < ncols; k += 1024) l[k] = k < zc ? (rhs ? rhs[k] : G[(size_t)zc * ncols + k]) : 0.0;
    __syncthreads();
    if (rhs)
        for (int k = 0; k < zc; ++k) {
            if (tid == 0) l[k] /= G[(size_t)k * ncols + k];
            __syncthreads();
            const double lk = l[k];
            for (int j = k + 1 + tid; j < zc; j += 1024) l[j] -= G[(size_t)j * ncols + k] * lk;
            __syncthreads();
        }
    for (int k = zc - 1; k >= 0; --k) {
        if (tid == 0) l[k] /= G[(size_t)k * ncols + k];
        __syncthreads();
        const double vk = l[k];
        for (int j = tid; j < k; j += 1024) l[j] -= G[(size_t)k * ncols + j] * vk;
        __syncthreads();
    }
    for (int k = tid; k < ncols; k += 1024) v[k] = l[k];
}

// u(r) = W(r, zc) - sum_q W(r, q) v(q), one wave per row, fixed-order lane tree.
__global__ void __launch_bounds__(256) k_pg_wv(int m, int ncols, int zc, int nwaves, const double* __restrict__ W, const int* __restrict__ wstart,
                                               const double* __restrict__ v, double* __restrict__ u) {
    const int r = blockIdx.x * 4 + threadIdx.x / kWave, lane = threadIdx.x % kWave;
    if (r >= m) return;
    double acc = 0.0;
    for (int P = 0; P < nwaves; ++P) {
        if (r < 4 * wstart[P]) continue;
        const int q = P * kTile + lane;
        if (q < zc) acc += W[(size_t)r * ncols + q] * v[q];
    }
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) u[r] = W[(size_t)r * ncols + zc] - acc;
}

// y = L^-T u (accumulate: y += L^-T u), one wave: band rows staged in LDS from the bottom up, lane 0 runs the chain.
__global__ void __launch_bounds__(kWave) k_pg_back(int nf, int accumulate, const double* __restrict__ L, const double* __restrict__ u,
                                                   double* __restrict__ y) {
    __shared__ double rows[(kChunk + 4) * kRow], uch[kChunk * 4];
    const int lane = threadIdx.x;
    double y1[4] = {}, y2[4] = {}, y3[4] = {}, y4[4] = {};
    for (int hi = nf; hi > 0; hi -= kChunk) {
        const int lo = max(0, hi - kChunk), cnt = min(nf, hi + 4) - lo;
        __syncthreads();
        for (int k = lane; k < cnt * kRow; k += kWave) rows[k] = L[(size_t)lo * kRow + k];
        for (int k = lane; k < (hi - lo) * 4; k += kWave) uch[k] = u[4 * lo + k];
        __syncthreads();
        if (lane == 0) {
            for (int a = hi - 1; a >= lo; --a) {
                double b[4];
                for (int k = 0; k < 4; ++k) b[k] = uch[4 * (a - lo) + k];
                // - sum_d L(a+d, a)^T y_{a+d}
                for (int d = 1; d <= 4; ++d) {
                    if (a + d >= nf) continue;
                    const double* B = rows + (a + d - lo) * kRow + 16 * d;
                    const double* yy = d == 1 ? y1 : d == 2 ? y2 : d == 3 ? y3 : y4;
                    for (int k = 0; k < 4; ++k)
                        for (int m = 0; m < 4; ++m) b[k] -= B[4 * m + k] * yy[m];
                }
                const double* D = rows + (a - lo) * kRow;
                for (int k = 3; k >= 0; --k) {
                    double v = b[k];
                    for (int m = k + 1; m < 4; ++m) v -= D[4 * m + k] * b[m];
                    b[k] = v / D[5 * k];
                }
                for (int k = 0; k < 4; ++k) { y4[k] = y3[k]; y3[k] = y2[k]; y2[k] = y1[k]; y1[k] = b[k]; y[4 * a + k] = accumulate ? y[4 * a + k] + b[k] : b[k]; }
            }
        }
    }
}

// Residual of the damped scaled system at y, per free keyframe a: r_a = -g_a - (A y)_a - (lmdiag_a / radius) y_a - (U U^T y)_a.  A from the band
// rows (blocks (a, a-d) of row a and the transposed blocks (a+d, a) of rows a+d); U U^T y from the loop edges with two free ends in loop order,
// as k_pg_forward scales them.  No atomics: two calls give the same bits.
__global__ void k_pg_resid(int n, int nf, int n_loops, const Edge* __restrict__ E, const double* __restrict__ eJ, const double* __restrict__ s,
                           const double* __restrict__ A, const double* __restrict__ lmdiag, double inv_radius, const double* __restrict__ g,
                           const double* __restrict__ y, double* __restrict__ res) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= nf) return;
    double acc[4];
    for (int k = 0; k < 4; ++k) acc[k] = -g[4 * a + k] - lmdiag[4 * a + k] * inv_radius * y[4 * a + k];
    const double* row = A + (size_t)a * kRow;
    for (int d = 0; d < kBand && a - d >= 0; ++d)
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) acc[r] -= row[16 * d + 4 * r + c] * y[4 * (a - d) + c];
    for (int d = 1; d < kBand && a + d < nf; ++d) {
        const double* B = A + (size_t)(a + d) * kRow + 16 * d;
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) acc[r] -= B[4 * c + r] * y[4 * (a + d) + c];
    }
    for (int l = 0; l < n_loops; ++l) {
        const int e = 4 * n + l;
        const Edge ed = E[e];
        if (ed.a < 0 || ed.fa < 0 || ed.fb < 0 || (ed.fa != a && ed.fb != a)) continue;
        for (int rr = 0; rr < 4; ++rr) {
            double ja[4], jb[4], t = 0.0;
            for (int c = 0; c < 4; ++c) { ja[c] = eJ[32 * e + 8 * rr + c] * s[4 * ed.fa + c]; jb[c] = eJ[32 * e + 8 * rr + 4 + c] * s[4 * ed.fb + c]; }
            for (int c = 0; c < 4; ++c) t += ja[c] * y[4 * ed.fa + c] + jb[c] * y[4 * ed.fb + c];
            const double* jm = ed.fa == a ? ja : jb;
            for (int k = 0; k < 4; ++k) acc[k] -= jm[k] * t;
        }
    }
    for (int k = 0; k < 4; ++k) res[4 * a + k] = acc[k];
}

// t(q) = sum_r W(r, q) W(r, zc) for q < zc over the rows column q's wave wrote (r >= 4 wstart), one lane per column, fixed row order.
__global__ void __launch_bounds__(kWave) k_pg_wtz(int nf, int ncols, int zc, const double* __restrict__ W, const int* __restrict__ wstart,
                                                  double* __restrict__ t) {
    const int q = blockIdx.x * kWave + threadIdx.x;
    if (q >= zc) return;
    double acc = 0.0;
    for (int r = 4 * wstart[q / kTile]; r < 4 * nf; ++r) acc += W[(size_t)r * ncols + q] * W[(size_t)r * ncols + zc];
    t[q] = acc;
}

// candidate x + delta (free keyframes; yaw through NormalizeAngle), |x_c - x|^2 and |x|^2 partials over the free variables
__global__ void k_pg_step(int n, const int* __restrict__ fidx, const double* __restrict__ s, const double* __restrict__ y, const double* __restrict__ x,
                          double* __restrict__ delta, double* __restrict__ xc, double* __restrict__ part_step) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int a = fidx[i];
    if (a < 0) { for (int k = 0; k < 4; ++k) xc[4 * i + k] = x[4 * i + k]; return; }
    double st = 0.0;
    for (int k = 0; k < 4; ++k) {
        const double dk = s[4 * a + k] * y[4 * a + k];
        delta[4 * a + k] = dk;
        const double v = k == 0 ? normalize_angle(x[4 * i] + dk) : x[4 * i + k] + dk;
        xc[4 * i + k] = v;
        st += (v - x[4 * i + k]) * (v - x[4 * i + k]);
    }
    part_step[a] = st;
}

__global__ void k_pg_xnorm(int n, const int* __restrict__ fidx, const double* __restrict__ x, double* __restrict__ part) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || fidx[i] < 0) return;
    double v = 0.0;
    for (int k = 0; k < 4; ++k) v += x[4 * i + k] * x[4 * i + k];
    part[fidx[i]] = v;
}

struct RedArgs { const double* p[4]; int n[4]; int is_max[4]; };

// out[k] = sum (or max) of p[k][0 .. n[k]): strided per-thread partials, then a fixed LDS tree.  One workgroup.
__global__ void __launch_bounds__(1024) k_pg_reduce(RedArgs ra, double* __restrict__ out) {
    __shared__ double sh[1024];
    const int tid = threadIdx.x;
    for (int k = 0; k < 4; ++k) {
        if (!ra.p[k]) continue;
        double acc = 0.0;
        for (int i = tid; i < ra.n[k]; i += 1024) acc = ra.is_max[k] ? fmax(acc, ra.p[k][i]) : acc + ra.p[k][i];
        sh[tid] = acc;
        __syncthreads();
        for (int w = 512; w >= 1; w >>= 1) {
            if (tid < w) sh[tid] = ra.is_max[k] ? fmax(sh[tid], sh[tid + w]) : sh[tid] + sh[tid + w];
            __syncthreads();
        }
        if (tid == 0) out[k] = sh[0];
        __syncthreads();
    }
}

}  // namespace uvspg

using namespace uvspg;

struct uvs_pose_graph : UvsHandle {          // no call is timed: opened without events
    int max_n = 0, max_l = 0, max_cols = 0;
    // inputs
    DevBuf<double> t, q; DevBuf<int> seq, fidx, kf_of_free, ucol, wstart;
    DevBuf<uvs_pg_loop> loops;
    // state
    DevBuf<double> x, xc, pr;
    DevBuf<Edge> E;
    DevBuf<double> er, eJ, ecost, emcc;
    DevBuf<double> band, L, g, hdiag, lmdiag, s, gproj;
    DevBuf<double> W, G, v, u, y, delta, part_step, part_x;
    DevBuf<double> res, wz;                     // refinement pass: residual, W_U^T L^-1 r
    DevBuf<double> scal; DevBuf<int> fail;      // device scalars
    PinnedBuf<double> h_scal;                   // pinned: 8 doubles + fail flags
};

namespace {

inline int grid_of(int n, int b) { return (n + b - 1) / b; }

// Sizes of one problem, from the host bookkeeping of pg_setup.
struct PgPlan {
    int n = 0, nl = 0, nf = 0, nu = 0, zc = 0, ncols = 0, nwaves = 0, n_slots = 0, m = 0, n_edges = 0;
};

// Checks `p`, numbers the free keyframes, orders the loop edges with two free ends (U columns, sorted by the older end's free index),
// uploads the problem and runs k_pg_prep + k_pg_meas.  `who` prefixes the error messages.
int pg_setup(uvs_pose_graph* pg, const uvs_pg_problem* p, const char* who, PgPlan& P) {
    if (!p || p->n < 1 || p->n_loops < 0 || !p->t || !p->q || !p->sequence || !p->constant || (p->n_loops > 0 && !p->loops)) {
        pg->err = std::string(who) + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG;
    }
    const int n = p->n, nl = p->n_loops;
    if (n > pg->max_n || nl > pg->max_l) { pg->err = std::string(who) + ": problem exceeds the capacity given to uvs_pg_create"; return UVS_ERR_CAPACITY; }
    for (int l = 0; l < nl; ++l) {
        const uvs_pg_loop& L = p->loops[l];
        if (L.cur < 0 || L.cur >= n || L.old < 0 || L.old >= n || L.old >= L.cur) {
            pg->err = std::string(who) + ": loop " + std::to_string(l) + " needs 0 <= old < cur < n"; return UVS_ERR_INVALID_ARG;
        }
    }
    std::vector<int> fidx(n), kf_of_free; kf_of_free.reserve(n);
    for (int i = 0; i < n; ++i) { fidx[i] = p->constant[i] ? -1 : (int)kf_of_free.size(); if (!p->constant[i]) kf_of_free.push_back(i); }
    const int nf = (int)kf_of_free.size();
    std::vector<int> ucol;
    for (int l = 0; l < nl; ++l) if (fidx[p->loops[l].old] >= 0 && fidx[p->loops[l].cur] >= 0) ucol.push_back(4 * n + l);
    std::stable_sort(ucol.begin(), ucol.end(), [&](int a, int b) { return fidx[p->loops[a - 4 * n].old] < fidx[p->loops[b - 4 * n].old]; });
    const int nu = (int)ucol.size(), zc = 4 * nu, ncols = ((zc + 1 + kTile - 1) / kTile) * kTile, nwaves = ncols / kTile;
    std::vector<int> wstart(nwaves, nf);
    for (int q = 0; q < zc; ++q) wstart[q / kTile] = std::min(wstart[q / kTile], fidx[p->loops[ucol[q / 4] - 4 * n].old]);
    wstart[zc / kTile] = 0;                                      // the -g column starts at row 0
    int n_edges = 0;
    for (int i = 0; i < n; ++i)
        for (int j = 1; j <= 4; ++j) if (i - j >= 0 && p->sequence[i] == p->sequence[i - j] && (fidx[i] >= 0 || fidx[i - j] >= 0)) ++n_edges;
    for (int l = 0; l < nl; ++l) if (fidx[p->loops[l].old] >= 0 || fidx[p->loops[l].cur] >= 0) ++n_edges;
    P.n = n; P.nl = nl; P.nf = nf; P.nu = nu; P.zc = zc; P.ncols = ncols; P.nwaves = nwaves; P.n_slots = 4 * n + nl; P.m = 4 * nf; P.n_edges = n_edges;

    UVS_HIP(pg->err, hipSetDevice(pg->device));
    hipStream_t st = pg->st;
    UVS_HIP(pg->err, hipMemcpyAsync(pg->t, p->t, (size_t)n * 3 * 8, hipMemcpyHostToDevice, st));
    UVS_HIP(pg->err, hipMemcpyAsync(pg->q, p->q, (size_t)n * 4 * 8, hipMemcpyHostToDevice, st));
    UVS_HIP(pg->err, hipMemcpyAsync(pg->seq, p->sequence, (size_t)n * 4, hipMemcpyHostToDevice, st));
    UVS_HIP(pg->err, hipMemcpyAsync(pg->fidx, fidx.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (nf) UVS_HIP(pg->err, hipMemcpyAsync(pg->kf_of_free, kf_of_free.data(), (size_t)nf * 4, hipMemcpyHostToDevice, st));
    if (nl) UVS_HIP(pg->err, hipMemcpyAsync(pg->loops, p->loops, (size_t)nl * sizeof(uvs_pg_loop), hipMemcpyHostToDevice, st));
    if (nu) UVS_HIP(pg->err, hipMemcpyAsync(pg->ucol, ucol.data(), (size_t)nu * 4, hipMemcpyHostToDevice, st));
    UVS_HIP(pg->err, hipMemcpyAsync(pg->wstart, wstart.data(), (size_t)nwaves * 4, hipMemcpyHostToDevice, st));
    UVS_HIP(pg->err, hipMemsetAsync(pg->fail, 0, 4 * 4, st));
    k_pg_prep<<<grid_of(n, 256), 256, 0, st>>>(n, pg->t, pg->q, pg->x, pg->pr);
    k_pg_meas<<<grid_of(P.n_slots, 256), 256, 0, st>>>(n, nl, pg->t, pg->q, pg->seq, pg->fidx, pg->x, pg->pr, pg->loops, pg->E);
    // the host vectors above go out of scope: the copies must have read them
    UVS_HIP(pg->err, hipStreamSynchronize(st));
    return UVS_OK;
}

// Fixed-order reduction of up to four partial arrays into h_scal[0..3]; the fail flags into h_scal + 8.  Synchronizes the stream.
int pg_reduce(uvs_pose_graph* pg, RedArgs ra) {
    hipStream_t st = pg->st;
    k_pg_reduce<<<1, 1024, 0, st>>>(ra, pg->scal);
    UVS_HIP(pg->err, hipMemcpyAsync(pg->h_scal, pg->scal, 4 * 8, hipMemcpyDeviceToHost, st));
    UVS_HIP(pg->err, hipMemcpyAsync(pg->h_scal + 8, pg->fail, 4 * 4, hipMemcpyDeviceToHost, st));
    UVS_HIP(pg->err, hipStreamSynchronize(st));
    return UVS_OK;
}

// Linearize at x: h_scal = {cost, gradient max norm, |x|^2}.  first: the Jacobi scaling from this Jacobian.
int pg_linearize(uvs_pose_graph* pg, const PgPlan& P, bool first) {
    hipStream_t st = pg->st;
    const int n = P.n, nf = P.nf, m = P.m, n_slots = P.n_slots;
    k_pg_lin<0><<<grid_of(n_slots, 256), 256, 0, st>>>(n_slots, 4 * n, pg->E, pg->x, nullptr, pg->er, pg->eJ, pg->ecost, nullptr);
    if (nf) {
        k_pg_assemble<<<grid_of(nf, 128), 128, 0, st>>>(n, nf, P.nl, pg->kf_of_free, pg->fidx, pg->E, pg->er, pg->eJ, pg->x, pg->band, pg->g, pg->hdiag, pg->gproj);
        if (first) k_pg_jacobi<<<grid_of(m, 256), 256, 0, st>>>(m, pg->hdiag, pg->s);
        k_pg_scale<<<grid_of(nf, 256), 256, 0, st>>>(nf, pg->s, pg->band, pg->g, pg->hdiag, pg->lmdiag, kMinDiag, kMaxDiag);
        k_pg_xnorm<<<grid_of(n, 256), 256, 0, st>>>(n, pg->fidx, pg->x, pg->part_x);
    }
    RedArgs ra = {{pg->ecost, nf ? pg->gproj : nullptr, nf ? pg->part_x : nullptr, nullptr}, {n_slots, nf, nf, 0}, {0, 1, 0, 0}};
    return pg_reduce(pg, ra);
}

// The damped scaled system (A + U U^T + diag(lmdiag) / radius) y = -g -> pg->y (nf > 0); fail flags on the device.  Asynchronous.
int pg_solve(uvs_pose_graph* pg, const PgPlan& P, double radius) {
    hipStream_t st = pg->st;
    const int nf = P.nf, nu = P.nu, zc = P.zc, ncols = P.ncols, nwaves = P.nwaves, m = P.m;
    UVS_HIP(pg->err, hipMemsetAsync(pg->fail, 0, 4, st));
    k_pg_factor<<<1, kWave, 0, st>>>(nf, pg->band, pg->lmdiag, 1.0 / radius, pg->L, pg->fail);
    k_pg_forward<<<nwaves, kWave, 0, st>>>(nf, ncols, nu, 0, 0, pg->L, pg->ucol, pg->E, pg->eJ, pg->s, pg->g, -1.0, pg->wstart, pg->W);
    if (nu) {
        k_pg_gram<<<nwaves * (nwaves + 1) / 2, 256, 0, st>>>(nf, ncols, pg->W, pg->wstart, pg->G);
        for (int k = 0; k < nwaves; ++k) {
            k_pg_potrf<<<1, 256, 0, st>>>(ncols, k, pg->G, pg->fail + 1);
            const int rest = nwaves - k - 1;
            if (rest > 0) {
                k_pg_trsm<<<rest, kTile, 0, st>>>(ncols, k, pg->G);
                k_pg_syrk<<<rest * (rest + 1) / 2, 256, 0, st>>>(ncols, k, nwaves, pg->G);
            }
        }
        k_pg_capsolve<<<1, 1024, 0, st>>>(ncols, zc, pg->G, nullptr, pg->v);
    } else {
        UVS_HIP(pg->err, hipMemsetAsync(pg->v, 0, (size_t)ncols * 8, st));
    }
    k_pg_wv<<<grid_of(m, 4), 256, 0, st>>>(m, ncols, zc, nwaves, pg->W, pg->wstart, pg->v, pg->u);
    k_pg_back<<<1, kWave, 0, st>>>(nf, 0, pg->L, pg->u, pg->y);
    if (UVS_PG_REFINE && nu) {       // y += (A + U U^T)^-1 r with the same L and capacitance factor, r = the FP64 residual at y
        k_pg_resid<<<grid_of(nf, 128), 128, 0, st>>>(P.n, nf, P.nl, pg->E, pg->eJ, pg->s, pg->band, pg->lmdiag, 1.0 / radius, pg->g, pg->y, pg->res);
        k_pg_forward<<<1, kWave, 0, st>>>(nf, ncols, nu, zc / kTile, 1, pg->L, pg->ucol, pg->E, pg->eJ, pg->s, pg->res, 1.0, pg->wstart, pg->W);
        k_pg_wtz<<<grid_of(zc, kWave), kWave, 0, st>>>(nf, ncols, zc, pg->W, pg->wstart, pg->wz);
        k_pg_capsolve<<<1, 1024, 0, st>>>(ncols, zc, pg->G, pg->wz, pg->v);
        k_pg_wv<<<grid_of(m, 4), 256, 0, st>>>(m, ncols, zc, nwaves, pg->W, pg->wstart, pg->v, pg->u);
        k_pg_back<<<1, kWave, 0, st>>>(nf, 1, pg->L, pg->u, pg->y);
    }
    return UVS_OK;
}

}  // namespace

extern "C" {

int uvs_pg_create(int device, int max_keyframes, int max_loops, uvs_pose_graph** out) {
    if (!out || max_keyframes < 1 || max_loops < 0) return UVS_ERR_INVALID_ARG;
    *out = nullptr;
    if (max_keyframes > UVS_PG_MAX_KEYFRAMES || max_loops > UVS_PG_MAX_LOOPS) return UVS_ERR_CAPACITY;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return UVS_ERR_NO_DEVICE;
    uvs_pose_graph* pg = new uvs_pose_graph();
    pg->max_n = max_keyframes; pg->max_l = max_loops;
    pg->max_cols = ((4 * max_loops + 1 + kTile - 1) / kTile) * kTile;
    int rc = pg->open(device, false);
    const size_t N = max_keyframes, Lm = std::max(1, max_loops), ES = 4 * N + Lm, C = pg->max_cols, M = 4 * N;
    const auto al = [&](auto& buf, size_t bytes) { if (rc == UVS_OK) rc = buf.ensure(bytes, pg->err); };
    al(pg->t, N * 3 * 8); al(pg->q, N * 4 * 8); al(pg->seq, N * 4); al(pg->fidx, N * 4);
    al(pg->kf_of_free, N * 4); al(pg->ucol, Lm * 4); al(pg->wstart, (C / kTile) * 4);
    al(pg->loops, Lm * sizeof(uvs_pg_loop));
    al(pg->x, N * 4 * 8); al(pg->xc, N * 4 * 8); al(pg->pr, N * 2 * 8); al(pg->E, ES * sizeof(Edge));
    al(pg->er, ES * 4 * 8); al(pg->eJ, ES * 32 * 8); al(pg->ecost, ES * 8); al(pg->emcc, ES * 8);
    al(pg->band, N * kRow * 8); al(pg->L, N * kRow * 8); al(pg->g, M * 8); al(pg->hdiag, M * 8);
    al(pg->lmdiag, M * 8); al(pg->s, M * 8); al(pg->gproj, N * 8);
    al(pg->W, M * C * 8); al(pg->G, C * C * 8); al(pg->v, C * 8); al(pg->u, M * 8); al(pg->y, M * 8);
    al(pg->delta, M * 8); al(pg->part_step, N * 8); al(pg->part_x, N * 8); al(pg->res, M * 8); al(pg->wz, C * 8);
    al(pg->scal, 16 * 8); al(pg->fail, 4 * 4);
    al(pg->h_scal, 32 * 8);
    if (rc != UVS_OK) { uvs_pg_destroy(pg); return rc; }
    *out = pg;
    return UVS_OK;
}

void uvs_pg_destroy(uvs_pose_graph* pg) { if (pg) { pg->close(); delete pg; } }

const char* uvs_pg_last_error(const uvs_pose_graph* pg) { return pg ? pg->err.c_str() : "null pose graph"; }

int uvs_pg_optimize(uvs_pose_graph* pg, const uvs_pg_problem* p, double* out_yaw_t, uvs_pg_report* rep) {
    if (!pg) return UVS_ERR_INVALID_ARG;
    pg->err.clear();
    if (!out_yaw_t) { pg->err = "uvs_pg_optimize: null pointer or bad count"; return UVS_ERR_INVALID_ARG; }
    PgPlan P;
    int rc = pg_setup(pg, p, "uvs_pg_optimize", P);
    if (rc) return rc;
    const int n = P.n, nf = P.nf, n_slots = P.n_slots;
    hipStream_t st = pg->st;
    uvs_pg_report R; std::memset(&R, 0, sizeof(R));
    R.n_free = nf; R.n_edges = P.n_edges; R.n_loop_columns = P.zc;

    // Ceres' defaults, max_num_iterations = 5 (pose_graph.cpp:433)
    const int max_iter = 5;
    const double init_radius = 1e4, max_radius = 1e16, min_radius = 1e-32, min_rel_dec = 1e-3;
    const double ftol = 1e-6, gtol = 1e-10, ptol = 1e-8;
    const int max_invalid = 5;

    if ((rc = pg_linearize(pg, P, true))) return rc;
    double cost = pg->h_scal[0], gmax = pg->h_scal[1], x_norm = std::sqrt(pg->h_scal[2]);
    R.initial_cost = cost; R.cost[0] = cost; R.radius[0] = init_radius; R.accepted[0] = 1;
    double radius = init_radius, decrease_factor = 2.0;
    int it = 0, invalid = 0, term = UVS_TERM_NO_CONVERGENCE, num_successful = 0;
    if (!std::isfinite(cost)) { R.status = UVS_ERR_NUMERIC; term = UVS_TERM_NUMERIC_FAILURE; }
    else if (nf == 0) term = UVS_TERM_FUNCTION_TOL;        // Ceres: no non-constant parameter blocks -> converged without an iteration
    else {
        while (true) {
            if (it >= max_iter) { term = UVS_TERM_NO_CONVERGENCE; break; }
            if (gmax <= gtol) { term = UVS_TERM_GRADIENT_TOL; break; }
            if (radius <= min_radius) { term = UVS_TERM_MIN_RADIUS; break; }
            ++it;
            if ((rc = pg_solve(pg, P, radius))) return rc;       // damped system -> y (scaled step)
            k_pg_step<<<grid_of(n, 256), 256, 0, st>>>(n, pg->fidx, pg->s, pg->y, pg->x, pg->delta, pg->xc, pg->part_step);
            k_pg_lin<1><<<grid_of(n_slots, 256), 256, 0, st>>>(n_slots, 4 * n, pg->E, pg->xc, pg->delta, pg->er, pg->eJ, pg->ecost, pg->emcc);
            RedArgs ra = {{pg->ecost, pg->emcc, pg->part_step, nullptr}, {n_slots, n_slots, nf, 0}, {0, 0, 0, 0}};
            if ((rc = pg_reduce(pg, ra))) return rc;
            const double cand_raw = pg->h_scal[0], mcc = pg->h_scal[1], step_norm = std::sqrt(pg->h_scal[2]);
            const int* hf = reinterpret_cast<const int*>(pg->h_scal + 8);
            const bool solve_ok = hf[0] == 0 && hf[1] == 0;
            R.model_cost_change[it] = mcc;
            if (!solve_ok || !std::isfinite(mcc) || !(mcc > 0.0) || !std::isfinite(step_norm)) {     // invalid step
                ++invalid;
                radius /= decrease_factor; decrease_factor *= 2.0;
                R.accepted[it] = -1; R.radius[it] = radius; R.cost[it] = cost; R.candidate_cost[it] = cost;
                if (invalid >= max_invalid) { term = UVS_TERM_INVALID_STEPS; break; }
                continue;
            }
            invalid = 0;
            const double cand = std::isfinite(cand_raw) ? cand_raw : 1.7976931348623157e308;
            R.candidate_cost[it] = cand;
            const double rho = (cost - cand) / mcc;
            const bool successful = rho > min_rel_dec;
            int stop = -1;
            if (step_norm <= ptol * (x_norm + ptol)) stop = UVS_TERM_PARAMETER_TOL;
            else if (std::fabs(cost - cand) <= ftol * cost) stop = UVS_TERM_FUNCTION_TOL;
            if (stop >= 0) { R.accepted[it] = 0; R.radius[it] = radius; R.cost[it] = cost; term = stop; break; }
            if (successful) {
                std::swap(pg->x, pg->xc);
                if ((rc = pg_linearize(pg, P, false))) return rc;
                cost = pg->h_scal[0]; gmax = pg->h_scal[1]; x_norm = std::sqrt(pg->h_scal[2]);
                radius = std::min(max_radius, radius / std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * rho - 1.0, 3)));
                decrease_factor = 2.0;
                ++num_successful;
                R.accepted[it] = 1;
            } else {
                radius /= decrease_factor; decrease_factor *= 2.0;
                R.accepted[it] = 0;
            }
            R.radius[it] = radius; R.cost[it] = cost;
        }
    }
    R.num_iterations = it; R.num_successful = num_successful; R.termination = term; R.final_cost = cost;
    UVS_HIP(pg->err, hipMemcpyAsync(out_yaw_t, pg->x, (size_t)n * 4 * 8, hipMemcpyDeviceToHost, st));
    UVS_HIP(pg->err, hipStreamSynchronize(st));
    if (rep) *rep = R;
    return R.status;
}

int uvs_pg_debug_step(uvs_pose_graph* pg, const uvs_pg_problem* p, double radius, double* delta, double* scal) {
    if (!pg) return UVS_ERR_INVALID_ARG;
    pg->err.clear();
    if (!delta || !scal) { pg->err = "uvs_pg_debug_step: null pointer or bad count"; return UVS_ERR_INVALID_ARG; }
    if (!std::isfinite(radius) || !(radius > 0.0)) { pg->err = "uvs_pg_debug_step: radius must be finite and > 0"; return UVS_ERR_INVALID_ARG; }
    PgPlan P;
    int rc = pg_setup(pg, p, "uvs_pg_debug_step", P);
    if (rc) return rc;
    if ((rc = pg_linearize(pg, P, true))) return rc;
    for (int k = 0; k < UVS_PG_DEBUG_SCAL_LEN; ++k) scal[k] = 0.0;
    scal[2] = P.zc; scal[3] = P.nf;
    if (P.nf == 0) return UVS_OK;
    hipStream_t st = pg->st;
    if ((rc = pg_solve(pg, P, radius))) return rc;
    k_pg_step<<<grid_of(P.n, 256), 256, 0, st>>>(P.n, pg->fidx, pg->s, pg->y, pg->x, pg->delta, pg->xc, pg->part_step);
    UVS_HIP(pg->err, hipMemcpyAsync(delta, pg->delta, (size_t)P.m * 8, hipMemcpyDeviceToHost, st));
    UVS_HIP(pg->err, hipMemcpyAsync(pg->h_scal + 8, pg->fail, 4 * 4, hipMemcpyDeviceToHost, st));
    UVS_HIP(pg->err, hipStreamSynchronize(st));
    const int* hf = reinterpret_cast<const int*>(pg->h_scal + 8);
    scal[0] = hf[0]; scal[1] = hf[1];
    return UVS_OK;
}

}  // extern "C"
