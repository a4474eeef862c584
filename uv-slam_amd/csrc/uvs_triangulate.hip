// uvs_triangulate.hip -- the state a solve starts from, for whole batches of landmarks at once (reference vins_estimator/src/feature_manager.cpp:
// triangulate :427-481, triangulateLine :504-589 with calcPluckerLine :827-902, the validity rule of setLineOrtho :352-416, the re-anchoring of
// removeBackShiftDepth :627-634) behind the uvs_tri_* calls of include/uvs_solver.h.  FP64, gfx950, one stream per handle, one lane per landmark.
//
// No kernel reads another landmark's data and no lane's arithmetic depends on its neighbours, so a landmark gives the same bits alone, in a
// batch of one window or in a batch of many.  Kernels of one uvs_tri_triangulate call, in stream order:
//   k_tri_cameras  thread per (window, frame): the camera pose R_wc = R(q_f) R(q_ex), t_wc = R(q_f) t_ex + p_f as 12 doubles.  A window's 11 x 12
//                  doubles are computed once and read by every landmark of the window through L2.
//   k_tri_points   lane per point.  For view k of the track (frame start + k, the start frame's own view included) the camera relative to the
//                  start camera, P = [R^T | -R^T t], f = obs / |obs|, and the two rows f0 P.row(2) - f2 P.row(0), f1 P.row(2) - f2 P.row(1) of the
//                  reference's svd_A.  The rows are never stored: each goes through four Givens rotations into the 4 x 4 upper triangle T of
//                  svd_A = Q T (10 doubles).  The right singular vectors of T are those of svd_A; they come from a one-sided Jacobi SVD of T
//                  (Hestenes: columns rotated in the fixed order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) until a sweep rotates nothing, at most
//                  kMaxSweeps sweeps; both routines live in uvs_svd_dev.h, which uvs_relative_pose.hip shares).  Both steps are orthogonal
//                  transformations of svd_A itself -- svd_A^T svd_A is never formed, so the condition number is not squared (DESIGN.md
//                  3.19).  depth = V[2] / V[3] of the column of the smallest norm.
//   k_tri_lines    lane per line: the two back-projected planes, the Pluecker line in the world, its orthonormal form.
// uvs_tri_check_lines runs k_tri_cameras and k_tri_check (lane per line), uvs_tri_shift_depth runs k_tri_shift (lane per point).
//
// Everything a lane holds lives in registers: the small matrices are fixed-size arrays that only fully unrolled loops index, no LDS, no
// atomics, no scratch (build() holds k_tri_* to 0 bytes per lane).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/uvs_solver.h"
#include "uvs_handle.h"
#include "uvs_svd_dev.h"

namespace uvstri {

constexpr int kNF = UVS_NUM_FRAMES;
constexpr int kThreads = 64;               // one wave per workgroup: 38 400 points are 600 workgroups over 256 compute units
constexpr double kPi = 3.14159265358979323846;

struct Cam { double R[3][3], t[3]; };      // camera -> world

__device__ __forceinline__ void quat_R(const double* q, double R[3][3]) {      // Eigen's Quaterniond(w, x, y, z).toRotationMatrix(), q = (x, y, z, w)
    const double qx = q[0], qy = q[1], qz = q[2], qw = q[3];
    const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz, twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx,
                 tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
    R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
}

__device__ __forceinline__ Cam load_cam(const double* __restrict__ cams, int window, int frame) {
    const double* c = cams + 12 * ((size_t)window * kNF + frame);
    Cam C;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) C.R[r][k] = c[3 * r + k];
        C.t[r] = c[9 + r];
    }
    return C;
}

__device__ __forceinline__ void cross3(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double norm3(const double a[3]) { return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
__device__ __forceinline__ void mul3(const double R[3][3], const double a[3], double o[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = R[r][0] * a[0] + R[r][1] * a[1] + R[r][2] * a[2];
}
__device__ __forceinline__ void mulT3(const double R[3][3], const double a[3], double o[3]) {      // R^T a
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = R[0][r] * a[0] + R[1][r] * a[1] + R[2][r] * a[2];
}
__device__ __forceinline__ bool positive_finite(double x) { return x > 0.0 && x <= 1.7976931348623157e308; }

// ---- camera poses of every (window, frame)
__global__ void __launch_bounds__(kThreads) k_tri_cameras(const double* __restrict__ pose, const double* __restrict__ ex_pose, int n_cams,
                                                        double* __restrict__ cams) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_cams) return;
    const double* p = pose + 7 * (size_t)i;
    const double* e = ex_pose + 7 * (size_t)(i / kNF);
    double Rb[3][3], Ri[3][3];
    quat_R(p + 3, Rb); quat_R(e + 3, Ri);
    double* o = cams + 12 * (size_t)i;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[3 * r + c] = Rb[r][0] * Ri[0][c] + Rb[r][1] * Ri[1][c] + Rb[r][2] * Ri[2][c];
        o[9 + r] = (Rb[r][0] * e[0] + Rb[r][1] * e[1] + Rb[r][2] * e[2]) + p[r];
    }
}

// ---- points: the DLT of feature_manager.cpp:437-478
__global__ void __launch_bounds__(kThreads) k_tri_points(const double* __restrict__ cams, const int32_t* __restrict__ pt_window,
                                                       const int32_t* __restrict__ pt_start, const int32_t* __restrict__ pt_obs_begin,
                                                       const double* __restrict__ pt_obs, int n_points, double init_depth,
                                                       double* __restrict__ depth, int32_t* __restrict__ flag) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_points) return;
    const int w = pt_window[i], s = pt_start[i], o0 = pt_obs_begin[i], nv = pt_obs_begin[i + 1] - o0;
    const Cam C0 = load_cam(cams, w, s);
    double T[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) T[r][c] = 0.0;
    for (int k = 0; k < nv; ++k) {
        const Cam C1 = load_cam(cams, w, s + k);
        const double dt[3] = {C1.t[0] - C0.t[0], C1.t[1] - C0.t[1], C1.t[2] - C0.t[2]};
        double t[3];
        mulT3(C0.R, dt, t);                                                     // t = R0^T (t1 - t0)
        double P[3][4];                                                         // [R^T | -R^T t] with R = R0^T R1
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) P[r][c] = C1.R[0][r] * C0.R[0][c] + C1.R[1][r] * C0.R[1][c] + C1.R[2][r] * C0.R[2][c];
#pragma unroll
        for (int r = 0; r < 3; ++r) P[r][3] = -(P[r][0] * t[0] + P[r][1] * t[1] + P[r][2] * t[2]);
        const double* ob = pt_obs + 3 * (size_t)(o0 + k);
        const double f[3] = {ob[0], ob[1], ob[2]};
        const double n = norm3(f), f0 = f[0] / n, f1 = f[1] / n, f2 = f[2] / n;
        double x0[4], x1[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) { x0[c] = f0 * P[2][c] - f2 * P[0][c]; x1[c] = f1 * P[2][c] - f2 * P[1][c]; }
        uvssvd::givens_row(T, x0);
        uvssvd::givens_row(T, x1);
    }
    // one-sided Jacobi on the columns of T: T V = U Sigma (uvs_svd_dev.h)
    double V[4][4], q[4];
    UVS_JACOBI_COLUMNS(4, T, V);
    uvssvd::smallest_column(T, V, q);
    const double v2 = q[2], v3 = q[3];
    double d = v2 / v3;
    int fl = 0;
    if (!(fabs(d) <= 1.7976931348623157e308)) { fl = 2; d = init_depth; }      // not finite: the reference lets it through (stated deviation)
    else if (d < 0.1) { fl = 1; d = init_depth; }
    depth[i] = d; flag[i] = fl;
}

// Eigen 3.3 Matrix3d::eulerAngles(0, 1, 2) of U, the branch with the first angle in [0, pi]
__device__ __forceinline__ void euler_xyz(const double U[3][3], double out[3]) {
    double r0 = atan2(U[1][2], U[2][2]), r1;
    const double c2 = sqrt(U[0][0] * U[0][0] + U[0][1] * U[0][1]);
    if (r0 > 0.0) { r0 -= kPi; r1 = atan2(-U[0][2], -c2); } else r1 = atan2(-U[0][2], c2);
    const double s1 = sin(r0), c1 = cos(r0);
    const double r2 = atan2(s1 * U[2][0] - c1 * U[1][0], c1 * U[1][1] - s1 * U[2][1]);
    out[0] = -r0; out[1] = -r1; out[2] = -r2;
}

// ---- lines: feature_manager.cpp:525-585
__global__ void __launch_bounds__(kThreads) k_tri_lines(const double* __restrict__ cams, const int32_t* __restrict__ ln_window,
                                                      const int32_t* __restrict__ ln_fi, const int32_t* __restrict__ ln_fj,
                                                      const double* __restrict__ sp_i, const double* __restrict__ ep_i,
                                                      const double* __restrict__ sp_j, const double* __restrict__ ep_j, int n_lines,
                                                      double* __restrict__ orth, int32_t* __restrict__ flag) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_lines) return;
    const int w = ln_window[i];
    const Cam L = load_cam(cams, w, ln_fi[i]), Rg = load_cam(cams, w, ln_fj[i]);
    const double spi[3] = {sp_i[3 * (size_t)i], sp_i[3 * (size_t)i + 1], sp_i[3 * (size_t)i + 2]};
    const double epi[3] = {ep_i[3 * (size_t)i], ep_i[3 * (size_t)i + 1], ep_i[3 * (size_t)i + 2]};
    const double spj[3] = {sp_j[3 * (size_t)i], sp_j[3 * (size_t)i + 1], sp_j[3 * (size_t)i + 2]};
    const double epj[3] = {ep_j[3 * (size_t)i], ep_j[3 * (size_t)i + 1], ep_j[3 * (size_t)i + 2]};
    double Rrel[3][3];                                                          // R_left^T R_right
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Rrel[r][c] = L.R[0][r] * Rg.R[0][c] + L.R[1][r] * Rg.R[1][c] + L.R[2][r] * Rg.R[2][c];
    const double dt[3] = {Rg.t[0] - L.t[0], Rg.t[1] - L.t[1], Rg.t[2] - L.t[2]};
    double trel[3], rs[3], re[3], a[3], b[3], dl[3], nl[3], dw[3], nw[3], txd[3], nxd[3];
    mulT3(L.R, dt, trel);
    mul3(Rrel, spj, rs); mul3(Rrel, epj, re);
    cross3(spi, epi, a); cross3(rs, re, b);
    const double beta = -(b[0] * trel[0] + b[1] * trel[1] + b[2] * trel[2]);
    cross3(b, a, dl);
#pragma unroll
    for (int k = 0; k < 3; ++k) nl[k] = a[k] * beta;                            // alpha = -a . 0 = 0
    mul3(L.R, dl, dw);
    mul3(L.R, nl, nw);
    cross3(L.t, dw, txd);
#pragma unroll
    for (int k = 0; k < 3; ++k) nw[k] += txd[k];
    cross3(nw, dw, nxd);
    const double nn = norm3(nw), nd = norm3(dw), nx = norm3(nxd);
    double out[4] = {0.0, 0.0, 0.0, 0.0};
    int fl = 2;
    if (positive_finite(nn) && positive_finite(nd) && positive_finite(nx)) {
        double U[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r) { U[r][0] = nw[r] / nn; U[r][1] = dw[r] / nd; U[r][2] = nxd[r] / nx; }
        euler_xyz(U, out);
        out[3] = atan2(nd, nn);
        fl = 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) orth[4 * (size_t)i + k] = out[k];
    flag[i] = fl;
}

// ---- the decision of setLineOrtho (feature_manager.cpp:352-416) with the OLD parameters
__global__ void __launch_bounds__(kThreads) k_tri_check(const double* __restrict__ cams, const int32_t* __restrict__ ln_window,
                                                      const int32_t* __restrict__ ln_start, const double* __restrict__ sp0,
                                                      const double* __restrict__ ep0, const double* __restrict__ orth_old, int n_lines,
                                                      int32_t* __restrict__ flag) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_lines) return;
    const Cam Cw = load_cam(cams, ln_window[i], ln_start[i]);
    const double* o = orth_old + 4 * (size_t)i;
    const double sa = sin(o[0]), ca = cos(o[0]), sb = sin(o[1]), cb = cos(o[1]), sc = sin(o[2]), cc = cos(o[2]), cphi = cos(o[3]), sphi = sin(o[3]);
    const double nw[3] = {cb * cc * cphi, (sa * sb * cc + ca * sc) * cphi, (-ca * sb * cc + sa * sc) * cphi};
    const double dw[3] = {-cb * sc * sphi, (-sa * sb * sc + ca * cc) * sphi, (ca * sb * sc + sa * cc) * sphi};
    double tcw[3], dc[3], nc[3], txd[3];
    mulT3(Cw.R, Cw.t, tcw);
#pragma unroll
    for (int k = 0; k < 3; ++k) tcw[k] = -tcw[k];
    mulT3(Cw.R, dw, dc); mulT3(Cw.R, nw, nc);
    cross3(tcw, dc, txd);
#pragma unroll
    for (int k = 0; k < 3; ++k) nc[k] += txd[k];
    const double sp[3] = {sp0[3 * (size_t)i], sp0[3 * (size_t)i + 1], sp0[3 * (size_t)i + 2]};
    const double ep[3] = {ep0[3 * (size_t)i], ep0[3 * (size_t)i + 1], ep0[3 * (size_t)i + 2]};
    const double slope = -(ep[0] - sp[0]) / (ep[1] - sp[1]);
    const double sp2[3] = {sp[0] + 1.0, slope + sp[1], 1.0}, ep2[3] = {ep[0] + 1.0, slope + ep[1], 1.0};
    double pis[3], pie[3], Ds[3], De[3];
    cross3(sp, sp2, pis); cross3(ep, ep2, pie);
    cross3(nc, pis, Ds); cross3(nc, pie, De);
    const double ws = -(dc[0] * pis[0] + dc[1] * pis[1] + dc[2] * pis[2]), we = -(dc[0] * pie[0] + dc[1] * pie[1] + dc[2] * pie[2]);
    flag[i] = (Ds[2] / ws < 0.0 || De[2] / we < 0.0) ? 2 : 1;
}

struct ShiftArgs { double mR[3][3], mP[3], nR[3][3], nP[3], init_depth; };

// ---- the re-anchoring of removeBackShiftDepth (feature_manager.cpp:627-634)
__global__ void __launch_bounds__(kThreads) k_tri_shift(ShiftArgs A, const double* __restrict__ uv0, const double* __restrict__ depth, int n_points,
                                                      double* __restrict__ depth_out, int32_t* __restrict__ flag) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_points) return;
    const double d = depth[i];
    const double p[3] = {uv0[3 * (size_t)i] * d, uv0[3 * (size_t)i + 1] * d, uv0[3 * (size_t)i + 2] * d};
    double wv[3];
    mul3(A.mR, p, wv);
#pragma unroll
    for (int k = 0; k < 3; ++k) wv[k] = (wv[k] + A.mP[k]) - A.nP[k];
    const double z = A.nR[0][2] * wv[0] + A.nR[1][2] * wv[1] + A.nR[2][2] * wv[2];
    const bool ok = z > 0.0;
    depth_out[i] = ok ? z : A.init_depth;
    flag[i] = ok ? 0 : 1;
}

}  // namespace uvstri

using namespace uvstri;

struct uvs_tri : UvsHandle {
    int max_windows = 0, max_points = 0, max_point_obs = 0, max_lines = 0;
    double init_depth = 5.0;                    // INIT_DEPTH of the reference's configurations; uvs_tri_set_init_depth
    float device_ms = 0.f;                      // uvs_tri_last_device_ms
    DevBuf<char> d_in, d_out;                   // packed inputs / outputs of one call
    PinnedBuf<char> h_in, h_out;                // pinned staging
    DevBuf<double> d_cams;                      // [windows][11][12]
};

namespace {

inline int blocks_for(int n) { return (n + kThreads - 1) / kThreads; }

// pose / ex_pose of n_windows windows at the head of the packed input; the offsets of both
struct FrameOffsets { size_t pose, ex; };
FrameOffsets take_frames(UvsArena& A, int n_windows) {
    FrameOffsets o;
    o.pose = A.take((size_t)n_windows * kNF * 7 * 8); o.ex = A.take((size_t)n_windows * 7 * 8);
    return o;
}

int fail(uvs_tri* t, const std::string& msg) { t->err = msg; return UVS_ERR_INVALID_ARG; }

// the checks every call shares on its frames and on a landmark's window index
int check_frames(uvs_tri* t, const char* fn, int n_windows, const double* pose, const double* ex_pose) {
    if (n_windows < 1 || !pose || !ex_pose) return fail(t, std::string(fn) + ": null pointer or n_windows < 1");
    if (n_windows > t->max_windows) return fail(t, std::string(fn) + ": more windows than the capacity given to uvs_tri_create");
    return UVS_OK;
}

}  // namespace

extern "C" {

int uvs_tri_create(int device, int max_windows, int max_points, int max_point_obs, int max_lines, uvs_tri** out) {
    if (!out || max_windows < 1 || max_points < 1 || max_point_obs < 2 || max_lines < 1) return UVS_ERR_INVALID_ARG;
    *out = nullptr;
    if (max_windows > UVS_TRI_MAX_WINDOWS || max_points > UVS_TRI_MAX_LANDMARKS || max_lines > UVS_TRI_MAX_LANDMARKS ||
        max_point_obs > UVS_TRI_MAX_LANDMARKS * UVS_NUM_FRAMES) return UVS_ERR_CAPACITY;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return UVS_ERR_NO_DEVICE;
    uvs_tri* h = new uvs_tri();
    h->max_windows = max_windows; h->max_points = max_points; h->max_point_obs = max_point_obs; h->max_lines = max_lines;
    // the largest packed input is uvs_tri_triangulate's; its outputs are the largest too
    UvsArena in; take_frames(in, max_windows);
    in.take((size_t)max_points * 4); in.take((size_t)max_points * 4); in.take(((size_t)max_points + 1) * 4); in.take((size_t)max_point_obs * 24);
    for (int k = 0; k < 3; ++k) in.take((size_t)max_lines * 4);
    for (int k = 0; k < 4; ++k) in.take((size_t)max_lines * 24);
    in.take((size_t)max_lines * 32);                                            // uvs_tri_check_lines' orth_old (its other arrays are a subset of the above)
    UvsArena sh; sh.take((size_t)max_points * 24); sh.take((size_t)max_points * 8);      // uvs_tri_shift_depth's uv0 and depth
    if (sh.o > in.o) in.o = sh.o;
    UvsArena o; o.take((size_t)max_points * 8); o.take((size_t)max_lines * 32); o.take((size_t)max_points * 4); o.take((size_t)max_lines * 4);
    int rc = h->open(device);
    if (rc == UVS_OK && (rc = h->d_in.ensure(in.o, h->err)) == UVS_OK && (rc = h->h_in.ensure(in.o, h->err)) == UVS_OK &&
        (rc = h->d_out.ensure(o.o, h->err)) == UVS_OK && (rc = h->h_out.ensure(o.o, h->err)) == UVS_OK)
        rc = h->d_cams.ensure((size_t)max_windows * kNF * 12 * 8, h->err);
    if (rc != UVS_OK) { uvs_tri_destroy(h); return rc; }
    *out = h;
    return UVS_OK;
}

void uvs_tri_destroy(uvs_tri* t) { if (t) { t->close(); delete t; } }

const char* uvs_tri_last_error(const uvs_tri* t) { return t ? t->err.c_str() : "null triangulation handle"; }

double uvs_tri_last_device_ms(const uvs_tri* t) { return t ? (double)t->device_ms : 0.0; }

int uvs_tri_set_init_depth(uvs_tri* t, double init_depth) {
    if (!t) return UVS_ERR_INVALID_ARG;
    t->err.clear();
    if (!(init_depth > 0.0) || !std::isfinite(init_depth)) return fail(t, "uvs_tri_set_init_depth: init_depth must be positive and finite");
    t->init_depth = init_depth;
    return UVS_OK;
}

int uvs_tri_triangulate(uvs_tri* t, const uvs_tri_batch* b, double init_depth, double* depth, int32_t* pt_flag, double* orth, int32_t* ln_flag) {
    if (!t) return UVS_ERR_INVALID_ARG;
    t->err.clear();
    const char* fn = "uvs_tri_triangulate";
    if (!b) return fail(t, std::string(fn) + ": null batch");
    const int np = b->n_points, nl = b->n_lines, nw = b->n_windows;
    if (np < 0 || nl < 0) return fail(t, std::string(fn) + ": negative count");
    if (np == 0 && nl == 0) return UVS_OK;                                      // nothing to do, nothing launched
    int rc = check_frames(t, fn, nw, b->pose, b->ex_pose);
    if (rc != UVS_OK) return rc;
    if (!(init_depth > 0.0) || !std::isfinite(init_depth)) return fail(t, std::string(fn) + ": init_depth must be positive and finite");
    if (np > t->max_points || nl > t->max_lines) return fail(t, std::string(fn) + ": more landmarks than the capacity given to uvs_tri_create");
    int n_obs = 0;
    if (np > 0) {
        if (!b->pt_window || !b->pt_start || !b->pt_obs_begin || !b->pt_obs || !depth || !pt_flag) return fail(t, std::string(fn) + ": null point array");
        if (b->pt_obs_begin[0] != 0) return fail(t, std::string(fn) + ": pt_obs_begin[0] must be 0");
        for (int k = 0; k < np; ++k) {
            const long long views = (long long)b->pt_obs_begin[k + 1] - b->pt_obs_begin[k];
            const int s = b->pt_start[k], w = b->pt_window[k];
            const std::string who = std::string(fn) + ": point " + std::to_string(k);
            if (views < 2 || views > kNF) return fail(t, who + ": a track has 2 .. 11 views");
            if (s < 0 || s + views > kNF) return fail(t, who + ": the track leaves the window");
            if (w < 0 || w >= nw || (k > 0 && w < b->pt_window[k - 1])) return fail(t, who + ": window index out of range or decreasing");
            if (b->pt_obs_begin[k + 1] > t->max_point_obs) return fail(t, std::string(fn) + ": more point observations than the capacity given to uvs_tri_create");
        }
        n_obs = b->pt_obs_begin[np];
    }
    if (nl > 0) {
        if (!b->ln_window || !b->ln_fi || !b->ln_fj || !b->ln_sp_i || !b->ln_ep_i || !b->ln_sp_j || !b->ln_ep_j || !orth || !ln_flag)
            return fail(t, std::string(fn) + ": null line array");
        for (int k = 0; k < nl; ++k) {
            const int fi = b->ln_fi[k], fj = b->ln_fj[k], w = b->ln_window[k];
            const std::string who = std::string(fn) + ": line " + std::to_string(k);
            if (fi < 0 || fj >= kNF || fj <= fi) return fail(t, who + ": needs 0 <= ln_fi < ln_fj <= 10");
            if (w < 0 || w >= nw || (k > 0 && w < b->ln_window[k - 1])) return fail(t, who + ": window index out of range or decreasing");
        }
    }
    // packed input: pose | ex_pose | pt_window | pt_start | pt_obs_begin | pt_obs | ln_window | ln_fi | ln_fj | sp_i | ep_i | sp_j | ep_j
    UvsArena A;
    const FrameOffsets fo = take_frames(A, nw);
    const size_t o_pw = A.take((size_t)np * 4), o_ps = A.take((size_t)np * 4), o_pb = A.take(((size_t)np + 1) * 4), o_po = A.take((size_t)n_obs * 24);
    const size_t o_lw = A.take((size_t)nl * 4), o_li = A.take((size_t)nl * 4), o_lj = A.take((size_t)nl * 4);
    const size_t o_si = A.take((size_t)nl * 24), o_ei = A.take((size_t)nl * 24), o_sj = A.take((size_t)nl * 24), o_ej = A.take((size_t)nl * 24);
    char* hi = t->h_in;
    std::memcpy(hi + fo.pose, b->pose, (size_t)nw * kNF * 56); std::memcpy(hi + fo.ex, b->ex_pose, (size_t)nw * 56);
    if (np) {
        std::memcpy(hi + o_pw, b->pt_window, (size_t)np * 4); std::memcpy(hi + o_ps, b->pt_start, (size_t)np * 4);
        std::memcpy(hi + o_pb, b->pt_obs_begin, ((size_t)np + 1) * 4); std::memcpy(hi + o_po, b->pt_obs, (size_t)n_obs * 24);
    }
    if (nl) {
        std::memcpy(hi + o_lw, b->ln_window, (size_t)nl * 4); std::memcpy(hi + o_li, b->ln_fi, (size_t)nl * 4); std::memcpy(hi + o_lj, b->ln_fj, (size_t)nl * 4);
        std::memcpy(hi + o_si, b->ln_sp_i, (size_t)nl * 24); std::memcpy(hi + o_ei, b->ln_ep_i, (size_t)nl * 24);
        std::memcpy(hi + o_sj, b->ln_sp_j, (size_t)nl * 24); std::memcpy(hi + o_ej, b->ln_ep_j, (size_t)nl * 24);
    }
    UvsArena O;
    const size_t o_d = O.take((size_t)np * 8), o_o = O.take((size_t)nl * 32), o_pf = O.take((size_t)np * 4), o_lf = O.take((size_t)nl * 4);
    char* di = t->d_in; char* dout = t->d_out;
    auto D = [&](size_t off) { return reinterpret_cast<const double*>(di + off); };
    auto I = [&](size_t off) { return reinterpret_cast<const int32_t*>(di + off); };
    hipStream_t st = t->st;
    UVS_HIP(t->err, hipSetDevice(t->device));
    UVS_HIP(t->err, hipMemcpyAsync(di, hi, A.o, hipMemcpyHostToDevice, st));
    UVS_HIP(t->err, hipEventRecord(t->ev0, st));
    k_tri_cameras<<<blocks_for(nw * kNF), kThreads, 0, st>>>(D(fo.pose), D(fo.ex), nw * kNF, t->d_cams);
    if (np) k_tri_points<<<blocks_for(np), kThreads, 0, st>>>(t->d_cams, I(o_pw), I(o_ps), I(o_pb), D(o_po), np, init_depth,
                                                            reinterpret_cast<double*>(dout + o_d), reinterpret_cast<int32_t*>(dout + o_pf));
    if (nl) k_tri_lines<<<blocks_for(nl), kThreads, 0, st>>>(t->d_cams, I(o_lw), I(o_li), I(o_lj), D(o_si), D(o_ei), D(o_sj), D(o_ej), nl,
                                                           reinterpret_cast<double*>(dout + o_o), reinterpret_cast<int32_t*>(dout + o_lf));
    UVS_HIP(t->err, hipGetLastError());
    UVS_HIP(t->err, hipEventRecord(t->ev1, st));
    UVS_HIP(t->err, hipMemcpyAsync(t->h_out, dout, O.o, hipMemcpyDeviceToHost, st));
    UVS_HIP(t->err, hipStreamSynchronize(st));
    UVS_HIP(t->err, hipEventElapsedTime(&t->device_ms, t->ev0, t->ev1));
    const char* ho = t->h_out;
    if (np) { std::memcpy(depth, ho + o_d, (size_t)np * 8); std::memcpy(pt_flag, ho + o_pf, (size_t)np * 4); }
    if (nl) { std::memcpy(orth, ho + o_o, (size_t)nl * 32); std::memcpy(ln_flag, ho + o_lf, (size_t)nl * 4); }
    return UVS_OK;
}

int uvs_tri_check_lines(uvs_tri* t, int n_windows, const double* pose, const double* ex_pose, int n_lines, const int32_t* ln_window,
                        const int32_t* ln_start, const double* ln_sp0, const double* ln_ep0, const double* orth_old, int32_t* flag) {
    if (!t) return UVS_ERR_INVALID_ARG;
    t->err.clear();
    const char* fn = "uvs_tri_check_lines";
    if (n_lines < 0) return fail(t, std::string(fn) + ": negative count");
    if (n_lines == 0) return UVS_OK;
    int rc = check_frames(t, fn, n_windows, pose, ex_pose);
    if (rc != UVS_OK) return rc;
    if (n_lines > t->max_lines) return fail(t, std::string(fn) + ": more lines than the capacity given to uvs_tri_create");
    if (!ln_window || !ln_start || !ln_sp0 || !ln_ep0 || !orth_old || !flag) return fail(t, std::string(fn) + ": null line array");
    for (int k = 0; k < n_lines; ++k) {
        const std::string who = std::string(fn) + ": line " + std::to_string(k);
        if (ln_start[k] < 0 || ln_start[k] >= kNF) return fail(t, who + ": start frame outside 0 .. 10");
        if (ln_window[k] < 0 || ln_window[k] >= n_windows || (k > 0 && ln_window[k] < ln_window[k - 1])) return fail(t, who + ": window index out of range or decreasing");
    }
    const size_t nl = n_lines;
    UvsArena A;
    const FrameOffsets fo = take_frames(A, n_windows);
    const size_t o_lw = A.take(nl * 4), o_ls = A.take(nl * 4), o_sp = A.take(nl * 24), o_ep = A.take(nl * 24), o_or = A.take(nl * 32);
    char* hi = t->h_in;
    std::memcpy(hi + fo.pose, pose, (size_t)n_windows * kNF * 56); std::memcpy(hi + fo.ex, ex_pose, (size_t)n_windows * 56);
    std::memcpy(hi + o_lw, ln_window, nl * 4); std::memcpy(hi + o_ls, ln_start, nl * 4);
    std::memcpy(hi + o_sp, ln_sp0, nl * 24); std::memcpy(hi + o_ep, ln_ep0, nl * 24); std::memcpy(hi + o_or, orth_old, nl * 32);
    char* di = t->d_in;
    auto D = [&](size_t off) { return reinterpret_cast<const double*>(di + off); };
    auto I = [&](size_t off) { return reinterpret_cast<const int32_t*>(di + off); };
    hipStream_t st = t->st;
    UVS_HIP(t->err, hipSetDevice(t->device));
    UVS_HIP(t->err, hipMemcpyAsync(di, hi, A.o, hipMemcpyHostToDevice, st));
    UVS_HIP(t->err, hipEventRecord(t->ev0, st));
    k_tri_cameras<<<blocks_for(n_windows * kNF), kThreads, 0, st>>>(D(fo.pose), D(fo.ex), n_windows * kNF, t->d_cams);
    k_tri_check<<<blocks_for(n_lines), kThreads, 0, st>>>(t->d_cams, I(o_lw), I(o_ls), D(o_sp), D(o_ep), D(o_or), n_lines,
                                                         reinterpret_cast<int32_t*>(t->d_out.get()));
    UVS_HIP(t->err, hipGetLastError());
    UVS_HIP(t->err, hipEventRecord(t->ev1, st));
    UVS_HIP(t->err, hipMemcpyAsync(t->h_out, t->d_out, nl * 4, hipMemcpyDeviceToHost, st));
    UVS_HIP(t->err, hipStreamSynchronize(st));
    UVS_HIP(t->err, hipEventElapsedTime(&t->device_ms, t->ev0, t->ev1));
    std::memcpy(flag, t->h_out, nl * 4);
    return UVS_OK;
}

int uvs_tri_shift_depth(uvs_tri* t, int n_points, const double* uv0, const double* depth, const double* marg_R, const double* marg_P,
                        const double* new_R, const double* new_P, double* depth_out, int32_t* flag) {
    if (!t) return UVS_ERR_INVALID_ARG;
    t->err.clear();
    const char* fn = "uvs_tri_shift_depth";
    if (n_points < 0) return fail(t, std::string(fn) + ": negative count");
    if (n_points == 0) return UVS_OK;
    if (n_points > t->max_points) return fail(t, std::string(fn) + ": more points than the capacity given to uvs_tri_create");
    if (!uv0 || !depth || !marg_R || !marg_P || !new_R || !new_P || !depth_out || !flag) return fail(t, std::string(fn) + ": null pointer");
    ShiftArgs S;
    for (int k = 0; k < 9; ++k) { S.mR[k / 3][k % 3] = marg_R[k]; S.nR[k / 3][k % 3] = new_R[k]; }
    for (int k = 0; k < 3; ++k) { S.mP[k] = marg_P[k]; S.nP[k] = new_P[k]; }
    S.init_depth = t->init_depth;
    const size_t n = n_points;
    UvsArena A;
    const size_t o_uv = A.take(n * 24), o_d = A.take(n * 8);
    UvsArena O;
    const size_t o_out = O.take(n * 8), o_fl = O.take(n * 4);
    char* hi = t->h_in; char* di = t->d_in; char* dout = t->d_out;
    std::memcpy(hi + o_uv, uv0, n * 24); std::memcpy(hi + o_d, depth, n * 8);
    hipStream_t st = t->st;
    UVS_HIP(t->err, hipSetDevice(t->device));
    UVS_HIP(t->err, hipMemcpyAsync(di, hi, A.o, hipMemcpyHostToDevice, st));
    UVS_HIP(t->err, hipEventRecord(t->ev0, st));
    k_tri_shift<<<blocks_for(n_points), kThreads, 0, st>>>(S, reinterpret_cast<const double*>(di + o_uv), reinterpret_cast<const double*>(di + o_d), n_points,
                                                          reinterpret_cast<double*>(dout + o_out), reinterpret_cast<int32_t*>(dout + o_fl));
    UVS_HIP(t->err, hipGetLastError());
    UVS_HIP(t->err, hipEventRecord(t->ev1, st));
    UVS_HIP(t->err, hipMemcpyAsync(t->h_out, dout, O.o, hipMemcpyDeviceToHost, st));
    UVS_HIP(t->err, hipStreamSynchronize(st));
    UVS_HIP(t->err, hipEventElapsedTime(&t->device_ms, t->ev0, t->ev1));
    std::memcpy(depth_out, t->h_out + o_out, n * 8); std::memcpy(flag, t->h_out + o_fl, n * 4);
    return UVS_OK;
}

}  // extern "C"
