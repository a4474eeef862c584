// uvs_relative_pose.hip -- the bootstrap's choice of its reference frame for batches of frame pairs (reference vins_estimator/src/estimator.cpp:
// 448-477 relativePose, initial/solve_5pts.cpp:193-227 solveRelativeRT with the file's own recoverPose / decomposeEssentialMat :5-182) behind
// the uvs_rp_* calls of include/uvs_solver.h, whose comment is the statement of the rule.  FP64, gfx950, a handle of its own with one stream.
//
// One upload (item table, points as given), three kernels in stream order, one download (result blocks, final masks):
//   k_rp_gate        a wavefront per item.  The lanes round the item's points to float32 into the buffer the RANSAC reads; the parallaxes of 64
//                    tracks are computed a lane each and summed in item order by one wave-uniform chain of additions, so the sum is the
//                    sequential one.  Lane 0 writes status, n, average_parallax and the item's `gated` word.  It compacts nothing.
//   k_ft_reject_run  <true> of uvs_ft_reject_kernel.h: the kernel of uvs_ft_reject, a workgroup of 256 per item; a gated item's leaves at once.
//                    F, the counts and the mask stay on the device.
//   k_rp_recover     a wavefront per item.  The 3 x 3 SVD of F by one-sided Jacobi, every lane the same arithmetic (wave-uniform), the signs
//                    and the determinant flips of the rule, R1, R2, t.  Then the lanes stride over the points: the two rows of the first view
//                    go through Givens rotations into a 4 x 4 triangle once, the two rows of each candidate's second view on top of a copy,
//                    and the null vector comes from the one-sided Jacobi of uvs_svd_dev.h (the routine of k_tri_points) -- A^T A is never
//                    formed.  A point's four verdicts are a nibble in its byte of the mask; the four counts are ballots and population
//                    counts, no atomics.  Lane 0 makes the choice and writes the block; the lanes reduce their nibbles to the chosen bit.
// No LDS and no scratch in k_rp_gate and k_rp_recover (build() holds k_rp_* to 0 bytes per lane).  No item reads another item's data, so an
// item gives the same bits alone or in a batch.  The window-level answer (the first item with ok) is host bookkeeping after the download.
//
// The unit claims bit equality for steps 1 to 3, so nothing in it is contracted:
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/uvs_solver.h"
#include "uvs_ft_reject_kernel.h"
#include "uvs_handle.h"
#include "uvs_svd_dev.h"

namespace uvsrp {

using uvsfr::FrItem;
constexpr int kWave = 64;

struct RpDev {                             // uvs_rp_params as the kernels take it
    double focal_length, min_parallax_px, max_depth;
    int min_corres, min_ransac_points, min_inliers;
};

// ---- steps 1 and 2
__global__ void __launch_bounds__(kWave) k_rp_gate(FrItem* __restrict__ items, const double* __restrict__ raw, double* __restrict__ rounded, RpDev P,
                                                  uvs_rp_item_result* __restrict__ res) {
    const int lane = threadIdx.x;
    const FrItem it = items[blockIdx.x];
    const int n = it.n;
    const double* L = raw + it.pts_off;
    const double* R = L + 2 * (size_t)n;
    double* o = rounded + it.pts_off;
    for (int k = lane; k < 4 * n; k += kWave) o[k] = (double)(float)L[k];      // left[n][2] | right[n][2], one after the other
    double sum = 0.0;
    for (int base = 0; base < n; base += kWave) {                            // wave-uniform
        const int i = base + lane;
        double p = 0.0;
        if (i < n) {
            const double dx = L[2 * i] - R[2 * i], dy = L[2 * i + 1] - R[2 * i + 1];
            p = sqrt(dx * dx + dy * dy);
        }
        const int m = min(kWave, n - base);
        for (int j = 0; j < m; ++j) sum = sum + __shfl(p, j, kWave);
    }
    if (lane == 0) {
        const double avg = n > 0 ? sum / (double)n : 0.0;
        int st = UVS_RP_OK;
        if (!(n > P.min_corres)) st = UVS_RP_FEW_CORRES;
        else if (!(avg * P.focal_length > P.min_parallax_px)) st = UVS_RP_LOW_PARALLAX;
        else if (!(n >= P.min_ransac_points)) st = UVS_RP_FEW_POINTS;
        items[blockIdx.x].gated = st != UVS_RP_OK ? 1 : 0;
        uvs_rp_item_result* r = res + blockIdx.x;
        r->status = st; r->n = n; r->average_parallax = avg;
    }
}

// the sign that makes the entry of largest magnitude (the first such) positive
__device__ __forceinline__ double sign_of_largest(double a, double b, double c) {
    double m = fabs(a), e = a;
    if (fabs(b) > m) { m = fabs(b); e = b; }
    if (fabs(c) > m) { e = c; }
    return e < 0.0 ? -1.0 : 1.0;
}

__device__ __forceinline__ void swap_columns(double A[3][3], double V[3][3], double s[3], int a, int b) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double x = A[r][a]; A[r][a] = A[r][b]; A[r][b] = x;
        const double y = V[r][a]; V[r][a] = V[r][b]; V[r][b] = y;
    }
    const double z = s[a]; s[a] = s[b]; s[b] = z;
}

// an item that ends in front of step 5: an all-zero mask, every field behind the RANSAC block zero, chosen = -1
__device__ __forceinline__ void write_nothing(uvs_rp_item_result* out, uint8_t* mo, int n, int lane, int status, const uvs_ft_reject_result& rr) {
    for (int i = lane; i < n; i += kWave) mo[i] = 0;
    if (lane == 0) {
        out->status = status;
        out->ransac = rr;
        out->good[0] = out->good[1] = out->good[2] = out->good[3] = 0;
        out->chosen = -1; out->inlier_cnt = 0; out->ok = 0; out->reserved = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j) { out->R[j] = 0.0; out->Rotation[j] = 0.0; }
#pragma unroll
        for (int j = 0; j < 3; ++j) { out->t[j] = 0.0; out->Translation[j] = 0.0; }
    }
}

// ---- steps 4 to 6
__global__ void __launch_bounds__(kWave) k_rp_recover(const FrItem* __restrict__ items, const double* __restrict__ pts, const uint8_t* __restrict__ keep,
                                                     const uvs_ft_reject_result* __restrict__ ransac, RpDev P, uvs_rp_item_result* __restrict__ res,
                                                     uint8_t* __restrict__ mask) {
    const int lane = threadIdx.x;
    const FrItem it = items[blockIdx.x];
    const int n = it.n;
    uvs_rp_item_result* out = res + blockIdx.x;
    uint8_t* mo = mask + it.keep_off;
    uvs_ft_reject_result rr;
    rr.status = UVS_FT_REJECT_SKIPPED; rr.n_inliers = 0; rr.hypothesis = -1; rr.root = -1; rr.iterations = 0; rr.reserved = 0;
#pragma unroll
    for (int j = 0; j < 9; ++j) rr.F[j] = 0.0;
    if (!it.gated) rr = ransac[blockIdx.x];
    if (it.gated || rr.status != UVS_FT_REJECT_OK) {                          // wave-uniform
        write_nothing(out, mo, n, lane, it.gated ? out->status : UVS_RP_NO_MODEL, rr);
        return;
    }
    // ---- step 4, every lane alike: F V = U diag(s) by one-sided Jacobi on the columns of F
    double A[3][3], V[3][3], s[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) A[r][c] = rr.F[3 * r + c];
    uvssvd::jacobi_columns<3>(A, V);
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = sqrt((A[0][c] * A[0][c] + A[1][c] * A[1][c]) + A[2][c] * A[2][c]);
    if (s[0] < s[1]) swap_columns(A, V, s, 0, 1);
    if (s[0] < s[2]) swap_columns(A, V, s, 0, 2);
    if (s[1] < s[2]) swap_columns(A, V, s, 1, 2);
    if (!(s[1] > 0.0 && s[0] <= 1.7976931348623157e308)) {                    // F of rank < 2 (or not finite) has no u_1 = F v_1 / s_1: no model; wave-uniform
        write_nothing(out, mo, n, lane, UVS_RP_NO_MODEL, rr);
        return;
    }
    double U[3][3];                                                           // columns u_k; V holds the columns v_k
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double sg = sign_of_largest(V[0][k], V[1][k], V[2][k]);
#pragma unroll
        for (int r = 0; r < 3; ++r) { V[r][k] = sg * V[r][k]; U[r][k] = sg * (A[r][k] / s[k]); }
    }
    {
        const double sg = sign_of_largest(V[0][2], V[1][2], V[2][2]);
#pragma unroll
        for (int r = 0; r < 3; ++r) V[r][2] = sg * V[r][2];
        const double c0 = U[1][0] * U[2][1] - U[2][0] * U[1][1], c1 = U[2][0] * U[0][1] - U[0][0] * U[2][1], c2 = U[0][0] * U[1][1] - U[1][0] * U[0][1];
        const double su = sign_of_largest(c0, c1, c2);
        U[0][2] = su * c0; U[1][2] = su * c1; U[2][2] = su * c2;
    }
    const double detU = uvsfr::det3(U[0][0], U[0][1], U[0][2], U[1][0], U[1][1], U[1][2], U[2][0], U[2][1], U[2][2]);
    const double detV = uvsfr::det3(V[0][0], V[0][1], V[0][2], V[1][0], V[1][1], V[1][2], V[2][0], V[2][1], V[2][2]);
    const double fu = detU < 0.0 ? -1.0 : 1.0, fv = detV < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) { U[r][k] = fu * U[r][k]; V[r][k] = fv * V[r][k]; }
    double R1[3][3], R2[3][3], t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double a = U[r][1] * V[c][0], b = U[r][0] * V[c][1], d = U[r][2] * V[c][2];
            R1[r][c] = (b - a) + d;                                           // U W V^T
            R2[r][c] = (a - b) + d;                                           // U W^T V^T
        }
        t[r] = U[r][2];
    }
    // ---- step 5: the lanes stride over the points
    const double* left = pts + it.pts_off;
    const double* right = left + 2 * (size_t)n;
    const uint8_t* kp = keep + it.keep_off;
    int g0 = 0, g1 = 0, g2 = 0, g3 = 0;
    for (int base = 0; base < n; base += kWave) {                            // wave-uniform
        const int i = base + lane;
        const bool live = i < n;
        const int ii = live ? i : 0;
        const double x1 = left[2 * ii], y1 = left[2 * ii + 1], x2 = right[2 * ii], y2 = right[2 * ii + 1];
        const bool kept = live && kp[ii] != 0;
        double T0[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) T0[r][c] = 0.0;
        {
            double a[4] = {-1.0, 0.0, x1, 0.0}, b[4] = {0.0, -1.0, y1, 0.0};  // x P0[2] - P0[0], y P0[2] - P0[1]
            uvssvd::givens_row(T0, a);
            uvssvd::givens_row(T0, b);
        }
        int nib = 0;
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            double Rk[3][3], tk[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) Rk[r][c] = (k & 1) ? R2[r][c] : R1[r][c];
                tk[r] = k >= 2 ? -t[r] : t[r];
            }
            double T[4][4], W[4][4], q[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) T[r][c] = T0[r][c];
            double a[4], b[4];
#pragma unroll
            for (int c = 0; c < 3; ++c) { a[c] = x2 * Rk[2][c] - Rk[0][c]; b[c] = y2 * Rk[2][c] - Rk[1][c]; }
            a[3] = x2 * tk[2] - tk[0]; b[3] = y2 * tk[2] - tk[1];
            uvssvd::givens_row(T, a);
            uvssvd::givens_row(T, b);
            uvssvd::jacobi_columns<4>(T, W);
            uvssvd::smallest_column(T, W, q);
            bool m = q[2] * q[3] > 0.0;
            const double X0 = q[0] / q[3], X1 = q[1] / q[3], X2 = q[2] / q[3];
            m = m && X2 < P.max_depth;
            const double Y2 = ((Rk[2][0] * X0 + Rk[2][1] * X1) + Rk[2][2] * X2) + tk[2];
            m = m && Y2 > 0.0 && Y2 < P.max_depth && kept;
            const int c = __popcll(__ballot(m));
            g0 += k == 0 ? c : 0; g1 += k == 1 ? c : 0; g2 += k == 2 ? c : 0; g3 += k == 3 ? c : 0;
            nib |= (m ? 1 : 0) << k;
        }
        if (live) mo[i] = (uint8_t)nib;
    }
    // ---- step 6
    int chosen = 3;
    if (g0 >= g1 && g0 >= g2 && g0 >= g3) chosen = 0;
    else if (g1 >= g0 && g1 >= g2 && g1 >= g3) chosen = 1;
    else if (g2 >= g0 && g2 >= g1 && g2 >= g3) chosen = 2;
    for (int i = lane; i < n; i += kWave) mo[i] = (uint8_t)((mo[i] >> chosen) & 1);      // each lane reads the bytes it wrote
    if (lane == 0) {
        const int cnt = chosen == 0 ? g0 : (chosen == 1 ? g1 : (chosen == 2 ? g2 : g3));
        const int ok = cnt > P.min_inliers ? 1 : 0;
        out->status = ok ? UVS_RP_OK : UVS_RP_FEW_INLIERS;
        out->ransac = rr;
        out->good[0] = g0; out->good[1] = g1; out->good[2] = g2; out->good[3] = g3;
        out->chosen = chosen; out->inlier_cnt = cnt; out->ok = ok; out->reserved = 0;
        double Rc[3][3], tc[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) Rc[r][c] = (chosen & 1) ? R2[r][c] : R1[r][c];
            tc[r] = chosen >= 2 ? -t[r] : t[r];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { out->R[3 * r + c] = Rc[r][c]; out->Rotation[3 * r + c] = Rc[c][r]; }
            out->t[r] = tc[r];
            out->Translation[r] = -((Rc[0][r] * tc[0] + Rc[1][r] * tc[1]) + Rc[2][r] * tc[2]);
        }
    }
}

}  // namespace uvsrp

using namespace uvsrp;

struct uvs_rp : UvsHandle {
    int max_items = 0, max_points = 0;
    hipEvent_t ev2 = nullptr, ev3 = nullptr;    // with the base's two: in front of and behind each of the three kernels
    float ms[3] = {0.f, 0.f, 0.f};              // uvs_rp_last_device_ms
    DevBuf<char> d_buf;                         // one call's uploaded, device-only and downloaded parts
    PinnedBuf<char> h_in, h_out;                // pinned staging
    ~uvs_rp() {
        if (ev2) (void)hipEventDestroy(ev2);
        if (ev3) (void)hipEventDestroy(ev3);
    }
};

namespace {

int fail(uvs_rp* h, const std::string& msg) { h->err = "uvs_rp_relative_pose: " + msg; return UVS_ERR_INVALID_ARG; }

}  // namespace

extern "C" {

int uvs_rp_create(int device, int max_items, int max_points, uvs_rp** out) {
    if (!out || max_items < 1 || max_points < 1) return UVS_ERR_INVALID_ARG;
    *out = nullptr;
    if (max_items > UVS_RP_MAX_ITEMS || max_points > UVS_FT_MAX_POINTS) return UVS_ERR_CAPACITY;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return UVS_ERR_NO_DEVICE;
    uvs_rp* h = new uvs_rp();
    h->max_items = max_items; h->max_points = max_points;
    int rc = h->open(device);
    if (rc == UVS_OK && (hipEventCreate(&h->ev2) != hipSuccess || hipEventCreate(&h->ev3) != hipSuccess)) rc = UVS_ERR_HIP;
    if (rc != UVS_OK) { uvs_rp_destroy(h); return rc; }
    *out = h;
    return UVS_OK;
}

void uvs_rp_destroy(uvs_rp* h) { if (h) { h->close(); delete h; } }

const char* uvs_rp_last_error(const uvs_rp* h) { return h ? h->err.c_str() : "null relative-pose handle"; }

void uvs_rp_default_params(uvs_rp_params* p) {
    if (!p) return;
    p->focal_length = 460.0; p->min_parallax_px = 30.0; p->f_threshold = 0.3 / 460; p->confidence = 0.99; p->max_depth = 50.0;
    p->min_corres = 20; p->min_ransac_points = 15; p->min_inliers = 12; p->reserved = 0;
}

double uvs_rp_last_device_ms(const uvs_rp* h, int part) { return h && part >= 0 && part < 3 ? (double)h->ms[part] : 0.0; }

int uvs_rp_relative_pose(uvs_rp* h, int n_items, const uvs_rp_item* items, const uvs_rp_params* params, uint8_t* mask,
                         uvs_rp_item_result* item_results, int n_windows, uvs_rp_window_result* window_results) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    if (!items || !params || !mask || !item_results || !window_results) return fail(h, "null pointer");
    if (n_items < 1 || n_items > h->max_items) return fail(h, "n_items must be 1 .. the capacity given to uvs_rp_create");
    if (n_windows < 1) return fail(h, "n_windows < 1");
    const uvs_rp_params& p = *params;
    if (!(std::isfinite(p.focal_length) && p.focal_length > 0.0) || !std::isfinite(p.min_parallax_px) || !(std::isfinite(p.f_threshold) && p.f_threshold > 0.0) ||
        !(p.confidence > 0.0 && p.confidence < 1.0) || !(std::isfinite(p.max_depth) && p.max_depth > 0.0))
        return fail(h, "focal_length, f_threshold and max_depth must be finite and positive, min_parallax_px finite, confidence in (0, 1)");
    if (p.min_ransac_points < 8 || p.min_corres < 0 || p.min_inliers < 0) return fail(h, "min_ransac_points must be >= 8, min_corres and min_inliers >= 0");
    size_t n_pts = 0;
    for (int i = 0; i < n_items; ++i) {
        const uvs_rp_item& it = items[i];
        const std::string who = "item " + std::to_string(i);
        if (it.window < 0 || it.window >= n_windows || (i > 0 && it.window < items[i - 1].window)) return fail(h, who + ": window index out of range or decreasing");
        if (it.frame_l < 0 || it.frame_l >= UVS_WINDOW_SIZE) return fail(h, who + ": frame_l outside 0 .. UVS_WINDOW_SIZE - 1");
        if (i > 0 && it.window == items[i - 1].window && it.frame_l <= items[i - 1].frame_l) return fail(h, who + ": frame_l must increase within a window");
        if (it.n < 0 || it.n > h->max_points) return fail(h, who + ": n must be 0 .. the capacity given to uvs_rp_create");
        if (it.n > 0 && (!it.left || !it.right)) return fail(h, who + ": null point array");
        for (int k = 0; k < 2 * it.n; ++k)
            if (!std::isfinite(it.left[k]) || !std::isfinite(it.right[k])) return fail(h, who + ": a coordinate is not finite");
        n_pts += (size_t)it.n;
    }
    // the layout of the call: items | points as given, uploaded;  rounded points | RANSAC results | RANSAC masks, device only;
    // result blocks | final masks, downloaded
    UvsArena A;
    const size_t o_items = A.take(n_items * sizeof(FrItem)), o_raw = A.take(n_pts * 32);
    const size_t in_bytes = A.o;
    const size_t o_pts = A.take(n_pts * 32), o_fr = A.take(n_items * sizeof(uvs_ft_reject_result)), o_keep = A.take(n_pts);
    const size_t o_res = A.take(n_items * sizeof(uvs_rp_item_result)), o_mask = A.take(n_pts);
    const size_t out_bytes = A.o - o_res;
    UVS_HIP(h->err, hipSetDevice(h->device));
    int rc;
    if ((rc = h->d_buf.ensure(A.o, h->err, grow_half)) != UVS_OK || (rc = h->h_in.ensure(in_bytes, h->err, grow_pinned)) != UVS_OK ||
        (rc = h->h_out.ensure(out_bytes, h->err, grow_pinned)) != UVS_OK) return rc;
    FrItem* F = reinterpret_cast<FrItem*>(h->h_in + o_items);
    double* Pt = reinterpret_cast<double*>(h->h_in + o_raw);
    size_t at = 0;
    for (int i = 0; i < n_items; ++i) {
        const size_t n = (size_t)items[i].n;
        F[i].n = (int)n; F[i].gated = 0; F[i].seed = items[i].seed; F[i].pts_off = (long long)(4 * at); F[i].keep_off = (long long)at;
        if (n) {
            std::memcpy(Pt + 4 * at, items[i].left, n * 16);
            std::memcpy(Pt + 4 * at + 2 * n, items[i].right, n * 16);
        }
        at += n;
    }
    RpDev P;
    P.focal_length = p.focal_length; P.min_parallax_px = p.min_parallax_px; P.max_depth = p.max_depth;
    P.min_corres = p.min_corres; P.min_ransac_points = p.min_ransac_points; P.min_inliers = p.min_inliers;
    char* D = h->d_buf;
    hipStream_t st = h->st;
    FrItem* d_items = reinterpret_cast<FrItem*>(D + o_items);
    double* d_pts = reinterpret_cast<double*>(D + o_pts);
    uvs_rp_item_result* d_res = reinterpret_cast<uvs_rp_item_result*>(D + o_res);
    uvs_ft_reject_result* d_fr = reinterpret_cast<uvs_ft_reject_result*>(D + o_fr);
    UVS_HIP(h->err, hipMemcpyAsync(D, h->h_in, in_bytes, hipMemcpyHostToDevice, st));
    UVS_HIP(h->err, hipEventRecord(h->ev0, st));
    k_rp_gate<<<n_items, kWave, 0, st>>>(d_items, reinterpret_cast<const double*>(D + o_raw), d_pts, P, d_res);
    UVS_HIP(h->err, hipGetLastError());
    UVS_HIP(h->err, hipEventRecord(h->ev1, st));
    uvsfr::k_ft_reject_run<true><<<n_items, uvsfr::kThreads, 0, st>>>(d_items, d_pts, p.f_threshold, p.confidence, 0, reinterpret_cast<uint8_t*>(D + o_keep), d_fr,
                                                                   nullptr, nullptr, nullptr);
    UVS_HIP(h->err, hipGetLastError());
    UVS_HIP(h->err, hipEventRecord(h->ev2, st));
    k_rp_recover<<<n_items, kWave, 0, st>>>(d_items, d_pts, reinterpret_cast<const uint8_t*>(D + o_keep), d_fr, P, d_res, reinterpret_cast<uint8_t*>(D + o_mask));
    UVS_HIP(h->err, hipGetLastError());
    UVS_HIP(h->err, hipEventRecord(h->ev3, st));
    UVS_HIP(h->err, hipMemcpyAsync(h->h_out, D + o_res, out_bytes, hipMemcpyDeviceToHost, st));
    UVS_HIP(h->err, hipStreamSynchronize(st));
    UVS_HIP(h->err, hipEventElapsedTime(&h->ms[0], h->ev0, h->ev1));
    UVS_HIP(h->err, hipEventElapsedTime(&h->ms[1], h->ev1, h->ev2));
    UVS_HIP(h->err, hipEventElapsedTime(&h->ms[2], h->ev2, h->ev3));
    std::memcpy(item_results, h->h_out, n_items * sizeof(uvs_rp_item_result));
    if (n_pts) std::memcpy(mask, h->h_out + (o_mask - o_res), n_pts);
    // the window-level answer: the first item of each window with ok
    for (int w = 0; w < n_windows; ++w) { std::memset(&window_results[w], 0, sizeof(uvs_rp_window_result)); window_results[w].l = -1; }
    for (int i = 0; i < n_items; ++i) {
        uvs_rp_window_result& wr = window_results[items[i].window];
        if (wr.l < 0 && item_results[i].ok) {
            wr.l = items[i].frame_l;
            std::memcpy(wr.Rotation, item_results[i].Rotation, sizeof wr.Rotation);
            std::memcpy(wr.Translation, item_results[i].Translation, sizeof wr.Translation);
        }
    }
    return UVS_OK;
}

}  // extern "C"
