// uvs_imu_preintegrate.hip -- IMU pre-integration for batches of intervals (uvs_imu_*, include/uvs_solver.h): IntegrationBase::push_back /
// propagate / midPointIntegration / repropagate (integration_base.h:30-158) and, optionally, the dead reckoning of Estimator::processIMU
// (estimator.cpp:104-117) in the same walk over the samples.  A handle of its own; one launch per call.
//
// The kernel (k_imu_preintegrate): ONE WAVEFRONT PER INTERVAL, one workgroup of 64 lanes per wavefront, so every index of the walk is wave-uniform.
//   - jacobian and covariance (15 x 15, padded to 16 x 16) stay in registers from the first sample to the last, in the C/D layout of
//     v_mfma_f64_16x16x4_f64: lane l, register r holds M[(l >> 4) + 4 r][l & 15].  Register s of such a matrix is, as it stands, the B operand
//     of k-slice s (rows 4 s .. 4 s + 3), and used as the A operand it is the same slice of the TRANSPOSE.
//   - per sample every lane computes the four entries F[l & 15][4 s + (l >> 4)] of the step matrix F (15 x 15) and the five entries
//     V[l & 15][4 s + (l >> 4)] of the noise map V (15 x 18, padded to 20): an A operand as it stands, and as a B operand the transpose.  Then
//         J' = F J                 4 MFMAs   A(f_s)  B(J_s)
//         G  = P^T F^T             4 MFMAs   A(P_s)  B(f_s)
//         P' = G^T F^T = F P F^T   4 MFMAs   A(G_s)  B(f_s)
//            + V N V^T             5 MFMAs   A(v_s n_s)  B(v_s)
//     17 MFMAs, no transposes, no LDS.  P is never assumed symmetric: the two products transpose it twice.
//   - the small state (delta_p/q/v, the 3 x 3 rotations) is computed by every lane alike; a lane then keeps row (l & 15) % 3 of each 3 x 3
//     block, from which its entries of F and V are picked by compare-and-select (no array is indexed at run time: no scratch).
//   - the samples are staged kChunk = 64 at a time, one per lane, and broadcast by v_readlane; the next chunk's loads are issued before the
//     current chunk is walked.  Global memory is written once, at the end.
// Entries of F and V that are structurally 0 or 1 are exactly 0.0 or 1.0, so the products with them are exact and the structural zeros and
// ones of jacobian (rows 9..14, columns 0..2, the zero blocks, sum_dt * I in J[0:3, 6:9]) come out exact.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/uvs_solver.h"
#include "uvs_handle.h"

namespace uvsimu {

constexpr int kWave = 64;
constexpr int kChunk = 64;                     // samples staged per chunk: lane l holds sample base + l (UVS_IMU_STAGE_CHUNK of the header)
static_assert(kChunk == UVS_IMU_STAGE_CHUNK, "the header states the staging chunk");
typedef double d4 __attribute__((ext_vector_type(4)));

struct Args {
    const int32_t* sample_begin; const double *acc_0, *gyr_0, *ba, *bg; const int32_t* frame_i;      // frame_i may be null
    const double *dt, *acc, *gyr;
    const double *state_p, *state_R, *state_v;                                                      // all null: no dead reckoning
    double gravity[3];
    double an2, gn2, aw2, gw2;                                                                      // the four noise variances
    uvs_imu_block* blocks; double *pred_p, *pred_R, *pred_v;
};

// a value of lane `src` (wave-uniform) to every lane
__device__ inline double bcast(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
__device__ inline double pick3(const double* v, int j) { return j == 0 ? v[0] : (j == 1 ? v[1] : v[2]); }
__device__ inline void cross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
// Eigen's toRotationMatrix() polynomial of q = (x, y, z, w), unit or not
__device__ inline void quat_R(const double* q, double R[3][3]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0][0] = 1.0 - 2.0 * (y * y + z * z); R[0][1] = 2.0 * (x * y - z * w); R[0][2] = 2.0 * (x * z + y * w);
    R[1][0] = 2.0 * (x * y + z * w); R[1][1] = 1.0 - 2.0 * (x * x + z * z); R[1][2] = 2.0 * (y * z - x * w);
    R[2][0] = 2.0 * (x * z - y * w); R[2][1] = 2.0 * (y * z + x * w); R[2][2] = 1.0 - 2.0 * (x * x + y * y);
}
__device__ inline void mat_vec(const double R[3][3], const double* v, double* o) {
    for (int a = 0; a < 3; ++a) o[a] = R[a][0] * v[0] + R[a][1] * v[1] + R[a][2] * v[2];
}

// two waves per SIMD: within 256 registers without scratch (four would spill), and 2 560 intervals are then one round of a 256-CU machine plus a quarter
__global__ void __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(2, 2))) k_imu_preintegrate(const Args A) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const int begin = __builtin_amdgcn_readfirstlane(A.sample_begin[k]), end = __builtin_amdgcn_readfirstlane(A.sample_begin[k + 1]);
    const bool reckon = A.state_p != nullptr;
    // the lane's row i of F and V, its row block and the row inside the block; its column of k-slice s is c = 4 s + kq
    const int i = lane & 15, kq = lane >> 4, rb = i / 3, ri = i - 3 * rb;
    const bool pv = rb == 0 || rb == 2;                                          // a row of delta_p or delta_v
    double nz[5];                                                               // the noise variance of the lane's column of V, slice by slice
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int cb = (4 * s + kq) / 3;
        nz[s] = (cb == 0 || cb == 2) ? A.an2 : (cb == 1 || cb == 3) ? A.gn2 : cb == 4 ? A.aw2 : cb == 5 ? A.gw2 : 0.0;
    }
    double ba[3], bg[3], a0[3], g0[3], dp[3] = {0, 0, 0}, dv[3] = {0, 0, 0}, dq[4] = {0, 0, 0, 1}, sum_dt = 0.0;
    for (int a = 0; a < 3; ++a) { ba[a] = A.ba[3 * k + a]; bg[a] = A.bg[3 * k + a]; a0[a] = A.acc_0[3 * k + a]; g0[a] = A.gyr_0[3 * k + a]; }
    double wP[3] = {0, 0, 0}, wV[3] = {0, 0, 0}, wR[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};      // the dead-reckoned state of frame j
    if (reckon)
        for (int a = 0; a < 3; ++a) {
            wP[a] = A.state_p[3 * k + a]; wV[a] = A.state_v[3 * k + a];
            for (int b = 0; b < 3; ++b) wR[a][b] = A.state_R[9 * k + 3 * a + b];
        }
    d4 J, P = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) J[r] = (kq + 4 * r == i && i < 15) ? 1.0 : 0.0;

    // the lane's sample of the current chunk, and of the next one
    double c_dt = 0, c_a[3] = {0, 0, 0}, c_g[3] = {0, 0, 0}, n_dt = 0, n_a[3] = {0, 0, 0}, n_g[3] = {0, 0, 0};
    if (begin + lane < end) {
        const int m = begin + lane;
        c_dt = A.dt[m];
        for (int a = 0; a < 3; ++a) { c_a[a] = A.acc[3 * (size_t)m + a]; c_g[a] = A.gyr[3 * (size_t)m + a]; }
    }
    for (int base = begin; base < end; base += kChunk) {
        const int m = base + kChunk + lane;                                      // read ahead: the next chunk, before this one is walked
        if (m < end) {
            n_dt = A.dt[m];
            for (int a = 0; a < 3; ++a) { n_a[a] = A.acc[3 * (size_t)m + a]; n_g[a] = A.gyr[3 * (size_t)m + a]; }
        }
        const int count = end - base < kChunk ? end - base : kChunk;
        for (int j = 0; j < count; ++j) {
            const double dt = bcast(c_dt, j);
            double a1[3], g1[3];
            for (int a = 0; a < 3; ++a) { a1[a] = bcast(c_a[a], j); g1[a] = bcast(c_g[a], j); }
            // ---- midPointIntegration: the small state, every lane alike
            double a0b[3], a1b[3], w[3];
            for (int a = 0; a < 3; ++a) { a0b[a] = a0[a] - ba[a]; a1b[a] = a1[a] - ba[a]; w[a] = 0.5 * (g0[a] + g1[a]) - bg[a]; }
            double Rq[3][3], Rr[3][3], rq[4];
            quat_R(dq, Rq);
            {
                const double bx = w[0] * dt / 2, by = w[1] * dt / 2, bz = w[2] * dt / 2;      // delta_q * (1, un_gyr dt / 2)
                rq[0] = dq[3] * bx + dq[0] + dq[1] * bz - dq[2] * by;
                rq[1] = dq[3] * by + dq[1] + dq[2] * bx - dq[0] * bz;
                rq[2] = dq[3] * bz + dq[2] + dq[0] * by - dq[1] * bx;
                rq[3] = dq[3] - dq[0] * bx - dq[1] * by - dq[2] * bz;
            }
            quat_R(rq, Rr);                                                     // un-normalised, as the reference uses it
            double u0[3], u1[3], un[3];
            mat_vec(Rq, a0b, u0); mat_vec(Rr, a1b, u1);
            for (int a = 0; a < 3; ++a) un[a] = 0.5 * (u0[a] + u1[a]);
            // ---- the lane's rows of the 3 x 3 blocks: row ri of Rq, Rr, Rq [a0]x + Rr [a1]x (I - [w]x dt), Rq + Rr, Rr [a1]x, I - [w]x dt
            double rowQ[3], rowR[3], e[3] = {ri == 0 ? 1.0 : 0.0, ri == 1 ? 1.0 : 0.0, ri == 2 ? 1.0 : 0.0};
            for (int b = 0; b < 3; ++b) {
                rowQ[b] = ri == 0 ? Rq[0][b] : (ri == 1 ? Rq[1][b] : Rq[2][b]);
                rowR[b] = ri == 0 ? Rr[0][b] : (ri == 1 ? Rr[1][b] : Rr[2][b]);
            }
            double qa0[3], row4[3], r4w[3], ew[3], row1[3], row3[3], rowT[3];
            cross(rowQ, a0b, qa0); cross(rowR, a1b, row4); cross(row4, w, r4w); cross(e, w, ew);      // (row of M) [v]x = row x v
            for (int b = 0; b < 3; ++b) { row1[b] = qa0[b] + (row4[b] - dt * r4w[b]); row3[b] = rowQ[b] + rowR[b]; rowT[b] = e[b] - dt * ew[b]; }
            const double dt2 = dt * dt, dt3 = dt2 * dt;
            const double s1 = rb == 0 ? -0.25 * dt2 : -0.5 * dt, s4 = rb == 0 ? 0.25 * dt3 : 0.5 * dt2;          // F: rows of delta_p / delta_v
            const double sq = rb == 0 ? 0.25 * dt2 : 0.5 * dt, sv = rb == 0 ? -0.125 * dt3 : -0.25 * dt2;      // V likewise
            double f[4], v[5];
#pragma unroll
            for (int s = 0; s < 5; ++s) {
                const int c = 4 * s + kq, cb = c / 3, cj = c - 3 * cb;
                const double idv = ri == cj ? 1.0 : 0.0;
                const double r4c = pick3(row4, cj);
                if (s < 4) {
                    const double m = cb == 1 ? (rb == 1 ? pick3(rowT, cj) : s1 * pick3(row1, cj)) : (cb == 3 ? s1 * pick3(row3, cj) : s4 * r4c);
                    const bool use_m = (pv && (cb == 1 || cb == 3 || cb == 4)) || (rb == 1 && cb == 1);
                    const double idc = (cb == rb && rb < 5) ? 1.0 : ((rb == 0 && cb == 2) ? dt : ((rb == 1 && cb == 4) ? -dt : 0.0));
                    f[s] = use_m ? m : idv * idc;
                }
                const double vm = cb == 0 ? sq * pick3(rowQ, cj) : (cb == 2 ? sq * pick3(rowR, cj) : sv * r4c);
                const double vid = (rb == 1 && (cb == 1 || cb == 3)) ? 0.5 * dt : (((rb == 3 && cb == 4) || (rb == 4 && cb == 5)) ? dt : 0.0);
                v[s] = (pv && cb < 4) ? vm : idv * vid;
            }
            // ---- jacobian = F jacobian; covariance = F covariance F^T + V noise V^T
            d4 Jn = {0, 0, 0, 0}, G = {0, 0, 0, 0}, Pn = {0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                Jn = __builtin_amdgcn_mfma_f64_16x16x4f64(f[s], J[s], Jn, 0, 0, 0);
                G = __builtin_amdgcn_mfma_f64_16x16x4f64(P[s], f[s], G, 0, 0, 0);
            }
#pragma unroll
            for (int s = 0; s < 5; ++s) Pn = __builtin_amdgcn_mfma_f64_16x16x4f64(v[s] * nz[s], v[s], Pn, 0, 0, 0);
#pragma unroll
            for (int s = 0; s < 4; ++s) Pn = __builtin_amdgcn_mfma_f64_16x16x4f64(G[s], f[s], Pn, 0, 0, 0);
            J = Jn; P = Pn;
            // ---- the dead reckoning of processIMU: rotation first, then the mean of the world accelerations at both ends
            if (reckon) {
                const double th[4] = {w[0] * dt / 2.0, w[1] * dt / 2.0, w[2] * dt / 2.0, 1.0};      // Utility::deltaQ(rate dt), not normalised
                double Rd[3][3], Rn[3][3], wa0[3], wa1[3];
                quat_R(th, Rd);
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) Rn[a][b] = wR[a][0] * Rd[0][b] + wR[a][1] * Rd[1][b] + wR[a][2] * Rd[2][b];
                mat_vec(wR, a0b, wa0); mat_vec(Rn, a1b, wa1);
                for (int a = 0; a < 3; ++a) {
                    const double a_mean = 0.5 * ((wa0[a] - A.gravity[a]) + (wa1[a] - A.gravity[a]));
                    wP[a] = wP[a] + dt * wV[a] + 0.5 * dt * dt * a_mean;
                    wV[a] = wV[a] + dt * a_mean;
                    for (int b = 0; b < 3; ++b) wR[a][b] = Rn[a][b];
                }
            }
            // ---- the step's results become the state
            const double nrm = sqrt(rq[0] * rq[0] + rq[1] * rq[1] + rq[2] * rq[2] + rq[3] * rq[3]);
            for (int a = 0; a < 4; ++a) dq[a] = rq[a] / nrm;
            for (int a = 0; a < 3; ++a) {
                dp[a] = dp[a] + dv[a] * dt + 0.5 * un[a] * dt * dt;
                dv[a] = dv[a] + un[a] * dt;
                a0[a] = a1[a]; g0[a] = g1[a];
            }
            sum_dt += dt;
        }
        c_dt = n_dt;
        for (int a = 0; a < 3; ++a) { c_a[a] = n_a[a]; c_g[a] = n_g[a]; }
    }

    // ---- written once
    uvs_imu_block* out = A.blocks + k;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = kq + 4 * r;
        if (row < 15 && i < 15) { out->jacobian[row * 15 + i] = J[r]; out->covariance[row * 15 + i] = P[r]; }
    }
    if (lane == 0) {
        out->sum_dt = sum_dt;
        for (int a = 0; a < 3; ++a) { out->delta_p[a] = dp[a]; out->delta_v[a] = dv[a]; out->linearized_ba[a] = ba[a]; out->linearized_bg[a] = bg[a]; }
        for (int a = 0; a < 4; ++a) out->delta_q[a] = dq[a];
        out->frame_i = A.frame_i ? A.frame_i[k] : 0;
        out->skip = sum_dt > 10.0 ? 1 : 0;
        if (reckon)
            for (int a = 0; a < 3; ++a) {
                A.pred_p[3 * k + a] = wP[a]; A.pred_v[3 * k + a] = wV[a];
                for (int b = 0; b < 3; ++b) A.pred_R[9 * k + 3 * a + b] = wR[a][b];
            }
    }
}

}  // namespace uvsimu

using namespace uvsimu;

struct uvs_imu : UvsHandle {
    int max_intervals = 0, max_samples = 0;
    double sigma[4] = {0.08, 0.004, 0.00004, 2.0e-6};      // acc_n, gyr_n, acc_w, gyr_w: the EuRoC values of host/parameters.h; uvs_imu_set_noise
    float device_ms = 0.f;                                 // uvs_imu_last_device_ms
    DevBuf<char> d_in, d_out;                              // packed inputs / outputs of one call
    PinnedBuf<char> h_in, h_out;                           // pinned staging
};

namespace {

int fail(uvs_imu* h, const std::string& msg, int rc = UVS_ERR_INVALID_ARG) { h->err = msg; return rc; }

// byte offsets of the packed input and output of a call of n intervals and m samples
struct Layout {
    size_t begin, acc_0, gyr_0, ba, bg, frame_i, dt, acc, gyr, sp, sR, sv, in_bytes;
    size_t blocks, pp, pR, pv, out_bytes;
    Layout(size_t n, size_t m) {
        UvsArena A;
        begin = A.take((n + 1) * 4); acc_0 = A.take(n * 24); gyr_0 = A.take(n * 24); ba = A.take(n * 24); bg = A.take(n * 24); frame_i = A.take(n * 4);
        dt = A.take(m * 8); acc = A.take(m * 24); gyr = A.take(m * 24); sp = A.take(n * 24); sR = A.take(n * 72); sv = A.take(n * 24);
        in_bytes = A.o;
        UvsArena O;
        blocks = O.take(n * sizeof(uvs_imu_block)); pp = O.take(n * 24); pR = O.take(n * 72); pv = O.take(n * 24);
        out_bytes = O.o;
    }
};

// without an early exit, so that the loop over a batch's samples vectorises (a compare and an integer OR per element)
bool all_finite(const double* v, size_t n) {
    int bad = 0;
    for (size_t k = 0; k < n; ++k) bad |= !(std::fabs(v[k]) <= 1.7976931348623157e308);
    return bad == 0;
}
// the index of the first dt that is negative or not finite, or -1
long first_bad_dt(const double* dt, size_t n) {
    int bad = 0;
    for (size_t k = 0; k < n; ++k) bad |= !(dt[k] >= 0.0 && dt[k] <= 1.7976931348623157e308);
    if (!bad) return -1;
    for (size_t k = 0; k < n; ++k)
        if (!(dt[k] >= 0.0 && dt[k] <= 1.7976931348623157e308)) return (long)k;
    return -1;
}

}  // namespace

extern "C" {

int uvs_imu_create(int device, int max_intervals, int max_samples, uvs_imu** out) {
    if (!out || max_intervals < 1 || max_samples < 1) return UVS_ERR_INVALID_ARG;
    *out = nullptr;
    if (max_intervals > UVS_IMU_MAX_INTERVALS || max_samples > UVS_IMU_MAX_SAMPLES) return UVS_ERR_CAPACITY;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return UVS_ERR_NO_DEVICE;
    uvs_imu* h = new uvs_imu();
    h->max_intervals = max_intervals; h->max_samples = max_samples;
    const Layout L((size_t)max_intervals, (size_t)max_samples);
    int rc = h->open(device);
    if (rc == UVS_OK && (rc = h->d_in.ensure(L.in_bytes, h->err)) == UVS_OK && (rc = h->h_in.ensure(L.in_bytes, h->err)) == UVS_OK &&
        (rc = h->d_out.ensure(L.out_bytes, h->err)) == UVS_OK)
        rc = h->h_out.ensure(L.out_bytes, h->err);
    if (rc != UVS_OK) { uvs_imu_destroy(h); return rc; }
    *out = h;
    return UVS_OK;
}

void uvs_imu_destroy(uvs_imu* h) { if (h) { h->close(); delete h; } }

const char* uvs_imu_last_error(const uvs_imu* h) { return h ? h->err.c_str() : "null pre-integration handle"; }

double uvs_imu_last_device_ms(const uvs_imu* h) { return h ? (double)h->device_ms : 0.0; }

int uvs_imu_set_noise(uvs_imu* h, double acc_n, double gyr_n, double acc_w, double gyr_w) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    const double s[4] = {acc_n, gyr_n, acc_w, gyr_w};
    for (double x : s)
        if (!(x > 0.0) || !std::isfinite(x)) return fail(h, "uvs_imu_set_noise: every noise value must be positive and finite");
    std::memcpy(h->sigma, s, sizeof(s));
    return UVS_OK;
}

int uvs_imu_preintegrate(uvs_imu* h, const uvs_imu_batch* b, uvs_imu_block* blocks, double* pred_p, double* pred_R, double* pred_v) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    const std::string fn = "uvs_imu_preintegrate";
    if (!b) return fail(h, fn + ": null batch");
    const int n = b->n_intervals;
    if (n < 0) return fail(h, fn + ": negative count");
    if (n == 0) return UVS_OK;                                                  // nothing to do, nothing launched
    if (n > h->max_intervals) return fail(h, fn + ": more intervals than the capacity given to uvs_imu_create", UVS_ERR_CAPACITY);
    if (!b->sample_begin || !b->acc_0 || !b->gyr_0 || !b->ba || !b->bg || !blocks) return fail(h, fn + ": null pointer");
    if (b->sample_begin[0] != 0) return fail(h, fn + ": sample_begin[0] must be 0");
    for (int k = 0; k < n; ++k) {
        if (b->sample_begin[k + 1] < b->sample_begin[k]) return fail(h, fn + ": sample_begin decreases at interval " + std::to_string(k));
        if (b->sample_begin[k + 1] > h->max_samples) return fail(h, fn + ": more samples than the capacity given to uvs_imu_create", UVS_ERR_CAPACITY);
    }
    const int m = b->sample_begin[n];
    if (m > 0 && (!b->dt || !b->acc || !b->gyr)) return fail(h, fn + ": null sample array");
    const int n_state = (b->state_p ? 1 : 0) + (b->state_R ? 1 : 0) + (b->state_v ? 1 : 0);
    if (n_state != 0 && n_state != 3) return fail(h, fn + ": state_p, state_R and state_v are all null or all set");
    const bool reckon = n_state == 3;
    if (reckon && (!pred_p || !pred_R || !pred_v)) return fail(h, fn + ": dead reckoning needs pred_p, pred_R and pred_v");
    if (const long k = first_bad_dt(b->dt, (size_t)m); k >= 0) return fail(h, fn + ": dt of sample " + std::to_string(k) + " is negative or not finite");
    if (!all_finite(b->acc, (size_t)m * 3) || !all_finite(b->gyr, (size_t)m * 3) || !all_finite(b->acc_0, (size_t)n * 3) || !all_finite(b->gyr_0, (size_t)n * 3))
        return fail(h, fn + ": a sample is not finite");
    if (!all_finite(b->ba, (size_t)n * 3) || !all_finite(b->bg, (size_t)n * 3)) return fail(h, fn + ": a bias is not finite");
    if (reckon && (!all_finite(b->state_p, (size_t)n * 3) || !all_finite(b->state_R, (size_t)n * 9) || !all_finite(b->state_v, (size_t)n * 3) ||
                   !all_finite(b->gravity, 3)))
        return fail(h, fn + ": a dead-reckoning state or the gravity is not finite");

    const Layout L((size_t)n, (size_t)m);
    char* hi = h->h_in;
    std::memcpy(hi + L.begin, b->sample_begin, ((size_t)n + 1) * 4);
    std::memcpy(hi + L.acc_0, b->acc_0, (size_t)n * 24); std::memcpy(hi + L.gyr_0, b->gyr_0, (size_t)n * 24);
    std::memcpy(hi + L.ba, b->ba, (size_t)n * 24); std::memcpy(hi + L.bg, b->bg, (size_t)n * 24);
    if (b->frame_i) std::memcpy(hi + L.frame_i, b->frame_i, (size_t)n * 4);
    if (m) { std::memcpy(hi + L.dt, b->dt, (size_t)m * 8); std::memcpy(hi + L.acc, b->acc, (size_t)m * 24); std::memcpy(hi + L.gyr, b->gyr, (size_t)m * 24); }
    if (reckon) { std::memcpy(hi + L.sp, b->state_p, (size_t)n * 24); std::memcpy(hi + L.sR, b->state_R, (size_t)n * 72); std::memcpy(hi + L.sv, b->state_v, (size_t)n * 24); }
    char* di = h->d_in; char* dout = h->d_out;
    auto D = [&](size_t off) { return reinterpret_cast<const double*>(di + off); };
    Args A{};
    A.sample_begin = reinterpret_cast<const int32_t*>(di + L.begin);
    A.acc_0 = D(L.acc_0); A.gyr_0 = D(L.gyr_0); A.ba = D(L.ba); A.bg = D(L.bg);
    A.frame_i = b->frame_i ? reinterpret_cast<const int32_t*>(di + L.frame_i) : nullptr;
    A.dt = D(L.dt); A.acc = D(L.acc); A.gyr = D(L.gyr);
    if (reckon) { A.state_p = D(L.sp); A.state_R = D(L.sR); A.state_v = D(L.sv); std::memcpy(A.gravity, b->gravity, sizeof(A.gravity)); }
    A.an2 = h->sigma[0] * h->sigma[0]; A.gn2 = h->sigma[1] * h->sigma[1]; A.aw2 = h->sigma[2] * h->sigma[2]; A.gw2 = h->sigma[3] * h->sigma[3];
    A.blocks = reinterpret_cast<uvs_imu_block*>(dout + L.blocks);
    A.pred_p = reinterpret_cast<double*>(dout + L.pp); A.pred_R = reinterpret_cast<double*>(dout + L.pR); A.pred_v = reinterpret_cast<double*>(dout + L.pv);
    const size_t out_bytes = reckon ? L.out_bytes : L.pp;                       // the predictions lie behind the blocks
    hipStream_t st = h->st;
    UVS_HIP(h->err, hipSetDevice(h->device));
    UVS_HIP(h->err, hipMemcpyAsync(di, hi, L.in_bytes, hipMemcpyHostToDevice, st));
    UVS_HIP(h->err, hipEventRecord(h->ev0, st));
    k_imu_preintegrate<<<n, kWave, 0, st>>>(A);
    UVS_HIP(h->err, hipGetLastError());
    UVS_HIP(h->err, hipEventRecord(h->ev1, st));
    UVS_HIP(h->err, hipMemcpyAsync(h->h_out, dout, out_bytes, hipMemcpyDeviceToHost, st));
    UVS_HIP(h->err, hipStreamSynchronize(st));
    UVS_HIP(h->err, hipEventElapsedTime(&h->device_ms, h->ev0, h->ev1));
    const char* ho = h->h_out;
    std::memcpy(blocks, ho + L.blocks, (size_t)n * sizeof(uvs_imu_block));
    if (reckon) { std::memcpy(pred_p, ho + L.pp, (size_t)n * 24); std::memcpy(pred_R, ho + L.pR, (size_t)n * 72); std::memcpy(pred_v, ho + L.pv, (size_t)n * 24); }
    return UVS_OK;
}

}  // extern "C"
