// uvs_feature_track.hip -- the tracking step of the point front end (reference feature_tracker/src/feature_tracker.cpp:86-95: pyramidal
// Lucas-Kanade with a 21 x 21 window, inBorder; :240-288: liftProjective of the tracked points) behind the uvs_ft_* calls of
// include/uvs_solver.h, whose comment is the statement of the numerics.  gfx950, one stream per handle.  Every sum over the window is an integer
// sum, so a wave reduction and a numpy .sum() agree; the FP64 of an iteration is a handful of operations in a fixed order, and this unit is
// compiled with -ffp-contract=off, so they round as written, which is what tests/ft_ref.py (the numpy restatement, the pin) does.
//
// The handle is csrc/uvs_ft_handle.h, shared with the detection unit (uvs_feature_detect.hip), which reads level 0 of a slot's stored pyramid.
// A tracker keeps, for each of its slots, two pyramids in one device buffer: the stored one and the one the next image is built into; a call
// swaps them.  Rows use pitch_of (uvs_handle.h: the width rounded up to 16 bytes), as the keyframe unit's.  Kernels of one call, in stream order:
//   k_ft_pyramid   one launch per level above 0, the item on the last grid axis, a thread per output pixel: five rows of five reads through
//                  reflect-101 (the 5 x 5 footprints of neighbouring threads overlap in L1 / L2; no LDS stage).
//   k_ft_track     ONE WAVE PER POINT, four waves per workgroup, the points of all items in one grid.  Per level the wave stages the 24 x 24
//                  footprint of the previous pyramid in LDS (its own region: no workgroup barrier, waves run different iteration counts) and
//                  lane t computes I, Dx, Dy of the window pixels t, t + 64, .. (7 per lane; Scharr on the fly from the footprint) into
//                  registers, where they stay for the level's iterations.  An iteration stages the 22 x 22 footprint of the new pyramid,
//                  accumulates (J - I) Dx and (J - I) Dy per lane and reduces them across the wave in 64 bits by a butterfly of shuffles, which
//                  leaves the totals in every lane; every lane then does the same FP64 step, so the loop's branches are wave-uniform.
//                  Lane 0 writes the point's outputs, its lift (uvs_cam_lift, uvs_camera_models.h) and, for uvs_ft_debug_point, the trace.
// The item of a slot that uvs_ft_set_equalize has switched on brings a raw image: it is not copied into level 0 but handed to
// uvsft::equalize_enqueue (uvs_feature_equalize.hip), which writes level 0 on the same stream before k_ft_pyramid runs.
// No kernel uses scratch (build() checks it), none indexes a register array at run time, and no atomic is used.
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

namespace uvsft {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxLevels = UVS_FT_MAX_LEVELS;
constexpr int kWin = UVS_FT_WINDOW, kHalf = kWin / 2, kPix = kWin * kWin;          // 21, 10, 441
constexpr int kPerLane = (kPix + 63) / 64;                                         // 7
constexpr int kPrevSide = kWin + 3, kNewSide = kWin + 1;                           // 24: the window, its bilinear neighbour, Scharr's ring; 22
constexpr int kPyrTW = 64, kPyrTH = 4;
static_assert(kPyrTW * kPyrTH == kThreads, "a thread per output pixel");
static_assert(UVS_FT_TRACE_HEADER + UVS_FT_MAX_ITERATIONS * UVS_FT_TRACE_ITER <= UVS_FT_TRACE_LEVEL, "trace layout");

struct FtItem {                        // device copy of one item: the geometry of its levels and where its two pyramids are
    int W[kMaxLevels], H[kMaxLevels], pitch[kMaxLevels];
    long long prev_off[kMaxLevels], new_off[kMaxLevels];      // byte offsets of the levels of the stored / the new pyramid in the pyramid buffer
};

// ---- one level of the pyramid from the level below it
__global__ void __launch_bounds__(kThreads) k_ft_pyramid(const FtItem* __restrict__ items, uint8_t* __restrict__ pyr, int level) {
    const FtItem* F = items + blockIdx.z;
    const int Wo = F->W[level], Ho = F->H[level], Wi = F->W[level - 1], Hi = F->H[level - 1], Pi = F->pitch[level - 1];
    const int x = blockIdx.x * kPyrTW + (threadIdx.x & 63), y = blockIdx.y * kPyrTH + (threadIdx.x >> 6);
    if (x >= Wo || y >= Ho) return;                           // the grid is sized for the largest item of the batch
    const uint8_t* in = pyr + F->new_off[level - 1];
    const int c0 = reflect101(2 * x - 2, Wi), c1 = reflect101(2 * x - 1, Wi), c2 = 2 * x, c3 = reflect101(2 * x + 1, Wi), c4 = reflect101(2 * x + 2, Wi);
    int v = 0;
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
        const uint8_t* row = in + (size_t)reflect101(2 * y + j, Hi) * Pi;
        const int h = (int)row[c0] + 4 * (int)row[c1] + 6 * (int)row[c2] + 4 * (int)row[c3] + (int)row[c4];
        v += (j == 0 ? 6 : (j == -1 || j == 1) ? 4 : 1) * h;
    }
    pyr[F->new_off[level] + (size_t)y * F->pitch[level] + x] = (uint8_t)((v + 128) >> 8);
}

// ---- the tracker
__device__ __forceinline__ void wave_sync() {                 // orders a wave's own LDS writes before its lanes' reads of them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ long long wave_sum(long long v) { // exact, and the same total in every lane
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

struct Weights { int ix, iy, w00, w01, w10, w11; };

__device__ __forceinline__ Weights window_weights(double cx, double cy) {
    const double ux = cx - (double)kHalf, uy = cy - (double)kHalf;
    const double fx = floor(ux), fy = floor(uy);
    const double a = ux - fx, b = uy - fy;
    Weights w;
    w.ix = (int)fx; w.iy = (int)fy;
    w.w00 = (int)rint((1.0 - a) * (1.0 - b) * 16384.0);
    w.w01 = (int)rint(a * (1.0 - b) * 16384.0);
    w.w10 = (int)rint((1.0 - a) * b * 16384.0);
    w.w11 = 16384 - w.w00 - w.w01 - w.w10;
    return w;
}

__device__ __forceinline__ bool inside(double x, double y, int W, int H) {      // false for a NaN
    return x >= 0.0 && x <= (double)(W - 1) && y >= 0.0 && y <= (double)(H - 1);
}

// side x side pixels of a level from (x0, y0) into the wave's LDS region, through reflect-101
__device__ __forceinline__ void stage(int* __restrict__ dst, const uint8_t* __restrict__ img, int W, int H, int pitch, int x0, int y0, int side, int lane) {
    for (int i = lane; i < side * side; i += 64) {
        const int r = i / side, c = i - r * side;
        dst[i] = (int)img[(size_t)reflect101(y0 + r, H) * pitch + reflect101(x0 + c, W)];
    }
}

__global__ void __launch_bounds__(kThreads) k_ft_track(const FtItem* __restrict__ items, const int* __restrict__ pt_item, const double* __restrict__ pts,
                                                     const uint8_t* __restrict__ pyr, UvsCamDev cam, int levels, int n_total,
                                                     double* __restrict__ next_xy, double* __restrict__ next_norm, int* __restrict__ status,
                                                     int* __restrict__ iterations, double* __restrict__ trace) {
    __shared__ int sPrev[kWaves][kPrevSide * kPrevSide];
    __shared__ int sNew[kWaves][kNewSide * kNewSide];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * kWaves + wave;
    if (g >= n_total) return;                                 // wave-uniform; the kernel has no workgroup barrier
    const FtItem* F = items + pt_item[g];
    int* fp = sPrev[wave];
    int* fn = sNew[wave];
    const double px = pts[2 * g], py = pts[2 * g + 1];
    const bool rec = trace != nullptr && lane == 0;
    double qx = 0.0, qy = 0.0;
    int st = -1, it0 = 0;
    for (int l = levels - 1; l >= 0 && st < 0; --l) {
        const double down = 1.0 / (double)(1 << l), up = (double)(1 << l);
        const double plx = px * down, ply = py * down;
        if (l == levels - 1) { qx = plx; qy = ply; } else { qx = qx * 2.0; qy = qy * 2.0; }
        const int W = F->W[l], H = F->H[l], P = F->pitch[l];
        double* tr = trace + (size_t)l * UVS_FT_TRACE_LEVEL;
        if (rec) { tr[0] = 1.0; tr[1] = plx; tr[2] = ply; }
        if (!inside(plx, ply, W, H)) {
            if (rec) { tr[14] = qx; tr[15] = qy; }
            st = UVS_FT_LOST_OUTSIDE; qx = qx * up; qy = qy * up;
            break;
        }
        const Weights wp = window_weights(plx, ply);
        wave_sync();                                          // the reads of the level before are done
        stage(fp, pyr + F->prev_off[l], W, H, P, wp.ix - 1, wp.iy - 1, kPrevSide, lane);
        wave_sync();
        int I[kPerLane], Dx[kPerLane], Dy[kPerLane];
        long long a11 = 0, a12 = 0, a22 = 0;
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) {
            const int pix = lane + 64 * k;
            I[k] = 0; Dx[k] = 0; Dy[k] = 0;
            if (pix < kPix) {
                const int y = pix / kWin, x = pix - y * kWin;
                const int* f = fp + y * kPrevSide + x;        // f[r * 24 + c]: footprint pixel (x + c, y + r); the window pixel is (x + 1, y + 1)
                int p[4][4];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) p[r][c] = f[r * kPrevSide + c];
                // Scharr at the four pixels the bilinear sample blends: (1, 1), (2, 1), (1, 2), (2, 2) of the 4 x 4 patch
#define UVS_FT_GX(r, c) (3 * (p[(r) - 1][(c) + 1] - p[(r) - 1][(c) - 1]) + 10 * (p[(r)][(c) + 1] - p[(r)][(c) - 1]) + 3 * (p[(r) + 1][(c) + 1] - p[(r) + 1][(c) - 1]))
#define UVS_FT_GY(r, c) (3 * (p[(r) + 1][(c) - 1] - p[(r) - 1][(c) - 1]) + 10 * (p[(r) + 1][(c)] - p[(r) - 1][(c)]) + 3 * (p[(r) + 1][(c) + 1] - p[(r) - 1][(c) + 1]))
                const int sI = wp.w00 * p[1][1] + wp.w01 * p[1][2] + wp.w10 * p[2][1] + wp.w11 * p[2][2];
                const int sX = wp.w00 * UVS_FT_GX(1, 1) + wp.w01 * UVS_FT_GX(1, 2) + wp.w10 * UVS_FT_GX(2, 1) + wp.w11 * UVS_FT_GX(2, 2);
                const int sY = wp.w00 * UVS_FT_GY(1, 1) + wp.w01 * UVS_FT_GY(1, 2) + wp.w10 * UVS_FT_GY(2, 1) + wp.w11 * UVS_FT_GY(2, 2);
#undef UVS_FT_GX
#undef UVS_FT_GY
                I[k] = (sI + 256) >> 9; Dx[k] = (sX + 8192) >> 14; Dy[k] = (sY + 8192) >> 14;
                a11 += (long long)Dx[k] * Dx[k]; a12 += (long long)Dx[k] * Dy[k]; a22 += (long long)Dy[k] * Dy[k];
            }
        }
        const long long A11i = wave_sum(a11), A12i = wave_sum(a12), A22i = wave_sum(a22);
        const double scale = 1.0 / 1048576.0;                 // 2^-20
        const double A11 = (double)A11i * scale, A12 = (double)A12i * scale, A22 = (double)A22i * scale;
        const double D = A11 * A22 - A12 * A12;
        const double t = A11 - A22;
        const double min_eig = (A22 + A11 - sqrt(t * t + 4.0 * A12 * A12)) / 882.0;
        const bool flat = min_eig < 1e-4 || D < 1.1920929e-7;
        if (rec) {
            tr[3] = wp.w00; tr[4] = wp.w01; tr[5] = wp.w10; tr[6] = wp.w11; tr[7] = (double)A11i; tr[8] = (double)A12i; tr[9] = (double)A22i;
            tr[10] = D; tr[11] = min_eig; tr[12] = flat ? 1.0 : 0.0;
        }
        if (flat) {
            if (rec) { tr[14] = qx; tr[15] = qy; }
            if (l == 0) st = UVS_FT_LOST_FLAT;
            continue;
        }
        int n = 0;
        double pdx = 0.0, pdy = 0.0;
        for (int j = 0; j < UVS_FT_MAX_ITERATIONS; ++j) {
            if (!inside(qx, qy, W, H)) { st = UVS_FT_LOST_OUTSIDE; break; }
            const Weights wq = window_weights(qx, qy);
            wave_sync();
            stage(fn, pyr + F->new_off[l], W, H, P, wq.ix, wq.iy, kNewSide, lane);
            wave_sync();
            long long s1 = 0, s2 = 0;
#pragma unroll
            for (int k = 0; k < kPerLane; ++k) {
                const int pix = lane + 64 * k;
                if (pix < kPix) {
                    const int y = pix / kWin, x = pix - y * kWin;
                    const int* f = fn + y * kNewSide + x;
                    const int sJ = wq.w00 * f[0] + wq.w01 * f[1] + wq.w10 * f[kNewSide] + wq.w11 * f[kNewSide + 1];
                    const int d = ((sJ + 256) >> 9) - I[k];
                    s1 += (long long)d * Dx[k]; s2 += (long long)d * Dy[k];
                }
            }
            const long long b1i = wave_sum(s1), b2i = wave_sum(s2);
            const double b1 = (double)b1i * scale, b2 = (double)b2i * scale;
            const double dx = (A12 * b2 - A22 * b1) / D;
            const double dy = (A12 * b1 - A11 * b2) / D;
            qx = qx + dx; qy = qy + dy;
            ++n;
            bool stop = dx * dx + dy * dy <= 1e-4;
            if (!stop && j > 0 && fabs(dx + pdx) < 0.01 && fabs(dy + pdy) < 0.01) {
                qx = qx - 0.5 * dx; qy = qy - 0.5 * dy;
                stop = true;
            }
            if (rec) {
                double* ti = tr + UVS_FT_TRACE_HEADER + UVS_FT_TRACE_ITER * j;
                ti[0] = wq.w00; ti[1] = wq.w01; ti[2] = wq.w10; ti[3] = wq.w11; ti[4] = (double)b1i; ti[5] = (double)b2i;
                ti[6] = dx; ti[7] = dy; ti[8] = qx; ti[9] = qy;
            }
            if (stop) break;
            pdx = dx; pdy = dy;
        }
        if (rec) { tr[13] = (double)n; tr[14] = qx; tr[15] = qy; }
        if (st == UVS_FT_LOST_OUTSIDE) { qx = qx * up; qy = qy * up; }
        if (l == 0) it0 = n;
    }
    if (st < 0) {                                             // level 0 was left with an estimate
        const int W = F->W[0], H = F->H[0];
        if (!inside(qx, qy, W, H)) st = UVS_FT_LOST_OUTSIDE;
        else {
            const double xr = rint(qx), yr = rint(qy);
            st = (1.0 <= xr && xr < (double)(W - 1) && 1.0 <= yr && yr < (double)(H - 1)) ? UVS_FT_TRACKED : UVS_FT_LOST_BORDER;
        }
    }
    if (lane == 0) {
        double mx = 0.0, my = 0.0;
        if (st == UVS_FT_TRACKED) { double ray[3]; uvs_cam_lift(cam, qx, qy, ray, mx, my); }
        next_xy[2 * g] = qx; next_xy[2 * g + 1] = qy;
        next_norm[2 * g] = mx; next_norm[2 * g + 1] = my;
        status[g] = st; iterations[g] = it0;
    }
}

}  // namespace uvsft

using namespace uvsft;

namespace {

struct FtOutLayout { size_t norm, status, iters, trace, total; };
// next_xy | next_norm | status | iterations | trace for n points
inline FtOutLayout out_layout(size_t n) {
    FtOutLayout L;
    L.norm = n * 16; L.status = L.norm + n * 16; L.iters = L.status + n * 4;
    L.trace = align_up(L.iters + n * 4, 16);
    L.total = L.trace + (size_t)kMaxLevels * UVS_FT_TRACE_LEVEL * 8;
    return L;
}

int ft_run(uvs_ft_tracker* h, const char* who_, int n_items, const uvs_ft_item* items, const uvs_kf_camera* camera, double* next_xy, int32_t* status,
           int32_t* iterations, double* next_norm, int32_t* results, double* trace) {
    const std::string fn = who_;
    h->err.clear();
    if (n_items < 1 || !items || (!camera && h->model.model < 0) || !next_xy || !status || !iterations || !next_norm || !results) {
        h->err = fn + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG;
    }
    if (n_items > h->max_streams) { h->err = fn + ": more items than the slots given to uvs_ft_create"; return UVS_ERR_CAPACITY; }
    UvsCamDev cam;
    if (const int rc = uvs_cam_of_call(h->model, camera, fn, h->err, &cam)) return rc;
    const int min_size = UVS_FT_MIN_SIZE << (h->levels - 1);
    std::vector<char> seen(h->max_streams, 0);
    size_t total = 0;
    for (int i = 0; i < n_items; ++i) {
        const uvs_ft_item& it = items[i];
        const std::string who = fn + ": item " + std::to_string(i);
        if (!it.image || it.n_points < 0 || (it.n_points > 0 && !it.points_xy)) { h->err = who + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG; }
        if (it.stream < 0 || it.stream >= h->max_streams) { h->err = who + ": the stream is not a slot of the handle"; return UVS_ERR_INVALID_ARG; }
        if (seen[it.stream]) { h->err = who + ": the stream appears twice in the call"; return UVS_ERR_INVALID_ARG; }
        seen[it.stream] = 1;
        if (it.width < min_size || it.height < min_size) { h->err = who + ": width and height must be at least 24 << (levels - 1)"; return UVS_ERR_INVALID_ARG; }
        if (it.width > h->max_width || it.height > h->max_height || it.n_points > h->max_points) {
            h->err = who + " exceeds the capacity given to uvs_ft_create"; return UVS_ERR_CAPACITY;
        }
        const uvs_ft_tracker::Slot& s = h->slots[it.stream];
        if (!s.holds && it.n_points > 0) { h->err = who + ": points for a slot that holds no image"; return UVS_ERR_INVALID_ARG; }
        if (s.holds && (s.W != it.width || s.H != it.height)) { h->err = who + ": the image size differs from the slot's (uvs_ft_reset first)"; return UVS_ERR_INVALID_ARG; }
        for (int k = 0; k < 2 * it.n_points; ++k)
            if (!std::isfinite(it.points_xy[k]) || std::fabs(it.points_xy[k]) > UVS_KF_MAX_COORD) {
                h->err = who + ": a point is not finite or beyond UVS_KF_MAX_COORD"; return UVS_ERR_INVALID_ARG;
            }
        total += (size_t)it.n_points;
    }
    // packed meta data: items | the item of every point | the points; the images follow in the pinned buffer only, each goes straight into its slot
    const size_t o_pi = align_up(n_items * sizeof(FtItem), 16), o_pts = align_up(o_pi + total * 4, 16), meta = o_pts + total * 16;
    FtItem* hf = reinterpret_cast<FtItem*>(h->h_in.get());
    int* h_pi = reinterpret_cast<int*>(h->h_in + o_pi);
    size_t po = 0;
    int top_w[kMaxLevels] = {0, 0, 0, 0}, top_h[kMaxLevels] = {0, 0, 0, 0};
    std::vector<EqJob> eq_jobs;                               // the items of equalized slots (uvs_ft_set_equalize); empty: the call is what it was without them
    for (int i = 0; i < n_items; ++i) {
        const uvs_ft_item& it = items[i];
        const uvs_ft_tracker::Slot& s = h->slots[it.stream];
        FtItem d;
        long long off[kMaxLevels];
        pyramid_layout(it.width, it.height, h->levels, d.W, d.H, d.pitch, off);
        const int stored = s.cur, fresh = 1 - s.cur;
        for (int l = 0; l < kMaxLevels; ++l) {
            d.prev_off[l] = (long long)((size_t)(2 * it.stream + stored) * h->pyr_bytes) + off[l];
            d.new_off[l] = (long long)((size_t)(2 * it.stream + fresh) * h->pyr_bytes) + off[l];
            top_w[l] = std::max(top_w[l], d.W[l]); top_h[l] = std::max(top_h[l], d.H[l]);
        }
        hf[i] = d;
        for (int k = 0; k < it.n_points; ++k) h_pi[po + k] = i;
        if (it.n_points) std::memcpy(h->h_in + o_pts + po * 16, it.points_xy, (size_t)it.n_points * 16);
        po += it.n_points;
        if (s.equalize) {                                     // the image is raw: uvs_feature_equalize.hip stages it and writes level 0
            eq_jobs.push_back(EqJob{it.image, it.width, it.height, s.eq_clip, s.eq_tiles_x, s.eq_tiles_y, h->d_pyr + d.new_off[0], d.pitch[0]});
            continue;
        }
        char* dst = h->h_in + h->in_meta + (size_t)i * h->img_slot;
        if (d.pitch[0] == d.W[0]) std::memcpy(dst, it.image, (size_t)d.W[0] * d.H[0]);
        else for (int y = 0; y < d.H[0]; ++y) { std::memcpy(dst + (size_t)y * d.pitch[0], it.image + (size_t)y * d.W[0], d.W[0]); }
    }
    const FtOutLayout L = out_layout(total);
    const FtItem* dF = reinterpret_cast<const FtItem*>(h->d_in.get());
    const int* dPi = reinterpret_cast<const int*>(h->d_in + o_pi);
    const double* dPts = reinterpret_cast<const double*>(h->d_in + o_pts);
    double* dXy = reinterpret_cast<double*>(h->d_out.get());
    double* dNorm = reinterpret_cast<double*>(h->d_out + L.norm);
    int* dSt = reinterpret_cast<int*>(h->d_out + L.status);
    int* dIt = reinterpret_cast<int*>(h->d_out + L.iters);
    double* dTrace = reinterpret_cast<double*>(h->d_out + L.trace);
    hipStream_t st = h->st;
    UVS_HIP(h->err, hipSetDevice(h->device));
    UVS_HIP(h->err, hipEventRecord(h->ev0, st));
    UVS_HIP(h->err, hipMemcpyAsync(h->d_in, h->h_in, meta, hipMemcpyHostToDevice, st));
    for (int i = 0; i < n_items; ++i)                         // level 0 of the new pyramid is the repacked image ...
        if (!h->slots[items[i].stream].equalize)
            UVS_HIP(h->err, hipMemcpyAsync(h->d_pyr + hf[i].new_off[0], h->h_in + h->in_meta + (size_t)i * h->img_slot, (size_t)hf[i].pitch[0] * hf[i].H[0],
                                           hipMemcpyHostToDevice, st));
    if (!eq_jobs.empty())                                     // ... or, of an equalized slot, the raw image through CLAHE
        if (const int rc = equalize_enqueue(h, (int)eq_jobs.size(), eq_jobs.data(), nullptr)) return rc;
    for (int l = 1; l < h->levels; ++l)
        k_ft_pyramid<<<dim3((top_w[l] + kPyrTW - 1) / kPyrTW, (top_h[l] + kPyrTH - 1) / kPyrTH, n_items), kThreads, 0, st>>>(dF, h->d_pyr, l);
    if (total) {
        if (trace) UVS_HIP(h->err, hipMemsetAsync(dTrace, 0, (size_t)kMaxLevels * UVS_FT_TRACE_LEVEL * 8, st));
        k_ft_track<<<(unsigned)((total + kWaves - 1) / kWaves), kThreads, 0, st>>>(dF, dPi, dPts, h->d_pyr, cam, h->levels, (int)total, dXy, dNorm, dSt, dIt,
                                                                                 trace ? dTrace : nullptr);
    }
    UVS_HIP(h->err, hipGetLastError());
    if (total) UVS_HIP(h->err, hipMemcpyAsync(h->h_out, h->d_out, trace ? L.total : L.trace, hipMemcpyDeviceToHost, st));
    UVS_HIP(h->err, hipEventRecord(h->ev1, st));
    UVS_HIP(h->err, hipStreamSynchronize(st));
    UVS_HIP(h->err, hipEventElapsedTime(&h->device_ms, h->ev0, h->ev1));
    for (int i = 0; i < n_items; ++i) {                       // the new pyramids are the stored ones now
        uvs_ft_tracker::Slot& s = h->slots[items[i].stream];
        s.cur = 1 - s.cur; s.holds = true; s.W = items[i].width; s.H = items[i].height;
    }
    if (total) {
        std::memcpy(next_xy, h->h_out, total * 16);
        std::memcpy(next_norm, h->h_out + L.norm, total * 16);
        std::memcpy(status, h->h_out + L.status, total * 4);
        std::memcpy(iterations, h->h_out + L.iters, total * 4);
        if (trace) std::memcpy(trace, h->h_out + L.trace, (size_t)kMaxLevels * UVS_FT_TRACE_LEVEL * 8);
    }
    po = 0;
    for (int i = 0; i < n_items; ++i) {
        int n = 0;
        for (int k = 0; k < items[i].n_points; ++k) n += status[po + k] == UVS_FT_TRACKED;
        results[i] = n;
        po += items[i].n_points;
    }
    return UVS_OK;
}

}  // namespace

extern "C" {

int uvs_ft_create(int device, int max_streams, int max_width, int max_height, int levels, int max_points, uvs_ft_tracker** out) {
    if (!out) return UVS_ERR_INVALID_ARG;
    *out = nullptr;
    if (max_streams < 1 || max_points < 1 || levels < 1 || levels > UVS_FT_MAX_LEVELS) return UVS_ERR_INVALID_ARG;
    if (max_width < (UVS_FT_MIN_SIZE << (levels - 1)) || max_height < (UVS_FT_MIN_SIZE << (levels - 1))) return UVS_ERR_INVALID_ARG;
    if (max_streams > UVS_FT_MAX_STREAMS || max_width > UVS_KF_MAX_WIDTH || max_height > UVS_KF_MAX_HEIGHT || max_points > UVS_FT_MAX_POINTS) return UVS_ERR_CAPACITY;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return UVS_ERR_NO_DEVICE;
    uvs_ft_tracker* h = new uvs_ft_tracker();
    h->max_streams = max_streams; h->max_width = max_width; h->max_height = max_height; h->levels = levels; h->max_points = max_points;
    h->slots.resize(max_streams);
    int W[kMaxLevels], H[kMaxLevels], P[kMaxLevels]; long long off[kMaxLevels];
    h->pyr_bytes = pyramid_layout(max_width, max_height, levels, W, H, P, off);      // every level of a smaller image is no larger than the level here
    h->img_slot = align_up((size_t)P[0] * H[0], 256);
    const size_t S = max_streams, N = S * max_points;
    h->in_meta = align_up(align_up(align_up(S * sizeof(FtItem), 16) + N * 4, 16) + N * 16, 256);
    const size_t out_bytes = out_layout(N).total;
    int rc = h->open(device);
    if (rc == UVS_OK && (rc = h->d_pyr.ensure(2 * S * h->pyr_bytes, h->err)) == UVS_OK && (rc = h->d_in.ensure(h->in_meta, h->err)) == UVS_OK &&
        (rc = h->d_out.ensure(out_bytes, h->err)) == UVS_OK && (rc = h->h_in.ensure(h->in_meta + S * h->img_slot, h->err)) == UVS_OK) {
        rc = h->h_out.ensure(out_bytes, h->err);
    }
    if (rc != UVS_OK) { uvs_ft_destroy(h); return rc; }
    *out = h;
    return UVS_OK;
}

void uvs_ft_destroy(uvs_ft_tracker* h) { if (h) { h->close(); delete h; } }

const char* uvs_ft_last_error(const uvs_ft_tracker* h) { return h ? h->err.c_str() : "null feature tracker"; }

double uvs_ft_last_device_ms(const uvs_ft_tracker* h) { return h ? (double)h->device_ms : 0.0; }

int uvs_ft_reset(uvs_ft_tracker* h, int stream) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    if (stream < 0 || stream >= h->max_streams) { h->err = "uvs_ft_reset: the stream is not a slot of the handle"; return UVS_ERR_INVALID_ARG; }
    h->slots[stream] = uvs_ft_tracker::Slot();
    return UVS_OK;
}

int uvs_ft_track(uvs_ft_tracker* h, int n_items, const uvs_ft_item* items, const uvs_kf_camera* camera, double* next_xy, int32_t* status,
                 int32_t* iterations, double* next_norm, int32_t* results) {
    if (!h) return UVS_ERR_INVALID_ARG;
    return ft_run(h, "uvs_ft_track", n_items, items, camera, next_xy, status, iterations, next_norm, results, nullptr);
}

int uvs_ft_debug_pyramid(uvs_ft_tracker* h, int stream, int32_t* level_sizes, uint8_t* pixels, int64_t pixels_capacity) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    if (!level_sizes || !pixels || stream < 0 || stream >= h->max_streams) { h->err = "uvs_ft_debug_pyramid: null pointer or bad stream"; return UVS_ERR_INVALID_ARG; }
    const uvs_ft_tracker::Slot& s = h->slots[stream];
    if (!s.holds) { h->err = "uvs_ft_debug_pyramid: the slot holds no image"; return UVS_ERR_INVALID_ARG; }
    int W[kMaxLevels], H[kMaxLevels], P[kMaxLevels]; long long off[kMaxLevels];
    pyramid_layout(s.W, s.H, h->levels, W, H, P, off);
    int64_t need = 0;
    for (int l = 0; l < h->levels; ++l) need += (int64_t)W[l] * H[l];
    if (pixels_capacity < need) { h->err = "uvs_ft_debug_pyramid: pixels_capacity is too small"; return UVS_ERR_CAPACITY; }
    UVS_HIP(h->err, hipSetDevice(h->device));
    const uint8_t* base = h->d_pyr + (size_t)(2 * stream + s.cur) * h->pyr_bytes;
    for (int l = 0; l < h->levels; ++l) {
        level_sizes[2 * l] = W[l]; level_sizes[2 * l + 1] = H[l];
        UVS_HIP(h->err, hipMemcpy2D(pixels, W[l], base + off[l], P[l], W[l], H[l], hipMemcpyDeviceToHost));
        pixels += (size_t)W[l] * H[l];
    }
    return UVS_OK;
}

int uvs_ft_debug_point(uvs_ft_tracker* h, const uvs_ft_item* item, const uvs_kf_camera* camera, double* trace, double* next_xy, int32_t* status,
                       int32_t* iterations, double* next_norm) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    if (!item || !trace || item->n_points != 1) { h->err = "uvs_ft_debug_point: null pointer, or not exactly one point"; return UVS_ERR_INVALID_ARG; }
    int32_t result = 0;
    return ft_run(h, "uvs_ft_debug_point", 1, item, camera, next_xy, status, iterations, next_norm, &result, trace);
}

}  // extern "C"
