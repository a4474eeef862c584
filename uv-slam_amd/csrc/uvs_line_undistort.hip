// uvs_line_undistort.hip -- undistortion of the line front end's images (the place of imageUndistortion and the margin crop in the reference's
// readImage4Line) behind uvs_lt_set_undistort, uvs_lt_set_undistort_model, uvs_lt_set_remap, uvs_lt_get_remap and uvs_lt_undistort of include/uvs_solver.h: a fixed-point
// map per slot and a bilinear remap with a zero border, the project's own rule, stated in the header and restated in tests/ud_ref.py, which
// this unit is held to word for word and byte for byte.  The handle is the line tracker's (csrc/uvs_lt_handle.h); uvs_lt_detect_track calls
// ud_launch for the items of mapped slots between its upload and its first kernel.  gfx950, the handle's one stream.
//
// This unit is compiled with -ffp-contract=off.  Two kernels:
//   k_lt_ud_map     once per uvs_lt_set_undistort or uvs_lt_set_undistort_model: a lane per output pixel, the output pinhole's ray through
//                   uvs_cam_project (csrc/uvs_camera_models.h; for a pinhole the header's FP64 chain), two int32 words out
//   k_lt_ud_remap   one launch for all items of a call (the item in grid.y).  The output image is packed (stride = Wo), so it and its map are
//                   flat arrays: a lane owns the four consecutive output pixels 4 t .. 4 t + 3, reads their eight map words as two 16-byte
//                   loads, its sixteen taps as byte loads (a raw frame stays in L2), and stores its four results as one dword; consecutive
//                   lanes so read consecutive 32 bytes of the map and write consecutive dwords.  The last lane of an image whose pixel count is
//                   no multiple of four handles the 1 .. 3 pixels left with word loads and byte stores.  Integers only: no LDS, no atomics,
//                   no floating point.
// Neither kernel uses scratch memory.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/uvs_solver.h"
#include "uvs_camera_models.h"
#include "uvs_lt_handle.h"

namespace uvslt {

constexpr int kUdThreads = 256;
constexpr int kUdLimit = 1 << 24;              // |X|, |Y| of a map word

struct UdOutput { double fx, fy, cx, cy; int Wo, Ho, cm, rm; };      // the pinhole of the undistorted image, its size, the margins

// ---- the map: the header's chain, one rounding per operation
// a raw position in pixels -> a map word: 5 fractional bits, clamped, a value that is not finite becomes -2^24
__device__ __forceinline__ int32_t ud_fix(double m) {
    const double v = rint(32.0 * m);
    if (!isfinite(v)) return -kUdLimit;
    return (int32_t)fmin(fmax(v, (double)-kUdLimit), (double)kUdLimit);
}

__global__ void __launch_bounds__(kUdThreads) k_lt_ud_map(UvsCamDev cam, UdOutput A, int32_t* __restrict__ map) {
    const int t = blockIdx.x * kUdThreads + threadIdx.x;
    if (t >= A.Wo * A.Ho) return;
    const int vo = t / A.Wo, uo = t - vo * A.Wo;
    const double u = (double)(uo + A.cm), v = (double)(vo + A.rm);
    const double x = (u - A.cx) / A.fx, y = (v - A.cy) / A.fy;
    double mx, my;
    uvs_cam_project(cam, x, y, 1.0, mx, my);
    map[2 * (size_t)t] = ud_fix(mx); map[2 * (size_t)t + 1] = ud_fix(my);
}

// ---- the remap
__device__ __forceinline__ unsigned ud_tap(const uint8_t* __restrict__ S, int W, int H, int y, int x) {
    return ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H) ? (unsigned)S[y * W + x] : 0u;      // y W + x < W H, which fits an int
}

__device__ __forceinline__ unsigned ud_pixel(const uint8_t* __restrict__ S, int W, int H, int X, int Y) {
    const int xi = X >> 5, yi = Y >> 5;        // |xi|, |yi| <= 2^19: xi + 1 and yi + 1 do not overflow
    const unsigned ax = (unsigned)(X & 31), ay = (unsigned)(Y & 31);
    const unsigned p00 = ud_tap(S, W, H, yi, xi), p01 = ud_tap(S, W, H, yi, xi + 1), p10 = ud_tap(S, W, H, yi + 1, xi), p11 = ud_tap(S, W, H, yi + 1, xi + 1);
    return ((32u - ax) * (32u - ay) * p00 + ax * (32u - ay) * p01 + (32u - ax) * ay * p10 + ax * ay * p11 + 512u) >> 10;
}

__global__ void __launch_bounds__(kUdThreads) k_lt_ud_remap(const UdItem* __restrict__ items, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst) {
    const UdItem I = items[blockIdx.y];
    const int p = 4 * (blockIdx.x * kUdThreads + threadIdx.x);      // the lane's first output pixel
    if (p >= I.n_out) return;
    const uint8_t* S = src + I.src_off;
    uint8_t* D = dst + I.dst_off;
    if (p + 4 <= I.n_out) {
        const int4* m = reinterpret_cast<const int4*>(I.map + 2 * (size_t)p);      // 8 p bytes into a hipMalloc'ed array, p a multiple of 4
        const int4 a = m[0], b = m[1];
        const unsigned o = ud_pixel(S, I.W, I.H, a.x, a.y) | ud_pixel(S, I.W, I.H, a.z, a.w) << 8 | ud_pixel(S, I.W, I.H, b.x, b.y) << 16 |
                           ud_pixel(S, I.W, I.H, b.z, b.w) << 24;
        *reinterpret_cast<unsigned*>(D + p) = o;                                    // dst_off is a multiple of 256 and p of 4
    } else {
        for (int q = p; q < I.n_out; ++q) D[q] = (uint8_t)ud_pixel(S, I.W, I.H, I.map[2 * (size_t)q], I.map[2 * (size_t)q + 1]);
    }
}

int ud_launch(uvs_lt_tracker* h, int n, const UdItem* items, const uint8_t* src, uint8_t* dst, int max_out) {
    const int quads = (max_out + 3) / 4;
    k_lt_ud_remap<<<dim3((quads + kUdThreads - 1) / kUdThreads, n), kUdThreads, 0, h->st>>>(items, src, dst);
    UVS_HIP(h->err, hipGetLastError());
    return UVS_OK;
}

namespace {

struct UdLayout { size_t o_img, in_used, o_out, used; };

// uvs_lt_undistort's one buffer: items | raw images (uploaded up to in_used) | outputs (downloaded from o_out)
UdLayout ud_layout(size_t n, const std::vector<size_t>& src_bytes, const std::vector<size_t>& out_bytes, std::vector<size_t>* src_off, std::vector<size_t>* out_off) {
    UdLayout Y;
    UvsArena a;
    (void)a.take(n * sizeof(UdItem));
    Y.o_img = a.o;
    for (size_t b : src_bytes) { const size_t at = a.take(b); if (src_off) src_off->push_back(at); }
    Y.in_used = Y.o_out = a.o;
    for (size_t b : out_bytes) { const size_t at = a.take(b); if (out_off) out_off->push_back(at); }
    Y.used = a.o;
    return Y;
}

// the size checks of the set calls
int ud_check_sizes(uvs_lt_tracker* h, const std::string& fn, int stream, int W, int H, int Wo, int Ho) {
    if (stream < 0 || stream >= h->max_streams) { h->err = fn + ": stream outside the handle's slots"; return UVS_ERR_INVALID_ARG; }
    if (W < UVS_LT_MIN_SIZE || H < UVS_LT_MIN_SIZE || Wo < UVS_LT_MIN_SIZE || Ho < UVS_LT_MIN_SIZE) {
        h->err = fn + ": a source or output width or height below UVS_LT_MIN_SIZE"; return UVS_ERR_INVALID_ARG;
    }
    if (W > h->max_width || H > h->max_height || Wo > h->max_width || Ho > h->max_height) {
        h->err = fn + " exceeds the capacity given to uvs_lt_create"; return UVS_ERR_CAPACITY;
    }
    return UVS_OK;
}

// What the two calls that build a slot's map on the device share once their camera has passed: the checks of the margins and the sizes, the
// slot's map memory, the kernel and the wait.  A holds the output pinhole; its sizes and margins are filled in here.
int ud_build_map(uvs_lt_tracker* h, const std::string& fn, int stream, const UvsCamDev& cam, UdOutput A, int width, int height, int col_margin, int row_margin) {
    if (col_margin < 0 || row_margin < 0) { h->err = fn + ": negative margin"; return UVS_ERR_INVALID_ARG; }
    if (width < UVS_LT_MIN_SIZE || height < UVS_LT_MIN_SIZE || col_margin > width / 2 || row_margin > height / 2) {      // before W - 2 cm is formed
        h->err = fn + ": a source or output width or height below UVS_LT_MIN_SIZE"; return UVS_ERR_INVALID_ARG;
    }
    const int Wo = width - 2 * col_margin, Ho = height - 2 * row_margin;
    int rc = ud_check_sizes(h, fn, stream, width, height, Wo, Ho);
    if (rc != UVS_OK) return rc;
    LtUndistort& U = h->ud[stream];
    UVS_HIP(h->err, hipSetDevice(h->device));
    U.on = false;                               // every argument has passed: a HIP failure below leaves the slot without a map, not with half of one
    if ((rc = U.map.ensure(8 * (size_t)Wo * Ho, h->err)) != UVS_OK) return rc;
    A.Wo = Wo; A.Ho = Ho; A.cm = col_margin; A.rm = row_margin;
    k_lt_ud_map<<<(Wo * Ho + kUdThreads - 1) / kUdThreads, kUdThreads, 0, h->st>>>(cam, A, U.map.get());
    UVS_HIP(h->err, hipGetLastError());
    UVS_HIP(h->err, hipStreamSynchronize(h->st));
    U.W = width; U.H = height; U.Wo = Wo; U.Ho = Ho; U.on = true;
    return UVS_OK;
}

}  // namespace

}  // namespace uvslt

using namespace uvslt;

extern "C" {

int uvs_lt_set_undistort(uvs_lt_tracker* h, int stream, const uvs_kf_camera* camera, int width, int height, int col_margin, int row_margin) {
    if (!h) return UVS_ERR_INVALID_ARG;
    const std::string fn = "uvs_lt_set_undistort";
    h->err.clear();
    if (stream < 0 || stream >= h->max_streams) { h->err = fn + ": stream outside the handle's slots"; return UVS_ERR_INVALID_ARG; }
    if (!camera) { h->ud[stream].on = false; return UVS_OK; }
    const uvs_camera_model model = uvs_cam_pinhole(*camera);
    UvsCamDev cam;
    if (const int rc = uvs_cam_take(&model, fn, h->err, &cam, true)) return rc;
    UdOutput A = {};
    A.fx = camera->fx; A.fy = camera->fy; A.cx = camera->cx; A.cy = camera->cy;      // the output pinhole is the camera's own
    return ud_build_map(h, fn, stream, cam, A, width, height, col_margin, row_margin);
}

int uvs_lt_set_undistort_model(uvs_lt_tracker* h, int stream, const uvs_camera_model* model, int width, int height, int col_margin, int row_margin,
                               double fx_out, double fy_out, double cx_out, double cy_out) {
    if (!h) return UVS_ERR_INVALID_ARG;
    const std::string fn = "uvs_lt_set_undistort_model";
    h->err.clear();
    if (stream < 0 || stream >= h->max_streams) { h->err = fn + ": stream outside the handle's slots"; return UVS_ERR_INVALID_ARG; }
    if (!model) { h->ud[stream].on = false; return UVS_OK; }
    UvsCamDev cam;
    if (const int rc = uvs_cam_take(model, fn, h->err, &cam)) return rc;
    if (!std::isfinite(fx_out) || !std::isfinite(fy_out) || !std::isfinite(cx_out) || !std::isfinite(cy_out) || !(fx_out > 0.0) || !(fy_out > 0.0)) {
        h->err = fn + ": the output pinhole must be finite, fx_out and fy_out positive"; return UVS_ERR_INVALID_ARG;
    }
    UdOutput A = {};
    A.fx = fx_out; A.fy = fy_out; A.cx = cx_out; A.cy = cy_out;
    return ud_build_map(h, fn, stream, cam, A, width, height, col_margin, row_margin);
}

int uvs_lt_set_remap(uvs_lt_tracker* h, int stream, int src_width, int src_height, int out_width, int out_height, const int32_t* map_xy) {
    if (!h) return UVS_ERR_INVALID_ARG;
    const std::string fn = "uvs_lt_set_remap";
    h->err.clear();
    if (!map_xy) { h->err = fn + ": null pointer"; return UVS_ERR_INVALID_ARG; }
    int rc = ud_check_sizes(h, fn, stream, src_width, src_height, out_width, out_height);
    if (rc != UVS_OK) return rc;
    const size_t words = 2 * (size_t)out_width * out_height;
    std::vector<int32_t> clamped(words);
    for (size_t i = 0; i < words; ++i) clamped[i] = std::min(std::max(map_xy[i], -kUdLimit), kUdLimit);
    LtUndistort& U = h->ud[stream];
    UVS_HIP(h->err, hipSetDevice(h->device));
    UVS_HIP(h->err, hipStreamSynchronize(h->st));
    if ((rc = U.map.ensure(4 * words, h->err)) != UVS_OK) { U.on = false; return rc; }
    U.on = false;
    UVS_HIP(h->err, hipMemcpy(U.map, clamped.data(), 4 * words, hipMemcpyHostToDevice));
    U.W = src_width; U.H = src_height; U.Wo = out_width; U.Ho = out_height; U.on = true;
    return UVS_OK;
}

int uvs_lt_get_remap(uvs_lt_tracker* h, int stream, int32_t* out_width, int32_t* out_height, int32_t* map_xy) {
    if (!h) return UVS_ERR_INVALID_ARG;
    const std::string fn = "uvs_lt_get_remap";
    h->err.clear();
    if (!out_width || !out_height) { h->err = fn + ": null pointer"; return UVS_ERR_INVALID_ARG; }
    if (stream < 0 || stream >= h->max_streams) { h->err = fn + ": stream outside the handle's slots"; return UVS_ERR_INVALID_ARG; }
    const LtUndistort& U = h->ud[stream];
    if (!U.on) { h->err = fn + ": the slot has no map"; return UVS_ERR_INVALID_ARG; }
    *out_width = U.Wo; *out_height = U.Ho;
    if (map_xy) {
        UVS_HIP(h->err, hipSetDevice(h->device));
        UVS_HIP(h->err, hipStreamSynchronize(h->st));
        UVS_HIP(h->err, hipMemcpy(map_xy, U.map, 8 * (size_t)U.Wo * U.Ho, hipMemcpyDeviceToHost));
    }
    return UVS_OK;
}

int uvs_lt_undistort(uvs_lt_tracker* h, int n_images, const uvs_lt_det_item* images, uint8_t* out) {
    if (!h) return UVS_ERR_INVALID_ARG;
    const std::string fn = "uvs_lt_undistort";
    h->err.clear();
    if (n_images < 1 || !images || !out) { h->err = fn + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG; }
    if (n_images > h->max_streams) { h->err = fn + ": more images than the capacity given to uvs_lt_create"; return UVS_ERR_CAPACITY; }
    std::vector<size_t> src_bytes, out_bytes, src_off, out_off;
    for (int b = 0; b < n_images; ++b) {
        const uvs_lt_det_item& it = images[b];
        const std::string who = fn + ": image " + std::to_string(b);
        if (!it.image) { h->err = who + ": null pointer"; return UVS_ERR_INVALID_ARG; }
        if (it.stream < 0 || it.stream >= h->max_streams) { h->err = who + ": stream outside the handle's slots"; return UVS_ERR_INVALID_ARG; }
        const LtUndistort& U = h->ud[it.stream];
        if (!U.on) { h->err = who + ": the slot has no map"; return UVS_ERR_INVALID_ARG; }
        if (it.width != U.W || it.height != U.H) { h->err = who + ": width or height is not the map's source size"; return UVS_ERR_INVALID_ARG; }
        src_bytes.push_back((size_t)U.W * U.H); out_bytes.push_back((size_t)U.Wo * U.Ho);
    }
    // the staging, at the handle's capacity, by the first call
    const size_t B = h->max_streams, px = (size_t)h->max_width * h->max_height;
    const size_t cap = ud_layout(B, std::vector<size_t>(B, px), std::vector<size_t>(B, px), nullptr, nullptr).used;
    int rc;
    if ((rc = h->h_ud_io.ensure(cap, h->err)) != UVS_OK || (rc = h->d_ud_io.ensure(cap, h->err)) != UVS_OK) return rc;
    const UdLayout Y = ud_layout(n_images, src_bytes, out_bytes, &src_off, &out_off);
    UdItem* hi = reinterpret_cast<UdItem*>(h->h_ud_io.get());
    int max_out = 0;
    for (int b = 0; b < n_images; ++b) {
        const LtUndistort& U = h->ud[images[b].stream];
        UdItem d;
        d.W = U.W; d.H = U.H; d.n_out = U.Wo * U.Ho; d.pad = 0; d.src_off = (long long)src_off[b]; d.dst_off = (long long)out_off[b]; d.map = U.map;
        hi[b] = d;
        std::memcpy(h->h_ud_io + src_off[b], images[b].image, src_bytes[b]);
        max_out = std::max(max_out, d.n_out);
    }
    uint8_t* dio = reinterpret_cast<uint8_t*>(h->d_ud_io.get());
    hipStream_t st = h->st;
    UVS_HIP(h->err, hipSetDevice(h->device));
    UVS_HIP(h->err, hipEventRecord(h->ev0, st));
    UVS_HIP(h->err, hipMemcpyAsync(h->d_ud_io, h->h_ud_io, Y.in_used, hipMemcpyHostToDevice, st));
    if ((rc = ud_launch(h, n_images, reinterpret_cast<const UdItem*>(dio), dio, dio, max_out)) != UVS_OK) return rc;
    UVS_HIP(h->err, hipMemcpyAsync(h->h_ud_io + Y.o_out, h->d_ud_io + Y.o_out, Y.used - Y.o_out, hipMemcpyDeviceToHost, st));
    UVS_HIP(h->err, hipEventRecord(h->ev1, st));
    UVS_HIP(h->err, hipStreamSynchronize(st));
    UVS_HIP(h->err, hipEventElapsedTime(&h->undistort_ms, h->ev0, h->ev1));
    size_t o = 0;
    for (int b = 0; b < n_images; ++b) { std::memcpy(out + o, h->h_ud_io + out_off[b], out_bytes[b]); o += out_bytes[b]; }
    return UVS_OK;
}

double uvs_lt_last_undistort_device_ms(const uvs_lt_tracker* h) { return h ? (double)h->undistort_ms : 0.0; }

}  // extern "C"
