// uvs_feature_equalize.hip -- the first step of the point front end's readImage (reference feature_tracker/src/feature_tracker.cpp:60-66:
// cv::createCLAHE(3.0, cv::Size(8, 8))->apply(_img, img) under EQUALIZE) behind uvs_ft_set_equalize / uvs_ft_equalize of include/uvs_solver.h,
// whose comment is the statement of the numerics.  gfx950, on the tracker's handle (csrc/uvs_ft_handle.h) and its one stream.  Everything up to a
// tile's LUT is integer, so any summation order gives the same bits; the float32 of a LUT entry is one conversion and one multiply, of a pixel
// the dozen operations of the bilinear blend in the order written, and this unit is compiled with -ffp-contract=off, so they round as written,
// which is what tests/cl_ref.py (the numpy restatement, the pin) does.
//
// uvsft::equalize_enqueue is the one entry: it packs the jobs' descriptors and raw images into the pinned staging buffer, uploads them in ONE
// copy and launches the two kernels on the handle's stream; it does not wait.  uvs_feature_track.hip calls it for the items whose slot is
// equalized (destination: level 0 of the slot's new pyramid), uvs_ft_equalize and uvs_ft_debug_equalize below for their images (destination:
// the call's output buffer).  The padded image is never made: both kernels read the raw image through reflect-101.  Kernels, in stream order:
//   k_ft_clahe_lut    one workgroup per (tile, image).  The tile's pixels are counted into an LDS histogram PER WAVE (a low-contrast tile puts
//                     all its pixels into a handful of bins, where the lanes of one histogram would queue up on LDS atomics; four histograms
//                     cut the queue to a quarter), the four are summed, thread i owning bin i from there on: the clip total by a wave
//                     reduction and four LDS words, the redistribution, a 256-wide inclusive scan (a shuffle scan per wave, the wave totals
//                     through LDS), one LUT byte per thread to global memory.
//   k_ft_clahe_apply  one workgroup per block of rows of a half-tile aligned region: between the centres of neighbouring tiles the floor of
//                     the tile coordinate is one value, so a region reads two LUTs per axis.  The range is not assumed but computed, by the
//                     pixel formula itself at the region's first and last pixel (x * (1 / tw) can round across a half), and up to 3 x 3 LUTs
//                     are staged in LDS.  A lane handles four adjacent pixels of a dword-aligned group: one dword read, one dword written, or
//                     single bytes where the group straddles the region's edge, since the neighbouring workgroup owns the other bytes.
// No kernel uses scratch (build() checks it) and none indexes a register array at run time; the LDS atomics are integer adds.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/uvs_solver.h"
#include "uvs_frontend_dev.h"
#include "uvs_ft_handle.h"

namespace uvsft {

constexpr int kEqThreads = 256, kEqWaves = kEqThreads / 64;
constexpr int kEqRows = 16;                 // rows of a region one apply workgroup handles
constexpr int kEqLutSide = 3;               // LUTs per axis an apply workgroup can stage
static_assert(kEqThreads == 256, "thread i owns bin i");

struct EqItem {                        // device copy of one job
    int W, H, src_pitch, dst_pitch;
    int tiles_x, tiles_y, tw, th;
    int clip, n_sub, pad0, pad1;            // n_sub: apply workgroups per region = ceil(th / kEqRows)
    float lut_scale, inv_tw, inv_th, pad2;
    long long src_off;                      // bytes from the staging buffer's head to the raw image
    long long lut_off;                      // bytes from the LUT buffer's head to the job's LUTs [tiles_y * tiles_x][256]
    uint8_t* dst;
    int* bins;                              // uvs_ft_debug_equalize: [tiles_y * tiles_x][256], else null
};

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ void __launch_bounds__(kEqThreads) k_ft_clahe_lut(const EqItem* __restrict__ items, const uint8_t* __restrict__ stage, uint8_t* __restrict__ luts) {
    __shared__ int sHist[kEqWaves][256];
    __shared__ int sPart[kEqWaves];
    const EqItem F = items[blockIdx.y];
    const int tile = blockIdx.x;
    if (tile >= F.tiles_x * F.tiles_y) return;                // the grid is sized for the job with the most tiles; uniform over the workgroup
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ty = tile / F.tiles_x, tx = tile - ty * F.tiles_x;
#pragma unroll
    for (int w = 0; w < kEqWaves; ++w) sHist[w][tid] = 0;
    __syncthreads();
    const uint8_t* img = stage + F.src_off;
    const int n = F.tw * F.th, x0 = tx * F.tw, y0 = ty * F.th;
    for (int i = tid; i < n; i += kEqThreads) {
        const int r = i / F.tw, c = i - r * F.tw;
        const int v = img[(size_t)reflect101(y0 + r, F.H) * F.src_pitch + reflect101(x0 + c, F.W)];
        atomicAdd(&sHist[wave][v], 1);
    }
    __syncthreads();
    int h = 0;
#pragma unroll
    for (int w = 0; w < kEqWaves; ++w) h += sHist[w][tid];
    if (F.clip > 0) {
        const int over = wave_sum_i(max(h - F.clip, 0));
        if (lane == 0) sPart[wave] = over;
        __syncthreads();
        int clipped = 0;
#pragma unroll
        for (int w = 0; w < kEqWaves; ++w) clipped += sPart[w];
        __syncthreads();                                      // sPart is used again by the scan
        const int batch = clipped / 256, residual = clipped - 256 * batch;
        h = min(h, F.clip) + batch;
        if (residual > 0) {
            const int step = max(256 / residual, 1), k = tid / step;
            if (tid - k * step == 0 && k < residual) h += 1;
        }
    }
    if (F.bins) F.bins[(size_t)tile * 256 + tid] = h;
    int s = h;                                                // inclusive scan over the 256 bins
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(s, off, 64);
        if (lane >= off) s += t;
    }
    if (lane == 63) sPart[wave] = s;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kEqWaves - 1; ++w) s += w < wave ? sPart[w] : 0;
    const float v = rintf((float)s * F.lut_scale);
    luts[F.lut_off + (size_t)tile * 256 + tid] = (uint8_t)(int)fminf(fmaxf(v, 0.0f), 255.0f);
}

// the tile coordinate of pixel i along one axis: floor(i * inv - 0.5) before it is clamped
__device__ __forceinline__ int tile_floor(int i, float inv, float& a) {
    const float f = (float)i * inv - 0.5f;
    const float fl = floorf(f);
    a = f - fl;
    return (int)fl;
}

__global__ void __launch_bounds__(kEqThreads) k_ft_clahe_apply(const EqItem* __restrict__ items, const uint8_t* __restrict__ stage, const uint8_t* __restrict__ luts) {
    __shared__ uint8_t sLut[kEqLutSide * kEqLutSide][256];
    const EqItem F = items[blockIdx.z];
    const int bx = blockIdx.x, by = blockIdx.y / F.n_sub, sub = blockIdx.y - by * F.n_sub;
    if (bx > F.tiles_x || by > F.tiles_y) return;             // uniform over the workgroup, as the returns below
    // region (bx, by): from half a tile before the grid line bx tw to half a tile after it, cut to the image
    const int hx = F.tw / 2, hy = F.th / 2;
    const int x0 = max(bx * F.tw - (F.tw - hx), 0), x1 = min(bx * F.tw + hx, F.W);
    const int ry0 = max(by * F.th - (F.th - hy), 0), ry1 = min(by * F.th + hy, F.H);
    const int y0 = ry0 + sub * kEqRows, y1 = min(y0 + kEqRows, ry1);
    if (x0 >= x1 || y0 >= y1) return;
    float dummy;
    const int lx = max(tile_floor(x0, F.inv_tw, dummy), 0), ly = max(tile_floor(y0, F.inv_th, dummy), 0);
    const int nx = min(tile_floor(x1 - 1, F.inv_tw, dummy) + 1, F.tiles_x - 1) - lx + 1;
    const int ny = min(tile_floor(y1 - 1, F.inv_th, dummy) + 1, F.tiles_y - 1) - ly + 1;
    if (nx > kEqLutSide || ny > kEqLutSide) return;           // cannot happen: a region is at most a tile wide and high
    const int tid = threadIdx.x;
    const uint8_t* L = luts + F.lut_off;
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) sLut[j * kEqLutSide + i][tid] = L[(size_t)((ly + j) * F.tiles_x + lx + i) * 256 + tid];
    __syncthreads();
    const uint8_t* img = stage + F.src_off;
    const int g0 = x0 >> 2, ng = ((x1 - 1) >> 2) - g0 + 1;     // dword-aligned groups of four pixels that touch the region
    const int total = ng * (y1 - y0);
    for (int i = tid; i < total; i += kEqThreads) {
        const int r = i / ng, g = g0 + (i - r * ng), y = y0 + r;
        float ya;
        const int tyf = tile_floor(y, F.inv_th, ya);
        const float ya1 = 1.0f - ya;
        const int ty1 = max(tyf, 0) - ly, ty2 = min(tyf + 1, F.tiles_y - 1) - ly;
        const uint32_t in = *reinterpret_cast<const uint32_t*>(img + (size_t)y * F.src_pitch + 4 * g);      // rows are 16-byte aligned and padded
        uint32_t out = 0;
        bool all = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = 4 * g + k;
            const bool live = x >= x0 && x < x1;
            all = all && live;
            const int xc = min(max(x, x0), x1 - 1);            // a dead lane computes a pixel of the region: its LUTs are staged
            const int v = live ? (int)((in >> (8 * k)) & 0xffu) : 0;
            float xa;
            const int txf = tile_floor(xc, F.inv_tw, xa);
            const float xa1 = 1.0f - xa;
            const int tx1 = max(txf, 0) - lx, tx2 = min(txf + 1, F.tiles_x - 1) - lx;
            const float l11 = (float)sLut[ty1 * kEqLutSide + tx1][v], l12 = (float)sLut[ty1 * kEqLutSide + tx2][v];
            const float l21 = (float)sLut[ty2 * kEqLutSide + tx1][v], l22 = (float)sLut[ty2 * kEqLutSide + tx2][v];
            const float res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya;
            const uint32_t o = (uint32_t)(int)fminf(fmaxf(rintf(res), 0.0f), 255.0f);
            out |= o << (8 * k);
        }
        uint8_t* dst = F.dst + (size_t)y * F.dst_pitch + 4 * g;
        if (all) *reinterpret_cast<uint32_t*>(dst) = out;
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * g + k >= x0 && 4 * g + k < x1) dst[k] = (uint8_t)(out >> (8 * k));
        }
    }
}

// Wp, Hp, tw, th, N, clip of the header's rule
static void equalize_geometry(int W, int H, double clip_limit, int tiles_x, int tiles_y, int* Wp, int* Hp, int* tw, int* th, int* N, int* clip) {
    if (W % tiles_x == 0 && H % tiles_y == 0) { *Wp = W; *Hp = H; }
    else { *Wp = W + tiles_x - W % tiles_x; *Hp = H + tiles_y - H % tiles_y; }      // a dimension that divides gains a full tile count: OpenCV's behaviour
    *tw = *Wp / tiles_x; *th = *Hp / tiles_y; *N = *tw * *th;
    *clip = clip_limit == 0.0 ? 0 : std::max((int)(clip_limit * (double)*N / 256.0), 1);
}

int equalize_enqueue(uvs_ft_tracker* h, int n, const EqJob* jobs, int32_t* dbg_bins_dev) {
    size_t o_img = align_up((size_t)n * sizeof(EqItem), 256), bytes = o_img, lut_bytes = 0;
    std::vector<EqItem> items(n);
    int top_tiles = 0, top_bx = 0, top_by = 0;
    for (int i = 0; i < n; ++i) {
        const EqJob& J = jobs[i];
        EqItem& d = items[i];
        int Wp, Hp, N;
        equalize_geometry(J.width, J.height, J.clip_limit, J.tiles_x, J.tiles_y, &Wp, &Hp, &d.tw, &d.th, &N, &d.clip);
        d.W = J.width; d.H = J.height; d.src_pitch = pitch_of(J.width); d.dst_pitch = J.dst_pitch;
        d.tiles_x = J.tiles_x; d.tiles_y = J.tiles_y;
        d.n_sub = (d.th + kEqRows - 1) / kEqRows; d.pad0 = d.pad1 = 0; d.pad2 = 0.f;
        d.lut_scale = 255.0f / (float)N; d.inv_tw = 1.0f / (float)d.tw; d.inv_th = 1.0f / (float)d.th;
        d.src_off = (long long)bytes; d.lut_off = (long long)lut_bytes;
        d.dst = J.dst; d.bins = i == 0 ? dbg_bins_dev : nullptr;
        bytes += align_up((size_t)d.src_pitch * d.H, 256);
        lut_bytes += (size_t)d.tiles_x * d.tiles_y * 256;
        top_tiles = std::max(top_tiles, d.tiles_x * d.tiles_y);
        top_bx = std::max(top_bx, d.tiles_x + 1); top_by = std::max(top_by, (d.tiles_y + 1) * d.n_sub);
    }
    int rc;
    if ((rc = h->h_eq_in.ensure(bytes, h->err, grow_pinned)) != UVS_OK || (rc = h->d_eq_in.ensure(h->h_eq_in.cap(), h->err)) != UVS_OK ||
        (rc = h->d_eq_lut.ensure(lut_bytes, h->err)) != UVS_OK) return rc;
    std::memcpy(h->h_eq_in.get(), items.data(), (size_t)n * sizeof(EqItem));
    for (int i = 0; i < n; ++i) {
        const EqItem& d = items[i];
        char* dst = h->h_eq_in + d.src_off;
        if (d.src_pitch == d.W) std::memcpy(dst, jobs[i].image, (size_t)d.W * d.H);
        else for (int y = 0; y < d.H; ++y) {
            std::memcpy(dst + (size_t)y * d.src_pitch, jobs[i].image + (size_t)y * d.W, d.W);
            std::memset(dst + (size_t)y * d.src_pitch + d.W, 0, d.src_pitch - d.W);
        }
    }
    const EqItem* dF = reinterpret_cast<const EqItem*>(h->d_eq_in.get());
    const uint8_t* dStage = reinterpret_cast<const uint8_t*>(h->d_eq_in.get());
    hipStream_t st = h->st;
    UVS_HIP(h->err, hipMemcpyAsync(h->d_eq_in, h->h_eq_in, bytes, hipMemcpyHostToDevice, st));
    k_ft_clahe_lut<<<dim3(top_tiles, n), kEqThreads, 0, st>>>(dF, dStage, h->d_eq_lut);
    k_ft_clahe_apply<<<dim3(top_bx, top_by, n), kEqThreads, 0, st>>>(dF, dStage, h->d_eq_lut);
    UVS_HIP(h->err, hipGetLastError());
    return UVS_OK;
}

}  // namespace uvsft

using namespace uvsft;

namespace {

// what uvs_ft_equalize and uvs_ft_debug_equalize share; dbg_*: the bins, the LUTs and the geometry of the ONE image
int eq_run(uvs_ft_tracker* h, const char* who_, int n_images, const uvs_ft_image* images, double clip_limit, int tiles_x, int tiles_y, uint8_t* out,
           int32_t* dbg_bins, uint8_t* dbg_luts, int32_t* dbg_info) {
    const std::string fn = who_;
    h->err.clear();
    if (n_images < 1 || !images || !out) { h->err = fn + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG; }
    if (n_images > h->max_streams) { h->err = fn + ": more images than the slots given to uvs_ft_create"; return UVS_ERR_CAPACITY; }
    if (const int rc = check_equalize(clip_limit, tiles_x, tiles_y, fn, h->err)) return rc;
    size_t out_bytes = 0;
    for (int i = 0; i < n_images; ++i) {
        const uvs_ft_image& im = images[i];
        const std::string who = fn + ": image " + std::to_string(i);
        if (!im.image) { h->err = who + ": null pointer"; return UVS_ERR_INVALID_ARG; }
        if (im.width < UVS_FT_MIN_SIZE || im.height < UVS_FT_MIN_SIZE) { h->err = who + ": width and height must be at least 24"; return UVS_ERR_INVALID_ARG; }
        if (im.width > h->max_width || im.height > h->max_height) { h->err = who + " exceeds the capacity given to uvs_ft_create"; return UVS_ERR_CAPACITY; }
        out_bytes += align_up((size_t)pitch_of(im.width) * im.height, 256);
    }
    const size_t T = (size_t)tiles_x * tiles_y, bins_at = align_up(out_bytes, 256), total = bins_at + (dbg_bins ? T * 256 * 4 : 0);
    UVS_HIP(h->err, hipSetDevice(h->device));
    int rc;
    if ((rc = h->d_eq_out.ensure(total, h->err)) != UVS_OK || (rc = h->h_eq_out.ensure(total, h->err, grow_pinned)) != UVS_OK) return rc;
    std::vector<EqJob> jobs(n_images);
    size_t o = 0;
    for (int i = 0; i < n_images; ++i) {
        const uvs_ft_image& im = images[i];
        jobs[i] = EqJob{im.image, im.width, im.height, clip_limit, tiles_x, tiles_y, reinterpret_cast<uint8_t*>(h->d_eq_out.get()) + o, pitch_of(im.width)};
        o += align_up((size_t)pitch_of(im.width) * im.height, 256);
    }
    hipStream_t st = h->st;
    UVS_HIP(h->err, hipEventRecord(h->ev0, st));
    if ((rc = equalize_enqueue(h, n_images, jobs.data(), dbg_bins ? reinterpret_cast<int32_t*>(h->d_eq_out + bins_at) : nullptr)) != UVS_OK) return rc;
    UVS_HIP(h->err, hipMemcpyAsync(h->h_eq_out, h->d_eq_out, total, hipMemcpyDeviceToHost, st));
    UVS_HIP(h->err, hipEventRecord(h->ev1, st));
    UVS_HIP(h->err, hipStreamSynchronize(st));
    UVS_HIP(h->err, hipEventElapsedTime(&h->equalize_ms, h->ev0, h->ev1));
    o = 0;
    for (int i = 0; i < n_images; ++i) {                      // packed in order, stride = width
        const int W = images[i].width, H = images[i].height, P = pitch_of(W);
        for (int y = 0; y < H; ++y) std::memcpy(out + (size_t)y * W, h->h_eq_out + o + (size_t)y * P, W);
        out += (size_t)W * H;
        o += align_up((size_t)P * H, 256);
    }
    if (dbg_bins) {
        std::memcpy(dbg_bins, h->h_eq_out + bins_at, T * 256 * 4);
        UVS_HIP(h->err, hipMemcpy(dbg_luts, h->d_eq_lut, T * 256, hipMemcpyDeviceToHost));
        int tw, th;
        equalize_geometry(images[0].width, images[0].height, clip_limit, tiles_x, tiles_y, &dbg_info[0], &dbg_info[1], &tw, &th, &dbg_info[2], &dbg_info[3]);
    }
    return UVS_OK;
}

}  // namespace

extern "C" {

int uvs_ft_set_equalize(uvs_ft_tracker* h, int stream, double clip_limit, int tiles_x, int tiles_y) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    if (stream < 0 || stream >= h->max_streams) { h->err = "uvs_ft_set_equalize: the stream is not a slot of the handle"; return UVS_ERR_INVALID_ARG; }
    uvs_ft_tracker::Slot& s = h->slots[stream];
    if (tiles_x == 0) { s.equalize = false; return UVS_OK; }
    if (const int rc = check_equalize(clip_limit, tiles_x, tiles_y, "uvs_ft_set_equalize", h->err)) return rc;
    s.equalize = true; s.eq_clip = clip_limit; s.eq_tiles_x = tiles_x; s.eq_tiles_y = tiles_y;
    return UVS_OK;
}

int uvs_ft_equalize(uvs_ft_tracker* h, int n_images, const uvs_ft_image* images, double clip_limit, int tiles_x, int tiles_y, uint8_t* out) {
    if (!h) return UVS_ERR_INVALID_ARG;
    return eq_run(h, "uvs_ft_equalize", n_images, images, clip_limit, tiles_x, tiles_y, out, nullptr, nullptr, nullptr);
}

double uvs_ft_last_equalize_device_ms(const uvs_ft_tracker* h) { return h ? (double)h->equalize_ms : 0.0; }

int uvs_ft_debug_equalize(uvs_ft_tracker* h, const uvs_ft_image* image, double clip_limit, int tiles_x, int tiles_y, int32_t* bins, uint8_t* luts,
                          uint8_t* out, int32_t* info) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    if (!image || !bins || !luts || !info) { h->err = "uvs_ft_debug_equalize: null pointer"; return UVS_ERR_INVALID_ARG; }
    return eq_run(h, "uvs_ft_debug_equalize", 1, image, clip_limit, tiles_x, tiles_y, out, bins, luts, info);
}

}  // extern "C"
