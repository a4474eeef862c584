// uvs_keyframe_features.hip -- the features a keyframe of the pose graph is built from (reference pose_graph/src/keyframe.cpp:14-41, 75-113:
// computeWindowBRIEFPoint, computeBRIEFPoint; ThirdParty/DVision/BRIEF.cpp:39-106; camera_models/PinholeCamera.cc:450-510, 678-694) behind the
// uvs_kf_* calls of include/uvs_solver.h.  gfx950, one stream per handle.  Integer arithmetic throughout, except the float32 add of BRIEF's
// coordinates and the FP64 of liftProjective; this unit is compiled with -ffp-contract=off, so those round as written, which is what
// tests/kf_ref.py (the numpy restatement, the pin) does.
//
// One call extracts a batch of frames.  The images are repacked on the host into rows of `pitch` = width rounded up to 16 bytes (so that every
// row starts 16-byte aligned whatever the width) and uploaded once; the blurred image and the score map use the same pitch.  Every kernel has
// the frame on its last grid axis and no kernel reads another frame's data, so a frame gives the same bits alone or in a batch.  Kernels of one
// call, in stream order:
//   k_kf_blur          64 x 32 tile, 4-pixel halo (reflect-101 applied while the tile is loaded, 4-byte loads where the dword is inside the
//                      row).  Rows: h = sum w p <= 255 * 256 as uint16 in LDS; columns: v = sum w h < 2^24; out = (v + 32768) >> 16, four
//                      pixels per 4-byte store.
//   k_kf_score         64 x 16 tile, 3-pixel halo (4 to the left, to keep the dwords aligned), four neighbouring pixels per lane and one
//                      4-byte store.  The 16 arc minima come from min over 2, 4, 8, 9 ring pixels by doubling; B = -(min over arcs of max d).
//                      Counts the corners of the frame (integer atomics: order-independent).
//   k_kf_select_mark   a wave per 64-pixel row segment: the 8-neighbour test, the wave's ballot is the segment's keep mask, its popcount
//                      the segment's count.
//   k_kf_select_scan   a workgroup per frame: exclusive scan of the segment counts in row-major segment order, two levels (a contiguous chunk
//                      per thread, then the 256 chunk sums in LDS); writes n_keypoints, n_returned and the status.
//   k_kf_select_emit   a wave per segment: keypoint number = segment base + popcount of the mask below the lane, so the list is in row-major
//                      order by construction, not by the arrival order of atomics; entries >= max_keypoints are dropped.
//   k_kf_describe      ONE WAVE PER POINT (first the frame's returned keypoints, then its window points): lane l evaluates tests l, 64 + l,
//                      128 + l, 192 + l, and four wave-wide ballots are the four words of the descriptor.  Lane 0 of a keypoint's wave also
//                      does its liftProjective.
// No kernel uses scratch (build() checks it) and none indexes an array at run time.
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
#include "uvs_handle.h"

namespace uvskf {

constexpr int kBits = UVS_KF_PATTERN_BITS;
constexpr int kThreads = 256;                     // every kernel: 4 waves
constexpr int kBlurTW = 64, kBlurTH = 32;         // output tile of k_kf_blur
constexpr int kBlurRows = kBlurTH + 8;            // with the halo
constexpr int kScoreTW = 64, kScoreTH = 16;       // output tile of k_kf_score
constexpr int kScoreRows = kScoreTH + 6;
constexpr int kTileDwords = (64 + 8) / 4;         // a tile row with 4 halo bytes on each side
constexpr int kSeg = 64;                          // pixels of a row segment = lanes of a wave
static_assert(kBits == 4 * 64, "four ballots of a wave64 make a descriptor");
static_assert(kBlurTW * kBlurTH == 8 * kThreads && kScoreTW * kScoreTH == 4 * kThreads, "tiles");

struct KfFrame {                   // device copy of one uvs_kf_frame
    int W, H, pitch, n_window;
    int w_off;                     // offset of the first window point in the concatenated arrays
    int segs_per_row, n_seg;       // row segments of 64 pixels
    int seg_off;                   // offset of the first segment in the segment arrays
    long long img_off;             // byte offset of the image / blurred image / score map in their buffers
};

__device__ __forceinline__ unsigned byte_of(uint32_t w, int k) { return (w >> (8 * k)) & 255u; }

// ---- blur: rows then columns of {7, 17, 32, 46, 52, 46, 32, 17, 7}, one rounding at the end
__global__ void __launch_bounds__(kThreads) k_kf_blur(const KfFrame* __restrict__ frames, const uint8_t* __restrict__ img, uint8_t* __restrict__ blur) {
    __shared__ uint32_t sSrc[kBlurRows * kTileDwords];        // 40 rows x 72 bytes: x0 - 4 .. x0 + 67
    __shared__ uint2 sH[kBlurRows * (kBlurTW / 4)];           // 40 rows x 64 uint16
    const KfFrame F = frames[blockIdx.z];
    const int x0 = blockIdx.x * kBlurTW, y0 = blockIdx.y * kBlurTH, tid = threadIdx.x;
    if (x0 >= F.W || y0 >= F.H) return;                       // the grid is sized for the largest frame of the batch
    const uint8_t* src = img + F.img_off;
    for (int i = tid; i < kBlurRows * kTileDwords; i += kThreads) {
        const int r = i / kTileDwords, c = i % kTileDwords;
        const uint8_t* row = src + (size_t)reflect101(y0 - 4 + r, F.H) * F.pitch;
        const int x = x0 - 4 + 4 * c;
        uint32_t v;
        if (x >= 0 && x + 3 < F.W) v = *reinterpret_cast<const uint32_t*>(row + x);
        else {
            v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) v |= (uint32_t)row[reflect101(x + k, F.W)] << (8 * k);
        }
        sSrc[i] = v;
    }
    __syncthreads();
    for (int i = tid; i < kBlurRows * (kBlurTW / 4); i += kThreads) {      // outputs x0 + 4 g .. + 3 of tile row r read tile bytes 4 g .. 4 g + 11
        const int r = i >> 4, g = i & 15;
        const uint32_t a = sSrc[r * kTileDwords + g], b = sSrc[r * kTileDwords + g + 1], c = sSrc[r * kTileDwords + g + 2];
        const unsigned p0 = byte_of(a, 0), p1 = byte_of(a, 1), p2 = byte_of(a, 2), p3 = byte_of(a, 3), p4 = byte_of(b, 0), p5 = byte_of(b, 1),
                       p6 = byte_of(b, 2), p7 = byte_of(b, 3), p8 = byte_of(c, 0), p9 = byte_of(c, 1), p10 = byte_of(c, 2), p11 = byte_of(c, 3);
        const unsigned h0 = 7u * (p0 + p8) + 17u * (p1 + p7) + 32u * (p2 + p6) + 46u * (p3 + p5) + 52u * p4;
        const unsigned h1 = 7u * (p1 + p9) + 17u * (p2 + p8) + 32u * (p3 + p7) + 46u * (p4 + p6) + 52u * p5;
        const unsigned h2 = 7u * (p2 + p10) + 17u * (p3 + p9) + 32u * (p4 + p8) + 46u * (p5 + p7) + 52u * p6;
        const unsigned h3 = 7u * (p3 + p11) + 17u * (p4 + p10) + 32u * (p5 + p9) + 46u * (p6 + p8) + 52u * p7;
        sH[i] = make_uint2(h0 | (h1 << 16), h2 | (h3 << 16));
    }
    __syncthreads();
    uint8_t* dst = blur + F.img_off;
    for (int i = tid; i < kBlurTH * (kBlurTW / 4); i += kThreads) {
        const int r = i >> 4, g = i & 15;
        const int y = y0 + r, x = x0 + 4 * g;
        if (y >= F.H || x >= F.pitch) continue;               // x is a multiple of 4 and the pitch one of 16: x + 3 < pitch
        uint2 q[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) q[t] = sH[(r + t) * (kBlurTW / 4) + g];
        unsigned v0, v1, v2, v3;
#define UVS_KF_COL(sel) (7u * (sel(q[0]) + sel(q[8])) + 17u * (sel(q[1]) + sel(q[7])) + 32u * (sel(q[2]) + sel(q[6])) + 46u * (sel(q[3]) + sel(q[5])) + 52u * sel(q[4]))
#define UVS_KF_S0(v) ((v).x & 0xffffu)
#define UVS_KF_S1(v) ((v).x >> 16)
#define UVS_KF_S2(v) ((v).y & 0xffffu)
#define UVS_KF_S3(v) ((v).y >> 16)
        v0 = UVS_KF_COL(UVS_KF_S0); v1 = UVS_KF_COL(UVS_KF_S1); v2 = UVS_KF_COL(UVS_KF_S2); v3 = UVS_KF_COL(UVS_KF_S3);
#undef UVS_KF_COL
#undef UVS_KF_S0
#undef UVS_KF_S1
#undef UVS_KF_S2
#undef UVS_KF_S3
        const unsigned o0 = (v0 + 32768u) >> 16, o1 = x + 1 < F.W ? (v1 + 32768u) >> 16 : 0u, o2 = x + 2 < F.W ? (v2 + 32768u) >> 16 : 0u,
                       o3 = x + 3 < F.W ? (v3 + 32768u) >> 16 : 0u;
        *reinterpret_cast<uint32_t*>(dst + (size_t)y * F.pitch + x) = (x < F.W ? o0 : 0u) | (o1 << 8) | (o2 << 16) | (o3 << 24);
    }
}

// ---- FAST 9-16 score map
__global__ void __launch_bounds__(kThreads) k_kf_score(const KfFrame* __restrict__ frames, const uint8_t* __restrict__ img, uint8_t* __restrict__ score,
                                                     uvs_kf_result* __restrict__ results) {
    __shared__ uint32_t sT[kScoreRows * kTileDwords];         // 22 rows x 72 bytes: y0 - 3 .. y0 + 18, x0 - 4 .. x0 + 67
    const KfFrame F = frames[blockIdx.z];
    const int x0 = blockIdx.x * kScoreTW, y0 = blockIdx.y * kScoreTH, tid = threadIdx.x;
    if (x0 >= F.W || y0 >= F.H) return;
    const uint8_t* src = img + F.img_off;
    for (int i = tid; i < kScoreRows * kTileDwords; i += kThreads) {
        const int r = i / kTileDwords, c = i % kTileDwords;
        const int y = y0 - 3 + r, x = x0 - 4 + 4 * c;
        uint32_t v = 0;                                       // outside the image: never part of an examined pixel's ring
        if (y >= 0 && y < F.H) {
            const uint8_t* row = src + (size_t)y * F.pitch;
            if (x >= 0 && x + 3 < F.W) v = *reinterpret_cast<const uint32_t*>(row + x);
            else {
#pragma unroll
                for (int k = 0; k < 4; ++k) if (x + k >= 0 && x + k < F.W) v |= (uint32_t)row[x + k] << (8 * k);
            }
        }
        sT[i] = v;
    }
    __syncthreads();
    const int r = tid >> 4, g = tid & 15;                     // pixels (x0 + 4 g + j, y0 + r), j = 0..3: tile rows r .. r + 6, tile bytes 4 g + 1 .. 4 g + 10
    uint32_t w[7][3];
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) w[a][b] = sT[(r + a) * kTileDwords + g + b];
    const int y = y0 + r;
    uint32_t packed = 0;
    int corners = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // tile byte of (dx, dy) relative to the lane's first dword: column j + 4 + dx, row 3 + dy
#define UVS_KF_PX(dx, dy) ((int)byte_of(w[3 + (dy)][(j + 4 + (dx)) >> 2], (j + 4 + (dx)) & 3))
        const int c = UVS_KF_PX(0, 0);
        int d[16];
        d[0] = UVS_KF_PX(0, -3) - c;  d[1] = UVS_KF_PX(1, -3) - c;  d[2] = UVS_KF_PX(2, -2) - c;   d[3] = UVS_KF_PX(3, -1) - c;
        d[4] = UVS_KF_PX(3, 0) - c;   d[5] = UVS_KF_PX(3, 1) - c;   d[6] = UVS_KF_PX(2, 2) - c;    d[7] = UVS_KF_PX(1, 3) - c;
        d[8] = UVS_KF_PX(0, 3) - c;   d[9] = UVS_KF_PX(-1, 3) - c;  d[10] = UVS_KF_PX(-2, 2) - c;  d[11] = UVS_KF_PX(-3, 1) - c;
        d[12] = UVS_KF_PX(-3, 0) - c; d[13] = UVS_KF_PX(-3, -1) - c; d[14] = UVS_KF_PX(-2, -2) - c; d[15] = UVS_KF_PX(-1, -3) - c;
#undef UVS_KF_PX
        int lo2[16], hi2[16], lo4[16], hi4[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) { lo2[i] = min(d[i], d[(i + 1) & 15]); hi2[i] = max(d[i], d[(i + 1) & 15]); }
#pragma unroll
        for (int i = 0; i < 16; ++i) { lo4[i] = min(lo2[i], lo2[(i + 2) & 15]); hi4[i] = max(hi2[i], hi2[(i + 2) & 15]); }
        int A = -256, Bn = 256;                               // A = max over arcs of min d; Bn = min over arcs of max d = -B
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int lo9 = min(min(lo4[i], lo4[(i + 4) & 15]), d[(i + 8) & 15]);
            const int hi9 = max(max(hi4[i], hi4[(i + 4) & 15]), d[(i + 8) & 15]);
            A = max(A, lo9); Bn = min(Bn, hi9);
        }
        const int s = max(A, -Bn), x = x0 + 4 * g + j;
        const bool examined = x >= 3 && x < F.W - 3 && y >= 3 && y < F.H - 3;
        const unsigned sc = examined && s > 20 ? (unsigned)(s - 1) : 0u;      // <= 254
        packed |= sc << (8 * j);
        corners += sc ? 1 : 0;
    }
    const int x = x0 + 4 * g;
    if (y < F.H && x < F.pitch) *reinterpret_cast<uint32_t*>(score + F.img_off + (size_t)y * F.pitch + x) = packed;
    // corners of the workgroup's four waves: a wave-wide sum by ballots of the count's three bits, then one atomic per wave
    const int wave_total = __popcll(__ballot(corners & 1)) + 2 * __popcll(__ballot(corners & 2)) + 4 * __popcll(__ballot(corners & 4));
    if ((tid & 63) == 0 && wave_total) atomicAdd(&results[blockIdx.z].n_corners_before_nms, wave_total);
}

// ---- non-maximum suppression: keep mask and count of every 64-pixel row segment
__global__ void __launch_bounds__(kThreads) k_kf_select_mark(const KfFrame* __restrict__ frames, const uint8_t* __restrict__ score,
                                                           unsigned long long* __restrict__ seg_mask, int* __restrict__ seg_cnt) {
    const KfFrame F = frames[blockIdx.y];
    const int seg = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (seg >= F.n_seg) return;                               // wave-uniform
    const int y = seg / F.segs_per_row, x = (seg % F.segs_per_row) * kSeg + lane;
    const uint8_t* p = score + F.img_off + (size_t)y * F.pitch + x;
    const int s = x < F.W ? (int)*p : 0;
    bool keep = false;
    if (s > 0) {                                              // an examined pixel: 3 <= x < W - 3, 3 <= y < H - 3, so the 8 neighbours are in the map
        const int P = F.pitch;
        keep = s > p[-P - 1] && s > p[-P] && s > p[-P + 1] && s > p[-1] && s > p[1] && s > p[P - 1] && s > p[P] && s > p[P + 1];
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) { seg_mask[F.seg_off + seg] = m; seg_cnt[F.seg_off + seg] = __popcll(m); }
}

// ---- exclusive scan of the segment counts of one frame; the frame's result
__global__ void __launch_bounds__(kThreads) k_kf_select_scan(const KfFrame* __restrict__ frames, const int* __restrict__ seg_cnt, int* __restrict__ seg_base,
                                                           uvs_kf_result* __restrict__ results, int max_keypoints) {
    __shared__ int sPart[kThreads];
    const KfFrame F = frames[blockIdx.x];
    const int total = uvs_segment_scan<kThreads>(seg_cnt + F.seg_off, seg_base + F.seg_off, F.n_seg, sPart);
    if (threadIdx.x == kThreads - 1) {
        uvs_kf_result* res = results + blockIdx.x;            // n_corners_before_nms: k_kf_score's
        res->status = total > max_keypoints ? UVS_KF_OVERFLOW : UVS_KF_OK;
        res->n_keypoints = total;
        res->n_returned = min(total, max_keypoints);
    }
}

// ---- ordered scatter of (x, y, score)
__global__ void __launch_bounds__(kThreads) k_kf_select_emit(const KfFrame* __restrict__ frames, const uint8_t* __restrict__ score,
                                                           const unsigned long long* __restrict__ seg_mask, const int* __restrict__ seg_base,
                                                           int max_keypoints, int32_t* __restrict__ xy, uint8_t* __restrict__ kp_score) {
    const KfFrame F = frames[blockIdx.y];
    const int seg = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (seg >= F.n_seg) return;
    const unsigned long long m = seg_mask[F.seg_off + seg];
    if (!((m >> lane) & 1ull)) return;
    const int idx = seg_base[F.seg_off + seg] + uvs_rank_below(m, lane);
    if (idx >= max_keypoints) return;
    const int y = seg / F.segs_per_row, x = (seg % F.segs_per_row) * kSeg + lane;
    const size_t o = (size_t)blockIdx.y * max_keypoints + idx;
    xy[2 * o] = x; xy[2 * o + 1] = y;
    kp_score[o] = score[F.img_off + (size_t)y * F.pitch + x];
}

// ---- BRIEF of the keypoints and of the window points, liftProjective of the keypoints: a wave per point
__global__ void __launch_bounds__(kThreads) k_kf_describe(const KfFrame* __restrict__ frames, UvsCamDev cam, const uint8_t* __restrict__ blur,
                                                        const int32_t* __restrict__ pattern, const uvs_kf_result* __restrict__ results,
                                                        const int32_t* __restrict__ xy, const float* __restrict__ window_uv, int max_keypoints,
                                                        double* __restrict__ norm, unsigned long long* __restrict__ desc,
                                                        unsigned long long* __restrict__ window_desc) {
    const int f = blockIdx.y;
    const KfFrame F = frames[f];
    const int n_ret = results[f].n_returned;                 // <= max_keypoints (k_kf_select_scan)
    const int item = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (item >= n_ret + F.n_window) return;                   // wave-uniform
    float u, v;
    unsigned long long* out;
    const bool keypoint = item < n_ret;
    if (keypoint) {
        const size_t o = (size_t)f * max_keypoints + item;
        const int x = xy[2 * o], y = xy[2 * o + 1];
        u = (float)x; v = (float)y;
        out = desc + 4 * o;
        if (lane == 0) {                                      // liftProjective of the call's camera or the handle's model
            double ray[3], mx_u, my_u;
            uvs_cam_lift(cam, (double)x, (double)y, ray, mx_u, my_u);
            norm[2 * o] = mx_u; norm[2 * o + 1] = my_u;
        }
    } else {
        const size_t o = (size_t)F.w_off + (item - n_ret);
        u = window_uv[2 * o]; v = window_uv[2 * o + 1];
        out = window_desc + 4 * o;
    }
    const uint8_t* im = blur + F.img_off;
    unsigned long long word[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = 64 * k + lane;
        const int xa = (int)(u + (float)pattern[i]), ya = (int)(v + (float)pattern[kBits + i]);
        const int xb = (int)(u + (float)pattern[2 * kBits + i]), yb = (int)(v + (float)pattern[3 * kBits + i]);
        bool bit = false;
        if (xa >= 0 && xa < F.W && ya >= 0 && ya < F.H && xb >= 0 && xb < F.W && yb >= 0 && yb < F.H)
            bit = im[(size_t)ya * F.pitch + xa] < im[(size_t)yb * F.pitch + xb];
        word[k] = __ballot(bit);
    }
    if (lane < 4) out[lane] = lane == 0 ? word[0] : lane == 1 ? word[1] : lane == 2 ? word[2] : word[3];
}

}  // namespace uvskf

using namespace uvskf;

struct uvs_kf_extractor : UvsHandle {
    int max_frames = 0, max_width = 0, max_height = 0, max_keypoints = 0, max_window = 0;
    float device_ms = 0.f;                      // uvs_kf_last_device_ms
    size_t slot = 0;                            // bytes of one image at the largest pitch and height, rounded up to 256
    size_t in_meta = 0;                         // bytes of (frames | window points) at capacity, rounded up to 256: the images follow
    DevBuf<char> d_in, d_out;                   // packed inputs (frames | window points | images) / outputs (results | norm | desc | window desc | xy | score) of one call
    PinnedBuf<char> h_in, h_out;                // pinned staging
    DevBuf<uint8_t> d_blur, d_score;            // blurred images, score maps: the images' layout
    DevBuf<unsigned long long> d_seg_mask;      // keep mask of every row segment
    DevBuf<int> d_seg_cnt, d_seg_base;          // its count, its exclusive prefix
    DevBuf<int32_t> d_pattern;                  // x1 | y1 | x2 | y2
    UvsCamDev model = uvs_cam_none();           // uvs_kf_set_camera_model: the keypoints are lifted through it while it is set (model.model >= 0)
};

namespace {

inline int segs_of(int width) { return (width + kSeg - 1) / kSeg; }

struct KfOutLayout { size_t norm, desc, wdesc, xy, score, total; };
// results | keypoints_norm | desc | window_desc | keypoints_xy | keypoint_score for n frames with tw window points in all
inline KfOutLayout out_layout(size_t n, size_t max_kp, size_t tw) {
    KfOutLayout L;
    L.norm = align_up(n * sizeof(uvs_kf_result), 16);
    L.desc = L.norm + n * max_kp * 16;
    L.wdesc = L.desc + n * max_kp * 32;
    L.xy = L.wdesc + tw * 32;
    L.score = L.xy + n * max_kp * 8;
    L.total = L.score + n * max_kp;
    return L;
}

int kf_run(uvs_kf_extractor* h, const char* who_, int n_frames, const uvs_kf_frame* frames, const uvs_kf_camera* camera, int32_t* keypoints_xy,
           uint8_t* keypoint_score, double* keypoints_norm, uint64_t* desc, uint64_t* window_desc, uvs_kf_result* results) {
    const std::string fn = who_;
    h->err.clear();
    if (n_frames < 1 || !frames || (!camera && h->model.model < 0) || !keypoints_xy || !keypoint_score || !keypoints_norm || !desc || !window_desc || !results) {
        h->err = fn + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG;
    }
    if (n_frames > h->max_frames) { h->err = fn + ": more frames than the capacity given to uvs_kf_create"; return UVS_ERR_CAPACITY; }
    UvsCamDev cam;
    if (const int rc = uvs_cam_of_call(h->model, camera, fn, h->err, &cam)) return rc;
    size_t tw = 0, img_bytes = 0, n_seg = 0;
    int max_w = 0, max_h = 0, max_nw = 0;
    for (int f = 0; f < n_frames; ++f) {
        const uvs_kf_frame& fr = frames[f];
        const std::string who = fn + ": frame " + std::to_string(f);
        if (!fr.image || fr.n_window < 0 || (fr.n_window > 0 && !fr.window_uv)) { h->err = who + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG; }
        if (fr.width < UVS_KF_MIN_SIZE || fr.height < UVS_KF_MIN_SIZE) { h->err = who + ": width and height must be at least UVS_KF_MIN_SIZE"; return UVS_ERR_INVALID_ARG; }
        if (fr.width > h->max_width || fr.height > h->max_height || fr.n_window > h->max_window) {
            h->err = who + " exceeds the capacity given to uvs_kf_create"; return UVS_ERR_CAPACITY;
        }
        for (int i = 0; i < 2 * fr.n_window; ++i)             // (int)(u + offset) is undefined beyond the range of int
            if (!std::isfinite(fr.window_uv[i]) || std::fabs(fr.window_uv[i]) > (float)UVS_KF_MAX_COORD) {
                h->err = who + ": a window point is not finite or beyond UVS_KF_MAX_COORD"; return UVS_ERR_INVALID_ARG;
            }
        tw += fr.n_window;
        max_w = std::max(max_w, fr.width); max_h = std::max(max_h, fr.height); max_nw = std::max(max_nw, fr.n_window);
    }
    // packed input: frames | window points | images (each image at a multiple of 256 bytes, rows of `pitch` bytes)
    const size_t o_win = align_up(n_frames * sizeof(KfFrame), 16), o_img = h->in_meta;
    KfFrame* hf = reinterpret_cast<KfFrame*>(h->h_in.get());
    size_t wo = 0;
    for (int f = 0; f < n_frames; ++f) {
        const uvs_kf_frame& fr = frames[f];
        KfFrame d;
        d.W = fr.width; d.H = fr.height; d.pitch = pitch_of(fr.width); d.n_window = fr.n_window; d.w_off = (int)wo;
        d.segs_per_row = segs_of(fr.width); d.n_seg = d.segs_per_row * fr.height; d.seg_off = (int)n_seg; d.img_off = (long long)img_bytes;
        hf[f] = d;
        if (fr.n_window) std::memcpy(h->h_in + o_win + wo * 8, fr.window_uv, (size_t)fr.n_window * 8);
        char* dst = h->h_in + o_img + img_bytes;
        if (d.pitch == d.W) std::memcpy(dst, fr.image, (size_t)d.W * d.H);
        else for (int y = 0; y < d.H; ++y) std::memcpy(dst + (size_t)y * d.pitch, fr.image + (size_t)y * d.W, d.W);
        wo += fr.n_window; n_seg += d.n_seg; img_bytes += align_up((size_t)d.pitch * d.H, 256);
    }
    const size_t max_kp = h->max_keypoints;
    const KfOutLayout L = out_layout(n_frames, max_kp, tw);
    const KfFrame* dF = reinterpret_cast<const KfFrame*>(h->d_in.get());
    const float* dWin = reinterpret_cast<const float*>(h->d_in + o_win);
    const uint8_t* dImg = reinterpret_cast<const uint8_t*>(h->d_in + o_img);
    uvs_kf_result* dRes = reinterpret_cast<uvs_kf_result*>(h->d_out.get());
    double* dNorm = reinterpret_cast<double*>(h->d_out + L.norm);
    unsigned long long* dDesc = reinterpret_cast<unsigned long long*>(h->d_out + L.desc);
    unsigned long long* dWdesc = reinterpret_cast<unsigned long long*>(h->d_out + L.wdesc);
    int32_t* dXy = reinterpret_cast<int32_t*>(h->d_out + L.xy);
    uint8_t* dSc = reinterpret_cast<uint8_t*>(h->d_out + L.score);
    const int waves = kThreads / 64;
    const unsigned seg_blocks = (unsigned)((max_h * segs_of(max_w) + waves - 1) / waves);
    const unsigned item_blocks = (unsigned)((h->max_keypoints + max_nw + waves - 1) / waves);
    hipStream_t st = h->st;
    UVS_HIP(h->err, hipSetDevice(h->device));
    UVS_HIP(h->err, hipEventRecord(h->ev0, st));
    UVS_HIP(h->err, hipMemcpyAsync(h->d_in, h->h_in, o_win + tw * 8, hipMemcpyHostToDevice, st));
    UVS_HIP(h->err, hipMemcpyAsync(h->d_in + o_img, h->h_in + o_img, img_bytes, hipMemcpyHostToDevice, st));
    UVS_HIP(h->err, hipMemsetAsync(dRes, 0, n_frames * sizeof(uvs_kf_result), st));
    k_kf_blur<<<dim3((max_w + kBlurTW - 1) / kBlurTW, (max_h + kBlurTH - 1) / kBlurTH, n_frames), kThreads, 0, st>>>(dF, dImg, h->d_blur);
    k_kf_score<<<dim3((max_w + kScoreTW - 1) / kScoreTW, (max_h + kScoreTH - 1) / kScoreTH, n_frames), kThreads, 0, st>>>(dF, dImg, h->d_score, dRes);
    k_kf_select_mark<<<dim3(seg_blocks, n_frames), kThreads, 0, st>>>(dF, h->d_score, h->d_seg_mask, h->d_seg_cnt);
    k_kf_select_scan<<<n_frames, kThreads, 0, st>>>(dF, h->d_seg_cnt, h->d_seg_base, dRes, h->max_keypoints);
    k_kf_select_emit<<<dim3(seg_blocks, n_frames), kThreads, 0, st>>>(dF, h->d_score, h->d_seg_mask, h->d_seg_base, h->max_keypoints, dXy, dSc);
    k_kf_describe<<<dim3(item_blocks, n_frames), kThreads, 0, st>>>(dF, cam, h->d_blur, h->d_pattern, dRes, dXy, dWin, h->max_keypoints, dNorm, dDesc, dWdesc);
    UVS_HIP(h->err, hipGetLastError());
    UVS_HIP(h->err, hipMemcpyAsync(h->h_out, h->d_out, L.total, hipMemcpyDeviceToHost, st));
    UVS_HIP(h->err, hipEventRecord(h->ev1, st));
    UVS_HIP(h->err, hipStreamSynchronize(st));
    UVS_HIP(h->err, hipEventElapsedTime(&h->device_ms, h->ev0, h->ev1));
    std::memcpy(results, h->h_out, n_frames * sizeof(uvs_kf_result));
    for (int f = 0; f < n_frames; ++f) {                      // the strided keypoint arrays: the returned entries only
        const size_t n = (size_t)results[f].n_returned, o = (size_t)f * max_kp;
        if (!n) continue;
        std::memcpy(keypoints_norm + 2 * o, h->h_out + L.norm + o * 16, n * 16);
        std::memcpy(desc + 4 * o, h->h_out + L.desc + o * 32, n * 32);
        std::memcpy(keypoints_xy + 2 * o, h->h_out + L.xy + o * 8, n * 8);
        std::memcpy(keypoint_score + o, h->h_out + L.score + o, n);
    }
    if (tw) std::memcpy(window_desc, h->h_out + L.wdesc, tw * 32);
    return UVS_OK;
}

}  // namespace

extern "C" {

int uvs_kf_create(int device, int max_frames, int max_width, int max_height, int max_keypoints, int max_window,
                  const int32_t* x1, const int32_t* y1, const int32_t* x2, const int32_t* y2, uvs_kf_extractor** out) {
    if (!out) return UVS_ERR_INVALID_ARG;
    *out = nullptr;
    if (!x1 || !y1 || !x2 || !y2 || max_frames < 1 || max_keypoints < 1 || max_window < 1 || max_width < UVS_KF_MIN_SIZE || max_height < UVS_KF_MIN_SIZE)
        return UVS_ERR_INVALID_ARG;
    if (max_frames > UVS_KF_MAX_FRAMES || max_width > UVS_KF_MAX_WIDTH || max_height > UVS_KF_MAX_HEIGHT || max_keypoints > UVS_LC_MAX_OLD ||
        max_window > UVS_LC_MAX_QUERY) return UVS_ERR_CAPACITY;
    std::vector<int32_t> pattern(4 * kBits);
    const int32_t* src[4] = {x1, y1, x2, y2};
    for (int a = 0; a < 4; ++a)
        for (int i = 0; i < kBits; ++i) {
            if (src[a][i] < -UVS_KF_MAX_PATTERN_OFFSET || src[a][i] > UVS_KF_MAX_PATTERN_OFFSET) return UVS_ERR_INVALID_ARG;
            pattern[a * kBits + i] = src[a][i];
        }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return UVS_ERR_NO_DEVICE;
    uvs_kf_extractor* h = new uvs_kf_extractor();
    h->max_frames = max_frames; h->max_width = max_width; h->max_height = max_height;
    h->max_keypoints = max_keypoints; h->max_window = max_window;
    const size_t B = max_frames, Wt = B * max_window;
    h->slot = align_up((size_t)pitch_of(max_width) * max_height, 256);
    h->in_meta = align_up(align_up(B * sizeof(KfFrame), 16) + Wt * 8, 256);
    const size_t in_bytes = h->in_meta + B * h->slot, out_bytes = out_layout(B, max_keypoints, Wt).total;
    const size_t segs = B * (size_t)max_height * segs_of(max_width);
    int rc = h->open(device);
    if (rc == UVS_OK && (rc = h->d_in.ensure(in_bytes, h->err)) == UVS_OK && (rc = h->d_out.ensure(out_bytes, h->err)) == UVS_OK &&
        (rc = h->h_in.ensure(in_bytes, h->err)) == UVS_OK && (rc = h->h_out.ensure(out_bytes, h->err)) == UVS_OK &&
        (rc = h->d_blur.ensure(B * h->slot, h->err)) == UVS_OK && (rc = h->d_score.ensure(B * h->slot, h->err)) == UVS_OK &&
        (rc = h->d_seg_mask.ensure(segs * 8, h->err)) == UVS_OK && (rc = h->d_seg_cnt.ensure(segs * 4, h->err)) == UVS_OK &&
        (rc = h->d_seg_base.ensure(segs * 4, h->err)) == UVS_OK && (rc = h->d_pattern.ensure(pattern.size() * 4, h->err)) == UVS_OK) {
        const hipError_t e = hipMemcpy(h->d_pattern, pattern.data(), pattern.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = hip_fail(h->err, e, "hipMemcpy");
    }
    if (rc != UVS_OK) { uvs_kf_destroy(h); return rc; }
    *out = h;
    return UVS_OK;
}

void uvs_kf_destroy(uvs_kf_extractor* h) { if (h) { h->close(); delete h; } }

const char* uvs_kf_last_error(const uvs_kf_extractor* h) { return h ? h->err.c_str() : "null keyframe-feature extractor"; }

double uvs_kf_last_device_ms(const uvs_kf_extractor* h) { return h ? (double)h->device_ms : 0.0; }

int uvs_kf_set_camera_model(uvs_kf_extractor* h, const uvs_camera_model* model) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    if (!model) { h->model = uvs_cam_none(); return UVS_OK; }
    UvsCamDev m;
    if (const int rc = uvs_cam_take(model, "uvs_kf_set_camera_model", h->err, &m)) return rc;
    h->model = m;
    return UVS_OK;
}

int uvs_kf_extract(uvs_kf_extractor* h, int n_frames, const uvs_kf_frame* frames, const uvs_kf_camera* camera, int32_t* keypoints_xy,
                   uint8_t* keypoint_score, double* keypoints_norm, uint64_t* desc, uint64_t* window_desc, uvs_kf_result* results) {
    if (!h) return UVS_ERR_INVALID_ARG;
    return kf_run(h, "uvs_kf_extract", n_frames, frames, camera, keypoints_xy, keypoint_score, keypoints_norm, desc, window_desc, results);
}

int uvs_kf_debug_frame(uvs_kf_extractor* h, const uvs_kf_frame* frame, const uvs_kf_camera* camera, uint8_t* blur, uint8_t* score,
                       int32_t* keypoints_xy, uint8_t* keypoint_score, double* keypoints_norm, uint64_t* desc, uint64_t* window_desc,
                       uvs_kf_result* result) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    if (!frame || !blur || !score) { h->err = "uvs_kf_debug_frame: null pointer"; return UVS_ERR_INVALID_ARG; }
    const int rc = kf_run(h, "uvs_kf_debug_frame", 1, frame, camera, keypoints_xy, keypoint_score, keypoints_norm, desc, window_desc, result);
    if (rc != UVS_OK) return rc;
    // the single frame sits at offset 0 of the blurred images and of the score maps, rows of pitch_of(width) bytes
    const size_t W = frame->width, H = frame->height, P = pitch_of(frame->width);
    UVS_HIP(h->err, hipMemcpy2D(blur, W, h->d_blur, P, W, H, hipMemcpyDeviceToHost));
    UVS_HIP(h->err, hipMemcpy2D(score, W, h->d_score, P, W, H, hipMemcpyDeviceToHost));
    return UVS_OK;
}

}  // extern "C"
