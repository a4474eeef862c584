// uvs_line_track.hip -- line tracking of the line front end (reference feature_tracker/src/line_feature_tracker.cpp: lineExtraction's
// lineBiDes->compute, lineMatching, the matches consumed at :351-433) behind the uvs_lt_* calls of include/uvs_solver.h: one 256-bit LBD
// descriptor per caller-supplied segment, the Hamming match of a slot's previous lines against the new ones with the 30 px endpoint gates,
// and the slots' previous lines resident on the device.  gfx950, one stream per handle.  The handle is csrc/uvs_lt_handle.h's, shared with the
// detection unit (uvs_line_detect.hip), which calls lt_run below for uvs_lt_detect_track.
//
// One call takes a batch of items; no kernel reads another item's data, so an item gives the same bits alone or in a batch.  This unit is
// compiled with -ffp-contract=off: products and sums round as written, which is what tests/lt_ref.py (the numpy restatement, the pin) does.
// Everything up to the row sums is integer arithmetic.  Kernels of one call, in stream order:
//   k_lt_gradient  thread per pixel: the Sobel gx | gy of the header's rule packed as two int16 in one 32-bit word, so that a sample of the
//                  support region is ONE gather
//   k_lt_prepare   thread per line: MakeKeyLine of the header (ordered ends, L, cq, sq, MX, MY, halfWidth, status) into geom[line][8], and
//                  the truncated gate points and the status into the slot's new set
//   k_lt_rows      one wave per (line, row h): the lanes stride over the L columns, gather, project, and the four 64-bit integer sums are
//                  reduced across the wave (exact in any order) into S[line][63][4]
//   k_lt_bands     one wave per line: lane 4 b + k < 36 owns the accumulators BS[b][k] and B2[b][k] and walks its (at most 21) rows serially,
//                  ascending, as the header orders them; lane 0 takes the serial sums of the normalisation; 32 lanes write the 32 bytes
//   k_lt_match     one workgroup per item: the current descriptors in LDS (1024 x 32 B), thread per previous line, 4 x __popcll per pair, the
//                  minimum of the packed key (distance << 16) | t; prev_of_cur is an integer maximum in LDS (exact in any order)
// No kernel uses scratch memory.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/uvs_solver.h"
#include "uvs_frontend_dev.h"
#include "uvs_lt_handle.h"

namespace uvslt {

constexpr int kGradThreads = 256, kPrepThreads = 64, kRowThreads = 256, kRowWaves = kRowThreads / 64, kBandThreads = 64, kMatchThreads = 256;
static_assert(kRows == 63 && kFloats == 72 && kBytes == 32, "9 bands of width 7, 4 sums, 32 of the 36 band pairs");
static_assert(kMaxLines <= 65536, "the packed match key keeps t in 16 bits");

// ---- gradient: gx in the low, gy in the high 16 bits
__global__ void __launch_bounds__(kGradThreads) k_lt_gradient(const LtItem* __restrict__ items, const uint8_t* __restrict__ in,
                                                              uint32_t* __restrict__ grad, size_t grad_stride) {
    const LtItem I = items[blockIdx.y];
    const int W = I.W, H = I.H;
    const uint8_t* p = in + I.img_off;
    uint32_t* g = grad + grad_stride * blockIdx.y;
    for (int i = blockIdx.x * kGradThreads + threadIdx.x; i < W * H; i += gridDim.x * kGradThreads) {
        const int x = i % W, y = i / W;
        g[i] = uvs_sobel_packed(p, W, H, x, y);
    }
}

// ---- MakeKeyLine
__global__ void __launch_bounds__(kPrepThreads) k_lt_prepare(const LtItem* __restrict__ items, const double* __restrict__ seg, int max_length,
                                                             int32_t* __restrict__ geom, int32_t* __restrict__ line_item,
                                                             int32_t* __restrict__ out_status) {
    const LtItem I = items[blockIdx.y];
    const int l = blockIdx.x * kPrepThreads + threadIdx.x;
    if (l >= I.n_lines) return;
    const int gl = I.l_off + l;
    const double* s = seg + 4 * (size_t)gl;
    double sx = s[0], sy = s[1], ex = s[2], ey = s[3];
    if (sx > ex) { const double tx = sx, ty = sy; sx = ex; sy = ey; ex = tx; ey = ty; }
    const double dx = ex - sx, dy = ey - sy;
    const double len = sqrt(dx * dx + dy * dy);
    const int L = (int)len;
    const int status = L < 2 ? UVS_LT_SHORT : L > max_length ? UVS_LT_LONG : UVS_LT_OK;
    int cq = 0, sq = 0, hw = 0;
    if (status == UVS_LT_OK) {
        cq = (int)rint(1024.0 * dx / len); sq = (int)rint(1024.0 * dy / len);
        hw = (L - 1) / 2;
    }
    int32_t* g = geom + 8 * (size_t)gl;
    g[0] = L; g[1] = cq; g[2] = sq; g[3] = (int)rint(512.0 * (sx + ex)); g[4] = (int)rint(512.0 * (sy + ey)); g[5] = hw; g[6] = status; g[7] = 0;
    line_item[gl] = blockIdx.y;
    out_status[gl] = status;
    I.slot_stat[l] = status;
    int32_t* e = I.slot_ends + 4 * (size_t)l;
    e[0] = (int)sx; e[1] = (int)sy; e[2] = (int)ex; e[3] = (int)ey;
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// ---- row sums: wave per (line, row)
__global__ void __launch_bounds__(kRowThreads) k_lt_rows(const LtItem* __restrict__ items, const int32_t* __restrict__ geom,
                                                         const int32_t* __restrict__ line_item, const uint32_t* __restrict__ grad,
                                                         size_t grad_stride, long long* __restrict__ S) {
    const int gl = blockIdx.x, lane = threadIdx.x & 63;
    const int h = blockIdx.y * kRowWaves + (threadIdx.x >> 6);
    if (h >= kRows) return;
    const int32_t* g = geom + 8 * (size_t)gl;
    long long s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    if (g[6] == UVS_LT_OK) {
        const int it = line_item[gl];
        const LtItem I = items[it];
        const int W = I.W, H = I.H, L = g[0], cq = g[1], sq = g[2], hw = g[5];
        const uint32_t* gr = grad + grad_stride * it;
        const int X0 = g[3] - (h - 31) * sq, Y0 = g[4] + (h - 31) * cq;
        for (int w = lane; w < L; w += 64) {
            const int X = X0 + (w - hw) * cq, Y = Y0 + (w - hw) * sq;
            const int x = min(max((X + 512) >> 10, 0), W - 1), y = min(max((Y + 512) >> 10, 0), H - 1);
            const uint32_t v = gr[y * W + x];
            const int gx = (int)(int16_t)(v & 0xFFFFu), gy = (int)(int16_t)(v >> 16);
            const int dl = gx * cq + gy * sq, dO = -gx * sq + gy * cq;
            s0 += max(dl, 0); s1 += max(-dl, 0); s2 += max(dO, 0); s3 += max(-dO, 0);
        }
        s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3);
    }
    if (lane == 0) {
        long long* o = S + 4 * ((size_t)gl * kRows + h);
        o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
    }
}

// ---- bands, normalisation, bits: wave per line
__global__ void __launch_bounds__(kBandThreads) k_lt_bands(const LtItem* __restrict__ items, const int32_t* __restrict__ geom,
                                                           const int32_t* __restrict__ line_item, const long long* __restrict__ S,
                                                           const double* __restrict__ tables, uint8_t* __restrict__ out_desc,
                                                           double* __restrict__ dbg_float) {
    __shared__ double sG[kRows], sLc[21], sD[kFloats], sScale[3];
    const int gl = blockIdx.x, lane = threadIdx.x;
    const LtItem I = items[line_item[gl]];
    uint8_t* slot = I.slot_desc + kBytes * (size_t)(gl - I.l_off);
    uint8_t* out = out_desc + kBytes * (size_t)gl;
    if (geom[8 * (size_t)gl + 6] != UVS_LT_OK) {
        if (lane < kBytes) { slot[lane] = 0; out[lane] = 0; }
        if (dbg_float) for (int i = lane; i < kFloats; i += kBandThreads) dbg_float[kFloats * (size_t)gl + i] = 0.0;
        return;
    }
    if (lane < kRows) sG[lane] = tables[lane];
    if (lane < 21) sLc[lane] = tables[kRows + lane];
    __syncthreads();
    if (lane < 36) {
        const int b = lane >> 2, k = lane & 3;
        const long long* s = S + 4 * (size_t)gl * kRows + k;
        double bs = 0.0, b2 = 0.0;
        const int h0 = max(0, 7 * (b - 1)), h1 = min(kRows - 1, 7 * (b + 1) + 6);
        for (int h = h0; h <= h1; ++h) {
            const double c = sLc[h - 7 * b + 7];
            const double r = sG[h] * (double)s[4 * h];
            const double r2 = r * r;
            bs = bs + c * r;
            b2 = b2 + (c * c) * r2;
        }
        const double inv = (b == 0 || b == 8) ? 1.0 / 14 : 1.0 / 21;
        const double m = bs * inv;
        const double v = b2 * inv - m * m;
        sD[8 * b + 2 * k] = m;
        sD[8 * b + 2 * k + 1] = sqrt(v > 0.0 ? v : 0.0);
    }
    __syncthreads();
    if (lane == 0) {
        double tm = 0.0, ts = 0.0;
        for (int i = 0; i < 36; ++i) { tm = tm + sD[2 * i] * sD[2 * i]; ts = ts + sD[2 * i + 1] * sD[2 * i + 1]; }
        sScale[0] = tm > 0.0 ? 1.0 / sqrt(tm) : 1.0;      // a multiplication by 1.0 changes nothing: the rule multiplies only if tm > 0
        sScale[1] = ts > 0.0 ? 1.0 / sqrt(ts) : 1.0;
    }
    __syncthreads();
    for (int i = lane; i < kFloats; i += kBandThreads) {
        const double v = sD[i] * sScale[i & 1];
        sD[i] = v > 0.4 ? 0.4 : v;
    }
    __syncthreads();
    if (lane == 0) {
        double tot = 0.0;
        for (int i = 0; i < kFloats; ++i) tot = tot + sD[i] * sD[i];
        sScale[2] = tot > 0.0 ? 1.0 / sqrt(tot) : 0.0;
    }
    __syncthreads();
    if (dbg_float) for (int i = lane; i < kFloats; i += kBandThreads) dbg_float[kFloats * (size_t)gl + i] = sScale[2] > 0.0 ? sD[i] * sScale[2] : 0.0;
    if (lane < kBytes) {
        // the lane-th pair (a, b) of (0, 1), (0, 2), .., (0, 8), (1, 2), ..
        int a = 0, p = lane;
        while (p >= 8 - a) { p -= 8 - a; ++a; }
        const int b = a + 1 + p;
        unsigned v = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) v |= (sD[8 * a + i] > sD[8 * b + i] ? 1u : 0u) << (7 - i);
        slot[lane] = (uint8_t)v; out[lane] = (uint8_t)v;
    }
}

// ---- match: workgroup per job, thread per previous line
__global__ void __launch_bounds__(kMatchThreads) k_lt_match(const LtMatchJob* __restrict__ jobs) {
    __shared__ unsigned long long sDesc[kMaxLines * 4];
    __shared__ int sOk[kMaxLines], sPoc[kMaxLines], sDist[kMaxLines];
    __shared__ int sMatched;
    const LtMatchJob J = jobs[blockIdx.x];
    const int tid = threadIdx.x, nq = min(J.n_prev, kMaxLines), nt = min(J.n_cur, kMaxLines);
    if (tid == 0) sMatched = 0;
    for (int i = tid; i < nt * 4; i += kMatchThreads) sDesc[i] = reinterpret_cast<const unsigned long long*>(J.cdesc)[i];      // every set is 32-byte aligned
    for (int t = tid; t < nt; t += kMatchThreads) { sOk[t] = J.cstat ? J.cstat[t] == UVS_LT_OK : 1; sPoc[t] = -1; }
    for (int q = tid; q < nq; q += kMatchThreads) sDist[q] = -1;
    __syncthreads();
    for (int q = tid; q < nq; q += kMatchThreads) {
        int mop = -1, dist = -1;
        if (!J.pstat || J.pstat[q] == UVS_LT_OK) {
            const unsigned long long* pd = reinterpret_cast<const unsigned long long*>(J.pdesc) + 4 * (size_t)q;
            const unsigned long long d[4] = {pd[0], pd[1], pd[2], pd[3]};
            unsigned best = 0xFFFFFFFFu;
            for (int t = 0; t < nt; ++t) {
                if (!sOk[t]) continue;
                const unsigned hd = __popcll(d[0] ^ sDesc[4 * t]) + __popcll(d[1] ^ sDesc[4 * t + 1]) + __popcll(d[2] ^ sDesc[4 * t + 2]) +
                                    __popcll(d[3] ^ sDesc[4 * t + 3]);
                best = min(best, (hd << 16) | (unsigned)t);
            }
            if (best != 0xFFFFFFFFu) {
                const int t = (int)(best & 0xFFFFu);
                dist = (int)(best >> 16);
                const int32_t* pe = J.pends + 4 * (size_t)q;
                const int32_t* ce = J.cends + 4 * (size_t)t;
                const long long ax = (long long)pe[0] - ce[0], ay = (long long)pe[1] - ce[1], bx = (long long)pe[2] - ce[2], by = (long long)pe[3] - ce[3];
                if (!(ax * ax + ay * ay > UVS_LT_GATE2 || bx * bx + by * by > UVS_LT_GATE2)) {
                    mop = t;
                    atomicMax(&sPoc[t], q);
                    atomicAdd(&sMatched, 1);
                }
            }
        }
        sDist[q] = dist;
        if (J.match_of_prev) J.match_of_prev[q] = mop;
        if (J.dist_prev) J.dist_prev[q] = dist;
    }
    __syncthreads();
    for (int t = tid; t < nt; t += kMatchThreads) {
        const int q = sPoc[t];
        if (J.prev_of_cur) J.prev_of_cur[t] = q;
        if (J.dist_cur) J.dist_cur[t] = q >= 0 ? sDist[q] : -1;
    }
    if (tid == 0 && J.result) J.result->n_matched = sMatched;
}

// ---- per item: n_described and the status
__global__ void __launch_bounds__(64) k_lt_count(const LtItem* __restrict__ items, const int32_t* __restrict__ status, uvs_lt_result* __restrict__ results) {
    const LtItem I = items[blockIdx.x];
    int c = 0;
    for (int l = threadIdx.x; l < I.n_lines; l += 64) c += status[I.l_off + l] == UVS_LT_OK;
    c = (int)wave_sum(c);
    if (threadIdx.x == 0) { results[blockIdx.x].n_described = c; results[blockIdx.x].n_matched = 0; results[blockIdx.x].status = 0; }
}

}  // namespace uvslt

using namespace uvslt;

namespace uvslt {

// One call's device work (uvs_lt_handle.h has the contract).
int lt_run(uvs_lt_tracker* h, int n_items, const uvs_lt_item* items, const std::vector<int>& slot_of, bool match, size_t tl, int max_n,
           double* dbg_float, LtLayout* layout, const uint8_t* dev_images, const size_t* dev_img_off) {
    std::vector<size_t> img_bytes, img_off;
    for (int b = 0; b < n_items; ++b) img_bytes.push_back((size_t)items[b].width * items[b].height);
    const LtLayout Y = lt_layout(n_items, tl, img_bytes, &img_off);
    *layout = Y;
    LtItem* hi = reinterpret_cast<LtItem*>(h->h_in.get());
    LtMatchJob* hj = reinterpret_cast<LtMatchJob*>(h->h_in + Y.o_jobs);
    uvs_lt_result* dRes = reinterpret_cast<uvs_lt_result*>(h->d_out.get());
    uint8_t* dDesc = reinterpret_cast<uint8_t*>(h->d_out + Y.o_desc);
    int32_t* dStat = reinterpret_cast<int32_t*>(h->d_out + Y.o_stat);
    int32_t* dPrev = reinterpret_cast<int32_t*>(h->d_out + Y.o_prev);
    int32_t* dDist = reinterpret_cast<int32_t*>(h->d_out + Y.o_dist);
    size_t lo = 0; int max_px = 0;
    for (int b = 0; b < n_items; ++b) {
        const uvs_lt_item& it = items[b];
        const int s = slot_of[b];
        const int nw = s < h->max_streams ? 1 - h->slots[s].cur : 0;      // the set that is not the previous one
        LtItem d;
        d.W = it.width; d.H = it.height; d.n_lines = it.n_lines; d.l_off = (int)lo; d.img_off = (long long)(dev_images ? dev_img_off[b] : img_off[b]);
        d.slot_desc = h->set_desc(s, nw); d.slot_ends = h->set_ends(s, nw); d.slot_stat = h->set_stat(s, nw);
        hi[b] = d;
        LtMatchJob j;
        std::memset(&j, 0, sizeof j);
        if (match) {
            const int pv = h->slots[s].cur;
            j.pdesc = h->set_desc(s, pv); j.pends = h->set_ends(s, pv); j.pstat = h->set_stat(s, pv); j.n_prev = h->slots[s].n_prev;
            j.cdesc = d.slot_desc; j.cends = d.slot_ends; j.cstat = d.slot_stat; j.n_cur = it.n_lines;
            j.prev_of_cur = dPrev + lo; j.dist_cur = dDist + lo; j.result = dRes + b;
        }
        hj[b] = j;
        if (it.n_lines) std::memcpy(h->h_in + Y.o_seg + lo * 32, it.segments, (size_t)it.n_lines * 32);
        if (!dev_images) std::memcpy(h->h_in + img_off[b], it.image, img_bytes[b]);
        lo += it.n_lines; max_px = std::max(max_px, it.width * it.height);
    }
    const LtItem* dI = reinterpret_cast<const LtItem*>(h->d_in.get());
    const LtMatchJob* dJ = reinterpret_cast<const LtMatchJob*>(h->d_in + Y.o_jobs);
    const double* dSeg = reinterpret_cast<const double*>(h->d_in + Y.o_seg);
    const uint8_t* dIn = dev_images ? dev_images : reinterpret_cast<const uint8_t*>(h->d_in.get());
    hipStream_t st = h->st;
    UVS_HIP(h->err, hipSetDevice(h->device));
    UVS_HIP(h->err, hipEventRecord(h->ev0, st));
    UVS_HIP(h->err, hipMemcpyAsync(h->d_in, h->h_in, dev_images ? Y.o_img : Y.in_used, hipMemcpyHostToDevice, st));
    k_lt_gradient<<<dim3(std::min((max_px + kGradThreads - 1) / kGradThreads, 1024), n_items), kGradThreads, 0, st>>>(dI, dIn, h->d_grad, h->grad_stride);
    if (tl) {
        k_lt_prepare<<<dim3((max_n + kPrepThreads - 1) / kPrepThreads, n_items), kPrepThreads, 0, st>>>(dI, dSeg, h->max_length, h->d_geom, h->d_line_item, dStat);
        k_lt_rows<<<dim3((unsigned)tl, (kRows + kRowWaves - 1) / kRowWaves), kRowThreads, 0, st>>>(dI, h->d_geom, h->d_line_item, h->d_grad, h->grad_stride, h->d_S);
        k_lt_bands<<<(unsigned)tl, kBandThreads, 0, st>>>(dI, h->d_geom, h->d_line_item, h->d_S, h->d_tables, dDesc, dbg_float);
    }
    k_lt_count<<<n_items, 64, 0, st>>>(dI, dStat, dRes);
    if (match) k_lt_match<<<n_items, kMatchThreads, 0, st>>>(dJ);
    UVS_HIP(h->err, hipGetLastError());
    UVS_HIP(h->err, hipMemcpyAsync(h->h_out, h->d_out, Y.out_used, hipMemcpyDeviceToHost, st));
    UVS_HIP(h->err, hipEventRecord(h->ev1, st));
    UVS_HIP(h->err, hipStreamSynchronize(st));
    return UVS_OK;
}

}  // namespace uvslt

extern "C" {

void uvs_lt_gauss_tables(double* G, double* Lc) {
    if (G) for (int h = 0; h < kRows; ++h) G[h] = std::exp(-(double)((h - 31) * (h - 31)) / 1922.0);       // 2 x 31^2
    if (Lc) for (int i = 0; i < 21; ++i) Lc[i] = std::exp(-(double)((i - 10) * (i - 10)) / 98.0);          // 2 x 7^2
}

int uvs_lt_create(int device, int max_streams, int max_width, int max_height, int max_lines, int max_length, uvs_lt_tracker** out) {
    if (!out || max_streams < 1 || max_lines < 1 || max_width < UVS_LT_MIN_SIZE || max_height < UVS_LT_MIN_SIZE || max_length < 2) return UVS_ERR_INVALID_ARG;
    *out = nullptr;
    if (max_streams > UVS_LT_MAX_STREAMS || max_width > UVS_KF_MAX_WIDTH || max_height > UVS_KF_MAX_HEIGHT || max_lines > UVS_LT_MAX_LINES ||
        max_length > UVS_LT_MAX_LENGTH) return UVS_ERR_CAPACITY;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return UVS_ERR_NO_DEVICE;
    uvs_lt_tracker* h = new uvs_lt_tracker();
    h->max_streams = max_streams; h->max_width = max_width; h->max_height = max_height; h->max_lines = max_lines; h->max_length = max_length;
    h->slots.assign(max_streams, LtSlot());
    h->ud.resize(max_streams);
    const size_t B = max_streams, Lt = B * max_lines, px = (size_t)max_width * max_height, sets = 2 * (B + 1) * (size_t)max_lines;
    h->grad_stride = px;
    // the larger of a full uvs_lt_track and a full uvs_lt_match (two descriptor sets and their gate points in, three index arrays out)
    const LtLayout Y = lt_layout(B, Lt, std::vector<size_t>(B, px), nullptr);
    UvsArena mi, mo;
    (void)mi.take(sizeof(LtMatchJob));
    for (int k = 0; k < 2; ++k) { (void)mi.take((size_t)max_lines * kBytes); (void)mi.take((size_t)max_lines * 16); }
    for (int k = 0; k < 3; ++k) (void)mo.take((size_t)max_lines * 4);
    h->in_bytes = std::max(Y.in_used, mi.o); h->out_bytes = std::max(Y.out_used, mo.o);
    int rc = h->open(device);
    if (rc == UVS_OK && (rc = h->d_in.ensure(h->in_bytes, h->err)) == UVS_OK && (rc = h->d_out.ensure(h->out_bytes, h->err)) == UVS_OK &&
        (rc = h->h_in.ensure(h->in_bytes, h->err)) == UVS_OK && (rc = h->h_out.ensure(h->out_bytes, h->err)) == UVS_OK &&
        (rc = h->d_grad.ensure(B * px * 4, h->err)) == UVS_OK && (rc = h->d_geom.ensure(Lt * 32, h->err)) == UVS_OK &&
        (rc = h->d_line_item.ensure(Lt * 4, h->err)) == UVS_OK && (rc = h->d_S.ensure(Lt * kRows * 32, h->err)) == UVS_OK &&
        (rc = h->d_tables.ensure((kRows + 21) * 8, h->err)) == UVS_OK && (rc = h->d_slot_desc.ensure(sets * kBytes, h->err)) == UVS_OK &&
        (rc = h->d_slot_ends.ensure(sets * 16, h->err)) == UVS_OK && (rc = h->d_slot_stat.ensure(sets * 4, h->err)) == UVS_OK)
        rc = h->d_dbg_float.ensure(kFloats * 8, h->err);
    if (rc == UVS_OK) {
        double tab[kRows + 21];
        uvs_lt_gauss_tables(tab, tab + kRows);
        const hipError_t e = hipMemcpy(h->d_tables, tab, sizeof tab, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = hip_fail(h->err, e, "hipMemcpy");
    }
    if (rc != UVS_OK) { uvs_lt_destroy(h); return rc; }
    *out = h;
    return UVS_OK;
}

void uvs_lt_destroy(uvs_lt_tracker* h) { if (h) { h->close(); delete h; } }

const char* uvs_lt_last_error(const uvs_lt_tracker* h) { return h ? h->err.c_str() : "null line tracker"; }

double uvs_lt_last_device_ms(const uvs_lt_tracker* h) { return h ? (double)h->device_ms : 0.0; }

int uvs_lt_reset(uvs_lt_tracker* h, int stream) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    if (stream < 0 || stream >= h->max_streams) { h->err = "uvs_lt_reset: stream outside the handle's slots"; return UVS_ERR_INVALID_ARG; }
    h->slots[stream].n_prev = 0;
    return UVS_OK;
}

int uvs_lt_track(uvs_lt_tracker* h, int n_items, const uvs_lt_item* items, uint8_t* desc, int32_t* line_status, int32_t* prev_index,
                 int32_t* distance, uvs_lt_result* results) {
    if (!h) return UVS_ERR_INVALID_ARG;
    const std::string fn = "uvs_lt_track";
    h->err.clear();
    if (n_items < 1 || !items || !desc || !line_status || !prev_index || !distance || !results) { h->err = fn + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG; }
    if (n_items > h->max_streams) { h->err = fn + ": more items than the capacity given to uvs_lt_create"; return UVS_ERR_CAPACITY; }
    size_t tl = 0; int max_n = 0;
    int rc = lt_check_items(h, fn, n_items, items, true, &tl, &max_n);
    if (rc != UVS_OK) return rc;
    std::vector<int> slot_of(n_items);
    for (int b = 0; b < n_items; ++b) slot_of[b] = items[b].stream;
    LtLayout Y;
    rc = lt_run(h, n_items, items, slot_of, true, tl, max_n, nullptr, &Y);
    if (rc != UVS_OK) return rc;
    UVS_HIP(h->err, hipEventElapsedTime(&h->device_ms, h->ev0, h->ev1));
    for (int b = 0; b < n_items; ++b) {          // the new lines become the slot's previous ones
        LtSlot& s = h->slots[items[b].stream];
        s.cur = 1 - s.cur; s.n_prev = items[b].n_lines;
    }
    std::memcpy(results, h->h_out, n_items * sizeof(uvs_lt_result));
    if (tl) {
        std::memcpy(desc, h->h_out + Y.o_desc, tl * kBytes);
        std::memcpy(line_status, h->h_out + Y.o_stat, tl * 4);
        std::memcpy(prev_index, h->h_out + Y.o_prev, tl * 4);
        std::memcpy(distance, h->h_out + Y.o_dist, tl * 4);
    }
    return UVS_OK;
}

int uvs_lt_match(uvs_lt_tracker* h, int n_prev, const uint8_t* prev_desc, const int32_t* prev_ends, int n_cur, const uint8_t* cur_desc,
                 const int32_t* cur_ends, int32_t* match_of_prev, int32_t* distance, int32_t* prev_of_cur) {
    if (!h) return UVS_ERR_INVALID_ARG;
    const std::string fn = "uvs_lt_match";
    h->err.clear();
    if (n_prev < 0 || n_cur < 0 || (n_prev > 0 && (!prev_desc || !prev_ends || !match_of_prev || !distance)) ||
        (n_cur > 0 && (!cur_desc || !cur_ends || !prev_of_cur))) { h->err = fn + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG; }
    if (n_prev > h->max_lines || n_cur > h->max_lines) { h->err = fn + ": more lines than the capacity given to uvs_lt_create"; return UVS_ERR_CAPACITY; }
    UvsArena in, out;
    const size_t o_job = in.take(sizeof(LtMatchJob)), o_pd = in.take((size_t)n_prev * kBytes), o_pe = in.take((size_t)n_prev * 16),
                 o_cd = in.take((size_t)n_cur * kBytes), o_ce = in.take((size_t)n_cur * 16);
    const size_t o_mop = out.take((size_t)n_prev * 4), o_dq = out.take((size_t)n_prev * 4), o_poc = out.take((size_t)n_cur * 4);
    LtMatchJob j;
    std::memset(&j, 0, sizeof j);
    j.pdesc = reinterpret_cast<const uint8_t*>(h->d_in + o_pd); j.pends = reinterpret_cast<const int32_t*>(h->d_in + o_pe);
    j.cdesc = reinterpret_cast<const uint8_t*>(h->d_in + o_cd); j.cends = reinterpret_cast<const int32_t*>(h->d_in + o_ce);
    j.n_prev = n_prev; j.n_cur = n_cur;
    j.match_of_prev = reinterpret_cast<int32_t*>(h->d_out + o_mop); j.dist_prev = reinterpret_cast<int32_t*>(h->d_out + o_dq);
    j.prev_of_cur = reinterpret_cast<int32_t*>(h->d_out + o_poc);
    std::memcpy(h->h_in + o_job, &j, sizeof j);
    if (n_prev) { std::memcpy(h->h_in + o_pd, prev_desc, (size_t)n_prev * kBytes); std::memcpy(h->h_in + o_pe, prev_ends, (size_t)n_prev * 16); }
    if (n_cur) { std::memcpy(h->h_in + o_cd, cur_desc, (size_t)n_cur * kBytes); std::memcpy(h->h_in + o_ce, cur_ends, (size_t)n_cur * 16); }
    hipStream_t st = h->st;
    UVS_HIP(h->err, hipSetDevice(h->device));
    UVS_HIP(h->err, hipMemcpyAsync(h->d_in, h->h_in, in.o, hipMemcpyHostToDevice, st));
    k_lt_match<<<1, kMatchThreads, 0, st>>>(reinterpret_cast<const LtMatchJob*>(h->d_in + o_job));
    UVS_HIP(h->err, hipGetLastError());
    UVS_HIP(h->err, hipMemcpyAsync(h->h_out, h->d_out, out.o, hipMemcpyDeviceToHost, st));
    UVS_HIP(h->err, hipStreamSynchronize(st));
    if (n_prev) { std::memcpy(match_of_prev, h->h_out + o_mop, (size_t)n_prev * 4); std::memcpy(distance, h->h_out + o_dq, (size_t)n_prev * 4); }
    if (n_cur) std::memcpy(prev_of_cur, h->h_out + o_poc, (size_t)n_cur * 4);
    return UVS_OK;
}

int uvs_lt_debug_line(uvs_lt_tracker* h, const uint8_t* image, int width, int height, const double* segment, int32_t* geom, int64_t* row_sums,
                      double* desc_float, uint8_t* desc) {
    if (!h) return UVS_ERR_INVALID_ARG;
    const std::string fn = "uvs_lt_debug_line";
    h->err.clear();
    if (!image || !segment || !geom || !row_sums || !desc_float || !desc) { h->err = fn + ": null pointer"; return UVS_ERR_INVALID_ARG; }
    uvs_lt_item it;
    it.image = image; it.stream = 0; it.width = width; it.height = height; it.n_lines = 1; it.segments = segment;
    size_t tl = 0; int max_n = 0;
    int rc = lt_check_items(h, fn, 1, &it, false, &tl, &max_n);
    if (rc != UVS_OK) return rc;
    LtLayout Y;
    rc = lt_run(h, 1, &it, std::vector<int>(1, h->max_streams), false, tl, max_n, h->d_dbg_float, &Y);
    if (rc != UVS_OK) return rc;
    std::memcpy(desc, h->h_out + Y.o_desc, kBytes);
    UVS_HIP(h->err, hipMemcpy(geom, h->d_geom, 32, hipMemcpyDeviceToHost));
    UVS_HIP(h->err, hipMemcpy(row_sums, h->d_S, (size_t)kRows * 32, hipMemcpyDeviceToHost));
    UVS_HIP(h->err, hipMemcpy(desc_float, h->d_dbg_float, kFloats * 8, hipMemcpyDeviceToHost));
    return UVS_OK;
}

}  // extern "C"
