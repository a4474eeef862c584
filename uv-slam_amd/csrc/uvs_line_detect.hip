// uvs_line_detect.hip -- segment detection of the line front end (the place of elsed.detect(forw_img) in the reference's lineExtraction)
// behind uvs_lt_detect, uvs_lt_detect_track and uvs_lt_debug_detect of include/uvs_solver.h: Burns-style line-support regions, the project's
// own rule, stated in the header and restated in tests/ld_ref.py, which this unit is held to bit for bit.  The handle is the line tracker's
// (csrc/uvs_lt_handle.h); uvs_lt_detect_track hands the returned segments to the tracking unit's lt_run with the images already on the device.
// gfx950, the handle's one stream.
//
// One call takes a batch of items; no kernel reads another item's data, so an item gives the same bits alone or in a batch.  This unit is
// compiled with -ffp-contract=off.  Everything up to the six moment sums is integer arithmetic, and every value that several threads combine is
// combined by an integer atomic (add, min, max), exact in any order: no float atomics.  Kernels of one call, in stream order; a thread owns a
// pixel, the rows of the thread space are padded to a multiple of 64 so that a wave is 64 consecutive pixels of ONE image row:
//   k_lt_det_blur      the 5 x 5 binomial as the header states it
//   k_lt_det_sectors   the packed Sobel of the blurred image, M, both sector maps; the first parents of the union-find: a pixel points at the
//                      start of its run of like sector inside its wave (a ballot of the run breaks), so the rows are already joined 64 wide
//   k_lt_det_link      union-find on global parents, both partitions: a pixel unites with its left neighbour across a wave's edge, with the
//                      pixel above, or with a diagonal one above where the pixel above does not already connect them; a union that the pixels to
//                      the left already imply is skipped (a region of a whole image unites only along its first column).  A union hooks the
//                      larger root under the smaller with an integer atomicMin; parents are read with relaxed agent-scope atomic loads
//   k_lt_det_flatten   parent = root = the region's name; a root clears its record and counts a region
//   k_lt_det_sizes     n per region
//   k_lt_det_moments   the vote, s, and the six sums of the regions with n >= min_pixels
//   k_lt_det_fit       thread per region: candidate test and the FP64 fit; the record then holds the fit
//   k_lt_det_extent    tmin, tmax by 64-bit integer min / max of the order-preserving image of the doubles
//   k_lt_det_keep      thread per region: length >= min_length appends (length, 2 name + partition) to the item's list, in no order
//   k_lt_det_rank      a workgroup per item: if more than max_lines were kept, the max_lines-th key of the ranking by a bitwise search over
//                      counts; the at most 1024 chosen ones in LDS, each ranked by counting, written at its rank
// The atomics of the sizes, sums and extents are pre-reduced inside a wave over the lanes that share a region (the first kRounds regions of a
// wave; further lanes add for themselves).  Every loop has a strictly decreasing quantity, written at the loop.  No kernel uses scratch memory.
//
// Deviation from the plan the issue suggested: the labelling has no tile-local pass in LDS.  The run starts of k_lt_det_sectors and the skipped
// implied unions leave so few unions on global memory that the tile pass was not built; DESIGN.md 3.15 has the timings.
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

namespace uvsld {

constexpr int kThreads = 256, kRankThreads = 1024, kRounds = 4;
constexpr unsigned kValid = 0x80000000u;       // in DetRec::s after the fit: the region is a candidate with a direction
constexpr int kNone = 255;
static_assert(UVS_LT_MAX_LINES <= kRankThreads, "the chosen segments are ranked a thread each");

struct DetItem { int W, H; long long img_off; };      // device copy of one item: size, offset of the image in the packed input

// what is kept at a region's name, 64 bytes.  Until k_lt_det_fit: v[0 .. 5] = S0, Sx, Sy, Sxx, Sxy, Syy.  From k_lt_det_fit on, for a region
// with kValid: v[0 .. 4] = the bits of mx, my, ux, uy, width2, v[5] = key(tmin), v[6] = key(tmax)
struct DetRec { int n; unsigned s; long long v[7]; };
static_assert(sizeof(DetRec) == 64, "one record per pixel and partition");

struct DetBufs {                   // the work space; every array is [items][...] with the strides of the handle's largest image
    size_t px;                     // max_width max_height
    const uint8_t* in; uint8_t* blur; uint32_t* grad; uint8_t* sec; uint8_t* vote; int32_t* label; DetRec* rec;
    unsigned long long* list_len; uint32_t* list_id;
    uvs_lt_det_result* res;
    double* seg; double* width2; int32_t* info;      // [items][max_lines] rows
    int max_lines;
};

// the thread's pixel: false (for the whole wave) beyond the item's padded rows; `in` says whether x is inside the row
__device__ __forceinline__ bool det_pixel(const DetItem& I, int& x, int& y, bool& in) {
    const int Wp = (I.W + 63) & ~63;
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= Wp * I.H) return false;
    y = t / Wp; x = t - y * Wp; in = x < I.W;
    return true;
}

__device__ __forceinline__ int load_parent(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of i.  A parent that differs from its pixel is smaller than it, so i strictly decreases
__device__ __forceinline__ int det_find(const int32_t* L, int i) {
    for (int p = load_parent(L + i); p != i; p = load_parent(L + i)) i = p;
    return i;
}

// joins the trees of a and b.  Each round takes the two roots, a > b, and tries to hook a under b.  If a was still a root, that is the end.
// If not, somebody gave a the parent `old` < a meanwhile (and our minimum may have replaced it by b): what remains is to join old and b, both
// smaller than a.  The larger of the pair strictly decreases from round to round, and a round is repeated only behind an atomicMin that
// lowered parent[a], ours or another thread's
__device__ __forceinline__ void det_unite(int32_t* L, int a, int b) {
    for (;;) {
        a = det_find(L, a); b = det_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;
    }
}

// the order-preserving image of a double in the unsigned 64-bit integers, and back
__device__ __forceinline__ unsigned long long key_of(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double double_of(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

__device__ __forceinline__ long long wave_sum_all(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_min_all(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ unsigned long long wave_max_all(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return v;
}

// ---- blur: sum_j k_j (sum_i k_i I[refl(y + j - 2)][refl(x + i - 2)]), the same integer as rows then columns
__global__ void __launch_bounds__(kThreads) k_lt_det_blur(const DetItem* __restrict__ items, DetBufs B) {
    const DetItem I = items[blockIdx.y];
    int x, y; bool in;
    if (!det_pixel(I, x, y, in) || !in) return;
    const uint8_t* p = B.in + I.img_off;
    const int xs[5] = {reflect101(x - 2, I.W), reflect101(x - 1, I.W), x, reflect101(x + 1, I.W), reflect101(x + 2, I.W)};
    int sum = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint8_t* r = p + (size_t)reflect101(y + j - 2, I.H) * I.W;
        const int row = r[xs[0]] + 4 * r[xs[1]] + 6 * r[xs[2]] + 4 * r[xs[3]] + r[xs[4]];
        sum += (j == 0 || j == 4 ? 1 : j == 2 ? 6 : 4) * row;
    }
    B.blur[B.px * blockIdx.y + (size_t)y * I.W + x] = (uint8_t)((sum + 128) >> 8);
}

// the header's step 3 for a gradient with M > 0
__device__ __forceinline__ void det_sectors(int gx, int gy, int& A, int& Bs) {
    int q, px, py;
    if (gx > 0 && gy >= 0) { q = 0; px = gx; py = gy; }
    else if (gx <= 0 && gy > 0) { q = 1; px = gy; py = -gx; }
    else if (gx < 0 && gy <= 0) { q = 2; px = -gx; py = -gy; }
    else { q = 3; px = -gy; py = gx; }
    A = 2 * q + (py >= px ? 1 : 0);
    Bs = (2 * q + (985 * py >= 408 * px ? 1 : 0) + (408 * py >= 985 * px ? 1 : 0)) & 7;
}

// ---- gradient, sectors, the run starts
__global__ void __launch_bounds__(kThreads) k_lt_det_sectors(const DetItem* __restrict__ items, DetBufs B, int T) {
    const DetItem I = items[blockIdx.y];
    int x, y; bool in;
    if (!det_pixel(I, x, y, in)) return;
    const int lane = threadIdx.x & 63, W = I.W;
    const size_t base = B.px * blockIdx.y;
    const int i = y * W + x;                               // meaningful where `in`
    int sA = kNone, sB = kNone;
    if (in) {
        const uint32_t g = uvs_sobel_packed(B.blur + base, W, I.H, x, y);
        const int gx = (int)(int16_t)(g & 0xFFFFu), gy = (int)(int16_t)(g >> 16);
        B.grad[base + i] = g;
        if (abs(gx) + abs(gy) >= T) det_sectors(gx, gy, sA, sB);
        B.sec[2 * base + i] = (uint8_t)sA; B.sec[2 * base + B.px + i] = (uint8_t)sB;
        B.vote[base + i] = (uint8_t)kNone;
    }
    const bool sup = sA != kNone;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int s = p ? sB : sA;
        const int left = __shfl_up(s, 1, 64);
        const bool brk = !(sup && lane > 0 && left == s);  // this lane starts a run (lane 0 always does)
        const unsigned long long m = __ballot(brk);
        const int start = 63 - __clzll((long long)(m & ((2ull << lane) - 1ull)));      // the last break at or below the lane; bit 0 is set
        if (in) B.label[2 * base + p * B.px + i] = sup ? i - (lane - start) : -1;
    }
    const unsigned long long ms = __ballot(sup);
    if (lane == 0 && ms) atomicAdd(&B.res[blockIdx.y].n_support, __popcll(ms));
}

// ---- the unions
__global__ void __launch_bounds__(kThreads) k_lt_det_link(const DetItem* __restrict__ items, DetBufs B) {
    const DetItem I = items[blockIdx.y];
    int x, y; bool in;
    if (!det_pixel(I, x, y, in) || !in) return;
    const int lane = threadIdx.x & 63, W = I.W, i = y * W + x;
    const size_t base = B.px * blockIdx.y;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const uint8_t* sc = B.sec + 2 * base + p * B.px;
        int32_t* L = B.label + 2 * base + p * B.px;
        const int s = sc[i];
        if (s == kNone) continue;
        const bool left = x > 0 && sc[i - 1] == s;
        if (left && lane == 0) det_unite(L, i, i - 1);     // inside a wave the run starts have joined them
        if (y > 0) {
            const bool up = sc[i - W] == s, nw = x > 0 && sc[i - W - 1] == s, ne = x < W - 1 && sc[i - W + 1] == s;
            if (up) {
                if (!(left && nw)) det_unite(L, i, i - W); // implied otherwise: i ~ left ~ nw (left's own pixel above) ~ up (same row)
            } else {
                if (nw && !left) det_unite(L, i, i - W - 1);      // with left: i ~ left ~ nw
                if (ne) det_unite(L, i, i - W + 1);
            }                                              // with up, both diagonals are implied: they are up's row neighbours
        }
    }
}

// ---- names; a root clears its record
__global__ void __launch_bounds__(kThreads) k_lt_det_flatten(const DetItem* __restrict__ items, DetBufs B) {
    const DetItem I = items[blockIdx.y];
    int x, y; bool in;
    if (!det_pixel(I, x, y, in)) return;
    const int lane = threadIdx.x & 63, i = y * I.W + x;
    const size_t base = B.px * blockIdx.y;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        int32_t* L = B.label + 2 * base + p * B.px;
        bool root = false;
        if (in && load_parent(L + i) >= 0) {
            const int r = det_find(L, i);
            __hip_atomic_store(L + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // another thread's find may pass here: old parent or root, both lead to r
            root = r == i;
            if (root) {
                DetRec* R = B.rec + 2 * base + p * B.px + i;
                R->n = 0; R->s = 0;
#pragma unroll
                for (int k = 0; k < 7; ++k) R->v[k] = 0;
            }
        }
        const unsigned long long m = __ballot(root);
        if (lane == 0 && m) atomicAdd(&B.res[blockIdx.y].n_regions[p], __popcll(m));
    }
}

// ---- sizes
__global__ void __launch_bounds__(kThreads) k_lt_det_sizes(const DetItem* __restrict__ items, DetBufs B) {
    const DetItem I = items[blockIdx.y];
    int x, y; bool in;
    if (!det_pixel(I, x, y, in)) return;
    const int lane = threadIdx.x & 63, i = y * I.W + x;
    const size_t base = B.px * blockIdx.y;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int root = in ? B.label[2 * base + p * B.px + i] : -1;
        DetRec* R = B.rec + 2 * base + p * B.px;
        const bool act = root >= 0;
        unsigned long long todo = __ballot(act);
        for (int round = 0; round < kRounds && todo; ++round) {      // todo loses at least its first lane
            const int leader = __ffsll((long long)todo) - 1;
            const int r = __shfl(root, leader, 64);
            const unsigned long long m = __ballot(act && root == r);
            if (lane == leader) atomicAdd(&R[r].n, __popcll(m));
            todo &= ~m;
        }
        if (act && ((todo >> lane) & 1ull)) atomicAdd(&R[root].n, 1);
    }
}

// ---- vote, support, moment sums
__global__ void __launch_bounds__(kThreads) k_lt_det_moments(const DetItem* __restrict__ items, DetBufs B, int min_pixels) {
    const DetItem I = items[blockIdx.y];
    int x, y; bool in;
    if (!det_pixel(I, x, y, in)) return;
    const int lane = threadIdx.x & 63, W = I.W, i = y * W + x;
    const size_t base = B.px * blockIdx.y;
    DetRec* RA = B.rec + 2 * base; DetRec* RB = RA + B.px;
    const int rootA = in ? B.label[2 * base + i] : -1;
    const bool sup = rootA >= 0;
    int rootB = -1, nA = 0, nB = 0, w = 0;
    if (sup) {
        rootB = B.label[2 * base + B.px + i];
        nA = RA[rootA].n; nB = RB[rootB].n;
        const uint32_t g = B.grad[base + i];
        w = abs((int)(int16_t)(g & 0xFFFFu)) + abs((int)(int16_t)(g >> 16));
        B.vote[base + i] = nA >= nB ? 0 : 1;
    }
    const bool voteA = nA >= nB;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        DetRec* R = p ? RB : RA;
        const int root = p ? rootB : rootA;
        const bool act = sup && (p ? nB : nA) >= min_pixels;
        const bool mine = act && (voteA == (p == 0));
        long long dx = 0, dy = 0;
        if (act) { dx = x - root % W; dy = y - root / W; }
        const long long w0 = act ? w : 0, wx = w0 * dx, wy = w0 * dy, wxx = wx * dx, wxy = wx * dy, wyy = wy * dy;
        unsigned long long todo = __ballot(act);
        for (int round = 0; round < kRounds && todo; ++round) {      // todo loses at least its first lane
            const int leader = __ffsll((long long)todo) - 1;
            const int r = __shfl(root, leader, 64);
            const bool sel = act && root == r;
            const unsigned long long m = __ballot(sel), mv = __ballot(sel && mine);
            const long long t0 = wave_sum_all(sel ? w0 : 0), t1 = wave_sum_all(sel ? wx : 0), t2 = wave_sum_all(sel ? wy : 0),
                            t3 = wave_sum_all(sel ? wxx : 0), t4 = wave_sum_all(sel ? wxy : 0), t5 = wave_sum_all(sel ? wyy : 0);
            if (lane == leader) {
                if (mv) atomicAdd(&R[r].s, (unsigned)__popcll(mv));
                unsigned long long* v = reinterpret_cast<unsigned long long*>(R[r].v);
                atomicAdd(v + 0, (unsigned long long)t0); atomicAdd(v + 1, (unsigned long long)t1); atomicAdd(v + 2, (unsigned long long)t2);
                atomicAdd(v + 3, (unsigned long long)t3); atomicAdd(v + 4, (unsigned long long)t4); atomicAdd(v + 5, (unsigned long long)t5);
            }
            todo &= ~m;
        }
        if (act && ((todo >> lane) & 1ull)) {
            if (mine) atomicAdd(&R[root].s, 1u);
            unsigned long long* v = reinterpret_cast<unsigned long long*>(R[root].v);
            atomicAdd(v + 0, (unsigned long long)w0); atomicAdd(v + 1, (unsigned long long)wx); atomicAdd(v + 2, (unsigned long long)wy);
            atomicAdd(v + 3, (unsigned long long)wxx); atomicAdd(v + 4, (unsigned long long)wxy); atomicAdd(v + 5, (unsigned long long)wyy);
        }
    }
}

// ---- the fit: thread per region (at its name)
__global__ void __launch_bounds__(kThreads) k_lt_det_fit(const DetItem* __restrict__ items, DetBufs B, int min_pixels) {
    const DetItem I = items[blockIdx.y];
    int x, y; bool in;
    if (!det_pixel(I, x, y, in) || !in) return;
    const int i = y * I.W + x;
    const size_t base = B.px * blockIdx.y;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (B.label[2 * base + p * B.px + i] != i) continue;
        DetRec* R = B.rec + 2 * base + p * B.px + i;
        const int n = R->n; const unsigned s = R->s;
        if (n < min_pixels || 2ll * s <= (long long)n) continue;
        const double S0 = (double)R->v[0], Sx = (double)R->v[1], Sy = (double)R->v[2], Sxx = (double)R->v[3], Sxy = (double)R->v[4], Syy = (double)R->v[5];
        const double mx = Sx / S0, my = Sy / S0;
        const double a = Sxx / S0 - mx * mx, c = Syy / S0 - my * my, b = Sxy / S0 - mx * my;
        const double h = (a - c) * 0.5;
        const double r = sqrt(h * h + b * b);
        double ux = a >= c ? h + r : b, uy = a >= c ? b : r - h;
        const double nrm = sqrt(ux * ux + uy * uy);
        if (nrm == 0.0) continue;
        ux = ux / nrm; uy = uy / nrm;
        const double width2 = (a + c) * 0.5 - r;
        R->v[0] = __double_as_longlong(mx); R->v[1] = __double_as_longlong(my); R->v[2] = __double_as_longlong(ux); R->v[3] = __double_as_longlong(uy);
        R->v[4] = __double_as_longlong(width2);
        R->v[5] = (long long)0xFFFFFFFFFFFFFFFFull; R->v[6] = 0;      // above and below every key
        R->s = s | kValid;
    }
}

// ---- tmin, tmax
__global__ void __launch_bounds__(kThreads) k_lt_det_extent(const DetItem* __restrict__ items, DetBufs B) {
    const DetItem I = items[blockIdx.y];
    int x, y; bool in;
    if (!det_pixel(I, x, y, in)) return;
    const int lane = threadIdx.x & 63, W = I.W, i = y * W + x;
    const size_t base = B.px * blockIdx.y;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        DetRec* R = B.rec + 2 * base + p * B.px;
        const int root = in ? B.label[2 * base + p * B.px + i] : -1;
        const bool act = root >= 0 && (R[root].s & kValid);
        unsigned long long k = 0;
        if (act) {
            const double mx = __longlong_as_double(R[root].v[0]), my = __longlong_as_double(R[root].v[1]), ux = __longlong_as_double(R[root].v[2]),
                         uy = __longlong_as_double(R[root].v[3]);
            const double dx = (double)(x - root % W), dy = (double)(y - root / W);
            k = key_of((dx - mx) * ux + (dy - my) * uy);
        }
        unsigned long long todo = __ballot(act);
        for (int round = 0; round < kRounds && todo; ++round) {      // todo loses at least its first lane
            const int leader = __ffsll((long long)todo) - 1;
            const int r = __shfl(root, leader, 64);
            const bool sel = act && root == r;
            const unsigned long long m = __ballot(sel);
            const unsigned long long lo = wave_min_all(sel ? k : 0xFFFFFFFFFFFFFFFFull), hi = wave_max_all(sel ? k : 0ull);
            if (lane == leader) {
                atomicMin(reinterpret_cast<unsigned long long*>(&R[r].v[5]), lo);
                atomicMax(reinterpret_cast<unsigned long long*>(&R[r].v[6]), hi);
            }
            todo &= ~m;
        }
        if (act && ((todo >> lane) & 1ull)) {
            atomicMin(reinterpret_cast<unsigned long long*>(&R[root].v[5]), k);
            atomicMax(reinterpret_cast<unsigned long long*>(&R[root].v[6]), k);
        }
    }
}

// ---- the kept segments, in no order
__global__ void __launch_bounds__(kThreads) k_lt_det_keep(const DetItem* __restrict__ items, DetBufs B, double min_length) {
    const DetItem I = items[blockIdx.y];
    int x, y; bool in;
    if (!det_pixel(I, x, y, in) || !in) return;
    const int i = y * I.W + x;
    const size_t base = B.px * blockIdx.y;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (B.label[2 * base + p * B.px + i] != i) continue;
        const DetRec* R = B.rec + 2 * base + p * B.px + i;
        if (!(R->s & kValid)) continue;
        const double length = double_of((unsigned long long)R->v[6]) - double_of((unsigned long long)R->v[5]);
        if (!(length >= min_length)) continue;
        const int slot = atomicAdd(&B.res[blockIdx.y].n_found, 1);      // at most one per region with n >= 2: fewer than px
        B.list_len[base + slot] = (unsigned long long)__double_as_longlong(length);      // positive: the bits order as the values
        B.list_id[base + slot] = 2u * (unsigned)i + (unsigned)p;
    }
}

// ---- ranking: workgroup per item
// the number of list entries for which pred holds, to every thread
template <class P>
__device__ __forceinline__ int rank_count(int K, int* sCnt, P pred) {
    int c = 0;
    for (int k = threadIdx.x; k < K; k += kRankThreads) c += pred(k) ? 1 : 0;
    c = (int)wave_sum_all(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(sCnt, c);
    __syncthreads();
    const int total = *sCnt;
    __syncthreads();
    if (threadIdx.x == 0) *sCnt = 0;
    __syncthreads();
    return total;
}

__global__ void __launch_bounds__(kRankThreads) k_lt_det_rank(const DetItem* __restrict__ items, DetBufs B) {
    __shared__ unsigned long long sLen[kRankThreads];
    __shared__ unsigned sId[kRankThreads];
    __shared__ int sCnt, sTake;
    const DetItem I = items[blockIdx.x];
    const size_t base = B.px * blockIdx.x;
    const unsigned long long* len = B.list_len + base;
    const uint32_t* id = B.list_id + base;
    uvs_lt_det_result* res = B.res + blockIdx.x;
    const int K = res->n_found, ML = B.max_lines, tid = threadIdx.x;
    if (tid == 0) { sCnt = 0; sTake = 0; }
    __syncthreads();
    // the last key of the ranking that is returned: (Ls, Is).  Ls = the largest value with at least ML lengths >= it, bit by bit from the top
    // (63 rounds); Is = the largest value with fewer than `need` ids below it among the lengths equal to Ls (26 rounds)
    unsigned long long Ls = 0; unsigned Is = 0xFFFFFFFFu;
    if (K > ML) {
        for (int bit = 62; bit >= 0; --bit) {
            const unsigned long long c = Ls | (1ull << bit);
            if (rank_count(K, &sCnt, [&](int k) { return len[k] >= c; }) >= ML) Ls = c;
        }
        const int need = ML - rank_count(K, &sCnt, [&](int k) { return len[k] > Ls; });      // >= 1
        Is = 0;
        for (int bit = 25; bit >= 0; --bit) {
            const unsigned c = Is | (1u << bit);
            if (rank_count(K, &sCnt, [&](int k) { return len[k] == Ls && id[k] < c; }) < need) Is = c;
        }
    }
    for (int k = tid; k < K; k += kRankThreads)
        if (len[k] > Ls || (len[k] == Ls && id[k] <= Is)) {
            const int at = atomicAdd(&sTake, 1);          // exactly min(K, ML) <= 1024 are taken
            if (at < kRankThreads) { sLen[at] = len[k]; sId[at] = id[k]; }
        }
    __syncthreads();
    const int n = min(min(K, ML), kRankThreads);
    if (tid < n) {
        const unsigned long long ml = sLen[tid]; const unsigned mi = sId[tid];
        int rank = 0;
        for (int k = 0; k < n; ++k) rank += (sLen[k] > ml || (sLen[k] == ml && sId[k] < mi)) ? 1 : 0;
        const int p = (int)(mi & 1u), name = (int)(mi >> 1);
        const DetRec* R = B.rec + 2 * base + p * B.px + name;
        const double mx = __longlong_as_double(R->v[0]), my = __longlong_as_double(R->v[1]), ux = __longlong_as_double(R->v[2]),
                     uy = __longlong_as_double(R->v[3]);
        const double tmin = double_of((unsigned long long)R->v[5]), tmax = double_of((unsigned long long)R->v[6]);
        const double bx = (double)(name % I.W) + mx, by = (double)(name / I.W) + my;
        const size_t row = (size_t)blockIdx.x * ML + rank;
        B.seg[4 * row] = bx + tmin * ux; B.seg[4 * row + 1] = by + tmin * uy; B.seg[4 * row + 2] = bx + tmax * ux; B.seg[4 * row + 3] = by + tmax * uy;
        B.width2[row] = __longlong_as_double(R->v[4]);
        B.info[4 * row] = name; B.info[4 * row + 1] = p; B.info[4 * row + 2] = R->n; B.info[4 * row + 3] = (int)(R->s & ~kValid);
    }
    if (tid == 0) { res->n_returned = n; res->status = K > ML ? UVS_LT_DET_OVERFLOW : UVS_LT_DET_OK; }
}

// ---- host
struct DetLayout { size_t o_img, in_used, o_seg, o_w2, o_info, out_used; };

DetLayout det_layout(size_t n, size_t max_lines, const std::vector<size_t>& img_bytes, std::vector<size_t>* img_off) {
    DetLayout Y;
    UvsArena in;
    (void)in.take(n * sizeof(DetItem));
    Y.o_img = in.o;
    for (size_t b : img_bytes) { const size_t at = in.take(b); if (img_off) img_off->push_back(at); }
    Y.in_used = in.o;
    UvsArena out;
    (void)out.take(n * sizeof(uvs_lt_det_result));
    Y.o_seg = out.take(n * max_lines * 32); Y.o_w2 = out.take(n * max_lines * 8); Y.o_info = out.take(n * max_lines * 16);
    Y.out_used = out.o;
    return Y;
}

int det_check(uvs_lt_tracker* h, const std::string& fn, int n_items, const uvs_lt_det_item* items, const uvs_lt_det_params* params, bool slots) {
    if (n_items > h->max_streams) { h->err = fn + ": more items than the capacity given to uvs_lt_create"; return UVS_ERR_CAPACITY; }
    if (params->grad_threshold < 1 || params->grad_threshold > UVS_LT_DET_MAX_THRESHOLD || params->min_pixels < 2 || !std::isfinite(params->min_length) ||
        !(params->min_length > 0.0)) {
        h->err = fn + ": grad_threshold must be 1 .. UVS_LT_DET_MAX_THRESHOLD, min_pixels >= 2, min_length finite and > 0"; return UVS_ERR_INVALID_ARG;
    }
    std::vector<char> seen(h->max_streams, 0);
    for (int b = 0; b < n_items; ++b) {
        const uvs_lt_det_item& it = items[b];
        const std::string who = fn + ": item " + std::to_string(b);
        if (!it.image) { h->err = who + ": null pointer"; return UVS_ERR_INVALID_ARG; }
        if (slots) {
            if (it.stream < 0 || it.stream >= h->max_streams) { h->err = who + ": stream outside the handle's slots"; return UVS_ERR_INVALID_ARG; }
            if (seen[it.stream]) { h->err = who + ": stream given twice"; return UVS_ERR_INVALID_ARG; }
            seen[it.stream] = 1;
        }
        if (it.width < UVS_LT_MIN_SIZE || it.height < UVS_LT_MIN_SIZE) { h->err = who + ": width or height below UVS_LT_MIN_SIZE"; return UVS_ERR_INVALID_ARG; }
        if (it.width > h->max_width || it.height > h->max_height) { h->err = who + " exceeds the capacity given to uvs_lt_create"; return UVS_ERR_CAPACITY; }
    }
    return UVS_OK;
}

// what a call with mapped slots (uvs_lt_set_undistort) adds behind the packed input: the remap's items, uploaded with it, and the undistorted
// images the remap writes, which are what the detection and the tracking then read
struct UdPlan { size_t o_items = 0, upload = 0, used = 0; std::vector<size_t> out_off; };

UdPlan ud_plan(size_t in_used, size_t n, const std::vector<size_t>& out_bytes) {
    UdPlan P;
    UvsArena a;
    a.o = in_used;
    P.o_items = a.take(n * sizeof(uvslt::UdItem));
    P.upload = a.o;
    for (size_t b : out_bytes) P.out_off.push_back(a.take(b));
    P.used = a.o;
    return P;
}

// the work space, at the handle's capacity, by the first call; with_maps: the input buffers also hold what ud_plan adds
int det_ensure(uvs_lt_tracker* h, bool with_maps) {
    const size_t B = h->max_streams, px = (size_t)h->max_width * h->max_height;
    const DetLayout Y = det_layout(B, h->max_lines, std::vector<size_t>(B, px), nullptr);
    size_t host_in = Y.in_used, dev_in = Y.in_used;
    if (with_maps) { const UdPlan P = ud_plan(Y.in_used, B, std::vector<size_t>(B, px)); host_in = P.upload; dev_in = P.used; }
    int rc;
    if ((rc = h->h_det_in.ensure(host_in, h->err)) != UVS_OK || (rc = h->d_det_in.ensure(dev_in, h->err)) != UVS_OK ||
        (rc = h->h_det_out.ensure(Y.out_used, h->err)) != UVS_OK || (rc = h->d_det_out.ensure(Y.out_used, h->err)) != UVS_OK ||
        (rc = h->d_det_blur.ensure(B * px, h->err)) != UVS_OK || (rc = h->d_det_sec.ensure(2 * B * px, h->err)) != UVS_OK ||
        (rc = h->d_det_vote.ensure(B * px, h->err)) != UVS_OK || (rc = h->d_det_grad.ensure(4 * B * px, h->err)) != UVS_OK ||
        (rc = h->d_det_label.ensure(8 * B * px, h->err)) != UVS_OK || (rc = h->d_det_rec.ensure(2 * B * px * sizeof(DetRec), h->err)) != UVS_OK ||
        (rc = h->d_det_list_len.ensure(8 * B * px, h->err)) != UVS_OK || (rc = h->d_det_list_id.ensure(4 * B * px, h->err)) != UVS_OK)
        return rc;
    return UVS_OK;
}

// One call's device work through the download and the wait (the arguments are checked); the images stay in d_det_in at img_off.
// maps: null, or per item the slot's undistortion or null (uvs_lt_detect_track with at least one mapped slot).  A mapped item's image is the raw
// frame: it is uploaded with the others, the remap writes the undistorted image behind the upload, and that image is the item's from there on
// (its offset in img_off; its size is the map's output size).
int det_run(uvs_lt_tracker* h, int n_items, const uvs_lt_det_item* items, const uvs_lt_det_params* params, DetLayout* layout, std::vector<size_t>* img_off,
            const std::vector<const LtUndistort*>* maps = nullptr) {
    int rc = det_ensure(h, maps != nullptr);
    if (rc != UVS_OK) return rc;
    std::vector<size_t> img_bytes;
    for (int b = 0; b < n_items; ++b) img_bytes.push_back((size_t)items[b].width * items[b].height);
    const DetLayout Y = det_layout(n_items, h->max_lines, img_bytes, img_off);
    *layout = Y;
    UdPlan P;
    int n_ud = 0, max_out = 0;
    if (maps) {
        std::vector<size_t> out_bytes;
        for (int b = 0; b < n_items; ++b) if ((*maps)[b]) out_bytes.push_back((size_t)(*maps)[b]->Wo * (*maps)[b]->Ho);
        P = ud_plan(Y.in_used, out_bytes.size(), out_bytes);
    }
    DetItem* hi = reinterpret_cast<DetItem*>(h->h_det_in.get());
    int max_threads = 0;
    for (int b = 0; b < n_items; ++b) {
        DetItem d;
        d.W = items[b].width; d.H = items[b].height; d.img_off = (long long)(*img_off)[b];
        std::memcpy(h->h_det_in + (*img_off)[b], items[b].image, img_bytes[b]);
        if (maps && (*maps)[b]) {
            const LtUndistort& U = *(*maps)[b];
            uvslt::UdItem u;
            u.W = U.W; u.H = U.H; u.n_out = U.Wo * U.Ho; u.pad = 0; u.src_off = d.img_off; u.dst_off = (long long)P.out_off[n_ud]; u.map = U.map;
            reinterpret_cast<uvslt::UdItem*>(h->h_det_in + P.o_items)[n_ud++] = u;
            max_out = std::max(max_out, u.n_out);
            d.W = U.Wo; d.H = U.Ho; d.img_off = u.dst_off;
            (*img_off)[b] = (size_t)u.dst_off;
        }
        hi[b] = d;
        max_threads = std::max(max_threads, ((d.W + 63) & ~63) * d.H);
    }
    DetBufs B;
    B.px = (size_t)h->max_width * h->max_height;
    B.in = reinterpret_cast<const uint8_t*>(h->d_det_in.get()); B.blur = h->d_det_blur; B.grad = h->d_det_grad; B.sec = h->d_det_sec; B.vote = h->d_det_vote;
    B.label = h->d_det_label; B.rec = reinterpret_cast<DetRec*>(h->d_det_rec.get()); B.list_len = h->d_det_list_len; B.list_id = h->d_det_list_id;
    B.res = reinterpret_cast<uvs_lt_det_result*>(h->d_det_out.get());
    B.seg = reinterpret_cast<double*>(h->d_det_out + Y.o_seg); B.width2 = reinterpret_cast<double*>(h->d_det_out + Y.o_w2);
    B.info = reinterpret_cast<int32_t*>(h->d_det_out + Y.o_info); B.max_lines = h->max_lines;
    const DetItem* dI = reinterpret_cast<const DetItem*>(h->d_det_in.get());
    const dim3 grid((max_threads + kThreads - 1) / kThreads, n_items);
    hipStream_t st = h->st;
    UVS_HIP(h->err, hipSetDevice(h->device));
    UVS_HIP(h->err, hipEventRecord(h->ev0, st));
    UVS_HIP(h->err, hipMemcpyAsync(h->d_det_in, h->h_det_in, maps ? P.upload : Y.in_used, hipMemcpyHostToDevice, st));
    if (n_ud) {
        uint8_t* din = reinterpret_cast<uint8_t*>(h->d_det_in.get());
        if ((rc = uvslt::ud_launch(h, n_ud, reinterpret_cast<const uvslt::UdItem*>(h->d_det_in + P.o_items), din, din, max_out)) != UVS_OK) return rc;
    }
    UVS_HIP(h->err, hipMemsetAsync(h->d_det_out, 0, Y.out_used, st));      // the counters of the results, and the rows that are not returned
    k_lt_det_blur<<<grid, kThreads, 0, st>>>(dI, B);
    k_lt_det_sectors<<<grid, kThreads, 0, st>>>(dI, B, params->grad_threshold);
    k_lt_det_link<<<grid, kThreads, 0, st>>>(dI, B);
    k_lt_det_flatten<<<grid, kThreads, 0, st>>>(dI, B);
    k_lt_det_sizes<<<grid, kThreads, 0, st>>>(dI, B);
    k_lt_det_moments<<<grid, kThreads, 0, st>>>(dI, B, params->min_pixels);
    k_lt_det_fit<<<grid, kThreads, 0, st>>>(dI, B, params->min_pixels);
    k_lt_det_extent<<<grid, kThreads, 0, st>>>(dI, B);
    k_lt_det_keep<<<grid, kThreads, 0, st>>>(dI, B, params->min_length);
    k_lt_det_rank<<<n_items, kRankThreads, 0, st>>>(dI, B);
    UVS_HIP(h->err, hipGetLastError());
    UVS_HIP(h->err, hipMemcpyAsync(h->h_det_out, h->d_det_out, Y.out_used, hipMemcpyDeviceToHost, st));
    UVS_HIP(h->err, hipEventRecord(h->ev1, st));
    UVS_HIP(h->err, hipStreamSynchronize(st));
    return UVS_OK;
}

void det_copy_out(uvs_lt_tracker* h, const DetLayout& Y, int n_items, double* seg, double* width2, int32_t* info, uvs_lt_det_result* results) {
    const size_t rows = (size_t)n_items * h->max_lines;
    std::memcpy(results, h->h_det_out, n_items * sizeof(uvs_lt_det_result));
    std::memcpy(seg, h->h_det_out + Y.o_seg, rows * 32);
    std::memcpy(width2, h->h_det_out + Y.o_w2, rows * 8);
    std::memcpy(info, h->h_det_out + Y.o_info, rows * 16);
}

}  // namespace uvsld

using namespace uvsld;

extern "C" {

int uvs_lt_detect(uvs_lt_tracker* h, int n_items, const uvs_lt_det_item* items, const uvs_lt_det_params* params, double* seg, double* width2,
                  int32_t* info, uvs_lt_det_result* results) {
    if (!h) return UVS_ERR_INVALID_ARG;
    const std::string fn = "uvs_lt_detect";
    h->err.clear();
    if (n_items < 1 || !items || !params || !seg || !width2 || !info || !results) { h->err = fn + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG; }
    int rc = det_check(h, fn, n_items, items, params, false);
    if (rc != UVS_OK) return rc;
    DetLayout Y; std::vector<size_t> img_off;
    rc = det_run(h, n_items, items, params, &Y, &img_off);
    if (rc != UVS_OK) return rc;
    UVS_HIP(h->err, hipEventElapsedTime(&h->detect_ms, h->ev0, h->ev1));
    det_copy_out(h, Y, n_items, seg, width2, info, results);
    return UVS_OK;
}

int uvs_lt_detect_track(uvs_lt_tracker* h, int n_items, const uvs_lt_det_item* items, const uvs_lt_det_params* params, double* seg, double* width2,
                        int32_t* info, uvs_lt_det_result* det_results, uint8_t* desc, int32_t* line_status, int32_t* prev_index, int32_t* distance,
                        uvs_lt_result* results) {
    if (!h) return UVS_ERR_INVALID_ARG;
    const std::string fn = "uvs_lt_detect_track";
    h->err.clear();
    if (n_items < 1 || !items || !params || !seg || !width2 || !info || !det_results || !desc || !line_status || !prev_index || !distance || !results) {
        h->err = fn + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG;
    }
    int rc = det_check(h, fn, n_items, items, params, true);
    if (rc != UVS_OK) return rc;
    // the items of mapped slots (uvs_lt_set_undistort) bring the raw frame; without one, `maps` stays empty and nothing below differs
    std::vector<const LtUndistort*> maps;
    for (int b = 0; b < n_items; ++b) {
        const LtUndistort& U = h->ud[items[b].stream];
        if (!U.on) continue;
        if (items[b].width != U.W || items[b].height != U.H) {
            h->err = fn + ": item " + std::to_string(b) + ": width or height is not the source size of the slot's map"; return UVS_ERR_INVALID_ARG;
        }
        maps.resize(n_items, nullptr);
        maps[b] = &U;
    }
    DetLayout Y; std::vector<size_t> img_off;
    rc = det_run(h, n_items, items, params, &Y, &img_off, maps.empty() ? nullptr : &maps);
    if (rc != UVS_OK) return rc;
    float det_ms = 0.f;
    UVS_HIP(h->err, hipEventElapsedTime(&det_ms, h->ev0, h->ev1));
    // the line counts are read back here: the tracking kernels' grids are sized by them on the host, as in uvs_lt_track
    const uvs_lt_det_result* dr = reinterpret_cast<const uvs_lt_det_result*>(h->h_det_out.get());
    const double* hseg = reinterpret_cast<const double*>(h->h_det_out + Y.o_seg);
    std::vector<uvs_lt_item> lit(n_items);
    std::vector<int> slot_of(n_items);
    size_t tl = 0; int max_n = 0;
    for (int b = 0; b < n_items; ++b) {
        lit[b].image = items[b].image; lit[b].stream = items[b].stream; lit[b].width = items[b].width; lit[b].height = items[b].height;
        if (!maps.empty() && maps[b]) { lit[b].width = maps[b]->Wo; lit[b].height = maps[b]->Ho; }      // the image on the device is the undistorted one
        lit[b].n_lines = dr[b].n_returned; lit[b].segments = hseg + 4 * (size_t)b * h->max_lines;
        slot_of[b] = items[b].stream;
        tl += lit[b].n_lines; max_n = std::max(max_n, lit[b].n_lines);
    }
    uvslt::LtLayout T;
    rc = uvslt::lt_run(h, n_items, lit.data(), slot_of, true, tl, max_n, nullptr, &T, reinterpret_cast<const uint8_t*>(h->d_det_in.get()), img_off.data());
    if (rc != UVS_OK) return rc;
    float trk_ms = 0.f;
    UVS_HIP(h->err, hipEventElapsedTime(&trk_ms, h->ev0, h->ev1));
    h->detect_ms = det_ms + trk_ms;
    for (int b = 0; b < n_items; ++b) {          // the new lines become the slot's previous ones
        LtSlot& s = h->slots[items[b].stream];
        s.cur = 1 - s.cur; s.n_prev = lit[b].n_lines;
    }
    det_copy_out(h, Y, n_items, seg, width2, info, det_results);
    std::memcpy(results, h->h_out, n_items * sizeof(uvs_lt_result));
    if (tl) {
        std::memcpy(desc, h->h_out + T.o_desc, tl * uvslt::kBytes);
        std::memcpy(line_status, h->h_out + T.o_stat, tl * 4);
        std::memcpy(prev_index, h->h_out + T.o_prev, tl * 4);
        std::memcpy(distance, h->h_out + T.o_dist, tl * 4);
    }
    return UVS_OK;
}

double uvs_lt_last_detect_device_ms(const uvs_lt_tracker* h) { return h ? (double)h->detect_ms : 0.0; }

int uvs_lt_debug_detect(uvs_lt_tracker* h, const uint8_t* image, int width, int height, const uvs_lt_det_params* params, uint8_t* blur, uint32_t* grad,
                        uint8_t* sector_a, uint8_t* sector_b, int32_t* name_a, int32_t* name_b, uint8_t* vote) {
    if (!h) return UVS_ERR_INVALID_ARG;
    const std::string fn = "uvs_lt_debug_detect";
    h->err.clear();
    if (!image || !params || !blur || !grad || !sector_a || !sector_b || !name_a || !name_b || !vote) { h->err = fn + ": null pointer"; return UVS_ERR_INVALID_ARG; }
    uvs_lt_det_item it;
    it.image = image; it.stream = 0; it.width = width; it.height = height; it.reserved = 0;
    int rc = det_check(h, fn, 1, &it, params, false);
    if (rc != UVS_OK) return rc;
    DetLayout Y; std::vector<size_t> img_off;
    rc = det_run(h, 1, &it, params, &Y, &img_off);
    if (rc != UVS_OK) return rc;
    const size_t n = (size_t)width * height, px = (size_t)h->max_width * h->max_height;
    UVS_HIP(h->err, hipMemcpy(blur, h->d_det_blur, n, hipMemcpyDeviceToHost));
    UVS_HIP(h->err, hipMemcpy(grad, h->d_det_grad, 4 * n, hipMemcpyDeviceToHost));
    UVS_HIP(h->err, hipMemcpy(sector_a, h->d_det_sec, n, hipMemcpyDeviceToHost));
    UVS_HIP(h->err, hipMemcpy(sector_b, h->d_det_sec + px, n, hipMemcpyDeviceToHost));
    UVS_HIP(h->err, hipMemcpy(name_a, h->d_det_label, 4 * n, hipMemcpyDeviceToHost));
    UVS_HIP(h->err, hipMemcpy(name_b, h->d_det_label + px, 4 * n, hipMemcpyDeviceToHost));
    UVS_HIP(h->err, hipMemcpy(vote, h->d_det_vote, n, hipMemcpyDeviceToHost));
    return UVS_OK;
}

}  // extern "C"
