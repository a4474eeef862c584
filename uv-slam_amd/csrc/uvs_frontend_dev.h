// uvs_frontend_dev.h -- the device helpers the front-end units share, one statement of each: the counter-based generator of the RANSAC units
// (uvs_loop_verify, uvs_vanishing_points, uvs_feature_reject), reflect-101 of the image units (uvs_keyframe_features, uvs_feature_track,
// uvs_feature_detect), the packed Sobel of the line units (uvs_line_track, uvs_line_detect) and the ordered compaction by 64-pixel row
// segments (k_kf_select_*, k_ft_detect_*).  Integer arithmetic only, so the
// contraction flag of the including unit does not matter; everything is inlined into the kernels that call it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// the splitmix64 finalizer
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// draw a of hypothesis (or sample) h: z = mix64(seed + 0x9E3779B97F4A7C15 * (1 + (h << 20) + a)) mod 2^64; tests/lc_ref.py, tests/vp_ref.py and
// tests/fr_ref.py restate it
__device__ __forceinline__ unsigned long long uvs_draw(unsigned long long seed, int h, int a) {
    return mix64(seed + 0x9E3779B97F4A7C15ull * (1ull + ((unsigned long long)h << 20) + (unsigned long long)a));
}

// cv::BORDER_REFLECT_101; exact for -n < i < 2 n - 1 (every index an output needs: the keyframe unit has n >= 9 and a halo of 4, a level of the
// tracker is at least 24 wide and its kernels reach at most 11 beyond it, the detection reaches 2), clamped beyond so that the lanes of a tile
// that hangs over the image still read inside it whatever they are given
__device__ __forceinline__ int reflect101(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return min(max(i, 0), n - 1);
}

// the Sobel gx, gy of uvs_ft_detect's rule at (x, y) of the 8-bit image p[H][W] (stride W), every read through reflect-101: gx in the low, gy in
// the high 16 bits of one word (|g| <= 1020), so that a sample of a gradient image is ONE gather (k_lt_gradient, k_lt_det_sectors)
__device__ __forceinline__ uint32_t uvs_sobel_packed(const uint8_t* __restrict__ p, int W, int H, int x, int y) {
    const int xm = reflect101(x - 1, W), xp = reflect101(x + 1, W), ym = reflect101(y - 1, H), yp = reflect101(y + 1, H);
    const int a = p[ym * W + xm], b = p[ym * W + x], c = p[ym * W + xp], d = p[y * W + xm], f = p[y * W + xp], q = p[yp * W + xm],
              r = p[yp * W + x], s = p[yp * W + xp];
    const int gx = (c - a) + 2 * (f - d) + (s - q);
    const int gy = (q - a) + 2 * (r - b) + (s - c);
    return ((uint32_t)gx & 0xFFFFu) | ((uint32_t)gy << 16);
}

// ---- ordered compaction by 64-pixel row segments: a mark kernel writes every segment's ballot and its popcount, a workgroup per item scans
// the counts (uvs_segment_scan), an emit kernel scatters a set lane to segment base + uvs_rank_below, so the list is in row-major order by
// construction.  The kernels keep their mark predicates, their payloads and the emit kernels' two early returns (not set, beyond the capacity).

// exclusive scan of cnt[0 .. n_seg) into base[] by one workgroup of kThreads, two levels: a contiguous chunk per thread, then the kThreads
// chunk sums in sPart[kThreads] (LDS).  Returns the inclusive sum at the calling thread: the total in thread kThreads - 1.
template <int kThreads>
__device__ __forceinline__ int uvs_segment_scan(const int* cnt, int* base, int n_seg, int* sPart) {
    const int tid = threadIdx.x;
    const int chunk = (n_seg + kThreads - 1) / kThreads;
    const int b = min(tid * chunk, n_seg), e = min(b + chunk, n_seg);
    int sum = 0;
    for (int i = b; i < e; ++i) sum += cnt[i];
    sPart[tid] = sum;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {            // inclusive scan of the chunk sums
        const int v = tid >= off ? sPart[tid - off] : 0;
        __syncthreads();
        sPart[tid] += v;
        __syncthreads();
    }
    int run = sPart[tid] - sum;
    for (int i = b; i < e; ++i) { base[i] = run; run += cnt[i]; }
    return sPart[tid];
}

// the set bits of a ballot below the lane: a set lane's number among the set lanes of its wave, so the emit slot of a segment's lane relative
// to the segment's base, and the slot of a lane in the LDS compactions of k_ft_detect_score and k_ft_detect_select
__device__ __forceinline__ int uvs_rank_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }
