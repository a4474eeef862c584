// uvs_pack.h -- host packing: uvs_window -> the blob the back-end kernels read (uvs_layout.h) and the layout of its workspace.
//
// Host-only (uvs_pack.cpp): the unit includes the C ABI header, uvs_layout.h and the standard library, nothing of HIP, and compiles with a plain
// g++ -std=c++17 as well as with hipcc's clang -- tools/pack_dump.cpp links it alone (tests/test_pack_blob.py, sanitizer runs).  Everything that talks
// to a device (upload_windows in uvs_solver.hip; the worker pool and the handle, uvs_solver_handle.h) stays outside.  The gather-group constants come from uvs_layout.h, so a variant
// library (tools/ab/build_variant.sh -DUVS_GLANES=...) rebuilds this unit with its kernels; the names are hidden so that two libraries in one
// process each keep their own packing.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "../../include/uvs_solver.h"
#include "uvs_layout.h"

namespace uvspack __attribute__((visibility("hidden"))) {

// UVS_OK, or the status and the text of the first rule `w` breaks (grouping and frame order of the observations, IMU frames, the prior's block table)
int validate_window(const uvs_window* w, std::string& err);

// where pack_window may put a blob instead of the caller's vector: a bump allocator over the pinned staging buffer of the handle (batch packing: the windows of a batch go
// straight to where the one host -> device copy starts; off = -1 afterwards: no room, the blob is in the vector)
struct PackDst { std::atomic<size_t>* bump; char* base; size_t cap; long long off = -1; };

// host threads of a packing job: UVS_PACK_THREADS when set, else the hardware threads / `share` but at most `most`; never below 1
int pack_threads(unsigned most, unsigned share);
// [0, n) split into `nt` contiguous ranges, one host thread each (nt <= 1: the caller's thread).  Used INSIDE the packing of one large window
// (configs[3]: 510 chunks, 135 000 observations); batches of small windows are threaded across windows instead (upload_windows).
template <class F> static void pack_parallel(int n, int nt, F&& fn) {
    if (nt <= 1 || n < 2) { fn(0, n, 0); return; }
    nt = std::min(nt, n);
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back([&, t] { fn((int)((long long)n * t / nt), (int)((long long)n * (t + 1) / nt), t); });
    fn(0, (int)((long long)n / nt), 0);
    for (auto& th : pool) th.join();
}
constexpr int kPackCacheMinObs = 20000;      // windows at least this large use the structure cache (and the inner packing threads)
int pack_inner_threads(int n_obs);

// The STRUCTURE of the last large window packed through a handle (index arrays, IMU links, prior block table, options): when the next window has the same
// structure -- the same landmarks observed from the same frames, only states and measurements moved on: repeated solves of one map, a benchmark loop --
// chunking, work split and gather lists (3/4 of the packing time) are reused and only the value sections of the blob are rewritten.  Compared exactly
// (memcmp of the arrays), no hashing.  Small windows do not use it: their structure changes with every frame of a live sequence.
struct PackCache {
    bool valid = false, device_holds_tables = false;
    int chunk_grid = 0, td_on = 0, ex_on = 0; bool all_blocks = false;
    int n_points = 0, n_pt_obs = 0, n_lines = 0, n_ln_obs = 0, n_imu = 0;
    std::vector<int32_t> pt_lm, pt_fi, pt_fj, ln_lm, ln_fj, ln_has_vp;
    int imu_fs[UVS_WINDOW_SIZE][2];
    bool have_prior = false; int prior_n = 0, prior_nb = 0; int prior_tab[5][UVS_MAX_PRIOR_BLOCKS];
    DevWin hdr;
    bool matches(const uvs_window* w, const uvs_options& o, int grid, bool all) const;
    void store(const uvs_window* w, const uvs_options& o, int grid, bool all, const DevWin& h);
};

// the VALUE sections of a blob (everything that is not index bookkeeping): header, frame states, landmark parameters, measurements, IMU blocks, prior
void fill_values(char* B, const DevWin& h, const uvs_window* w, bool td_on, int threads);

// appends the blob of `w` to `out` (8-byte aligned) -- or places it through `dst` -- and returns its header
// chunk_grid > 0 (large-window path): the landmark chunks are made SMALLER than the LDS staging area allows so that their number is a
// multiple of chunk_grid (the persistent workgroups of k_large_chunks / k_large_backsub then all carry the same number of chunks), or
// -- a shard with few landmarks -- so that every compute unit gets one
int pack_window(const uvs_window* w_in, const uvs_options& opts, std::vector<char>& out, DevWin& hdr, std::string& err, int chunk_grid = 0, PackCache* cache = nullptr, PackDst* dst = nullptr, bool all_blocks = false);

}  // namespace uvspack
