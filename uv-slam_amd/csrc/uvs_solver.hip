// uvs_solver.hip -- C ABI (include/uvs_solver.h) of the MI355X sliding-window solver: the handle's life, uploads, launches and downloads of the persistent kernel
// (k_solve; this unit holds its 256-thread instantiation, uvs_solve512.hip the 512-thread one), the batch and stream calls.  The handle itself is uvs_solver_handle.h; the host packing
// (uvs_window -> blob) is the host-only unit uvs_pack.h / uvs_pack.cpp, uvs_evaluate and the marginalization are uvs_marginalize.hip, the large-window calls uvs_large.hip.
//
// Build (see __graft_entry__.build(), which compiles every unit of csrc/ and links them into libuvs_solver.so):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -c uvs_solver.hip
//
// There is NO CPU path in this library: uvs_create() fails with UVS_ERR_NO_DEVICE when no HIP device
// is present and every compute entry point runs HIP kernels.  The CPU oracle under oracle/ is test
// infrastructure and is never linked or called from here.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>

#define UVS_UNIT solve256
#define UVS_EMIT_K_SOLVE 1      // (the 256-thread k_solve_dstep is its own translation unit: uvs_solve_dstep256.hip)
#include "uvs_solver_handle.h"

using namespace uvsdev;
using namespace uvspack;

// the 512-thread instantiation of the persistent kernel (uvs_solve512.hip) and the 256-thread debug-step one (uvs_solve_dstep256.hip)
extern "C" {
int uvs_k_solve512_init(const unsigned char* fa, const unsigned char* fb, int n);
int uvs_k_solve512_launch(int n_windows, hipStream_t stream, char* blobs, const long long* blob_off, double* ws_all, const long long* ws_off,
                           const void* kopts, size_t kopts_bytes, uvs_report* reports, const void* dbg, size_t dbg_bytes);
size_t uvs_k_solve512_arg_bytes(int which);
int uvs_k_solve512_dstep_launch(hipStream_t stream, char* blobs, const long long* blob_off, double* ws_all, const long long* ws_off,
                                const void* kopts, size_t kopts_bytes, uvs_report* reports, const void* ds, size_t ds_bytes);
int uvs_k_solve256d_init(const unsigned char* fa, const unsigned char* fb, int n);
int uvs_k_solve256d_launch(hipStream_t stream, char* blobs, const long long* blob_off, double* ws_all, const long long* ws_off,
                           const void* kopts, size_t kopts_bytes, uvs_report* reports, const void* ds, size_t ds_bytes);
int uvs_k_solve512_timeline(long long* out, size_t n);
}

extern "C" {

int uvs_abi_version(void) { return UVS_ABI_VERSION; }

void uvs_default_options(uvs_options* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->max_num_iterations = 10;          // euroc_config.yaml:56
    o->estimate_extrinsic = 0;           // :26
    o->estimate_td = 0;                  // :73
    o->function_tol_keeps_candidate = 0;
    o->focal_length = 461.6;             // :20
    o->point_sqrt_info = 461.6 / 1.6;    // estimator.cpp:17
    o->line_factor = 300.0; o->vp_factor = 10.0;   // :86-87
    o->loss_point = 1.0; o->loss_line = 0.1; o->loss_vp = 1.0;   // estimator.cpp:765-772
    o->gravity[0] = 0.0; o->gravity[1] = 0.0; o->gravity[2] = 9.81007;   // :64
    o->initial_trust_region_radius = 1e4; o->max_trust_region_radius = 1e16; o->min_trust_region_radius = 1e-32;
    o->min_relative_decrease = 1e-3; o->min_lm_diagonal = 1e-6; o->max_lm_diagonal = 1e32;
    o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8;
    o->max_consecutive_invalid_steps = 5; o->jacobi_scaling = 1;
    o->max_solver_time_in_seconds = 0.0;      // no wall-clock cap (the reference sets 0.1 s / 0.08 s, estimator.cpp:987-991: two orders of magnitude above a solve here)
}

const char* uvs_status_string(int st) {
    switch (st) {
        case UVS_OK: return "ok";
        case UVS_ERR_INVALID_ARG: return "invalid argument";
        case UVS_ERR_UNSUPPORTED: return "unsupported configuration";
        case UVS_ERR_NO_DEVICE: return "no HIP device (this library has no CPU path)";
        case UVS_ERR_HIP: return "HIP runtime error";
        case UVS_ERR_CAPACITY: return "capacity exceeded";
        case UVS_ERR_NUMERIC: return "numeric failure";
    }
    return "unknown";
}

const char* uvs_last_error(const uvs_solver* s) { return s ? s->err.c_str() : "null solver"; }

// host-only: the packing of `w` as uvs_batch_upload() would do it, nothing touches a device (CPU tests of the chunk / list layout, timing)
int uvs_debug_pack_layout(const uvs_options* o, const uvs_window* w, int32_t* info) {
    if (!o || !w || !info) return UVS_ERR_INVALID_ARG;
    std::vector<char> blob; DevWin h; std::string err;
    const char* grid_env = std::getenv("UVS_DEBUG_CHUNK_GRID");      // CPU tests of the large-window chunking (uvs_large_begin passes the device's CU count)
    const int rc = pack_window(w, *o, blob, h, err, grid_env ? std::atoi(grid_env) : 0, nullptr);
    if (rc != UVS_OK) return rc;
    const int32_t v[12] = {h.blob_bytes, h.ws_doubles, h.n_chunks, h.n_pt_obs, h.n_relo, h.pt_rec, h.pt_xslots, h.max_chunk_doubles, UVS_S_DOUBLES, h.n_parts, h.n_cimg, h.n_pblk};
    std::memcpy(info, v, sizeof(v));
    return UVS_OK;
}

int uvs_reduced_dim(const uvs_options* o) { return 15 * UVS_NUM_FRAMES + ((o && o->estimate_extrinsic) ? 6 : 0); }

int uvs_create(const uvs_options* opts, int device, int max_batch, int max_points, int max_point_obs, int max_lines,
               int max_line_obs, uvs_solver** out) {
    if (!opts || !out || max_batch < 1 || max_points < 0 || max_point_obs < 0 || max_lines < 0 || max_line_obs < 0) return UVS_ERR_INVALID_ARG;
    if (opts->max_num_iterations < 0) return UVS_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return UVS_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return UVS_ERR_NO_DEVICE;
    uvs_solver* s = new uvs_solver();
    s->opts = *opts; s->device = device; s->max_batch = max_batch;
    s->max_points = max_points; s->max_point_obs = max_point_obs; s->max_lines = max_lines; s->max_line_obs = max_line_obs;
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess) { uvs_destroy(s); return UVS_ERR_HIP; }
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) s->n_cus = cus; }
    // block table for the output-stationary gather
    unsigned char fa[UVS_NBLK], fb[UVS_NBLK];
    for (int i = 0, b = 0; i < UVS_NF; ++i) for (int j = 0; j <= i; ++j, ++b) { fa[b] = (unsigned char)i; fb[b] = (unsigned char)j; }
    // ... copied into every unit built from the kernel header, each of which opts its kernels into the LDS they ask for (uvs_solve_kernel.h: unit_init) -- a per-device function
    // attribute: every handle (the buffer sets of uvs_batch_stream too) sets it for its own device, the current one since hipSetDevice above
    if (uvs_k_solve512_arg_bytes(0) != sizeof(KOpts) || uvs_k_solve512_arg_bytes(1) != sizeof(DebugOut) || uvs_k_solve512_arg_bytes(2) != sizeof(DebugStep) ||
        unit_init(fa, fb, UVS_NBLK, {(const void*)k_solve}) != UVS_OK || uvs_k_solve512_init(fa, fb, UVS_NBLK) != UVS_OK || uvs_k_solve256d_init(fa, fb, UVS_NBLK) != UVS_OK ||
        marg_unit_init(fa, fb, UVS_NBLK) != UVS_OK || large_unit_init(fa, fb, UVS_NBLK) != UVS_OK) { uvs_destroy(s); return UVS_ERR_HIP; }
    { const char* e = std::getenv("UVS_KSOLVE_NT"); s->ksolve_nt = (e && std::atoi(e) == 256) ? 256 : 512; }
    { const char* e = std::getenv("UVS_DEBUG_LARGE_GRID"); s->large_grid = e ? std::max(0, std::atoi(e)) : 0; }
    { const char* e = std::getenv("UVS_LARGE_CHUNKS_NT"); s->large_chunks_nt = (e && std::atoi(e) == 256) ? 256 : 512; }
    { const char* e = std::getenv("UVS_LARGE_SOLVE_NT"); s->large_solve_nt = (e && std::atoi(e) == 256) ? 256 : 512; }      // A/B switch: 256 = the one-wave-per-SIMD instantiation of the persistent kernel
    *out = s;
    return UVS_OK;
}

}  // extern "C"

// gathers the per-window outputs into one contiguous buffer: tab[3 b] = {source offset in ws, doubles, destination offset}; the reports
// follow the states (rep_dst = offset of the report array in `out`, in doubles; sizeof(uvs_report) is a multiple of 8)
static_assert(sizeof(uvs_report) % 8 == 0, "uvs_report is copied as doubles");
__global__ void k_pack_outputs(const double* ws, const long long* tab, double* out, const uvs_report* reps, long long rep_dst) {
    const long long src = tab[3 * blockIdx.x], cnt = tab[3 * blockIdx.x + 1], dst = tab[3 * blockIdx.x + 2];
    for (long long t = threadIdx.x; t < cnt; t += blockDim.x) out[dst + t] = ws[src + t];
    constexpr int RD = (int)(sizeof(uvs_report) / 8);
    const double* r = (const double*)(reps + blockIdx.x);
    for (int t = threadIdx.x; t < RD; t += blockDim.x) out[rep_dst + (long long)blockIdx.x * RD + t] = r[t];
}

int upload_windows(uvs_solver* s, int n, const uvs_window* const* ws, bool wait, int chunk_grid, bool out_direct, bool all_blocks) {
    if (!s || n < 1 || !ws) return UVS_ERR_INVALID_ARG;
    if (n > s->max_batch) { s->err = "batch larger than max_batch"; return UVS_ERR_CAPACITY; }
    UVS_HIP(s->err, hipSetDevice(s->device));
    s->hdrs.resize(n); s->blob_off.resize(n); s->ws_off.resize(n);
    long long wtot = 0;
    for (int b = 0; b < n; ++b)
        if (ws[b] && (ws[b]->n_points > s->max_points || ws[b]->n_point_obs + std::max(ws[b]->n_relo_obs, 0) > s->max_point_obs || ws[b]->n_lines > s->max_lines || ws[b]->n_line_obs > s->max_line_obs)) {
            s->err = "window exceeds the capacity given to uvs_create (max_points / max_point_obs / max_lines / max_line_obs)"; s->n_loaded = 0; return UVS_ERR_CAPACITY;
        }
    // Packing (index bookkeeping of the gather lists: the analogue of Ceres' problem construction) is independent per window: a batch is
    // packed by several host threads into per-window buffers and concatenated -- 0.3 ms per window on one core was 83 ms for the 256-window
    // batch, 45 x the solve it feeds.  UVS_PACK_THREADS overrides the thread count (1 = the serial path, also taken for small batches).
    int nthreads = 1;
    static const bool sprof_ = std::getenv("UVS_STREAM_PROFILE") != nullptr;      // stage times of an upload on stderr (where the end-to-end rate of uvs_batch_stream goes)
    const auto tp0_ = std::chrono::steady_clock::now();
    auto tp1_ = tp0_, tp2_ = tp0_, tp3_ = tp0_;
    size_t packed_total = 0;      // > 0: the windows sit in s->slot_blobs (threaded path) and go straight into the pinned staging buffer below
    bool packed_direct = false;   // ... or are there already (packed in place)
    if (n >= 8) {
        nthreads = std::min(pack_threads(32u, 2u), n);      // (half the hardware threads at most: SMT siblings share a core)
    }
    bool values_only = false;      // structure-cache hit AND the device still holds this window's tables: only the value sections travel
    if (n == 1 && ws[0] && ws[0]->n_point_obs + ws[0]->n_line_obs >= kPackCacheMinObs && !std::getenv("UVS_NO_PACK_CACHE")) {
        if (!s->pack_cache) s->pack_cache = std::make_unique<PackCache>();
        const bool was_valid = s->pack_cache->valid, dev = s->pack_cache->device_holds_tables;
        s->blob_off[0] = 0;
        int rc = pack_window(ws[0], s->opts, s->host_blobs, s->hdrs[0], s->err, chunk_grid, s->pack_cache.get(), nullptr, all_blocks);
        if (rc != UVS_OK) { s->n_loaded = 0; return rc; }
        values_only = !out_direct && was_valid && dev && s->pack_cache->valid && s->pack_cache->device_holds_tables;      // (a miss resets both flags; the stream patches every staged header -- DevWin::out_host -- so the whole blob travels)
    } else if (nthreads == 1) {
        s->host_blobs.clear();
        if (s->pack_cache) { s->pack_cache->valid = false; s->pack_cache->device_holds_tables = false; }
        for (int b = 0; b < n; ++b) {
            s->blob_off[b] = (long long)s->host_blobs.size();
            int rc = pack_window(ws[b], s->opts, s->host_blobs, s->hdrs[b], s->err, chunk_grid, nullptr, nullptr, all_blocks);
            if (rc != UVS_OK) { s->n_loaded = 0; return rc; }
        }
    } else {
        if (s->pack_cache) { s->pack_cache->valid = false; s->pack_cache->device_holds_tables = false; }
        // per-slot buffers that live in the handle: a fresh 260 KB vector per window was a page fault per 4 KB of it, every batch (0.9 ms per window
        // on a cold buffer against 0.12 ms on a warm one)
        if ((int)s->slot_blobs.size() < n) s->slot_blobs.resize(n);
        std::vector<int> rcs(n, UVS_OK); std::vector<std::string> errs(n); std::vector<long long> placed(n, -1);
        // The windows go STRAIGHT into the pinned staging buffer when it is large enough (it is from the second batch of a size on: the first one takes the vectors and
        // sizes the buffer): every worker claims room with an atomic bump, so the blobs sit in completion order -- the kernel finds them through blob_off.  The buffer
        // may still feed the previous upload's copy: drain first.
        UVS_HIP(s->err, hipStreamSynchronize(s->stream));
        std::atomic<size_t> bump{0};
        const size_t direct_cap = s->h_up.cap() > (size_t)n * 40 + 64 ? s->h_up.cap() - (size_t)n * 40 - 64 : 0;
        const auto job = [&](int t) {
            for (int b = t; b < n; b += nthreads) {
                PackDst d{&bump, direct_cap ? s->h_up.get() : nullptr, direct_cap, -1};
                s->slot_blobs[b].clear();
                rcs[b] = pack_window(ws[b], s->opts, s->slot_blobs[b], s->hdrs[b], errs[b], chunk_grid, nullptr, &d, all_blocks);
                placed[b] = d.off;
            }
        };
        if (pack_pool(s).ensure(nthreads)) s->pool->run(nthreads, job);
        else { const int nt_ = nthreads; nthreads = 1; job(0); nthreads = nt_; }      // (no worker threads: this thread packs everything)
        bool all_placed = direct_cap > 0;
        for (int b = 0; b < n; ++b) {
            if (rcs[b] != UVS_OK) { s->err = errs[b]; s->n_loaded = 0; return rcs[b]; }      // the first failing window in batch order, as the serial path reports it
            if (placed[b] < 0) all_placed = false;
        }
        size_t total = 0;
        if (all_placed) { for (int b = 0; b < n; ++b) s->blob_off[b] = placed[b]; total = bump.load(); packed_direct = true; }
        else {
            // (a window that found no room has its blob in its vector; one that did is copied back out: this path runs when the batch outgrew the buffer)
            for (int b = 0; b < n; ++b) if (placed[b] >= 0) s->slot_blobs[b].assign(s->h_up + placed[b], s->h_up + placed[b] + s->hdrs[b].blob_bytes);
            for (int b = 0; b < n; ++b) { s->blob_off[b] = (long long)total; total += s->slot_blobs[b].size(); }
        }
        packed_total = total;
    }
    tp1_ = std::chrono::steady_clock::now();      // packing ends here; the offset tables and the drain of the stream follow
    for (int b = 0; b < n; ++b) { s->ws_off[b] = wtot; wtot += s->hdrs[b].ws_doubles; }
    s->out_tab.resize(3 * (size_t)n); s->out_total = 0;
    for (int b = 0; b < n; ++b) {
        const DevWin& h = s->hdrs[b];
        const long long cnt = UVS_XDIM + (long long)h.n_points + 4 * (long long)h.n_lines;
        s->out_tab[3 * b] = s->ws_off[b] + h.w_out; s->out_tab[3 * b + 1] = cnt; s->out_tab[3 * b + 2] = s->out_total;
        s->out_total += cnt;
    }
    int rc;
    const size_t raw_bytes = packed_total ? packed_total : s->host_blobs.size();
    const size_t blob_bytes = (raw_bytes + 7) & ~(size_t)7, up_bytes = blob_bytes + (size_t)n * 40;
    // the staging buffer may still feed the previous upload's copy (the single-window path does not wait for it): drain before reuse
    UVS_HIP(s->err, hipStreamSynchronize(s->stream));
    tp2_ = std::chrono::steady_clock::now();
    // every upload is staged in pinned memory together with its tables: ONE DMA copy that the host need not wait for (a copy from the pageable vector
    // is staged by the runtime anyway, synchronously and on one thread); a large blob (configs[3]: 13 MB) is moved there by several threads
    if ((rc = s->h_up.ensure(up_bytes + (packed_total && !packed_direct ? up_bytes / 8 + 4096 : 0), s->err, grow_pinned)) != UVS_OK) return rc;      // (slack: the next batch of this size packs in place)
    { char* before = s->d_blobs; if ((rc = s->d_blobs.ensure(up_bytes, s->err)) != UVS_OK) return rc; if (s->d_blobs != before) values_only = false; }
    // all doubles of a blob precede its int tables (pack_window: i = 2 d), so the value sections are ONE prefix
    const size_t value_bytes = values_only ? (size_t)4 * (size_t)s->hdrs[0].i_pt_lm : 0;
    if ((rc = s->d_outpack.ensure((size_t)s->out_total * 8 + (size_t)n * sizeof(uvs_report), s->err)) != UVS_OK) return rc;
    if ((rc = s->d_ws.ensure((size_t)wtot * 8, s->err)) != UVS_OK) return rc;
    if ((rc = s->d_reports.ensure((size_t)n * sizeof(uvs_report), s->err)) != UVS_OK) return rc;
    if (packed_direct) { /* the blobs are in the staging buffer already */ }
    else if (packed_total) {      // every packing thread moves its own windows (67 MB for 256 canonical windows: one core would need ~10 ms)
        const auto cp = [&](int t) { for (int b = t; b < n; b += nthreads) std::memcpy(s->h_up + s->blob_off[b], s->slot_blobs[b].data(), s->slot_blobs[b].size()); };
        if (s->pool && s->pool->ensure(nthreads)) s->pool->run(nthreads, cp); else for (int t = 0; t < nthreads; ++t) cp(t);
    } else if (s->host_blobs.size() > ((size_t)4 << 20)) {
        const size_t nb_ = values_only ? value_bytes : s->host_blobs.size(); const int ct = pack_inner_threads(1 << 30);
        pack_parallel((int)((nb_ + 65535) >> 16), ct, [&](int c0, int c1, int) { const size_t a0 = (size_t)c0 << 16, a1 = std::min(nb_, (size_t)c1 << 16); if (a1 > a0) std::memcpy(s->h_up + a0, s->host_blobs.data() + a0, a1 - a0); });
    } else std::memcpy(s->h_up, s->host_blobs.data(), s->host_blobs.size());
    tp3_ = std::chrono::steady_clock::now();
    if (out_direct) {
        if ((rc = s->h_out.ensure((size_t)s->out_total * 8 + (size_t)n * sizeof(uvs_report), s->err, grow_pinned)) != UVS_OK) return rc;
        void* dp = nullptr; UVS_HIP(s->err, hipHostGetDevicePointer(&dp, s->h_out, 0));
        for (int b = 0; b < n; ++b) ((DevWin*)(s->h_up + s->blob_off[b]))->out_host = (int64_t)(uintptr_t)((double*)dp + s->out_tab[3 * (size_t)b + 2]);
    }
    long long* tabs = (long long*)(s->h_up + blob_bytes);
    std::memcpy(tabs, s->blob_off.data(), (size_t)n * 8);
    std::memcpy(tabs + n, s->ws_off.data(), (size_t)n * 8);
    std::memcpy(tabs + 2 * (size_t)n, s->out_tab.data(), (size_t)n * 24);
    s->d_blob_off = (long long*)(s->d_blobs + blob_bytes); s->d_ws_off = s->d_blob_off + n; s->d_out_tab = s->d_blob_off + 2 * (size_t)n;
    if (values_only) {      // the tables of this window are on the device already (structure cache): the value prefix and the three small offset tables
        UVS_HIP(s->err, hipMemcpyAsync(s->d_blobs, s->h_up, value_bytes, hipMemcpyHostToDevice, s->stream));
        UVS_HIP(s->err, hipMemcpyAsync(s->d_blobs + blob_bytes, s->h_up + blob_bytes, (size_t)n * 40, hipMemcpyHostToDevice, s->stream));
    } else UVS_HIP(s->err, hipMemcpyAsync(s->d_blobs, s->h_up, up_bytes, hipMemcpyHostToDevice, s->stream));
    if (sprof_ && n > 1) {
        const auto tp4_ = std::chrono::steady_clock::now();
        auto ms_ = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "upload n=%d threads=%d bytes=%zu: pack %.3f ms, tables + drain of the stream %.3f, copy to pinned %.3f, enqueue %.3f\n", n, nthreads, up_bytes, ms_(tp0_, tp1_), ms_(tp1_, tp2_), ms_(tp2_, tp3_), ms_(tp3_, tp4_));
    }
    if (wait) UVS_HIP(s->err, hipStreamSynchronize(s->stream));
    if (s->pack_cache && s->pack_cache->valid && n == 1) s->pack_cache->device_holds_tables = true;
    s->n_loaded = n;
    return UVS_OK;
}

extern "C" {

int uvs_batch_upload(uvs_solver* s, int n, const uvs_window* const* ws) { return upload_windows(s, n, ws, true); }

// rep_direct: (uvs_batch_stream after upload_windows(out_direct)) the reports go into the pinned result buffer as well
static int launch_solve(uvs_solver* s, int debug, float* elapsed_ms, bool wait = true, bool rep_direct = false) {
    if (s->n_loaded < 1) { s->err = "no batch uploaded"; return UVS_ERR_INVALID_ARG; }
    UVS_HIP(s->err, hipSetDevice(s->device));
    KOpts ko = make_kopts(s->opts, debug);
    uvs_report* d_reports = s->d_reports;
    if (rep_direct) {
        void* dp = nullptr; UVS_HIP(s->err, hipHostGetDevicePointer(&dp, s->h_out, 0));
        d_reports = (uvs_report*)((double*)dp + s->out_total);
    }
    DebugOut dbg; std::memset(&dbg, 0, sizeof(dbg));
    if (debug) {
        if (const int rc = s->d_dbg.ensure(sizeof(double) * (UVS_RD * UVS_RD + 5 * UVS_RD + 40), s->err)) return rc;
        dbg.S = s->d_dbg; dbg.g = dbg.S + UVS_RD * UVS_RD; dbg.hd = dbg.g + UVS_RD; dbg.dd = dbg.hd + UVS_RD; dbg.step = dbg.dd + UVS_RD; dbg.scal = dbg.step + UVS_RD;
    }
    UVS_HIP(s->err, hipEventRecord(s->ev0, s->stream));
    if (s->ksolve_nt == 512) { if (uvs_k_solve512_launch(s->n_loaded, s->stream, s->d_blobs, s->d_blob_off, s->d_ws, s->d_ws_off, &ko, sizeof(ko), d_reports, &dbg, sizeof(dbg)) != UVS_OK) { s->err = "k_solve (512 threads): argument layout mismatch between the translation units"; return UVS_ERR_HIP; } }
    else hipLaunchKernelGGL(k_solve, dim3(s->n_loaded), dim3(NT), LDS_BYTES, s->stream, s->d_blobs, s->d_blob_off, s->d_ws, s->d_ws_off, ko, d_reports, dbg);
    UVS_HIP(s->err, hipGetLastError());
    UVS_HIP(s->err, hipEventRecord(s->ev1, s->stream));
    if (!wait) return UVS_OK;
    UVS_HIP(s->err, hipStreamSynchronize(s->stream));
    if (elapsed_ms) UVS_HIP(s->err, hipEventElapsedTime(elapsed_ms, s->ev0, s->ev1));
    return UVS_OK;
}

int uvs_batch_solve(uvs_solver* s, float* elapsed_ms) {
    if (!s) return UVS_ERR_INVALID_ARG;
    return launch_solve(s, 0, elapsed_ms);
}

// the two halves of a download: enqueue (gather kernel + ONE copy into pinned memory, nothing waits) and finish (wait, unpack)
// `direct`: the gather kernel writes into the pinned host buffer itself and no copy is enqueued (uvs_batch_stream with UVS_STREAM_D2H_COPY=2; its default lets k_solve write the results)
static int download_enqueue(uvs_solver* s, int n, bool direct = false) {
    // every window's final state (frames | inv_depth | line_orth, written by k_solve into its workspace) and its report are gathered on the
    // device and fetched with ONE copy into pinned memory (256 windows were 256 synchronous round trips once)
    const size_t nst = (size_t)(s->out_tab[3 * (size_t)(n - 1) + 2] + s->out_tab[3 * (size_t)(n - 1) + 1]);      // doubles of the first n states
    const size_t tot = nst * 8 + (size_t)n * sizeof(uvs_report);
    int rc;
    if ((rc = s->h_out.ensure(tot, s->err, grow_pinned)) != UVS_OK) return rc;
    double* out = s->d_outpack;
    if (direct) { void* dp = nullptr; UVS_HIP(s->err, hipHostGetDevicePointer(&dp, s->h_out, 0)); out = (double*)dp; }
    hipLaunchKernelGGL(k_pack_outputs, dim3(n), dim3(256), 0, s->stream, s->d_ws, s->d_out_tab, out, s->d_reports, (long long)nst);
    UVS_HIP(s->err, hipGetLastError());
    if (!direct) UVS_HIP(s->err, hipMemcpyAsync(s->h_out, s->d_outpack, tot, hipMemcpyDeviceToHost, s->stream));
    return UVS_OK;
}
static int download_finish(uvs_solver* s, int n, uvs_state* states, uvs_report* reps) {
    UVS_HIP(s->err, hipStreamSynchronize(s->stream));
    const size_t nst = (size_t)(s->out_tab[3 * (size_t)(n - 1) + 2] + s->out_tab[3 * (size_t)(n - 1) + 1]);
    int worst = UVS_OK;
    const uvs_report* hr = (const uvs_report*)(s->h_out + nst * 8);
    for (int b = 0; b < n; ++b) if (hr[b].status != UVS_OK) worst = hr[b].status;
    if (reps) std::memcpy(reps, hr, sizeof(uvs_report) * (size_t)n);
    for (int b = 0; states && b < n; ++b) {
        const DevWin& h = s->hdrs[b];
        const double* buf = (const double*)s->h_out.get() + s->out_tab[3 * (size_t)b + 2];
        uvs_state& st = states[b];
        std::memcpy(st.pose, buf, sizeof(double) * 77);
        std::memcpy(st.speedbias, buf + 77, sizeof(double) * 99);
        std::memcpy(st.ex_pose, buf + 176, sizeof(double) * 7);
        st.td = buf[183];
        std::memcpy(st.relo_pose, buf + 184, sizeof(double) * 7);
        if (st.inv_depth) std::memcpy(st.inv_depth, buf + UVS_XDIM, sizeof(double) * h.n_points);
        if (st.line_orth) std::memcpy(st.line_orth, buf + UVS_XDIM + h.n_points, sizeof(double) * 4 * h.n_lines);
    }
    return worst;
}

int uvs_batch_download(uvs_solver* s, int n, uvs_state* states, uvs_report* reps) {
    if (!s || n < 1 || n > s->n_loaded) return UVS_ERR_INVALID_ARG;
    UVS_HIP(s->err, hipSetDevice(s->device));
    const int rc = download_enqueue(s, n);      // (written by the gather kernel instead -- as the stream does -- the call takes as long: 1.370 ms either way for one window, 0.17 ms for 256 states)
    if (rc != UVS_OK) return rc;
    return download_finish(s, n, states, reps);
}

// A STREAM of batches, end to end: packing (host threads), upload, solve and download of consecutive batches overlap.  Three buffer sets -- this handle and two
// twins created on first use with the same options and capacities, each with its own stream, pinned staging and device buffers -- take turns: while the GPU runs
// k_solve -> gather of batch k on one set, the copy engine moves batch k + 1 into the second and the host packs batch k + 2 into the third; a set is drained (wait +
// unpack) right before it is reused.  Results equal uvs_batch_upload / solve / download of each batch (same packing, same kernel).
// What it took to make copy and kernel overlap (round 5; tools/micro_overlap.hip, tools/stream_trace.py, profiles/r05_stream_timeline*.txt, r05_stream_ab.txt):
//   * With TWO sets and the results fetched by a device-to-host copy enqueued behind k_solve, the upload of batch k + 1 -- enqueued on the other stream while k_solve of batch k
//     ran -- did not start until that download had been done, i.e. after the kernel: copy and kernel strictly alternated (95 - 105 k solves/s).  The device itself overlaps
//     them completely (micro_overlap).  Nothing is enqueued behind k_solve any more: k_solve writes every window's final state and report into the pinned result buffer
//     itself (DevWin::out_host, patched into the staged headers by upload_windows; the report pointer of the launch) -- UVS_STREAM_D2H_COPY=2: a gather kernel does, =1: gather
//     kernel + copy, the old form.
//   * three sets, and the kernels of consecutive batches chained by events, see below.
// With these the stream runs at 155 - 170 k solves/s: 1.50 - 1.65 ms per batch beside a kernel of 1.45 ms.
// (An in-kernel prefetch of the next batch -- k_solve's idle wave reading the pinned buffer -- was built before the first point was understood and is slower than the copy
// engine: tools/experiments/r05_stream_prefetch.patch.)
int uvs_batch_stream(uvs_solver* s, int n_batches, int per_batch, const uvs_window* const* ws, uvs_state* states, uvs_report* reps, double* wall_ms) {
    if (!s || n_batches < 1 || per_batch < 1 || !ws) return UVS_ERR_INVALID_ARG;
    if (per_batch > s->max_batch) { s->err = "batch larger than max_batch"; return UVS_ERR_CAPACITY; }
    // THREE buffer sets by default (UVS_STREAM_SETS=2: two): with two, the host can pack batch k only after batch k - 2 has been solved, and pack + copy (1.0 + 0.85 ms) then sit on
    // the critical path of every second kernel (1.72 ms per batch measured); with three the GPU always has a copied batch waiting
    // (the three knobs are read per CALL, not once per process: tools/stream_ab.py alternates the configurations inside one process, on the same windows)
    // UVS_STREAM_SETS=4: a fourth set with at most two kernels in flight (below) -- a batch of slack for a host whose packing threads get descheduled.  Measured against the three-set default
    // in four alternating A/Bs on busy and quiet hosts (profiles/r06_stream_ab_four_sets.txt): medians 172.5 / 173.6 / 150.8 k against 173.5 / 175.8 / 174.8 k, tighter quartiles in one of
    // them, wider in another -- the host's noise decides, not the set count; the default stays three.
    const int NS = [] { const char* e = std::getenv("UVS_STREAM_SETS"); const int v = e ? std::atoi(e) : 3; return v == 2 || v == 4 ? v : 3; }();
    for (auto* t : {&s->twin, &s->twin2, &s->twin3}) {
        if ((t == &s->twin2 && NS < 3) || (t == &s->twin3 && NS < 4)) break;
        if (!*t) {
            uvs_solver* ts = nullptr; const int rc = uvs_create(&s->opts, s->device, s->max_batch, s->max_points, s->max_point_obs, s->max_lines, s->max_line_obs, &ts);
            if (rc != UVS_OK) { s->err = "uvs_batch_stream: could not create a buffer set"; return rc; }
            t->reset(ts);
        }
        if (!(*t)->pool) { (void)pack_pool(s); (*t)->pool = s->pool; }      // one pool of packing threads for all sets (they pack one after the other)
    }
    const auto t0 = std::chrono::steady_clock::now();
    uvs_solver* set[4] = {s, s->twin.get(), s->twin2.get(), s->twin3.get()};
    // UVS_STREAM_CHAIN=1: the kernels of consecutive batches chained by events (round 5's default).  Round 6 measured both forms alternately in one process, ten runs of 32 batches each
    // (tools/stream_ab.py, profiles/r06_stream_ab.txt): un-chained 175.4 k solves/s median (quartiles 171.3 - 175.9 k), chained 167.5 k (167.3 - 167.8 k) -- the chain is steadier and
    // 4.5 % slower (a batch's kernel then never starts under the tail of the previous one, whose last workgroups leave compute units idle), so the default is un-chained.
    const bool chain_ = [] { const char* e = std::getenv("UVS_STREAM_CHAIN"); return e && e[0] == '1'; }();
    const int d2h_ = [] { const char* e = std::getenv("UVS_STREAM_D2H_COPY"); return e ? std::atoi(e) : 0; }();      // 0: k_solve writes the results into the pinned buffer; 1: gather kernel + device-to-host copy; 2: the gather kernel writes them
    for (int j = 0; j < NS; ++j) if (!set[j]->ev_done) UVS_HIP(s->err, hipEventCreateWithFlags(&set[j]->ev_done, hipEventDisableTiming));
    int pending[4] = {-1, -1, -1, -1};      // batch index in flight on each set
    // the resident blobs of this call carry addresses into its pinned result buffers (DevWin::out_host): whatever way the call ends, a later uvs_batch_solve needs its own upload
    struct Invalidate { uvs_solver** set; int n; bool on; ~Invalidate() { if (on) for (int j = 0; j < n; ++j) set[j]->n_loaded = 0; } } invalidate_{set, NS, d2h_ == 0};
    int worst = UVS_OK;
    const auto drain = [&](int q) -> int {
        if (pending[q] < 0) return UVS_OK;
        const size_t off = (size_t)pending[q] * per_batch;
        const int rc = download_finish(set[q], per_batch, states ? states + off : nullptr, reps ? reps + off : nullptr);
        pending[q] = -1;
        if (rc != UVS_OK && rc != UVS_ERR_NUMERIC) { if (set[q] != s) s->err = set[q]->err; return rc; }
        if (rc != UVS_OK) worst = rc;
        return UVS_OK;
    };
    static const bool sprof_ = std::getenv("UVS_STREAM_PROFILE") != nullptr;
    for (int k = 0; k < n_batches; ++k) {
        const int q = k % NS;
        const auto td0_ = std::chrono::steady_clock::now();
        int rc = drain(q);
        if (sprof_) fprintf(stderr, "stream batch %d: drain (wait + unpack of batch %d) %.3f ms\n", k, k - NS, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - td0_).count());
        if (rc == UVS_OK) rc = upload_windows(set[q], per_batch, ws + (size_t)k * per_batch, false, 0, d2h_ == 0);
        // (UVS_STREAM_CHAIN=1) the kernels run one after the other (an event chain through the sets): two k_solve launches on two streams otherwise share the compute units workgroup by
        // workgroup, both finish late and together, and the host -- which packs batch k + 1 into the set of the batch that finishes first -- stalls and then has two batches to pack in a row
        if (rc == UVS_OK && chain_ && k > 0 && hipStreamWaitEvent(set[q]->stream, set[(k - 1) % NS]->ev_done, 0) != hipSuccess) { s->err = "hipStreamWaitEvent failed"; rc = UVS_ERR_HIP; }
        // four sets, un-chained: at most TWO kernels in flight (batch k waits for batch k - 2), so that the fourth set is slack for the host and not a third kernel sharing the compute units
        const bool chain2_ = !chain_ && NS == 4;
        if (rc == UVS_OK && chain2_ && k > 1 && hipStreamWaitEvent(set[q]->stream, set[(k - 2) % NS]->ev_done, 0) != hipSuccess) { s->err = "hipStreamWaitEvent failed"; rc = UVS_ERR_HIP; }
        if (rc == UVS_OK) rc = launch_solve(set[q], 0, nullptr, false, d2h_ == 0);
        if (rc == UVS_OK && (chain_ || chain2_) && hipEventRecord(set[q]->ev_done, set[q]->stream) != hipSuccess) { s->err = "hipEventRecord failed"; rc = UVS_ERR_HIP; }
        if (rc == UVS_OK && d2h_ != 0) rc = download_enqueue(set[q], per_batch, d2h_ == 2);
        if (rc != UVS_OK) {
            // batch k failed before it was enqueued: the batch still in flight on the OTHER buffer set (k - 1) is delivered like the ones before it, so that on
            // return every batch < k holds results and nothing from k on does; the first error code is the one returned
            if (set[q] != s) s->err = set[q]->err;
            const std::string first_err = s->err;
            for (int j = 1; j < NS; ++j) (void)drain((q + j) % NS);      // (oldest first)
            for (int j = 0; j < NS; ++j) (void)hipStreamSynchronize(set[j]->stream);
            s->err = first_err;
            return rc;
        }
        pending[q] = k;
    }
    for (int j = 0; j < NS; ++j) { const int rc = drain((n_batches + j) % NS); if (rc != UVS_OK) return rc; }      // (oldest first)
    if (wall_ms) *wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return worst;
}

int uvs_solve_window(uvs_solver* s, const uvs_window* w, uvs_state* out, uvs_report* rep) {
    if (!s || !w || !out || !rep) return UVS_ERR_INVALID_ARG;
    const uvs_window* arr[1] = {w};
    // one stream, one wait: pinned upload -> k_solve -> k_pack_outputs -> pinned download (uvs_batch_download synchronizes)
    int rc = upload_windows(s, 1, arr, false);
    if (rc != UVS_OK) return rc;
    rc = launch_solve(s, 0, nullptr, false);
    if (rc != UVS_OK) return rc;
    return uvs_batch_download(s, 1, out, rep);
}

// Diagnostic entry (parity tests): reduced system of the FIRST linearization of window 0 of the uploaded batch.
// S_lower[176*176] row-major (damped, landmark-Schur-reduced, padded index 16*frame+dof), g/hd/dd/step[176], scal[UVS_DEBUG_SCAL_LEN].
int uvs_debug_first_iteration(uvs_solver* s, const uvs_window* w, double* S_lower, double* g, double* hd, double* dd, double* step, double* scal) {
    if (!s || !w) return UVS_ERR_INVALID_ARG;
    const uvs_window* arr[1] = {w};
    int rc = uvs_batch_upload(s, 1, arr);
    if (rc != UVS_OK) return rc;
    const char* tl_path = std::getenv("UVS_DEBUG_LIN_TIMELINE");      // debug: (stamp, clock) log of every wave's steps through the linearizations of this solve, written to this file
    rc = launch_solve(s, tl_path ? 5 : std::getenv("UVS_DEBUG_GATHER_TIMERS") ? 2 : std::getenv("UVS_DEBUG_ASM_TIMERS") ? 3 : std::getenv("UVS_DEBUG_CHOL_TIMELINE") ? 4 : 1, nullptr);      // 2 / 3: the four per-wave timer slots carry the gather / the assembly's sub-steps instead of the Cholesky column phase
    if (rc != UVS_OK) return rc;
    if (tl_path) {
        std::vector<long long> tl(8 * TL_PER_WAVE * 2);
        if ((s->ksolve_nt == 512 ? uvs_k_solve512_timeline(tl.data(), tl.size()) == UVS_OK : hipMemcpyFromSymbol(tl.data(), HIP_SYMBOL(g_lin_tl), tl.size() * 8) == hipSuccess)) { if (FILE* f = std::fopen(tl_path, "wb")) { std::fwrite(tl.data(), 8, tl.size(), f); std::fclose(f); } }
    }
    const size_t nS = (size_t)UVS_RD * UVS_RD;
    if (S_lower) UVS_HIP(s->err, hipMemcpy(S_lower, s->d_dbg, nS * 8, hipMemcpyDeviceToHost));
    if (g) UVS_HIP(s->err, hipMemcpy(g, s->d_dbg + nS, UVS_RD * 8, hipMemcpyDeviceToHost));
    if (hd) UVS_HIP(s->err, hipMemcpy(hd, s->d_dbg + nS + UVS_RD, UVS_RD * 8, hipMemcpyDeviceToHost));
    if (dd) UVS_HIP(s->err, hipMemcpy(dd, s->d_dbg + nS + 2 * UVS_RD, UVS_RD * 8, hipMemcpyDeviceToHost));
    if (step) UVS_HIP(s->err, hipMemcpy(step, s->d_dbg + nS + 3 * UVS_RD, UVS_RD * 8, hipMemcpyDeviceToHost));
    if (scal) UVS_HIP(s->err, hipMemcpy(scal, s->d_dbg + nS + 4 * UVS_RD, UVS_DEBUG_SCAL_LEN * 8, hipMemcpyDeviceToHost));
    return UVS_OK;
}

// Diagnostic entry (step tests): the damped step of the first linearization of `w` at radii[0], then at radii[1], ... each the way `form` handles a
// rejected step (form 0, k_solve: re-damping of the stored linearization; form 1, k_large_*: re-linearization at the same state).  step[k * n_step ...] = unscaled tangent step in the layout of include/uvs_solver.h, scal[k * UVS_DEBUG_SCAL_LEN ...] its scalars.
int uvs_debug_step(uvs_solver* s, const uvs_window* w, int form, int n_radii, const double* radii, int n_step, double* step, double* scal) {
    if (!s || !w || !radii || !step || !scal || n_radii < 1 || (form != 0 && form != 1)) { if (s) s->err = "uvs_debug_step: bad argument"; return UVS_ERR_INVALID_ARG; }
    for (int k = 0; k < n_radii; ++k) if (!std::isfinite(radii[k]) || !(radii[k] > 0.0)) { s->err = "uvs_debug_step: a radius that is not finite or <= 0"; return UVS_ERR_INVALID_ARG; }
    if (w->n_points < 0 || w->n_lines < 0) { s->err = "uvs_debug_step: negative landmark count"; return UVS_ERR_INVALID_ARG; }
    const uvs_options& o = s->opts;
    const int ex = o.estimate_extrinsic ? 1 : 0, td = o.estimate_td ? 1 : 0, relo = w->n_relo_obs > 0 ? 1 : 0;
    const long long n_fr = 165 + 6 * ex + td + 6 * relo;
    if ((long long)n_step != n_fr + w->n_points + 4LL * w->n_lines) { s->err = "uvs_debug_step: step length does not match the layout"; return UVS_ERR_INVALID_ARG; }
    if (form == 1) return debug_step_large(s, w, n_radii, radii, n_step, step, scal);
    const long long stride = UVS_DSTEP_FR + (long long)w->n_points + 4LL * w->n_lines;
    std::vector<double> raw((size_t)(stride * n_radii)), rsc((size_t)UVS_DEBUG_SCAL_LEN * n_radii, 0.0);
    int rc = UVS_OK;
    {
        const uvs_window* arr[1] = {w};
        if ((rc = uvs_batch_upload(s, 1, arr)) != UVS_OK) return rc;
        UVS_HIP(s->err, hipSetDevice(s->device));
        const size_t need = sizeof(double) * ((size_t)n_radii + (size_t)(stride * n_radii) + (size_t)UVS_DEBUG_SCAL_LEN * n_radii);
        if ((rc = s->d_dbg.ensure(need, s->err)) != UVS_OK) return rc;
        double* d_radii = s->d_dbg; double* d_steps = d_radii + n_radii; double* d_scal = d_steps + stride * n_radii;
        UVS_HIP(s->err, hipMemcpy(d_radii, radii, sizeof(double) * n_radii, hipMemcpyHostToDevice));
        UVS_HIP(s->err, hipMemset(d_steps, 0, sizeof(double) * (size_t)(stride * n_radii + (long long)UVS_DEBUG_SCAL_LEN * n_radii)));
        KOpts ko = make_kopts(o, 0);
        ko.r0 = radii[0]; ko.max_it = n_radii; ko.gtol = -1.0; ko.rmin = 0.0; ko.max_ticks = 0; ko.max_invalid = n_radii + 1;      // nothing ends the loop before the last radius
        DebugStep ds; ds.radii = d_radii; ds.n = n_radii; ds.stride = stride; ds.steps = d_steps; ds.scal = d_scal;
        if (s->ksolve_nt == 512) { if (uvs_k_solve512_dstep_launch(s->stream, s->d_blobs, s->d_blob_off, s->d_ws, s->d_ws_off, &ko, sizeof(ko), s->d_reports, &ds, sizeof(ds)) != UVS_OK) { s->err = "k_solve_dstep (512 threads): argument layout mismatch"; return UVS_ERR_HIP; } }
        else if (uvs_k_solve256d_launch(s->stream, s->d_blobs, s->d_blob_off, s->d_ws, s->d_ws_off, &ko, sizeof(ko), s->d_reports, &ds, sizeof(ds)) != UVS_OK) { s->err = "k_solve_dstep (256 threads): argument layout mismatch"; return UVS_ERR_HIP; }
        UVS_HIP(s->err, hipGetLastError());
        UVS_HIP(s->err, hipStreamSynchronize(s->stream));
        UVS_HIP(s->err, hipMemcpy(raw.data(), d_steps, sizeof(double) * raw.size(), hipMemcpyDeviceToHost));
        UVS_HIP(s->err, hipMemcpy(rsc.data(), d_scal, sizeof(double) * rsc.size(), hipMemcpyDeviceToHost));
    }
    // padded device layout -> the ABI's: frames (16 f + dof, dof < 15), extrinsic, td, relo_Pose, landmarks
    for (int k = 0; k < n_radii; ++k) {
        const double* r = raw.data() + (size_t)k * stride; double* d = step + (size_t)k * n_step;
        long long j = 0;
        for (int f = 0; f < UVS_NF; ++f) for (int a = 0; a < 15; ++a) d[j++] = r[16 * f + a];
        if (ex) for (int a = 0; a < 6; ++a) d[j++] = r[UVS_EX_INDEX(a)];
        if (td) d[j++] = r[UVS_TD_INDEX];
        if (relo) for (int a = 0; a < 6; ++a) d[j++] = r[16 * UVS_RELO_FRAME + a];
        std::memcpy(d + j, r + UVS_DSTEP_FR, sizeof(double) * (size_t)(stride - UVS_DSTEP_FR));
        std::memcpy(scal + (size_t)k * UVS_DEBUG_SCAL_LEN, rsc.data() + (size_t)k * UVS_DEBUG_SCAL_LEN, sizeof(double) * UVS_DEBUG_SCAL_LEN);
    }
    return UVS_OK;
}

}  // extern "C"

// Only the steps whose order matters; every buffer frees itself (~uvs_solver).
extern "C" void uvs_destroy(uvs_solver* s) {
    if (!s) return;
    marg_worker_release(s);
    s->twin.reset(); s->twin2.reset(); s->twin3.reset();
    uvs_large_comm_destroy(s);
    (void)hipSetDevice(s->device);      // teardown: nothing useful to do with an error
    delete s;
}
