// uvs_solver_handle.h -- the handle of the sliding-window solver (struct uvs_solver) and what the three units behind its calls share: uvs_solver.hip (the handle's life, uploads,
// the persistent kernel), uvs_marginalize.hip (uvs_evaluate, uvs_marginalize*) and uvs_large.hip (uvs_large_*).  Host only: no device code is defined here.
#pragma once
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <functional>
#include <memory>
#include <mutex>
#include <pthread.h>
#include <sched.h>
#include <string>
#include <thread>
#include <vector>

#include "../../include/uvs_solver.h"
#include "uvs_hip_buf.h"
#include "uvs_layout.h"
#include "uvs_pack.h"
#include "uvs_solve_kernel.h"      // KOpts

// (nothing below is part of the ABI: the names are hidden, so that two libraries in one process -- an A/B variant beside the product -- each keep their own)
#pragma GCC visibility push(hidden)

// Worker threads of a handle for batch packing: created once, woken per batch (sixteen std::thread creations and joins per batch -- twice: packing, then the copy into
// the pinned staging buffer -- were a third of a millisecond of the 2.5 ms a 256-window batch spends on the host).
struct PackPool {
    std::vector<std::thread> th; std::mutex m; std::condition_variable cv_go, cv_done;
    const std::function<void(int)>* job = nullptr; int gen = 0, pending = 0; bool stop = false;
    // A worker joins at the generation that was current when it was created (`seen0`): a pool that grows after it has run must not hand the new thread the job of a
    // run() that has already returned (its std::function lived on that run()'s stack) nor let it decrement a `pending` it was never counted in.
    void worker(int t, int seen0) {
        int seen = seen0;
        // UVS_PACK_PIN=1: worker t stays on the (t + 1)-th CPU of the process's affinity mask (CPU 0 of the mask is left to the calling thread; on the EPYC hosts of the MI355X
        // boxes the SMT sibling of CPU i is i + 128, so the first 32 are distinct cores).  Off by default: on a shared host a pinned worker cannot move away from a core
        // another tenant is using (tools/stream_ab.py measures both; profiles/r06_stream_ab.txt)
        if (const char* e = std::getenv("UVS_PACK_PIN")) if (e[0] == '1') {
            cpu_set_t all; CPU_ZERO(&all);
            if (sched_getaffinity(0, sizeof(all), &all) == 0) {
                int want = t + 1, cpu = -1, count = CPU_COUNT(&all);
                if (count > 1) { want %= count; for (int c = 0; c < CPU_SETSIZE; ++c) if (CPU_ISSET(c, &all) && want-- == 0) { cpu = c; break; } }
                if (cpu >= 0) { cpu_set_t one; CPU_ZERO(&one); CPU_SET(cpu, &one); (void)pthread_setaffinity_np(pthread_self(), sizeof(one), &one); }
            }
        }
        for (;;) {
            const std::function<void(int)>* f;
            { std::unique_lock<std::mutex> lk(m); cv_go.wait(lk, [&] { return stop || gen != seen; }); if (stop) return; seen = gen; f = job; }
            if (f == nullptr) continue;      // (a generation whose run() is already over: nothing to do, nothing to count)
            (*f)(t);
            { std::lock_guard<std::mutex> lk(m); if (--pending == 0) cv_done.notify_one(); }
        }
    }
    bool ensure(int n) {      // false: thread creation failed (the caller packs on its own thread).  Called by the thread that calls run(), never beside a run() in flight.
        try {
            while ((int)th.size() < n) {
                const int t = (int)th.size(); int g0;
                { std::lock_guard<std::mutex> lk(m); g0 = gen; }
                th.emplace_back([this, t, g0] { worker(t, g0); });
            }
        } catch (...) { return false; }
        return true;
    }
    void run(int n, const std::function<void(int)>& f) {      // f(0 .. n-1) on n workers (n <= th.size()), the caller waits; workers beyond n see the generation and return at once
        const std::function<void(int)> g = [&](int t) { if (t < n) f(t); };
        { std::lock_guard<std::mutex> lk(m); job = &g; pending = (int)th.size(); ++gen; }
        cv_go.notify_all();
        std::unique_lock<std::mutex> lk(m); cv_done.wait(lk, [&] { return pending == 0; });
        job = nullptr;      // `g` dies with this frame
    }
    ~PackPool() { { std::lock_guard<std::mutex> lk(m); stop = true; } cv_go.notify_all(); for (auto& t : th) t.join(); }
};

// device + pinned-host staging of one evaluation, kept by the solver handle (no allocation on the per-call path once it has grown)
namespace uvsdev {
struct EvalScratch {
    DevBuf<double> d;                          // device
    PinnedBuf<double> h;                       // pinned host
    std::vector<double> work[11];              // host work arrays of the marginalization, kept between calls (a fresh 160 KB vector per call is an mmap / page-fault / munmap round trip)
};
}

// completed in uvs_marginalize.hip, the only unit that looks inside them
struct MargDevScratch;
struct MargBatchBuf;
struct MargWorker;
struct DestroySolver { void operator()(uvs_solver* s) const { uvs_destroy(s); } };
// Every buffer of a handle is an owning member; ~uvs_solver (uvs_marginalize.hip, where the marginalization types it owns are complete) releases what has no owner type,
// uvs_destroy what must go first.
struct uvs_solver {
    uvs_options opts;
    int device;
    int max_batch;
    int max_points = 0, max_point_obs = 0, max_lines = 0, max_line_obs = 0;      // per-window capacities promised at uvs_create
    std::unique_ptr<uvs_solver, DestroySolver> twin;       // second buffer set of uvs_batch_stream (created on first use, destroyed with this handle)
    std::unique_ptr<uvs_solver, DestroySolver> twin2;      // ... and the third (in flight at once: a batch being packed, one being copied, one being solved)
    std::unique_ptr<uvs_solver, DestroySolver> twin3;      // ... and a fourth (UVS_STREAM_SETS=4: one more batch of slack for a host whose packing threads get descheduled)
    hipEvent_t ev_done = nullptr;            // recorded behind a set's k_solve in the stream: the next set's launch waits for it (the kernels of consecutive batches run one after the other)
    int n_cus = 256;                         // compute units of the device
    int large_solve_nt = 512;                // ... and for k_large_solve (UVS_LARGE_SOLVE_NT=256)
    int large_chunks_nt = 512;               // likewise for k_large_chunks (UVS_LARGE_CHUNKS_NT=256 selects the 256-thread kernel of uvs_large.hip)
    int ksolve_nt = 512;                     // which instantiation of the persistent kernel launch_solve uses (uvs_solve512.hip / the 256-thread one of uvs_solver.hip)
    int large_grid = 0;                      // UVS_DEBUG_LARGE_GRID (step tests, read at uvs_create): fewer chunk workgroups than the device offers, so that a small window walks the persistent loops
    int chunk_wgs() const { return std::max(1, large_grid > 0 ? std::min(large_grid, n_cus - 1) : n_cus - 1); }      // chunk workgroups of the persistent large-window kernels: one compute unit stays free for the frame-terms workgroup of the same launch
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    // batch state
    int n_loaded = 0;
    std::vector<DevWin> hdrs;                // host copies of the per-window headers
    std::vector<long long> blob_off, ws_off;
    std::vector<char> host_blobs;
    std::unique_ptr<MargDevScratch> marg_dev;      // buffers of the device marginalization (sub-window blob, its workspace, the reduced system)
    std::unique_ptr<MargBatchBuf> marg_batch;      // ... and of uvs_marginalize_batch (allocated on first use)
    std::unique_ptr<MargWorker> marg_worker;       // uvs_marginalize_resident_begin(): the marginalization runs on this handle's worker thread (created on first use, kept: a thread per call was
    uvs_prior marg_job_out;                        // 30 - 60 us of every optimization() of a replay); its result waits in marg_job_out
    std::unique_ptr<uvspack::PackCache> pack_cache;         // structure of the last large single window (allocated on first use)
    std::vector<std::vector<char>> slot_blobs;      // batch uploads: one packing buffer per batch slot, kept (with its pages) from batch to batch
    std::shared_ptr<PackPool> pool;                 // ... and the worker threads that fill them (pack_pool() below; a buffer set of uvs_batch_stream shares its owner's)
    // ONE host -> device copy per upload: [blobs | blob_off[n] | ws_off[n] | out_tab[3 n]] staged in pinned memory; the three tables
    // live behind the blobs in the same device allocation (d_blob_off / d_ws_off / d_out_tab point into it)
    DevBuf<char> d_blobs;
    PinnedBuf<char> h_up;                    // pinned upload staging
    DevBuf<double> d_ws;
    long long* d_blob_off = nullptr; long long* d_ws_off = nullptr;
    // ONE device -> host copy per download: per window {source offset in d_ws, doubles, destination offset} -> k_pack_outputs gathers the
    // final states AND the reports into one contiguous device buffer [states | reports[n]] -> pinned host buffer
    std::vector<long long> out_tab; long long* d_out_tab = nullptr; DevBuf<double> d_outpack; long long out_total = 0;
    PinnedBuf<char> h_out;                   // pinned download staging
    DevBuf<uvs_report> d_reports;
    DevBuf<double> d_dbg;
    uvsdev::EvalScratch eval_scratch;                // uvs_evaluate / uvs_marginalize staging
    // large-window (configs[3]) run state: value-initialized at the start of every solve (large_prologue) ...
    struct Large {
        bool active = false; int n_chunks = 0, sel = 0, it = 0, invalid = 0, nsucc = 0, pending = 0, term = 0, status = 0;
        bool need_lin = true, first = true, done = false;
        bool stored = false; int backsub_wgs = 0;              // the last uvs_large_step ran the storing back-substitution (uvs_large_debug_step), on so many chunk workgroups
        double radius = 0, decr = 2, cost = 0, gmax = 0, x_norm = 0, local_x2 = 0;
        uvs_report rep;
        double frame_x2 = 0;                                    // frame part of ||x||^2 (the landmark part is per rank: local_x2)
        double relo_pose_in[7] = {0, 0, 0, 0, 0, 0, 0};      // passes through to uvs_large_finish (this path takes no relocalization blocks)
        int grid = 0;                                           // chunk workgroups of k_large_chunks / k_large_backsub = partial rows (min(n_chunks, compute units)); every launch adds ONE for the frame terms
        std::chrono::steady_clock::time_point t_begin;          // start of the host-driven loop (options.max_solver_time_in_seconds)
    } L;
    // ... and what one solve leaves to the next: the device buffers of the loop and the communicator
    struct LargeBufs {
        DevBuf<double> d_state, d_partials, d_reduced, d_bsums, d_out, d_sc5;
        DevBuf<double> d_ctl; DevBuf<uvs_report> d_rep;         // fused loop: trust-region state and report on the device
        DevBuf<double> d_fimg;                                  // frame image of the reduced system (k_large_chunks' extra workgroup -> k_large_solve)
        void* comm = nullptr; int rank = 0, nranks = 1;         // RCCL communicator owned by the handle (uvs_large_comm_init)
        int step_nranks = 1;                                    // ranks the caller all-reduces the step-wise form over (uvs_large_set_nranks)
        bool debug_step = false; DevBuf<double> d_lstep;        // uvs_large_set_debug_step: uvs_large_step runs k_large_backsub_dstep, which stores the step [UVS_DSTEP_FR | points | 4 x lines]
    } LB;
    uvs_solver(); ~uvs_solver();      // both out of line: each needs the destructors of the members above
};

inline uvsdev::KOpts make_kopts(const uvs_options& o, int debug) {
    uvsdev::KOpts k;
    k.max_it = o.max_num_iterations; k.ex_free = o.estimate_extrinsic; k.keep_cand = o.function_tol_keeps_candidate; k.jacobi = o.jacobi_scaling;
    k.sqrt_info = o.point_sqrt_info; k.line_factor = o.line_factor; k.vp_factor = o.vp_factor;
    k.loss_pt = o.loss_point; k.loss_ln = o.loss_line; k.loss_vp = o.loss_vp;
    k.G[0] = o.gravity[0]; k.G[1] = o.gravity[1]; k.G[2] = o.gravity[2];
    k.r0 = o.initial_trust_region_radius; k.rmax = o.max_trust_region_radius; k.rmin = o.min_trust_region_radius;
    k.min_rel = o.min_relative_decrease; k.dlo = o.min_lm_diagonal; k.dhi = o.max_lm_diagonal;
    k.ftol = o.function_tolerance; k.gtol = o.gradient_tolerance; k.ptol = o.parameter_tolerance;
    k.max_ticks = o.max_solver_time_in_seconds > 0.0 ? std::max(1LL, (long long)(o.max_solver_time_in_seconds * 1e8)) : 0LL;      // wall_clock64(): 100 MHz
    k.max_invalid = o.max_consecutive_invalid_steps; k.debug = debug;
    { const char* e = std::getenv("UVS_REDAMP"); k.redamp = (e && e[0] == '0') ? 0 : 1; }      // diagnostic switch, read per launch (tests, A/B): 0 = re-linearize after every rejected step
    { const char* e = std::getenv("UVS_LINE_AHEAD"); k.line_ahead = (e && e[0] == '0') ? 0 : 1; }      // diagnostic switch, read per launch (tests, A/B): 0 = no line chunk's pass A runs ahead of its entry barrier
    { const char* e = std::getenv("UVS_LINE_B1"); k.line_b1 = (e && e[0] == '0') ? 0 : 1; }      // diagnostic switch, read per launch (tests, A/B): 0 = one lane per line in pass B1 of a line chunk and in the line half of a re-damping
    return k;
}

// the handle's packing threads: one creation path (upload_windows and uvs_marginalize_batch run their jobs on them)
inline PackPool& pack_pool(uvs_solver* s) { if (!s->pool) s->pool = std::make_shared<PackPool>(); return *s->pool; }

// What crosses the units.  Each unit's init copies the block table into the unit's own __constant__ arrays and sets the dynamic-LDS attribute of its kernels for the
// current device (uvs_solve_kernel.h: unit_init); uvs_create calls them all.
// uvs_solver.hip.  out_direct: (uvs_batch_stream) every staged header gets the address of its window's slot in the pinned result buffer (DevWin::out_host): k_solve then writes the final state there itself
int upload_windows(uvs_solver* s, int n, const uvs_window* const* ws, bool wait, int chunk_grid = 0, bool out_direct = false, bool all_blocks = false);
// uvs_marginalize.hip
int marg_unit_init(const unsigned char* fa, const unsigned char* fb, int n);
void marg_worker_release(uvs_solver* s);      // uvs_destroy: waits for a marginalization begun and never waited for (it still uses the handle), then ends the worker thread
// uvs_large.hip
int large_unit_init(const unsigned char* fa, const unsigned char* fb, int n);
int debug_step_large(uvs_solver* s, const uvs_window* w, int n_radii, const double* radii, int n_step, double* step, double* scal);      // uvs_debug_step, form 1
#pragma GCC visibility pop
