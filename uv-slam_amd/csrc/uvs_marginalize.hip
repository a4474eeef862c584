// uvs_marginalize.hip -- uvs_evaluate and the marginalization calls of the C ABI (include/uvs_solver.h) on the handle of uvs_solver_handle.h: MARGIN_OLD on the device
// (k_marg_linearize + the host finish of uvs_marg.h), the handle's worker thread (uvs_marginalize_resident_begin / uvs_marginalize_wait) and the batch of windows
// (k_marg_linearize_batch + k_marg_finish).  Kernels of this unit, 256 threads like everything outside uvs_solve512.hip: k_evaluate, k_marg_linearize, k_marg_linearize_batch,
// k_marg_finish.  uvs_evaluate lives here because uvs_marg.h reaches k_evaluate through run_evaluate, and a kernel is defined in one unit.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

#define UVS_UNIT marg256
#include "uvs_solver_handle.h"
#include "uvs_eval_kernel.h"
#include "uvs_marg_kernel.h"
#include "uvs_marg.h"      // LAST: its file-scope `#pragma clang fp contract(...)` must not reach any device code (the kernels are built with the command-line default)

using namespace uvsdev;
using namespace uvspack;

int marg_unit_init(const unsigned char* fa, const unsigned char* fb, int n) {
    if (const int rc = unit_init(fa, fb, n, {(const void*)k_evaluate, (const void*)k_marg_linearize, (const void*)k_marg_linearize_batch})) return rc;
    return hipFuncSetAttribute((const void*)uvsmarg::k_marg_finish, hipFuncAttributeMaxDynamicSharedMemorySize, (int)uvsmarg::MF_LDS_BYTES) == hipSuccess ? UVS_OK : UVS_ERR_HIP;
}

// ---------------------------------------------------------------- MARGIN_OLD on the device (round 3)
// The factors the reference marginalizes (estimator.cpp:1002-1135) form a small window of their own; ONE linearization of it by the solver's own kernels
// (k_marg_linearize) delivers the assembled and landmark-eliminated system, and only the elimination of frame 0's 15 dofs and the n x n factorization stay
// on the host (uvs_marg.h: marg_finish).  Returns UVS_OK, an error, or kMargFallback when the host path must take the call (no such factors, a landmark
// block that is not safely regular, relocalization blocks in the way).
namespace { constexpr int kMargFallback = 1000; }
struct MargDevScratch {
    std::vector<int32_t> pt_lm, pt_fi, pt_fj, ln_lm, ln_fj, ln_vpf; std::vector<double> pt_pi, pt_pj, pt_vi, pt_vj, pt_tdi, pt_tdj, invd, ln_sp, ln_ep, ln_vp, lorth;
    std::vector<uvs_imu_block> imu; std::vector<int> pmap, lmap, lstart;
    std::vector<char> blob;
    DevBuf<char> d_blob; DevBuf<double> d_ws, d_out; PinnedBuf<char> h_out, h_up;
};
// The sub-window of the factors MARGIN_OLD reads (estimator.cpp:1002-1135): the prior, the IMU link of frame 0, the observations of the points anchored in frame 0 and of the lines
// that start there (without their anchor observation).  Its arrays live in M; used[] = the frame blocks (ids: pose f -> f ; speedbias f -> 11 + f ; ex -> 22 ; td -> 23) it touches.
static int marg_build_sub(uvs_solver* s, const uvs_window* w, MargDevScratch& M, bool used[24], uvs_window& sub, std::string& err_) {
    std::string& serr = err_;
    for (int k = 0; k < 24; ++k) used[k] = false;
    const bool td_on = s->opts.estimate_td != 0;
    const int NFR = UVS_NF;
    // the sub-window below is cut out of the caller's arrays BEFORE pack_window sees them: same checks first
    { const int rv = validate_window(w, serr); if (rv != UVS_OK) return rv; }
    if (td_on && w->n_point_obs > 0 && (!w->pt_vel_i || !w->pt_vel_j || !w->pt_td_i || !w->pt_td_j)) { serr = "estimate_td needs pt_vel_i / pt_vel_j / pt_td_i / pt_td_j"; return UVS_ERR_INVALID_ARG; }
    // ---- the sub-window: which blocks it touches (ids: pose f -> f ; speedbias f -> 11 + f ; ex -> 22 ; td -> 23)
    const bool have_prior = w->prior && w->prior->n > 0;
    if (have_prior) for (int b = 0; b < w->prior->n_blocks; ++b) {
        const uvs_prior& p = *w->prior;
        used[p.block_kind[b] == UVS_BLOCK_POSE ? p.block_frame[b] : p.block_kind[b] == UVS_BLOCK_SPEEDBIAS ? NFR + p.block_frame[b] : p.block_kind[b] == UVS_BLOCK_TD ? 23 : 22] = true;
    }
    M.imu.clear();
    for (int b = 0; b < w->n_imu; ++b) {
        if (w->imu[b].frame_i != 0 || !(w->imu[b].sum_dt < 10.0)) continue;
        uvs_imu_block ib = w->imu[b]; ib.skip = 0; M.imu.push_back(ib);
        used[0] = used[NFR] = used[1] = used[NFR + 1] = true;
    }
    M.pmap.assign(std::max(w->n_points, 1), -1); M.lmap.assign(std::max(w->n_lines, 1), -1); M.lstart.assign(std::max(w->n_lines, 1), -1);
    M.pt_lm.clear(); M.pt_fi.clear(); M.pt_fj.clear(); M.pt_pi.clear(); M.pt_pj.clear(); M.pt_vi.clear(); M.pt_vj.clear(); M.pt_tdi.clear(); M.pt_tdj.clear(); M.invd.clear();
    for (int k = 0; k < w->n_point_obs; ++k) {
        if (w->pt_fi[k] != 0) continue;
        const int lm = w->pt_lm[k];
        if (M.pmap[lm] < 0) { M.pmap[lm] = (int)M.invd.size(); M.invd.push_back(w->inv_depth[lm]); }
        M.pt_lm.push_back(M.pmap[lm]); M.pt_fi.push_back(0); M.pt_fj.push_back(w->pt_fj[k]);
        for (int q = 0; q < 3; ++q) { M.pt_pi.push_back(w->pt_pi[3 * k + q]); M.pt_pj.push_back(w->pt_pj[3 * k + q]); }
        if (td_on) { for (int q = 0; q < 2; ++q) { M.pt_vi.push_back(w->pt_vel_i[2 * k + q]); M.pt_vj.push_back(w->pt_vel_j[2 * k + q]); } M.pt_tdi.push_back(w->pt_td_i[k]); M.pt_tdj.push_back(w->pt_td_j[k]); }
        used[0] = used[w->pt_fj[k]] = used[22] = true; if (td_on) used[23] = true;
    }
    M.ln_lm.clear(); M.ln_fj.clear(); M.ln_vpf.clear(); M.ln_sp.clear(); M.ln_ep.clear(); M.ln_vp.clear(); M.lorth.clear();
    for (int k = 0; k < w->n_line_obs; ++k) if (M.lstart[w->ln_lm[k]] < 0) M.lstart[w->ln_lm[k]] = w->ln_fj[k];
    for (int k = 0; k < w->n_line_obs; ++k) {
        const int lm = w->ln_lm[k], fj = w->ln_fj[k];
        if (M.lstart[lm] != 0 || fj == 0) continue;      // lines that start in frame 0, without the anchor observation (estimator.cpp:1102-1104)
        if (M.lmap[lm] < 0) { M.lmap[lm] = (int)(M.lorth.size() / 4); for (int q = 0; q < 4; ++q) M.lorth.push_back(w->line_orth[4 * lm + q]); }
        M.ln_lm.push_back(M.lmap[lm]); M.ln_fj.push_back(fj); M.ln_vpf.push_back(w->ln_has_vp[k] ? 1 : 0);
        for (int q = 0; q < 3; ++q) { M.ln_sp.push_back(w->ln_sp[3 * k + q]); M.ln_ep.push_back(w->ln_ep[3 * k + q]); M.ln_vp.push_back(w->ln_vp[3 * k + q]); }
        used[fj] = true;
    }
    if (M.imu.empty() && M.pt_lm.empty() && M.ln_lm.empty() && !have_prior) return kMargFallback;
    std::memset(&sub, 0, sizeof(sub));
    std::memcpy(sub.pose, w->pose, sizeof(sub.pose)); std::memcpy(sub.speedbias, w->speedbias, sizeof(sub.speedbias)); std::memcpy(sub.ex_pose, w->ex_pose, sizeof(sub.ex_pose));
    sub.td = w->td; for (int q = 0; q < 7; ++q) sub.relo_pose[q] = q == 6 ? 1.0 : 0.0;
    sub.n_points = (int)M.invd.size(); sub.n_point_obs = (int)M.pt_lm.size(); sub.inv_depth = M.invd.data();
    sub.pt_lm = M.pt_lm.data(); sub.pt_fi = M.pt_fi.data(); sub.pt_fj = M.pt_fj.data(); sub.pt_pi = M.pt_pi.data(); sub.pt_pj = M.pt_pj.data();
    if (td_on) { sub.pt_vel_i = M.pt_vi.data(); sub.pt_vel_j = M.pt_vj.data(); sub.pt_td_i = M.pt_tdi.data(); sub.pt_td_j = M.pt_tdj.data(); }
    sub.n_lines = (int)(M.lorth.size() / 4); sub.n_line_obs = (int)M.ln_lm.size(); sub.line_orth = M.lorth.data();
    sub.ln_lm = M.ln_lm.data(); sub.ln_fj = M.ln_fj.data(); sub.ln_has_vp = M.ln_vpf.data(); sub.ln_sp = M.ln_sp.data(); sub.ln_ep = M.ln_ep.data(); sub.ln_vp = M.ln_vp.data();
    sub.n_imu = (int)M.imu.size(); sub.imu = M.imu.data(); sub.prior = have_prior ? w->prior : nullptr;
    return UVS_OK;
}
// Ordering of the frame blocks of a device-linearized sub-window: the dropped ones (Pose[0], SpeedBias[0]) first, then the kept ones in id order.  map[i] = index of row i in
// k_marg_linearize's padded reduced system (16 x frame + dof, the extrinsic / time-offset slots).
static void marg_frame_order(const bool used[24], std::vector<int>& pos, std::vector<int>& keep_ids, int& md, int& n, std::vector<int>& map) {
    const int NFR = UVS_NF;
    auto lsize = [&](int id) { return id < NFR ? 6 : id < 2 * NFR ? 9 : id == 22 ? 6 : 1; };
    auto pad = [&](int id, int q) { return id < NFR ? 16 * id + q : id < 2 * NFR ? 16 * (id - NFR) + 6 + q : id == 22 ? UVS_EX_INDEX(q) : UVS_TD_INDEX; };
    pos.assign(24, -1); keep_ids.clear(); map.clear();
    md = 0;
    for (int id : {0, NFR}) if (used[id]) { pos[id] = md; md += lsize(id); for (int q = 0; q < lsize(id); ++q) map.push_back(pad(id, q)); }
    int N = md;
    for (int id = 0; id < 24; ++id) if (used[id] && id != 0 && id != NFR) { pos[id] = N; N += lsize(id); keep_ids.push_back(id); for (int q = 0; q < lsize(id); ++q) map.push_back(pad(id, q)); }
    n = N - md;
}
static int marginalize_old_device(uvs_solver* s, const uvs_window* w, uvs_prior* out) {
    if (std::getenv("UVS_MARG_HOST")) return kMargFallback;      // (relocalization blocks are not marginalized, estimator.cpp:1002-1228: the sub-window simply leaves them out)
    const bool prof = std::getenv("UVS_MARG_PROFILE") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    if (!s->marg_dev) s->marg_dev = std::make_unique<MargDevScratch>();
    MargDevScratch& M = *s->marg_dev;
    bool used[24]; uvs_window sub;
    { const int rb = marg_build_sub(s, w, M, used, sub, s->err); if (rb != UVS_OK) return rb; }
    // ---- pack with a FREE extrinsic (the prior keeps para_Ex_Pose), upload, one linearization
    uvs_options o = s->opts; o.estimate_extrinsic = 1; o.initial_trust_region_radius = 1e300;
    DevWin h; M.blob.clear();
    const auto tp0 = std::chrono::steady_clock::now();
    int rc = pack_window(&sub, o, M.blob, h, s->err);
    const auto tp1 = std::chrono::steady_clock::now();
    if (rc == UVS_ERR_UNSUPPORTED || rc == UVS_ERR_CAPACITY) return kMargFallback;
    if (rc != UVS_OK) return rc;
    UVS_HIP(s->err, hipSetDevice(s->device));
    if ((rc = M.d_blob.ensure(M.blob.size(), s->err, grow_half)) != UVS_OK || (rc = M.d_ws.ensure((size_t)h.ws_doubles * 8, s->err, grow_half)) != UVS_OK ||
        (rc = M.d_out.ensure(MARG_OUT * 8, s->err)) != UVS_OK || (rc = M.h_out.ensure(MARG_OUT * 8, s->err)) != UVS_OK ||
        (rc = M.h_up.ensure(M.blob.size(), s->err, grow_pinned)) != UVS_OK) return rc;
    UVS_HIP(s->err, hipStreamSynchronize(s->stream));      // the staging buffer may still feed the previous call's copy
    const auto tq0 = std::chrono::steady_clock::now();
    std::memcpy(M.h_up, M.blob.data(), M.blob.size());
    const auto tq1 = std::chrono::steady_clock::now();
    UVS_HIP(s->err, hipMemcpyAsync(M.d_blob, M.h_up, M.blob.size(), hipMemcpyHostToDevice, s->stream));
    const KOpts ko = make_kopts(o, 0);
    hipLaunchKernelGGL(k_marg_linearize, dim3(1), dim3(NT), LDS_BYTES, s->stream, M.d_blob, M.d_ws, ko, M.d_out);
    UVS_HIP(s->err, hipGetLastError());
    UVS_HIP(s->err, hipMemcpyAsync(M.h_out, M.d_out, MARG_OUT * 8, hipMemcpyDeviceToHost, s->stream));
    const auto tq2 = std::chrono::steady_clock::now();
    UVS_HIP(s->err, hipStreamSynchronize(s->stream));
    const auto t1 = std::chrono::steady_clock::now();
    if (prof) { auto us = [](auto a_, auto b_) { return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(b_ - a_).count() * 1e-3; };
                std::fprintf(stderr, "[uvs_marginalize] device path: sub-window %.0f us, pack %.0f us (%zu bytes), upload + kernel + download %.0f us (allocations + drain %.0f, copy into pinned %.0f, three enqueues %.0f, wait %.0f)\n",
                             us(t0, tp0), us(tp0, tp1), M.blob.size(), us(tp1, t1), us(tp1, tq0), us(tq0, tq1), us(tq1, tq2), us(tq2, t1)); }
    const double* S = (const double*)M.h_out.get(); const double* g = S + UVS_RD * (UVS_RD + 1) / 2; const double* scal = g + UVS_RD;
    if (scal[1] != 0.0 || !std::isfinite(scal[0])) return kMargFallback;      // a landmark block the reference's eps cut would touch: the host path applies that cut
    // ---- ordering: the dropped frame blocks (Pose[0], SpeedBias[0]) first, then the kept ones in id order
    std::vector<int> pos, keep_ids, map; int md = 0, n = 0;
    marg_frame_order(used, pos, keep_ids, md, n, map);
    const int N = md + n;
    if (n > UVS_MAX_PRIOR_DIM || (int)keep_ids.size() > UVS_MAX_PRIOR_BLOCKS) { s->err = "prior capacity"; return UVS_ERR_CAPACITY; }
    if (md == 0 || n == 0) return kMargFallback;
    std::vector<double>&A = s->eval_scratch.work[0], &bv = s->eval_scratch.work[1];
    A.assign((size_t)N * N, 0.0); bv.assign(N, 0.0);
    for (int i = 0; i < N; ++i) {
        const int ia = map[i];
        bv[i] = g[ia];
        for (int j = 0; j < N; ++j) { const int ib = map[j]; const int hi = ia >= ib ? ia : ib, lo = ia >= ib ? ib : ia; A[(size_t)i * N + j] = S[(size_t)hi * (hi + 1) / 2 + lo]; }
    }
    double us_pre[3] = {(double)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count() * 1e-3, 0.0, 0.0};
    const int rf = marg_finish(N, md, md, n, A, bv, pos, keep_ids, w, 0, out, s->eval_scratch, prof, us_pre);
    if (rf != UVS_OK) s->err = "marginalization: the linearized system is not finite";
    return rf;
}

extern "C" {

int uvs_evaluate(uvs_solver* s, const uvs_window* w, int robust, uvs_eval* out) {
    if (!s || !w || !out) return UVS_ERR_INVALID_ARG;
    const uvs_window* arr[1] = {w};
    int rc = uvs_batch_upload(s, 1, arr);
    if (rc != UVS_OK) return rc;
    return run_evaluate(s->device, s->stream, s->d_blobs, s->d_ws, s->hdrs[0], make_kopts(s->opts, 0), robust, out, s->err, s->eval_scratch);
}

}  // extern "C"

// The handle's marginalization worker (uvs_marginalize_resident_begin / uvs_marginalize_wait): ONE thread per handle, created on the first begin and parked on a condition
// variable between jobs.
struct MargWorker {
    std::thread th; std::mutex m; std::condition_variable cv_job, cv_done;
    uvs_solver* s = nullptr; const uvs_window* w = nullptr; int flag = 0, rc = UVS_OK;
    bool has_job = false, done = false, stop = false, in_flight = false;
    void loop() {
        for (;;) {
            std::unique_lock<std::mutex> lk(m);
            cv_job.wait(lk, [&] { return stop || has_job; });
            if (stop) return;
            has_job = false;
            const uvs_window* w_ = w; const int f_ = flag;
            lk.unlock();
            const int r = uvs_marginalize_resident(s, w_, f_, &s->marg_job_out);
            lk.lock();
            rc = r; done = true;
            cv_done.notify_all();
        }
    }
    ~MargWorker() {      // waits for a marginalization begun and never waited for: it still uses the handle
        if (in_flight) { std::unique_lock<std::mutex> lk(m); cv_done.wait(lk, [&] { return done; }); }
        { std::lock_guard<std::mutex> lk(m); stop = true; }
        cv_job.notify_one();
        if (th.joinable()) th.join();
    }
};
static bool marg_in_flight(const uvs_solver* s) { return s->marg_worker && s->marg_worker->in_flight; }      // (only the caller's thread reads / writes in_flight)
static int marg_worker_begin(uvs_solver* s, const uvs_window* w, int flag) {
    if (!s->marg_worker) {
        auto mw = std::make_unique<MargWorker>(); mw->s = s;
        try { mw->th = std::thread([w_ = mw.get()] { w_->loop(); }); }
        catch (const std::exception& e) {      // (std::system_error when no thread can be created: nothing may cross the C boundary)
            s->err = std::string("uvs_marginalize_resident_begin: could not start the worker thread: ") + e.what();
            return UVS_ERR_HIP;
        }
        s->marg_worker = std::move(mw);
    }
    MargWorker& mw = *s->marg_worker;
    { std::lock_guard<std::mutex> lk(mw.m); mw.w = w; mw.flag = flag; mw.has_job = true; mw.done = false; }
    mw.in_flight = true;
    mw.cv_job.notify_one();
    return UVS_OK;
}
void marg_worker_release(uvs_solver* s) { s->marg_worker.reset(); }
static int marg_worker_wait(uvs_solver* s) {
    MargWorker& mw = *s->marg_worker;
    std::unique_lock<std::mutex> lk(mw.m);
    mw.cv_done.wait(lk, [&] { return mw.done; });
    mw.done = false; mw.in_flight = false;
    return mw.rc;
}

// MARGIN_SECOND_NEW (estimator.cpp:1159-1228) marginalizes Pose[WINDOW_SIZE - 1] out of the OLD PRIOR and reads nothing else: no factor is evaluated, so no kernel runs and nothing is
// copied -- r = r0 + J0 dx, A = J0^T J0, b = J0^T r, the 6 x 6 elimination and the n x n factorization are host work (uvs_marg.h).  Round 5 packed and uploaded the window and
// evaluated it on the device to obtain that one vector r (0.2 ms of the 0.5 ms a call took).
static int marginalize_second_new_host(uvs_solver* s, const uvs_window* w, uvs_prior* out) {
    { const int rv = validate_window(w, s->err); if (rv != UVS_OK) return rv; }
    // (the same complaint the packing of the window made when this path still uploaded it)
    if (s->opts.estimate_td != 0 && w->n_point_obs > 0 && (!w->pt_vel_i || !w->pt_vel_j || !w->pt_td_i || !w->pt_td_j)) { s->err = "estimate_td needs pt_vel_i / pt_vel_j / pt_td_i / pt_td_j"; return UVS_ERR_INVALID_ARG; }
    DevWin h; std::memset(&h, 0, sizeof(h)); h.td_on = s->opts.estimate_td != 0;
    return run_marginalize(s->device, s->stream, nullptr, nullptr, h, w, make_kopts(s->opts, 0), 1, out, s->err, s->eval_scratch);
}

extern "C" {

int uvs_marginalize(uvs_solver* s, const uvs_window* w, int flag, uvs_prior* out) {
    if (!s || !w || !out || (flag != 0 && flag != 1)) return UVS_ERR_INVALID_ARG;
    if (flag == 1) return marginalize_second_new_host(s, w, out);
    if (flag == 0) { const int rd = marginalize_old_device(s, w, out); if (rd != kMargFallback) return rd; }
    const uvs_window* arr[1] = {w};
    const auto tu0 = std::chrono::steady_clock::now();
    int rc = uvs_batch_upload(s, 1, arr);
    if (rc != UVS_OK) return rc;
    if (std::getenv("UVS_MARG_PROFILE")) std::fprintf(stderr, "[uvs_marginalize] upload %.0f us\n", (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - tu0).count() * 1e-3);
    return run_marginalize(s->device, s->stream, s->d_blobs, s->d_ws, s->hdrs[0], w, make_kopts(s->opts, 0), flag, out, s->err, s->eval_scratch);
}


int uvs_marginalize_resident(uvs_solver* s, const uvs_window* w, int flag, uvs_prior* out) {
    if (!s || !w || !out || (flag != 0 && flag != 1)) return UVS_ERR_INVALID_ARG;
    if (s->n_loaded != 1) { s->err = "uvs_marginalize_resident: no single resident window"; return UVS_ERR_INVALID_ARG; }
    const DevWin& h = s->hdrs[0];
    const int pn = (w->prior && w->prior->n > 0) ? w->prior->n : 0;
    if (h.n_points != w->n_points || h.n_pt_obs - h.n_relo != w->n_point_obs || h.n_lines != w->n_lines || h.n_ln_obs != w->n_line_obs || h.n_imu != w->n_imu || h.prior_n != pn) {
        s->err = "uvs_marginalize_resident: the window does not match the resident one"; return UVS_ERR_INVALID_ARG;
    }
    if (flag == 1) return marginalize_second_new_host(s, w, out);      // (reads the old prior only: host work, no device round trip)
    if (flag == 0) { const int rd = marginalize_old_device(s, w, out); if (rd != kMargFallback) return rd; }      // (needs nothing of the resident blob: the factors of frame 0 travel as a window of their own)
    UVS_HIP(s->err, hipSetDevice(s->device));
    // state sections of the resident blob: frames[184] = pose | speedbias | ex_pose | td, inverse depths, line parameters
    // staged in the pinned upload buffer (copies from the caller's pageable arrays would each be a synchronous staging round trip)
    const size_t nst = 184 + (size_t)h.n_points + 4 * (size_t)h.n_lines;
    UVS_HIP(s->err, hipStreamSynchronize(s->stream));      // the staging buffer may still feed an earlier copy
    int rcp;
    if ((rcp = s->h_up.ensure(nst * 8, s->err, grow_pinned)) != UVS_OK) return rcp;
    double* fr = (double*)s->h_up.get();
    std::memcpy(fr, w->pose, 77 * 8); std::memcpy(fr + 77, w->speedbias, 99 * 8); std::memcpy(fr + 176, w->ex_pose, 7 * 8); fr[183] = w->td;
    if (h.n_points) std::memcpy(fr + 184, w->inv_depth, (size_t)h.n_points * 8);
    if (h.n_lines) std::memcpy(fr + 184 + h.n_points, w->line_orth, (size_t)h.n_lines * 32);
    char* blob = s->d_blobs + s->blob_off[0];
    UVS_HIP(s->err, hipMemcpyAsync(blob + (size_t)h.d_frames * 8, fr, 184 * 8, hipMemcpyHostToDevice, s->stream));
    if (h.n_points) UVS_HIP(s->err, hipMemcpyAsync(blob + (size_t)h.d_invd * 8, fr + 184, (size_t)h.n_points * 8, hipMemcpyHostToDevice, s->stream));
    if (h.n_lines) UVS_HIP(s->err, hipMemcpyAsync(blob + (size_t)h.d_line * 8, fr + 184 + h.n_points, (size_t)h.n_lines * 32, hipMemcpyHostToDevice, s->stream));
    return run_marginalize(s->device, s->stream, s->d_blobs, s->d_ws, s->hdrs[0], w, make_kopts(s->opts, 0), flag, out, s->err, s->eval_scratch);
}

int uvs_marginalize_resident_begin(uvs_solver* s, const uvs_window* w, int flag) {
    if (!s || !w || (flag != 0 && flag != 1)) return UVS_ERR_INVALID_ARG;
    if (marg_in_flight(s)) { s->err = "uvs_marginalize_resident_begin: the previous marginalization has not been waited for"; return UVS_ERR_INVALID_ARG; }
    // the worker owns the handle until uvs_marginalize_wait(): device selection is per thread, everything else (stream, pinned buffers, scratch) is the handle's own
    return marg_worker_begin(s, w, flag);
}
int uvs_marginalize_wait(uvs_solver* s, uvs_prior* out) {
    if (!s || !out) return UVS_ERR_INVALID_ARG;
    if (!marg_in_flight(s)) { s->err = "uvs_marginalize_wait: no marginalization in flight"; return UVS_ERR_INVALID_ARG; }
    const int rc = marg_worker_wait(s);
    if (rc == UVS_OK) *out = s->marg_job_out;
    return rc;
}

}  // extern "C"


// ---------------------------------------------------------------- marginalization of a BATCH of windows (round 6, ABI v7)
// Per window the same result as uvs_marginalize(), with everything that is O(n^3) on the device for all windows at once: the sub-windows of the MARGIN_OLD windows are packed by the
// handle's packing threads and linearized by ONE launch (k_marg_linearize_batch: assembly + elimination of the dropped landmarks), the dropped frame block, the Schur complement and the
// n x n eigen-decomposition of every window run in ONE launch of k_marg_finish (uvs_marg_kernel.h: parallel cyclic Jacobi).  MARGIN_SECOND_NEW windows send their prior-only system
// (assembled on the packing threads) to the same kernel.  A window the device path does not take (a landmark or frame block the reference's eps cut would touch, a system larger than
// the kernel's LDS layout, no factors at all) goes through uvs_marginalize() on the calling thread.
struct MargBatchBuf {
    PinnedBuf<char> h_stage;      // pinned: blobs | tables | descriptors | dense systems
    PinnedBuf<char> h_out;        // pinned: finish outputs | linearization scalars
    DevBuf<char> d_blobs; DevBuf<double> d_ws, d_lin; DevBuf<char> d_tab; DevBuf<double> d_in, d_out;
    std::vector<MargDevScratch> thread_sub; std::vector<EvalScratch> thread_eval;
};
namespace {
struct MargBatchItem {
    int path = 3;      // 0: *out is final already; 1: device linearization + device finish (MARGIN_OLD); 2: device finish of a host-assembled system (MARGIN_SECOND_NEW); 3: uvs_marginalize()
    int rc = UVS_OK; std::string err;
    bool used[24]; std::vector<int> pos, keep_ids, map; int md = 0, n = 0;
    std::vector<char> blob; DevWin h;
    std::vector<double> dense;      // path 2: A [N][N] | b [N]
};
}
extern "C" int uvs_marginalize_batch(uvs_solver* s, int n_win, const uvs_window* const* ws, const int* flags, uvs_prior* out, int* status) {
    using namespace uvsmarg;
    if (!s || n_win < 0 || (n_win > 0 && (!ws || !flags || !out))) return UVS_ERR_INVALID_ARG;
    for (int b = 0; b < n_win; ++b) if (!ws[b] || (flags[b] != 0 && flags[b] != 1)) { s->err = "uvs_marginalize_batch: null window or flag outside {0, 1}"; return UVS_ERR_INVALID_ARG; }
    if (marg_in_flight(s)) { s->err = "uvs_marginalize_batch: a marginalization begun with uvs_marginalize_resident_begin has not been waited for"; return UVS_ERR_INVALID_ARG; }
    if (n_win == 0) return UVS_OK;
    UVS_HIP(s->err, hipSetDevice(s->device));
    if (!s->marg_batch) s->marg_batch = std::make_unique<MargBatchBuf>();
    MargBatchBuf& B = *s->marg_batch;
    const bool prof = std::getenv("UVS_MARG_PROFILE") != nullptr;
    const auto tb0 = std::chrono::steady_clock::now();
    auto tb1 = tb0, tb2 = tb0, tb3 = tb0;
    int nthreads = 1;
    if (n_win >= 4) {
        nthreads = std::min(pack_threads(32u, 2u), n_win);
    }
    if ((int)B.thread_sub.size() < nthreads) { B.thread_sub.resize(nthreads); B.thread_eval.resize(nthreads); }
    std::vector<MargBatchItem> items((size_t)n_win);
    uvs_options o_sub = s->opts; o_sub.estimate_extrinsic = 1; o_sub.initial_trust_region_radius = 1e300;      // (as marginalize_old_device: the prior keeps para_Ex_Pose)
    const bool host_only = std::getenv("UVS_MARG_HOST") != nullptr;
    // ---- host stage, per window, on the packing threads
    const auto job = [&](int t) {
        for (int b = t; b < n_win; b += nthreads) {
            MargBatchItem& it = items[b]; const uvs_window* w = ws[b];
            it.path = 3;
            if (host_only) continue;
            if (flags[b] == 0) {
                uvs_window sub;
                const int rb = marg_build_sub(s, w, B.thread_sub[t], it.used, sub, it.err);
                if (rb == kMargFallback) continue;
                if (rb != UVS_OK) { it.rc = rb; it.path = 0; continue; }
                const int rp = pack_window(&sub, o_sub, it.blob, it.h, it.err);
                if (rp == UVS_ERR_UNSUPPORTED || rp == UVS_ERR_CAPACITY) continue;
                if (rp != UVS_OK) { it.rc = rp; it.path = 0; continue; }
                marg_frame_order(it.used, it.pos, it.keep_ids, it.md, it.n, it.map);
                if (it.n > UVS_MAX_PRIOR_DIM || (int)it.keep_ids.size() > UVS_MAX_PRIOR_BLOCKS) { it.err = "prior capacity"; it.rc = UVS_ERR_CAPACITY; it.path = 0; continue; }
                if (it.md == 0 || it.n == 0 || it.md > MF_MD || it.n > MF_NKEEP || it.md + it.n > MF_NMAX) continue;
                it.path = 1;
            } else {
                { const int rv = validate_window(w, it.err); if (rv != UVS_OK) { it.rc = rv; it.path = 0; continue; } }
                if (s->opts.estimate_td != 0 && w->n_point_obs > 0 && (!w->pt_vel_i || !w->pt_vel_j || !w->pt_td_i || !w->pt_td_j)) { it.err = "estimate_td needs pt_vel_i / pt_vel_j / pt_td_i / pt_td_j"; it.rc = UVS_ERR_INVALID_ARG; it.path = 0; continue; }
                DevWin h; std::memset(&h, 0, sizeof(h)); h.td_on = s->opts.estimate_td != 0;
                MargSystem ms; bool done = false;
                EvalScratch& sc = B.thread_eval[t];
                const int ra = marg_assemble_host(s->device, s->stream, nullptr, nullptr, h, w, make_kopts(s->opts, 0), 1, &out[b], it.err, sc, ms, done);
                if (ra != UVS_OK || done) { it.rc = ra; it.path = 0; continue; }
                if (ms.m != ms.md || ms.md > MF_MD || ms.n > MF_NKEEP || ms.N > MF_NMAX || ms.md == 0 || ms.n == 0) continue;      // (never for MARGIN_SECOND_NEW: it drops one pose and no landmark)
                it.md = ms.md; it.n = ms.n; it.pos = ms.pos; it.keep_ids = ms.keep_ids;
                it.dense.assign(sc.work[0].begin(), sc.work[0].begin() + (size_t)ms.N * ms.N);
                it.dense.insert(it.dense.end(), sc.work[1].begin(), sc.work[1].begin() + ms.N);
                it.path = 2;
            }
        }
    };
    if (nthreads > 1) { if (pack_pool(s).ensure(nthreads)) s->pool->run(nthreads, job); else { const int nt_ = nthreads; nthreads = 1; job(0); nthreads = nt_; } }
    else job(0);
    tb1 = std::chrono::steady_clock::now();
    // ---- device stage: finish slots = the path-1 windows (their linearization slots), then the path-2 windows
    std::vector<int> slot_win; slot_win.reserve(n_win);
    for (int b = 0; b < n_win; ++b) if (items[b].path == 1) slot_win.push_back(b);
    const int n1 = (int)slot_win.size();
    for (int b = 0; b < n_win; ++b) if (items[b].path == 2) slot_win.push_back(b);
    const int nfin = (int)slot_win.size();
    const int n1_prof = n1, nfin_prof = nfin;
    if (nfin > 0) {
        // staging layout: [blobs (8-byte aligned each)] [blob_off n1][ws_off n1] [desc nfin x MF_DESC ints] [dense (nfin - n1) x MF_IN doubles]
        std::vector<long long> blob_off(std::max(n1, 1)), ws_off(std::max(n1, 1));
        size_t blob_total = 0; long long ws_total = 0;
        for (int q = 0; q < n1; ++q) { const MargBatchItem& it = items[slot_win[q]]; blob_off[q] = (long long)blob_total; blob_total += (it.blob.size() + 255) & ~(size_t)255; ws_off[q] = ws_total; ws_total += it.h.ws_doubles; }
        const size_t tab_bytes = (size_t)n1 * 16 + (size_t)nfin * MF_DESC * 4, dense_bytes = (size_t)(nfin - n1) * MF_IN * 8;
        int rc;
        if ((rc = B.h_stage.ensure(blob_total + tab_bytes + dense_bytes + 64, s->err, grow_pinned)) != UVS_OK) return rc;
        if ((rc = B.h_out.ensure((size_t)nfin * MF_OUT * 8 + (size_t)std::max(n1, 1) * 64, s->err, grow_pinned)) != UVS_OK) return rc;
        if ((rc = B.d_blobs.ensure(std::max<size_t>(blob_total, 256), s->err)) != UVS_OK) return rc;
        if ((rc = B.d_ws.ensure(std::max<size_t>((size_t)ws_total * 8, 256), s->err)) != UVS_OK) return rc;
        if ((rc = B.d_lin.ensure((size_t)std::max(n1, 1) * MARG_OUT * 8, s->err)) != UVS_OK) return rc;
        if ((rc = B.d_tab.ensure(tab_bytes + 64, s->err)) != UVS_OK) return rc;
        if ((rc = B.d_in.ensure(std::max<size_t>(dense_bytes, 256), s->err)) != UVS_OK) return rc;
        if ((rc = B.d_out.ensure((size_t)nfin * MF_OUT * 8, s->err)) != UVS_OK) return rc;
        UVS_HIP(s->err, hipStreamSynchronize(s->stream));      // the staging buffer may still feed an earlier call's copies
        char* hb = B.h_stage; char* ht = hb + blob_total; char* hd = ht + ((tab_bytes + 7) & ~(size_t)7);
        for (int q = 0; q < n1; ++q) { const MargBatchItem& it = items[slot_win[q]]; std::memcpy(hb + blob_off[q], it.blob.data(), it.blob.size()); }
        long long* t_off = (long long*)ht; int* t_desc = (int*)(ht + (size_t)n1 * 16);
        for (int q = 0; q < n1; ++q) { t_off[q] = blob_off[q]; t_off[n1 + q] = ws_off[q]; }
        for (int q = 0; q < nfin; ++q) {
            const MargBatchItem& it = items[slot_win[q]]; int* d = t_desc + (size_t)q * MF_DESC;
            std::memset(d, 0, MF_DESC * 4);
            d[0] = it.md + it.n; d[1] = it.md; d[2] = it.n; d[3] = q < n1 ? 0 : 1;
            if (q < n1) for (int i = 0; i < it.md + it.n; ++i) d[4 + i] = it.map[i];
            else std::memcpy(hd + (size_t)(q - n1) * MF_IN * 8, it.dense.data(), it.dense.size() * 8);
        }
        if (n1 > 0) UVS_HIP(s->err, hipMemcpyAsync(B.d_blobs, hb, blob_total, hipMemcpyHostToDevice, s->stream));
        UVS_HIP(s->err, hipMemcpyAsync(B.d_tab, ht, tab_bytes, hipMemcpyHostToDevice, s->stream));
        if (nfin > n1) {      // (likewise only the used head N^2 + N of every dense input slot)
            int N_max = 1; for (int q = n1; q < nfin; ++q) N_max = std::max(N_max, items[slot_win[q]].md + items[slot_win[q]].n);
            UVS_HIP(s->err, hipMemcpy2DAsync(B.d_in, (size_t)MF_IN * 8, hd, (size_t)MF_IN * 8, (size_t)(N_max * N_max + N_max) * 8, (size_t)(nfin - n1), hipMemcpyHostToDevice, s->stream));
        }
        const KOpts ko = make_kopts(o_sub, 0);
        if (n1 > 0) {
            hipLaunchKernelGGL(k_marg_linearize_batch, dim3(n1), dim3(NT), LDS_BYTES, s->stream, B.d_blobs, (const long long*)B.d_tab.get(), B.d_ws, (const long long*)B.d_tab.get() + n1, ko, B.d_lin);
            UVS_HIP(s->err, hipGetLastError());
        }
        // (path-2 slots read their dense system at slot - n1: the pointer is shifted so that the kernel's `in_all + MF_IN * blockIdx.x` lands there)
        hipLaunchKernelGGL(k_marg_finish, dim3(nfin), dim3(MF_NT), MF_LDS_BYTES, s->stream, (const int*)(B.d_tab + (size_t)n1 * 16), (const double*)B.d_in - (size_t)n1 * MF_IN, (const double*)B.d_lin, (int)MARG_OUT,
                           (int)UVS_RD, B.d_out, 1e-8);
        UVS_HIP(s->err, hipGetLastError());
        int n_max = 1; for (int q = 0; q < nfin; ++q) n_max = std::max(n_max, items[slot_win[q]].n);
        // (only the used head of every output slot travels: status | r0 | J0 [n][n])
        UVS_HIP(s->err, hipMemcpy2DAsync(B.h_out, (size_t)MF_OUT * 8, B.d_out, (size_t)MF_OUT * 8, (size_t)(MF_OUT_J + n_max * n_max) * 8, (size_t)nfin, hipMemcpyDeviceToHost, s->stream));
        double* h_scal = (double*)(B.h_out + (size_t)nfin * MF_OUT * 8);
        if (n1 > 0) UVS_HIP(s->err, hipMemcpy2DAsync(h_scal, 64, B.d_lin + (MARG_OUT - 8), (size_t)MARG_OUT * 8, 64, (size_t)n1, hipMemcpyDeviceToHost, s->stream));
        tb2 = std::chrono::steady_clock::now();
        UVS_HIP(s->err, hipStreamSynchronize(s->stream));
        tb3 = std::chrono::steady_clock::now();
        if (prof) { double sw = 0, swmax = 0, rot = 0, cut = 0, cy[3] = {0, 0, 0}; for (int q = 0; q < nfin; ++q) { const double* fo = (const double*)B.h_out.get() + (size_t)q * MF_OUT; sw += fo[MF_OUT_S + 1]; swmax = std::max(swmax, fo[MF_OUT_S + 1]); rot += fo[MF_OUT_S + 2]; cut += fo[MF_OUT_S + 3]; for (int k = 0; k < 3; ++k) cy[k] += fo[MF_OUT_S + 4 + k]; }
                    std::fprintf(stderr, "[uvs_marginalize_batch] k_marg_finish: %.1f Jacobi sweeps (most: %.0f), %.0f rotations, %.1f eigenvalues cut per window (mean over %d); shader-clock cycles per window: first rotation parameters of the sweeps %.0f k, A passes %.0f k, V passes (beside the next step's parameters) %.0f k\n",
                                 sw / nfin, swmax, rot / nfin, cut / nfin, nfin, cy[0] / nfin * 1e-3, cy[1] / nfin * 1e-3, cy[2] / nfin * 1e-3); }
        for (int q = 0; q < nfin; ++q) {
            const int b = slot_win[q]; MargBatchItem& it = items[b];
            const double* fo = (const double*)B.h_out.get() + (size_t)q * MF_OUT;
            const int st = (int)fo[MF_OUT_S];
            if (q < n1 && (h_scal[8 * q + 1] != 0.0 || !std::isfinite(h_scal[8 * q]))) { it.path = 3; continue; }      // a landmark block the reference's eps cut would touch: the host path applies that cut
            if (st == MF_NONFINITE) { it.rc = UVS_ERR_NUMERIC; it.err = "marginalization: the linearized system is not finite"; it.path = 0; continue; }
            if (st != MF_OK) { it.path = 3; continue; }
            uvs_prior* po = &out[b];
            std::memset(po, 0, sizeof(*po));
            po->n = it.n;
            std::memcpy(po->linearized_jacobians, fo + MF_OUT_J, (size_t)it.n * it.n * 8);
            std::memcpy(po->linearized_residuals, fo + MF_OUT_R, (size_t)it.n * 8);
            marg_fill_blocks(po, it.pos, it.keep_ids, it.md, ws[b], flags[b]);
            it.path = 0;
        }
    }
    // ---- the windows the device path did not take
    int first_bad = UVS_OK;
    for (int b = 0; b < n_win; ++b) {
        MargBatchItem& it = items[b];
        if (it.path == 3) { it.rc = uvs_marginalize(s, ws[b], flags[b], &out[b]); if (it.rc != UVS_OK) it.err = s->err; }
        if (status) status[b] = it.rc;
        if (it.rc != UVS_OK && first_bad == UVS_OK) { first_bad = it.rc; s->err = it.err; }
    }
    if (prof) {
        auto us = [](auto a_, auto b_) { return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(b_ - a_).count() * 1e-3; };
        int n_fb = 0; for (int b = 0; b < n_win; ++b) n_fb += items[b].path == 3 ? 1 : 0;
        std::fprintf(stderr, "[uvs_marginalize_batch] %d windows on %d threads: host stage (sub-windows, packing, prior-only systems) %.0f us, staging + enqueue %.0f us, device (copies, k_marg_linearize_batch x %d, k_marg_finish x %d) %.0f us, priors + one-window fallbacks (%d) %.0f us\n",
                     n_win, nthreads, us(tb0, tb1), us(tb1, tb2), us(tb2, tb3), n1_prof, nfin_prof, n_fb, us(tb3, std::chrono::steady_clock::now()));
    }
    return first_bad;
}

// Defined here, where the marginalization types a handle owns are complete.
uvs_solver::uvs_solver() = default;
uvs_solver::~uvs_solver() {
    for (hipEvent_t e : {ev_done, ev0, ev1}) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
}
