// uvs_large.hip -- the large single window (configs[3]) of the C ABI (include/uvs_solver.h) on the handle of uvs_solver_handle.h, landmark-sharded over the compute units and
// optionally over several GPUs: the step-wise calls (uvs_large_begin ... uvs_large_finish, the caller all-reduces between them), form 1 of uvs_debug_step, the RCCL communicator
// and the fused loop (uvs_large_solve_fused).  Kernels of this unit: the 256-thread k_large_* (uvs_large_kernel.h); k_large_chunks and k_large_solve also exist with 512 threads
// in uvs_solve512.hip, which is what the handle launches by default.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <dlfcn.h>

#define UVS_UNIT large256
#include "uvs_solver_handle.h"
#include "uvs_large_kernel.h"

using namespace uvsdev;

// the 512-thread instantiations of k_large_chunks and k_large_solve (uvs_solve512.hip)
extern "C" {
int uvs_k_large_chunks512_prof(long long* out, size_t n);
int uvs_k_large_solve512_launch(hipStream_t stream, char* blob, double* ws, const void* kopts, size_t kopts_bytes, double* state, const double* reduced, int first, double radius, double* out,
                                 const double* ctl, int rank, int nranks, const double* fimg);
int uvs_k_large_chunks512_launch(int grid, hipStream_t stream, char* blob, double* ws, const void* kopts, size_t kopts_bytes, const double* state, int sel, int first, double radius,
                                  double* partials, const double* ctl, int rank, int nranks, int n_chunk_wgs, double* fimg);
}

int large_unit_init(const unsigned char* fa, const unsigned char* fb, int n) {
    return unit_init(fa, fb, n, {(const void*)k_large_chunks, (const void*)k_large_solve, (const void*)k_large_backsub});
}

// ------------------------------------------------------------------ large single window (configs[3]), optionally multi-GPU
// What uvs_large_begin and uvs_large_solve_fused do once the window is uploaded: a fresh run state, the buffers of the loop, ||x||^2.
static int large_prologue(uvs_solver* s, const uvs_window* w) {
    auto& L = s->L; auto& LB = s->LB; const DevWin& h = s->hdrs[0];
    L = {};      // (the buffers and the communicator in LB stay)
    L.n_chunks = h.n_chunks; L.radius = s->opts.initial_trust_region_radius;
    L.grid = std::min(h.n_chunks, s->chunk_wgs());
    const std::pair<DevBuf<double>*, size_t> bufs[] = {{&LB.d_state, LG_STATE}, {&LB.d_reduced, LG_XCH_ALL}, {&LB.d_out, 64}, {&LB.d_sc5, 8}, {&LB.d_fimg, LG_FIMG},
                                                       {&LB.d_partials, (size_t)std::max(L.grid, 1) * LG_ROW}, {&LB.d_bsums, (size_t)std::max(L.n_chunks, 1) * 8}};      // doubles
    for (const auto& b : bufs) if (const int rc = b.first->ensure(b.second * 8, s->err)) return rc;
    double x2 = 0.0, l2 = 0.0;      // ||x||^2: frames (identical on every rank) and this rank's landmarks (summed over the ranks by the first all-reduce)
    for (int f = 0; f < UVS_NUM_FRAMES; ++f) { for (int k = 0; k < 7; ++k) x2 += w->pose[f][k] * w->pose[f][k]; for (int k = 0; k < 9; ++k) x2 += w->speedbias[f][k] * w->speedbias[f][k]; }
    if (s->opts.estimate_td) x2 += w->td * w->td;
    if (s->opts.estimate_extrinsic) for (int k = 0; k < 7; ++k) x2 += w->ex_pose[k] * w->ex_pose[k];
    if (w->n_relo_obs > 0) for (int k = 0; k < 7; ++k) x2 += w->relo_pose[k] * w->relo_pose[k];      // relo_Pose is a free block of the problem (estimator.cpp:947)
    for (int k = 0; k < w->n_points; ++k) l2 += w->inv_depth[k] * w->inv_depth[k];
    for (int k = 0; k < 4 * w->n_lines; ++k) l2 += w->line_orth[k] * w->line_orth[k];
    L.local_x2 = l2; L.x_norm = std::sqrt(x2 + l2); L.frame_x2 = x2;
    std::memcpy(L.relo_pose_in, w->relo_pose, sizeof(L.relo_pose_in));
    return UVS_OK;
}

// Step-wise so that the caller can all-reduce the two device vectors between steps (RCCL through torch.distributed in
// bench.py / api.py; nothing to reduce on one GPU):
//   uvs_large_begin -> loop { uvs_large_linearize -> [all-reduce SUM of uvs_large_reduced()] -> uvs_large_step
//                             -> [all-reduce SUM of uvs_large_scalars()] -> uvs_large_decide } -> uvs_large_finish
extern "C" {

int uvs_large_set_nranks(uvs_solver* s, int nranks) {
    if (!s || nranks < 1) return UVS_ERR_INVALID_ARG;
    s->LB.step_nranks = nranks;
    return UVS_OK;
}

int uvs_large_begin(uvs_solver* s, const uvs_window* w) {
    if (!s || !w) return UVS_ERR_INVALID_ARG;
    // the fused form's rule (uvs_large_solve_fused): a shard cannot tell whether relo_Pose is a free block of the all-reduced system, and the relo2 tail of the
    // reduced vector is not exchanged
    if (s->LB.step_nranks > 1 && w->n_relo_obs > 0) { s->L.active = false; s->err = "relocalization blocks are not taken by a landmark-sharded solve over several ranks"; return UVS_ERR_UNSUPPORTED; }
    const uvs_window* arr[1] = {w};
    int rc = upload_windows(s, 1, arr, true, s->chunk_wgs(), false, s->LB.step_nranks > 1);
    if (rc != UVS_OK) return rc;
    const bool fresh = !s->LB.d_reduced;      // (zeroed once, when it is first allocated)
    if ((rc = large_prologue(s, w)) != UVS_OK) return rc;
    auto& L = s->L; auto& LB = s->LB; const DevWin& h = s->hdrs[0];
    L.active = true;
    if (fresh) UVS_HIP(s->err, hipMemset(LB.d_reduced, 0, LG_XCH_ALL * 8));
    UVS_HIP(s->err, hipMemsetAsync(LB.d_state, 0, LG_STATE * 8, s->stream));
    // frames -> state.X ; landmark parameters -> workspace buffer 0 (device-to-device from the blob)
    UVS_HIP(s->err, hipMemcpyAsync(LB.d_state + LS_X, s->d_blobs + (size_t)h.d_frames * 8, UVS_XDIM * 8, hipMemcpyDeviceToDevice, s->stream));
    if (h.n_points) UVS_HIP(s->err, hipMemcpyAsync(s->d_ws + h.w_invd0, s->d_blobs + (size_t)h.d_invd * 8, (size_t)h.n_points * 8, hipMemcpyDeviceToDevice, s->stream));
    if (h.n_lines) UVS_HIP(s->err, hipMemcpyAsync(s->d_ws + h.w_line0, s->d_blobs + (size_t)h.d_line * 8, (size_t)h.n_lines * 32, hipMemcpyDeviceToDevice, s->stream));
    UVS_HIP(s->err, hipStreamSynchronize(s->stream));
    L.t_begin = std::chrono::steady_clock::now();
    return UVS_OK;
}

// landmark part of ||x||^2 of THIS rank (sum over ranks + frames gives Ceres' x_norm^2); set the global value with uvs_large_set_landmark_x2
double uvs_large_local_x2(const uvs_solver* s) { return s ? s->L.local_x2 : 0.0; }
void uvs_large_set_landmark_x2(uvs_solver* s, double all_ranks_x2) { if (s) { auto& L = s->L; L.x_norm = std::sqrt(L.x_norm * L.x_norm - L.local_x2 + all_ranks_x2); L.local_x2 = all_ranks_x2; } }

int uvs_large_need_linearize(const uvs_solver* s) { return s && s->L.active && !s->L.done && s->L.need_lin; }
int uvs_large_done(const uvs_solver* s) { return !s || !s->L.active || s->L.done; }
double* uvs_large_reduced(uvs_solver* s, int* n) { if (n) *n = LG_RED; return s ? s->LB.d_reduced.get() : nullptr; }     // DEVICE pointer; [LG_ACC+1] is a MAX entry
double* uvs_large_scalars(uvs_solver* s, int* n) { if (n) *n = 6; return s ? s->LB.d_sc5.get() : nullptr; }             // DEVICE pointer; [5] = this rank's "time is up" vote (SUM over ranks > 0 ends the solve on every rank)

// host-staged access to the two exchange vectors (which = 0: reduced[LG_RED], 1: scalars[5]); set != 0 writes host -> device
int uvs_large_exchange_host(uvs_solver* s, int which, double* buf, int set) {
    if (!s || !s->L.active || !buf) return UVS_ERR_INVALID_ARG;
    double* d = which == 0 ? s->LB.d_reduced.get() : s->LB.d_sc5.get(); const size_t n = which == 0 ? LG_RED : 6;
    UVS_HIP(s->err, hipSetDevice(s->device));
    if (set) UVS_HIP(s->err, hipMemcpy(d, buf, n * 8, hipMemcpyHostToDevice)); else UVS_HIP(s->err, hipMemcpy(buf, d, n * 8, hipMemcpyDeviceToHost));
    return UVS_OK;
}

int uvs_large_linearize(uvs_solver* s) {
    if (!s || !s->L.active) return UVS_ERR_INVALID_ARG;
    auto& L = s->L; auto& LB = s->LB;
    UVS_HIP(s->err, hipSetDevice(s->device));
    KOpts ko = make_kopts(s->opts, 0);
    if (s->large_chunks_nt == 512) { if (uvs_k_large_chunks512_launch(L.grid + 1, s->stream, s->d_blobs, s->d_ws, &ko, sizeof(ko), LB.d_state, L.sel, L.first ? 1 : 0, L.radius, LB.d_partials, nullptr, 0, 0, L.grid, LB.d_fimg) != UVS_OK) { s->err = "k_large_chunks (512 threads): argument layout mismatch"; return UVS_ERR_HIP; } }
    else hipLaunchKernelGGL(k_large_chunks, dim3(L.grid + 1), dim3(NT), LDS_BYTES, s->stream, s->d_blobs, s->d_ws, ko, LB.d_state, L.sel, L.first ? 1 : 0, L.radius, LB.d_partials, LargeCtl{nullptr, 0, 0}, L.grid, LB.d_fimg);
    { const int n_ent = s->hdrs[0].relo2 ? LG_ROW : LG_RED; hipLaunchKernelGGL(k_large_reduce, dim3((n_ent + 15) / 16), dim3(256), 0, s->stream, LB.d_partials, L.grid, LB.d_reduced, LargeCtl{nullptr, 0, 0}, n_ent); }
    UVS_HIP(s->err, hipGetLastError());
    UVS_HIP(s->err, hipStreamSynchronize(s->stream));
    return UVS_OK;
}

int uvs_large_step(uvs_solver* s) {
    if (!s || !s->L.active) return UVS_ERR_INVALID_ARG;
    auto& L = s->L; auto& LB = s->LB;
    UVS_HIP(s->err, hipSetDevice(s->device));
    KOpts ko = make_kopts(s->opts, 0);
    if (s->large_solve_nt == 512) { if (uvs_k_large_solve512_launch(s->stream, s->d_blobs, s->d_ws, &ko, sizeof(ko), LB.d_state, LB.d_reduced, L.first ? 1 : 0, L.radius, LB.d_out, nullptr, 0, 0, LB.d_fimg) != UVS_OK) { s->err = "k_large_solve (512 threads): argument layout mismatch"; return UVS_ERR_HIP; } }
    else hipLaunchKernelGGL(k_large_solve, dim3(1), dim3(NT), LDS_BYTES, s->stream, s->d_blobs, s->d_ws, ko, LB.d_state, LB.d_reduced, L.first ? 1 : 0, L.radius, LB.d_out, LargeCtl{nullptr, 0, 0}, LB.d_fimg);
    L.stored = LB.debug_step;
    { const int bg = std::min(L.n_chunks, UVS_LARGE_OCC * s->chunk_wgs()); L.backsub_wgs = bg;      // (UVS_LARGE_OCC workgroups per compute unit: the kernel asks for little LDS and half the registers)
      if (LB.debug_step) {      // diagnostic (uvs_large_set_debug_step): the storing instantiation of the same body
          const DevWin& h = s->hdrs[0];
          const size_t n = (size_t)UVS_DSTEP_FR + (size_t)h.n_points + 4 * (size_t)h.n_lines;
          if (const int rc = LB.d_lstep.ensure(n * 8, s->err)) return rc;
          UVS_HIP(s->err, hipMemsetAsync(LB.d_lstep, 0, n * 8, s->stream));
          if (L.n_chunks == 0) UVS_HIP(s->err, hipMemcpyAsync(LB.d_lstep, LB.d_state + LS_DLT, UVS_RD * 8, hipMemcpyDeviceToDevice, s->stream));      // no landmark chunk, no back-substitution: the frame step as k_large_solve left it
          hipLaunchKernelGGL(k_large_backsub_dstep, dim3(bg + 1), dim3(NT), LDS_BYTES_BACKSUB, s->stream, s->d_blobs, s->d_ws, ko, LB.d_state, L.sel, LB.d_bsums, LargeCtl{nullptr, 0, 0}, bg, LB.d_out, LB.d_lstep.get());
      } else
      hipLaunchKernelGGL(k_large_backsub, dim3(bg + 1), dim3(NT), LDS_BYTES_BACKSUB, s->stream, s->d_blobs, s->d_ws, ko, LB.d_state, L.sel, LB.d_bsums, LargeCtl{nullptr, 0, 0}, bg, LB.d_out); }
    hipLaunchKernelGGL(k_large_sum_bsums, dim3(1), dim3(256), 0, s->stream, LB.d_bsums, L.n_chunks, LB.d_sc5, LargeCtl{nullptr, 0, 0}, 0LL);
    UVS_HIP(s->err, hipGetLastError());
    UVS_HIP(s->err, hipStreamSynchronize(s->stream));
    // options.max_solver_time_in_seconds on the host-driven loop: this process's vote travels as scalar [5], so that ranks which all-reduce the scalars decide together
    const uvs_options& o = s->opts;
    const double vote = (o.max_solver_time_in_seconds > 0.0 && L.it > 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - L.t_begin).count() >= o.max_solver_time_in_seconds) ? 1.0 : 0.0;
    if (o.max_solver_time_in_seconds > 0.0) UVS_HIP(s->err, hipMemcpy(LB.d_sc5 + 5, &vote, 8, hipMemcpyHostToDevice));
    return UVS_OK;
}

// The scalars of one step: the frame part (k_large_solve, identical on every rank) plus the landmark sums of the ranks.  uvs_large_decide and uvs_large_debug_step read them here.
struct LargeStepScal { double gd, dd2, step2, xc2, mcc, cand; };
static LargeStepScal large_step_scalars(const double* out, const double* sc) {
    LargeStepScal v;
    v.gd = out[LO_GD] + sc[0]; v.dd2 = out[LO_DD2] + sc[1]; v.step2 = out[LO_STEP2] + sc[2]; v.xc2 = out[LO_XC2] + sc[3];
    v.mcc = 0.5 * (v.dd2 - v.gd);
    v.cand = out[LO_FRAMECOST] + sc[4];
    return v;
}

// Host side of the trust-region loop (same order of tests as k_solve / SURVEY.md Appendix B).  Call after uvs_large_step (and after the
// caller all-reduced uvs_large_scalars()).  Note: on this path a (re)linearization is implied by need_lin BEFORE the next step.
int uvs_large_decide(uvs_solver* s) {
    if (!s || !s->L.active) return UVS_ERR_INVALID_ARG;
    auto& L = s->L; auto& LB = s->LB; const uvs_options& o = s->opts;
    double out[LO_N + 8], sc[6];
    UVS_HIP(s->err, hipMemcpy(out, LB.d_out, sizeof(double) * (LO_N + 4), hipMemcpyDeviceToHost));
    UVS_HIP(s->err, hipMemcpy(sc, LB.d_sc5, sizeof(sc), hipMemcpyDeviceToHost));
    uvs_report& rep = L.rep;
    const double lc = out[LO_COST]; const double gm = out[LO_GMAX];
    if (L.first) {
        L.cost = lc; L.gmax = gm; L.first = false;
        rep.initial_cost = lc; rep.cost[0] = lc; rep.radius[0] = L.radius; rep.gradient_max_norm[0] = gm; rep.accepted[0] = 1;
        if (!std::isfinite(lc)) { L.term = UVS_TERM_NUMERIC_FAILURE; L.status = UVS_ERR_NUMERIC; L.done = true; return UVS_OK; }
    } else if (L.pending > 0) { L.cost = lc; L.gmax = gm; rep.cost[L.pending] = lc; rep.gradient_max_norm[L.pending] = gm; }
    L.pending = 0; L.need_lin = false;
    if (L.it >= o.max_num_iterations) { L.term = UVS_TERM_NO_CONVERGENCE; L.done = true; return UVS_OK; }
    if (o.max_solver_time_in_seconds > 0.0 && L.it > 0 && sc[5] > 0.0) {      // the host's clock, read in uvs_large_step; the vote is part of the scalars the ranks all-reduce, so every rank stops at the same iteration
        L.term = UVS_TERM_MAX_TIME; L.done = true; return UVS_OK;
    }
    if (L.gmax <= o.gradient_tolerance) { L.term = UVS_TERM_GRADIENT_TOL; L.done = true; return UVS_OK; }
    if (L.radius <= o.min_trust_region_radius) { L.term = UVS_TERM_MIN_RADIUS; L.done = true; return UVS_OK; }
    ++L.it;
    const int ti = L.it < UVS_MAX_ITER ? L.it : UVS_MAX_ITER;
    const LargeStepScal ss = large_step_scalars(out, sc);
    const double step2 = ss.step2, xc2 = ss.xc2, mcc = ss.mcc;
    double cand = ss.cand;
    bool ok = out[LO_CHOLOK] != 0.0 && std::isfinite(mcc) && std::isfinite(step2);
    rep.model_cost_change[ti] = mcc;
    if (!ok || !(mcc > 0.0)) {
        ++L.invalid; L.radius /= L.decr; L.decr *= 2.0; L.need_lin = true;
        rep.accepted[ti] = -1; rep.cost[ti] = L.cost; rep.candidate_cost[ti] = L.cost; rep.radius[ti] = L.radius; rep.gradient_max_norm[ti] = L.gmax;
        if (L.invalid >= o.max_consecutive_invalid_steps) { L.term = UVS_TERM_INVALID_STEPS; L.done = true; }
        return UVS_OK;
    }
    L.invalid = 0;
    if (!std::isfinite(cand)) cand = 1.7976931348623157e308;
    const double step_norm = std::sqrt(step2), rel = (L.cost - cand) / mcc;
    const bool successful = rel > o.min_relative_decrease;
    rep.candidate_cost[ti] = cand; rep.step_norm[ti] = step_norm; rep.relative_decrease[ti] = rel; rep.cost[ti] = L.cost; rep.radius[ti] = L.radius; rep.gradient_max_norm[ti] = L.gmax;
    bool stop = false;
    if (step_norm <= o.parameter_tolerance * (L.x_norm + o.parameter_tolerance)) { L.term = UVS_TERM_PARAMETER_TOL; stop = true; }
    else if (std::fabs(L.cost - cand) <= o.function_tolerance * L.cost) { L.term = UVS_TERM_FUNCTION_TOL; stop = true; }
    if (stop && !(o.function_tol_keeps_candidate && successful)) { L.done = true; return UVS_OK; }
    if (successful) {
        UVS_HIP(s->err, hipMemcpyAsync(LB.d_state + LS_X, LB.d_state + LS_XC, UVS_XDIM * 8, hipMemcpyDeviceToDevice, s->stream));   // stream-ordered with the next launch (a plain D2D hipMemcpy
        // runs on the null stream, which this non-blocking stream does not wait for)
        L.sel ^= 1; ++L.nsucc; L.x_norm = std::sqrt(xc2);
        L.radius = L.radius / std::fmax(1.0 / 3.0, 1.0 - std::pow(2.0 * rel - 1.0, 3.0));
        L.radius = std::fmin(o.max_trust_region_radius, L.radius); L.decr = 2.0;
        L.cost = cand; L.need_lin = true; L.pending = ti;
        rep.accepted[ti] = 1; rep.cost[ti] = L.cost; rep.radius[ti] = L.radius;
        if (stop || L.it >= o.max_num_iterations) { if (!stop) L.term = UVS_TERM_NO_CONVERGENCE; L.done = true; }
    } else {
        L.radius /= L.decr; L.decr *= 2.0; L.need_lin = true;
        rep.accepted[ti] = 0; rep.radius[ti] = L.radius;
        if (L.it >= o.max_num_iterations) { L.term = UVS_TERM_NO_CONVERGENCE; L.done = true; }
    }
    return UVS_OK;
}

int uvs_large_set_debug_step(uvs_solver* s, int on) {
    if (!s) return UVS_ERR_INVALID_ARG;
    s->LB.debug_step = on != 0;
    return UVS_OK;
}

// padded device layout of a stored step -> the ABI's: frames (16 f + dof, dof < 15), extrinsic, td, relo_Pose, landmarks
static void dstep_to_abi(const double* r, long long n_lm, bool ex, bool td, bool relo, double* d) {
    long long j = 0;
    for (int f = 0; f < UVS_NF; ++f) for (int a = 0; a < 15; ++a) d[j++] = r[16 * f + a];
    if (ex) for (int a = 0; a < 6; ++a) d[j++] = r[UVS_EX_INDEX(a)];
    if (td) d[j++] = r[UVS_TD_INDEX];
    if (relo) for (int a = 0; a < 6; ++a) d[j++] = r[16 * UVS_RELO_FRAME + a];
    std::memcpy(d + j, r + UVS_DSTEP_FR, sizeof(double) * (size_t)n_lm);
}
static long long dstep_len(const uvs_options& o, int n_points, int n_lines, bool relo) {
    return 165 + (o.estimate_extrinsic ? 6 : 0) + (o.estimate_td ? 1 : 0) + (relo ? 6 : 0) + (long long)n_points + 4LL * n_lines;
}

int uvs_large_debug_step(uvs_solver* s, double next_radius, int n_step, double* step, double* scal) {
    if (!s || !s->L.active || !step || !scal) { if (s) s->err = "uvs_large_debug_step: null pointer or no step-wise solve in progress"; return UVS_ERR_INVALID_ARG; }
    auto& L = s->L; auto& LB = s->LB; const DevWin& h = s->hdrs[0];
    if (!LB.debug_step || !L.stored || !LB.d_lstep) { s->err = "uvs_large_debug_step: uvs_large_set_debug_step(1) and one uvs_large_step come first"; return UVS_ERR_INVALID_ARG; }
    if (std::isnan(next_radius) || std::isinf(next_radius) || next_radius < 0.0) { s->err = "uvs_large_debug_step: the next radius must be finite and >= 0"; return UVS_ERR_INVALID_ARG; }
    const bool relo = h.relo_on != 0;
    if ((long long)n_step != dstep_len(s->opts, h.n_points, h.n_lines, relo)) { s->err = "uvs_large_debug_step: step length does not match the layout"; return UVS_ERR_INVALID_ARG; }
    const size_t n_lm = (size_t)h.n_points + 4 * (size_t)h.n_lines;
    std::vector<double> raw(UVS_DSTEP_FR + n_lm);
    double out[LO_N + 8], sc[6];
    UVS_HIP(s->err, hipSetDevice(s->device));
    UVS_HIP(s->err, hipMemcpy(raw.data(), LB.d_lstep, raw.size() * 8, hipMemcpyDeviceToHost));
    UVS_HIP(s->err, hipMemcpy(out, LB.d_out, sizeof(double) * (LO_N + 4), hipMemcpyDeviceToHost));
    UVS_HIP(s->err, hipMemcpy(sc, LB.d_sc5, sizeof(sc), hipMemcpyDeviceToHost));
    dstep_to_abi(raw.data(), (long long)n_lm, s->opts.estimate_extrinsic != 0, s->opts.estimate_td != 0, relo, step);
    const LargeStepScal ss = large_step_scalars(out, sc);
    std::memset(scal, 0, sizeof(double) * UVS_DEBUG_SCAL_LEN);
    scal[0] = out[LO_COST]; scal[1] = out[LO_GMAX]; scal[2] = out[LO_CHOLOK]; scal[3] = ss.mcc; scal[4] = ss.step2;
    scal[5] = L.n_chunks; scal[6] = L.grid; scal[7] = L.backsub_wgs;      // the launch geometry this step really ran with
    if (next_radius > 0.0) { L.first = false; L.radius = next_radius; L.need_lin = true; }      // what uvs_large_decide does to a rejected step, at the caller's radius
    return UVS_OK;
}

}  // extern "C"

// uvs_debug_step, form 1: the step-wise calls themselves with the storing back-substitution, each radius handled as a rejection of the one before
int debug_step_large(uvs_solver* s, const uvs_window* w, int n_radii, const double* radii, int n_step, double* step, double* scal) {
    const bool was = s->LB.debug_step;
    s->LB.debug_step = true;
    int rc = uvs_large_begin(s, w);      // (refuses relocalization blocks when uvs_large_set_nranks announced several ranks)
    if (rc == UVS_OK) s->L.radius = radii[0];
    for (int k = 0; k < n_radii && rc == UVS_OK; ++k) {
        if ((rc = uvs_large_linearize(s)) != UVS_OK) break;
        if ((rc = uvs_large_step(s)) != UVS_OK) break;
        rc = uvs_large_debug_step(s, k + 1 < n_radii ? radii[k + 1] : 0.0, n_step, step + (size_t)k * n_step, scal + (size_t)k * UVS_DEBUG_SCAL_LEN);
    }
    s->LB.debug_step = was; s->L.active = false;
    return rc;
}

extern "C" {

int uvs_large_finish(uvs_solver* s, uvs_state* out, uvs_report* rep) {
    if (!s || !s->L.active || !out || !rep) return UVS_ERR_INVALID_ARG;
    auto& L = s->L; auto& LB = s->LB; const DevWin& h = s->hdrs[0];
    L.rep.status = L.status; L.rep.termination = L.term; L.rep.num_iterations = L.it; L.rep.num_successful = L.nsucc; L.rep.final_cost = L.cost;
    *rep = L.rep;
    double fr[UVS_XDIM];
    UVS_HIP(s->err, hipMemcpy(fr, LB.d_state + LS_X, sizeof(fr), hipMemcpyDeviceToHost));
    std::memcpy(out->pose, fr, 77 * 8); std::memcpy(out->speedbias, fr + 77, 99 * 8); std::memcpy(out->ex_pose, fr + 176, 7 * 8); out->td = fr[183];
    std::memcpy(out->relo_pose, fr + 184, sizeof(out->relo_pose));      // optimized when the window carries relocalization blocks, the input value otherwise
    if (out->inv_depth && h.n_points) UVS_HIP(s->err, hipMemcpy(out->inv_depth, s->d_ws + (L.sel ? h.w_invd1 : h.w_invd0), (size_t)h.n_points * 8, hipMemcpyDeviceToHost));
    if (out->line_orth && h.n_lines) UVS_HIP(s->err, hipMemcpy(out->line_orth, s->d_ws + (L.sel ? h.w_line1 : h.w_line0), (size_t)h.n_lines * 32, hipMemcpyDeviceToHost));
    L.active = false;
    return L.status;
}

// single-GPU convenience: the loop above with nothing to all-reduce; elapsed_ms (may be NULL) = wall time of the loop
int uvs_large_solve(uvs_solver* s, const uvs_window* w, uvs_state* out, uvs_report* rep) {
    if (!s) return UVS_ERR_INVALID_ARG;
    // one process, nothing exchanged: the rank count of the step-wise form (uvs_large_set_nranks) does not apply, and stays set for the next step-wise solve
    const int nr = s->LB.step_nranks; s->LB.step_nranks = 1;
    int rc = uvs_large_begin(s, w);
    s->LB.step_nranks = nr;
    if (rc != UVS_OK) return rc;
    while (!uvs_large_done(s)) {
        if (uvs_large_need_linearize(s)) { if ((rc = uvs_large_linearize(s)) != UVS_OK) return rc; }
        if ((rc = uvs_large_step(s)) != UVS_OK) return rc;
        if ((rc = uvs_large_decide(s)) != UVS_OK) return rc;
    }
    return uvs_large_finish(s, out, rep);
}


// ---------------------------------------------------------------- fused loop: RCCL communicator owned by the handle, control on the device
// RCCL is resolved at run time (dlopen): the library itself carries no dependency on it, a process that already holds RCCL (PyTorch)
// shares that copy.  UVS_RCCL_LIB overrides the search.
namespace {
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, uvs_rccl_id, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    std::string err;
};
RcclApi& rccl() {
    static RcclApi api;
    if (api.lib || !api.err.empty()) return api;
    const char* env = std::getenv("UVS_RCCL_LIB");
    if (env && *env) api.lib = dlopen(env, RTLD_NOW);            // an explicit library is taken as given, even when the process already holds another RCCL (PyTorch's)
    else {
        const char* names[2] = {"librccl.so.1", "librccl.so"};
        for (int pass = 0; pass < 2 && !api.lib; ++pass)          // first a copy that is already loaded, then a fresh one
            for (const char* n : names) { api.lib = dlopen(n, RTLD_NOW | (pass == 0 ? RTLD_NOLOAD : 0)); if (api.lib) break; }
    }
    if (!api.lib) { api.err = "RCCL not found (librccl.so / librccl.so.1; set UVS_RCCL_LIB)"; return api; }
    api.GetUniqueId = (int (*)(void*))dlsym(api.lib, "ncclGetUniqueId");
    api.CommInitRank = (int (*)(void**, int, uvs_rccl_id, int))dlsym(api.lib, "ncclCommInitRank");
    api.CommDestroy = (int (*)(void*))dlsym(api.lib, "ncclCommDestroy");
    api.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(api.lib, "ncclAllReduce");
    api.GetErrorString = (const char* (*)(int))dlsym(api.lib, "ncclGetErrorString");
    if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllReduce) { api.err = "RCCL symbols missing"; api.lib = nullptr; }
    return api;
}
constexpr int kNcclDouble = 8, kNcclSum = 0;      // rccl.h: ncclFloat64 = 8, ncclSum = 0
}  // namespace

int uvs_large_comm_unique_id(uvs_rccl_id* id) {
    if (!id) return UVS_ERR_INVALID_ARG;
    RcclApi& r = rccl();
    if (!r.lib) return UVS_ERR_UNSUPPORTED;
    return r.GetUniqueId(id) == 0 ? UVS_OK : UVS_ERR_HIP;
}

int uvs_large_comm_init(uvs_solver* s, int nranks, int rank, const uvs_rccl_id* id) {
    if (!s || nranks < 1 || nranks > LG_MAXRANKS || rank < 0 || rank >= nranks || (nranks > 1 && !id)) return UVS_ERR_INVALID_ARG;
    auto& LB = s->LB;
    uvs_large_comm_destroy(s);
    LB.rank = rank; LB.nranks = nranks;
    if (nranks == 1 && !id) return UVS_OK;                        // nothing to exchange (with an id a one-rank communicator is built all the same: exercises the RCCL path on one GPU)
    RcclApi& r = rccl();
    if (!r.lib) { s->err = r.err; return UVS_ERR_UNSUPPORTED; }
    UVS_HIP(s->err, hipSetDevice(s->device));
    const int rc = r.CommInitRank(&LB.comm, nranks, *id, rank);
    if (rc != 0) { s->err = std::string("ncclCommInitRank: ") + (r.GetErrorString ? r.GetErrorString(rc) : "error"); LB.comm = nullptr; LB.nranks = 1; LB.rank = 0; return UVS_ERR_HIP; }
    return UVS_OK;
}

void uvs_large_comm_destroy(uvs_solver* s) {
    if (!s) return;
    auto& LB = s->LB;
    if (LB.comm) { (void)hipSetDevice(s->device); rccl().CommDestroy(LB.comm); LB.comm = nullptr; }
    LB.rank = 0; LB.nranks = 1;
}

// Error inside the enqueue loop of the fused solve: drain what is already on the stream and leave the handle idle.  With several ranks the
// peers are still inside their collective -- the communicator must be considered broken afterwards (uvs_large_comm_destroy + re-init).
static int fused_abort(uvs_solver* s, const char* what) {
    (void)hipStreamSynchronize(s->stream);
    s->L.active = false;
    s->err = what;
    return UVS_ERR_HIP;
}

// ONE large window, landmark-sharded over the ranks of the handle's communicator (`w` = this rank's landmarks, frames / IMU / prior
// replicated), the whole Levenberg-Marquardt loop enqueued on the handle's stream without a host round trip: per iteration
//   k_large_chunks -> k_large_reduce -> ncclAllReduce(reduced, SUM, in place) -> k_large_solve -> k_large_backsub -> k_large_sum_bsums
//   -> ncclAllReduce(5 scalars) -> k_large_decide
// Every rank decides on identical numbers, so all ranks follow the same path; kernels of iterations after termination return at once.
int uvs_large_solve_fused(uvs_solver* s, const uvs_window* w, uvs_state* out, uvs_report* rep, float* loop_ms) {
    if (!s || !w || !out || !rep) return UVS_ERR_INVALID_ARG;
    // ONE stream, ONE wait: pinned upload -> k_large_init -> the passes -> k_large_pack -> pinned download.  (The step-wise API keeps
    // uvs_large_begin's host-side copies; here every small copy / memset is a line of k_large_init.)
    const uvs_window* arr[1] = {w};
    int rc = upload_windows(s, 1, arr, false, s->chunk_wgs(), false, s->LB.nranks > 1);
    if (rc != UVS_OK) return rc;
    auto& L = s->L; auto& LB = s->LB; const DevWin& h = s->hdrs[0]; const uvs_options& o = s->opts;
    // relocalization blocks are per-landmark, so a landmark shard may hold none of them while the all-reduced system carries the other ranks' relo_Pose rows: a rank
    // cannot tell from its own shard whether relo_Pose is a free block.  Not taken by a multi-rank solve (NO rank may pass n_relo_obs > 0; one rank takes them).
    if (LB.nranks > 1 && w->n_relo_obs > 0) { s->err = "relocalization blocks are not taken by a landmark-sharded solve over several ranks"; return UVS_ERR_UNSUPPORTED; }
    if ((rc = large_prologue(s, w)) != UVS_OK) return rc;      // (inactive until work is enqueued, below: an allocation failure leaves the handle idle)
    constexpr int RD = (int)(sizeof(uvs_report) / 8);
    const size_t out_doubles = 64 + RD + UVS_XDIM + (size_t)h.n_points + 4 * (size_t)h.n_lines;
    if ((rc = LB.d_ctl.ensure(64 * 8, s->err)) != UVS_OK || (rc = LB.d_rep.ensure(sizeof(uvs_report), s->err)) != UVS_OK ||
        (rc = s->d_outpack.ensure(out_doubles * 8, s->err)) != UVS_OK || (rc = s->h_out.ensure(out_doubles * 8, s->err, grow_pinned)) != UVS_OK) return rc;
    L.active = true;
    hipLaunchKernelGGL(k_large_init, dim3(16), dim3(256), 0, s->stream, s->d_blobs, s->d_ws, LB.d_state, LB.d_ctl, LB.d_rep, LB.d_reduced, o.initial_trust_region_radius, L.frame_x2, L.local_x2);
    const char* lprof = std::getenv("UVS_LARGE_PROF");      // debug: per-workgroup timeline of the LAST k_large_chunks launch, written to this file
    const KOpts ko = make_kopts(o, lprof ? 7 : 0);
    const LargeCtl lc{LB.d_ctl, LB.rank, LB.nranks};
    RcclApi& r = rccl();
    const int passes = std::max(1, o.max_num_iterations);
    const int rows = L.grid;
    const int bgrid = std::min(L.n_chunks, UVS_LARGE_OCC * s->chunk_wgs());      // k_large_backsub runs UVS_LARGE_OCC workgroups per compute unit
    UVS_HIP(s->err, hipEventRecord(s->ev0, s->stream));
    for (int p = 0; p < passes; ++p) {
        if (s->large_chunks_nt == 512) { if (uvs_k_large_chunks512_launch(L.grid + 1, s->stream, s->d_blobs, s->d_ws, &ko, sizeof(ko), LB.d_state, 0, 0, 0.0, LB.d_partials, lc.ctl, lc.rank, lc.nranks, L.grid, LB.d_fimg) != UVS_OK) return fused_abort(s, "k_large_chunks (512 threads): argument layout mismatch"); }
        else hipLaunchKernelGGL(k_large_chunks, dim3(L.grid + 1), dim3(NT), LDS_BYTES, s->stream, s->d_blobs, s->d_ws, ko, LB.d_state, 0, 0, 0.0, LB.d_partials, lc, L.grid, LB.d_fimg);
        // (summing the partial rows inside k_large_solve instead of by a launch of its own was measured: one workgroup needs 15-24 us for what 314 do in 5)
        { const int n_ent = s->hdrs[0].relo2 ? LG_ROW : LG_RED; hipLaunchKernelGGL(k_large_reduce, dim3((n_ent + 15) / 16), dim3(256), 0, s->stream, LB.d_partials, rows, LB.d_reduced, lc, n_ent); }
        if (LB.comm) { const int e = r.AllReduce(LB.d_reduced, LB.d_reduced, LG_XCH, kNcclDouble, kNcclSum, LB.comm, s->stream); if (e != 0) return fused_abort(s, "ncclAllReduce(reduced) failed"); }
        if (s->large_solve_nt == 512) { if (uvs_k_large_solve512_launch(s->stream, s->d_blobs, s->d_ws, &ko, sizeof(ko), LB.d_state, LB.d_reduced, 0, 0.0, LB.d_out, lc.ctl, lc.rank, lc.nranks, LB.d_fimg) != UVS_OK) return fused_abort(s, "k_large_solve (512 threads): argument layout mismatch"); }
        else hipLaunchKernelGGL(k_large_solve, dim3(1), dim3(NT), LDS_BYTES, s->stream, s->d_blobs, s->d_ws, ko, LB.d_state, LB.d_reduced, 0, 0.0, LB.d_out, lc, LB.d_fimg);
        hipLaunchKernelGGL(k_large_backsub, dim3(bgrid + 1), dim3(NT), LDS_BYTES_BACKSUB, s->stream, s->d_blobs, s->d_ws, ko, LB.d_state, 0, LB.d_bsums, lc, bgrid, LB.d_out);
        if (LB.comm) {
            hipLaunchKernelGGL(k_large_sum_bsums, dim3(1), dim3(256), 0, s->stream, LB.d_bsums, L.n_chunks, LB.d_sc5, lc, ko.max_ticks);
            const int e = r.AllReduce(LB.d_sc5, LB.d_sc5, 8, kNcclDouble, kNcclSum, LB.comm, s->stream); if (e != 0) return fused_abort(s, "ncclAllReduce(step scalars) failed");
            hipLaunchKernelGGL(k_large_decide, dim3(1), dim3(256), 0, s->stream, LB.d_ctl, LB.d_state, LB.d_out, LB.d_sc5, LB.d_reduced, ko, LB.d_rep, (const double*)nullptr, 0);
        } else hipLaunchKernelGGL(k_large_decide, dim3(1), dim3(256), 0, s->stream, LB.d_ctl, LB.d_state, LB.d_out, LB.d_sc5, LB.d_reduced, ko, LB.d_rep, (const double*)LB.d_bsums, L.n_chunks);
    }
    UVS_HIP(s->err, hipEventRecord(s->ev1, s->stream));
    hipLaunchKernelGGL(k_large_pack, dim3(16), dim3(256), 0, s->stream, s->d_blobs, s->d_ws, LB.d_state, LB.d_ctl, LB.d_rep, s->d_outpack);
    UVS_HIP(s->err, hipGetLastError());
    UVS_HIP(s->err, hipMemcpyAsync(s->h_out, s->d_outpack, out_doubles * 8, hipMemcpyDeviceToHost, s->stream));
    UVS_HIP(s->err, hipStreamSynchronize(s->stream));
    if (loop_ms) UVS_HIP(s->err, hipEventElapsedTime(loop_ms, s->ev0, s->ev1));
    if (lprof) {
        std::vector<long long> tp(1024 * 8);
        if ((s->large_chunks_nt == 512 ? uvs_k_large_chunks512_prof(tp.data(), tp.size()) == UVS_OK : hipMemcpyFromSymbol(tp.data(), HIP_SYMBOL(g_large_prof), tp.size() * 8) == hipSuccess)) { if (FILE* f = std::fopen(lprof, "wb")) { const int hdr[2] = {L.grid + 1, L.n_chunks}; std::fwrite(hdr, 4, 2, f); std::fwrite(tp.data(), 8, tp.size(), f); std::fclose(f); } }
    }
    const double* ho = (const double*)s->h_out.get();
    const double* ctl = ho;
    L.active = false;
    const bool unterminated = ctl[LC_DONE] == 0.0;      // cannot happen since k_large_decide tests the iteration cap on every branch; if it ever does, the caller still gets the last accepted state
    L.sel = (int)ctl[LC_SEL]; L.it = (int)ctl[LC_IT]; L.nsucc = (int)ctl[LC_NSUCC]; L.term = (int)ctl[LC_TERM]; L.status = (int)ctl[LC_STATUS]; L.cost = ctl[LC_COST]; L.done = true;
    std::memcpy(rep, ho + 64, sizeof(uvs_report));
    if (unterminated) {
        L.status = UVS_ERR_NUMERIC; L.term = UVS_TERM_NO_CONVERGENCE;
        rep->status = L.status; rep->termination = L.term; rep->num_iterations = L.it; rep->num_successful = L.nsucc; rep->final_cost = L.cost;
        s->err = "fused large-window loop did not terminate within max_num_iterations passes";
    }
    L.rep = *rep;
    const double* fr = ho + 64 + RD;
    std::memcpy(out->pose, fr, 77 * 8); std::memcpy(out->speedbias, fr + 77, 99 * 8); std::memcpy(out->ex_pose, fr + 176, 7 * 8); out->td = fr[183];
    std::memcpy(out->relo_pose, fr + 184, sizeof(out->relo_pose));      // optimized when the window carries relocalization blocks, the input value otherwise
    if (out->inv_depth && h.n_points) std::memcpy(out->inv_depth, fr + UVS_XDIM, (size_t)h.n_points * 8);
    if (out->line_orth && h.n_lines) std::memcpy(out->line_orth, fr + UVS_XDIM + h.n_points, (size_t)h.n_lines * 32);
    return L.status;
}

}  // extern "C"
