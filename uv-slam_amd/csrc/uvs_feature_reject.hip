// uvs_feature_reject.hip -- the outlier rejection of the point front end (reference feature_tracker/src/feature_tracker.cpp:149-182 rejectWithF:
// cv::findFundamentalMat(.., FM_RANSAC, F_THRESHOLD, 0.99, status)) behind uvs_ft_reject of include/uvs_solver.h, whose comment is the statement
// of the numerics.  gfx950, on the tracker handle's stream (uvs_ft_handle.h).  It reads no image: one upload carries the item table and the packed
// normalized points, one download the keep masks and the result blocks.  Every FP64 operation is one of + - * / sqrt in the order the header
// gives, and this unit is compiled with -ffp-contract=off, so they round as written, which is what tests/fr_ref.py (the numpy restatement, the
// pin) does; the one log is in the stopping rule.
//
// One kernel, k_ft_reject_run<false> of uvs_ft_reject_kernel.h (the header it shares with csrc/uvs_relative_pose.hip, which describes it): a
// workgroup of 256 per item, a thread per hypothesis, in rounds of 256 hypotheses.  This file is the host side: the checks, the packing, the launch.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/uvs_solver.h"
#include "uvs_ft_handle.h"
#include "uvs_ft_reject_kernel.h"

using namespace uvsfr;

namespace {

// what uvs_ft_reject and uvs_ft_debug_reject share; dbg_*: every hypothesis of the ONE item
int fr_run(uvs_ft_tracker* h, const char* who_, int n_items, const uvs_ft_reject_item* items, double threshold, double confidence, uint8_t* keep,
           uvs_ft_reject_result* results, int32_t* dbg_samples, double* dbg_models, int32_t* dbg_counts) {
    const std::string fn = who_;
    h->err.clear();
    if (!items || !keep || !results) { h->err = fn + ": null pointer"; return UVS_ERR_INVALID_ARG; }
    if (n_items < 1 || n_items > h->max_streams) { h->err = fn + ": n_items must be 1 .. the slots given to uvs_ft_create"; return UVS_ERR_INVALID_ARG; }
    if (!(std::isfinite(threshold) && threshold > 0.0)) { h->err = fn + ": threshold must be finite and positive"; return UVS_ERR_INVALID_ARG; }
    if (!(confidence > 0.0 && confidence < 1.0)) { h->err = fn + ": confidence must be in (0, 1)"; return UVS_ERR_INVALID_ARG; }
    size_t n_pts = 0;
    for (int i = 0; i < n_items; ++i) {
        const uvs_ft_reject_item& it = items[i];
        const std::string who = fn + ": item " + std::to_string(i);
        if (it.n_points < 0 || it.n_points > h->max_points) { h->err = who + ": n_points must be 0 .. the capacity given to uvs_ft_create"; return UVS_ERR_INVALID_ARG; }
        if (it.n_points > 0 && (!it.prev_norm || !it.next_norm)) { h->err = who + ": null pointer"; return UVS_ERR_INVALID_ARG; }
        for (int k = 0; k < 2 * it.n_points; ++k)
            if (!std::isfinite(it.prev_norm[k]) || !std::isfinite(it.next_norm[k])) { h->err = who + ": a coordinate is not finite"; return UVS_ERR_INVALID_ARG; }
        n_pts += (size_t)it.n_points;
    }
    // the layout of the call: items | points, uploaded;  results | keep, downloaded;  the debug arrays
    UvsArena A;
    const size_t o_items = A.take(n_items * sizeof(FrItem)), o_pts = A.take(n_pts * 32);
    const size_t in_bytes = A.o;
    const size_t o_res = A.take(n_items * sizeof(uvs_ft_reject_result)), o_keep = A.take(n_pts);
    const size_t out_bytes = A.o - o_res;
    const size_t o_smp = A.take(dbg_samples ? (size_t)kHyp * kModel * 4 : 0), o_cnt = A.take(dbg_samples ? (size_t)kHyp * 3 * 4 : 0);
    const size_t o_mod = A.take(dbg_samples ? (size_t)kHyp * 27 * 8 : 0);
    UVS_HIP(h->err, hipSetDevice(h->device));
    int rc;
    if ((rc = h->d_rej.ensure(A.o, h->err)) != UVS_OK || (rc = h->h_rej_in.ensure(in_bytes, h->err, grow_pinned)) != UVS_OK ||
        (rc = h->h_rej_out.ensure(out_bytes, h->err, grow_pinned)) != UVS_OK) return rc;
    FrItem* F = reinterpret_cast<FrItem*>(h->h_rej_in + o_items);
    double* P = reinterpret_cast<double*>(h->h_rej_in + o_pts);
    size_t at = 0;
    for (int i = 0; i < n_items; ++i) {
        const size_t n = (size_t)items[i].n_points;
        F[i].n = (int)n; F[i].gated = 0; F[i].seed = items[i].seed; F[i].pts_off = (long long)(4 * at); F[i].keep_off = (long long)at;
        if (n) {
            std::memcpy(P + 4 * at, items[i].prev_norm, n * 16);
            std::memcpy(P + 4 * at + 2 * n, items[i].next_norm, n * 16);
        }
        at += n;
    }
    char* D = h->d_rej;
    hipStream_t st = h->st;
    UVS_HIP(h->err, hipEventRecord(h->ev0, st));
    UVS_HIP(h->err, hipMemcpyAsync(D, h->h_rej_in, in_bytes, hipMemcpyHostToDevice, st));
    k_ft_reject_run<false><<<n_items, kThreads, 0, st>>>(reinterpret_cast<const FrItem*>(D + o_items), reinterpret_cast<const double*>(D + o_pts), threshold, confidence,
                                                 dbg_samples ? 1 : 0, reinterpret_cast<uint8_t*>(D + o_keep), reinterpret_cast<uvs_ft_reject_result*>(D + o_res),
                                                 reinterpret_cast<int32_t*>(D + o_smp), reinterpret_cast<double*>(D + o_mod), reinterpret_cast<int32_t*>(D + o_cnt));
    UVS_HIP(h->err, hipGetLastError());
    UVS_HIP(h->err, hipMemcpyAsync(h->h_rej_out, D + o_res, out_bytes, hipMemcpyDeviceToHost, st));
    UVS_HIP(h->err, hipEventRecord(h->ev1, st));
    UVS_HIP(h->err, hipStreamSynchronize(st));
    UVS_HIP(h->err, hipEventElapsedTime(&h->reject_ms, h->ev0, h->ev1));
    std::memcpy(results, h->h_rej_out, n_items * sizeof(uvs_ft_reject_result));
    if (n_pts) std::memcpy(keep, h->h_rej_out + (o_keep - o_res), n_pts);
    if (dbg_samples) {
        UVS_HIP(h->err, hipMemcpy(dbg_samples, D + o_smp, (size_t)kHyp * kModel * 4, hipMemcpyDeviceToHost));
        UVS_HIP(h->err, hipMemcpy(dbg_counts, D + o_cnt, (size_t)kHyp * 3 * 4, hipMemcpyDeviceToHost));
        UVS_HIP(h->err, hipMemcpy(dbg_models, D + o_mod, (size_t)kHyp * 27 * 8, hipMemcpyDeviceToHost));
    }
    return UVS_OK;
}

}  // namespace

extern "C" {

int uvs_ft_reject(uvs_ft_tracker* h, int n_items, const uvs_ft_reject_item* items, double threshold, double confidence, uint8_t* keep,
                  uvs_ft_reject_result* results) {
    if (!h) return UVS_ERR_INVALID_ARG;
    return fr_run(h, "uvs_ft_reject", n_items, items, threshold, confidence, keep, results, nullptr, nullptr, nullptr);
}

double uvs_ft_last_reject_device_ms(const uvs_ft_tracker* h) { return h ? (double)h->reject_ms : 0.0; }

int uvs_ft_debug_reject(uvs_ft_tracker* h, const uvs_ft_reject_item* item, double threshold, double confidence, int32_t* samples, double* models,
                        int32_t* counts, uint8_t* keep, uvs_ft_reject_result* result) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    if (!item || !samples || !models || !counts) { h->err = "uvs_ft_debug_reject: null pointer"; return UVS_ERR_INVALID_ARG; }
    return fr_run(h, "uvs_ft_debug_reject", 1, item, threshold, confidence, keep, result, samples, models, counts);
}

}  // extern "C"
