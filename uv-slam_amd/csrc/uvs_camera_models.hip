// uvs_camera_models.hip -- the camera models of the front ends beyond the pinhole (MEI, Kannala-Brandt; csrc/uvs_camera_models.h states them)
// behind uvs_ft_set_camera_model, uvs_ft_lift and uvs_ft_project of include/uvs_solver.h.  The handle is the point tracker's
// (csrc/uvs_ft_handle.h); uvs_kf_set_camera_model sits with its handle in csrc/uvs_keyframe_features.hip, uvs_lt_set_undistort_model with
// the map kernel in csrc/uvs_line_undistort.hip.  The in-kernel lifts of uvs_ft_track, uvs_ft_detect and uvs_kf_extract call the same device function as
// k_cm_lift, so a point gets the same bits from either.  gfx950, the handle's one stream.
//
// This unit is compiled with -ffp-contract=off.  Two kernels, a lane per point, no LDS, no atomics, no scratch memory:
//   k_cm_lift      pixel -> ray and normalized point.  PINHOLE / MEI: multiplies and adds, at most two divides and one sqrt.  KANNALA_BRANDT:
//                  one sqrt, the root search (at most UVS_CAM_KB_ITERATIONS steps of ~20 FP64 operations and one divide; a lane leaves
//                  the loop when its step no longer moves, the wave when all have: 2 .. 7 steps inside the shipped images), one sin and
//                  one cos of an argument in [0, pi], four divides.  FP64 divides and the library's sin / cos are tens of instructions
//                  each; at one point per lane the kernel is bound by them, not by its 56 bytes of traffic per point.
//   k_cm_project   ray -> pixel; KANNALA_BRANDT: one sqrt, one atan2, the polynomial, two divides.
// The model is a kernel argument (UvsCamDev, 120 bytes): wave-uniform, so the branch on the model id is a scalar branch.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/uvs_solver.h"
#include "uvs_camera_models.h"
#include "uvs_ft_handle.h"

namespace uvscm {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads) k_cm_lift(UvsCamDev m, int n, const double* __restrict__ xy, double* __restrict__ ray,
                                                    double* __restrict__ norm) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (size_t)n) return;
    double r[3], nx, ny;
    uvs_cam_lift(m, xy[2 * i], xy[2 * i + 1], r, nx, ny);
    ray[3 * i] = r[0]; ray[3 * i + 1] = r[1]; ray[3 * i + 2] = r[2];
    norm[2 * i] = nx; norm[2 * i + 1] = ny;
}

__global__ void __launch_bounds__(kThreads) k_cm_project(UvsCamDev m, int n, const double* __restrict__ ray, double* __restrict__ xy) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (size_t)n) return;
    double u, v;
    uvs_cam_project(m, ray[3 * i], ray[3 * i + 1], ray[3 * i + 2], u, v);
    xy[2 * i] = u; xy[2 * i + 1] = v;
}

namespace {

// uvs_ft_lift (lift) and uvs_ft_project: n_in doubles per point up, n_out down, through the handle's (xy | ray | norm) buffer
int cm_points(uvs_ft_tracker* h, const std::string& fn, const uvs_camera_model* model, int n, bool lift, const double* in, double* out_a, double* out_b) {
    h->err.clear();
    if (!model || n < 0 || !in || (!lift && !out_a)) { h->err = fn + ": null pointer or bad count"; return UVS_ERR_INVALID_ARG; }
    UvsCamDev m;
    if (const int rc = uvs_cam_take(model, fn, h->err, &m)) return rc;
    if (n == 0) return UVS_OK;
    const size_t N = (size_t)n, o_ray = N * 16, o_norm = o_ray + N * 24, total = o_norm + N * 16;
    UVS_HIP(h->err, hipSetDevice(h->device));
    int rc;
    if ((rc = h->d_cm.ensure(total, h->err)) != UVS_OK || (rc = h->h_cm.ensure(total, h->err, grow_pinned)) != UVS_OK) return rc;
    double* dXy = reinterpret_cast<double*>(h->d_cm.get());
    double* dRay = reinterpret_cast<double*>(h->d_cm + o_ray);
    double* dNorm = reinterpret_cast<double*>(h->d_cm + o_norm);
    const unsigned blocks = (unsigned)((N + kThreads - 1) / kThreads);
    hipStream_t st = h->st;
    if (lift) {
        std::memcpy(h->h_cm, in, N * 16);
        UVS_HIP(h->err, hipMemcpyAsync(dXy, h->h_cm, N * 16, hipMemcpyHostToDevice, st));
        k_cm_lift<<<blocks, kThreads, 0, st>>>(m, n, dXy, dRay, dNorm);
        UVS_HIP(h->err, hipGetLastError());
        UVS_HIP(h->err, hipMemcpyAsync(h->h_cm + o_ray, h->d_cm + o_ray, total - o_ray, hipMemcpyDeviceToHost, st));
        UVS_HIP(h->err, hipStreamSynchronize(st));
        if (out_a) std::memcpy(out_a, h->h_cm + o_ray, N * 24);
        if (out_b) std::memcpy(out_b, h->h_cm + o_norm, N * 16);
    } else {
        std::memcpy(h->h_cm + o_ray, in, N * 24);
        UVS_HIP(h->err, hipMemcpyAsync(dRay, h->h_cm + o_ray, N * 24, hipMemcpyHostToDevice, st));
        k_cm_project<<<blocks, kThreads, 0, st>>>(m, n, dRay, dXy);
        UVS_HIP(h->err, hipGetLastError());
        UVS_HIP(h->err, hipMemcpyAsync(h->h_cm, dXy, N * 16, hipMemcpyDeviceToHost, st));
        UVS_HIP(h->err, hipStreamSynchronize(st));
        std::memcpy(out_a, h->h_cm, N * 16);
    }
    return UVS_OK;
}

}  // namespace

}  // namespace uvscm

using namespace uvscm;

extern "C" {

int uvs_ft_set_camera_model(uvs_ft_tracker* h, const uvs_camera_model* model) {
    if (!h) return UVS_ERR_INVALID_ARG;
    h->err.clear();
    if (!model) { h->model = uvs_cam_none(); return UVS_OK; }
    UvsCamDev m;
    if (const int rc = uvs_cam_take(model, "uvs_ft_set_camera_model", h->err, &m)) return rc;
    h->model = m;
    return UVS_OK;
}

int uvs_ft_lift(uvs_ft_tracker* h, const uvs_camera_model* model, int n, const double* xy, double* ray, double* norm) {
    if (!h) return UVS_ERR_INVALID_ARG;
    return cm_points(h, "uvs_ft_lift", model, n, true, xy, ray, norm);
}

int uvs_ft_project(uvs_ft_tracker* h, const uvs_camera_model* model, int n, const double* ray, double* xy) {
    if (!h) return UVS_ERR_INVALID_ARG;
    return cm_points(h, "uvs_ft_project", model, n, false, ray, xy, nullptr);
}

}  // extern "C"
